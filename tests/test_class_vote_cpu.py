"""CPU-only checks of the per-class vote (include/pvnet_classes.h, libpvnet_classes.so; pvnet_vote_v3_prepared of libpvnet_vote.so;
voting.ransac_voting_layer_v2): the new library's exports, ABI version and header constants against pvnet_amd/_abi.py, every bad
argument of the new entry points rejected before any HIP call, the overlay module's export under the reference's name and positional
signature, the voting library's kernel count and ABI version unchanged, the register rule for the new kernels, and the numpy
restatement of the split (tests/class_split_restatement.py) against hand-made label images.
What holds for every side library alike (header against table, the built library's symbols, the register tool's selection, the loud
failure without it) is in tests/test_side_libraries_cpu.py."""
import ast
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import ransac_voting_oracle as O
from pvnet_amd import _abi, build
from tests import class_split_restatement as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "pvnet_classes.h")).read()
VOTE_HDR = open(os.path.join(ROOT, "include", "pvnet_vote.h")).read()
REFERENCE = os.environ.get("PVNET_REFERENCE", "/root/reference")
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -3
EXPORTS = {"pvnet_classes_abi_version", "pvnet_class_split", "pvnet_class_split_logits"}
# ransac_voting_gpu.py:99-100 of the reference
V2_POSITIONAL = ["mask", "vertex", "class_num", "round_hyp_num", "inlier_thresh", "confidence", "max_iter", "min_num", "max_num",
                 "refine_iter_num"]
V2_DEFAULTS = [0.999, 0.99, 20, 5, 30000, 1]


@pytest.fixture(scope="module")
def libs():
    build.build()
    from pvnet_amd import voting
    return _abi.load_classes_library(), voting.load_library()


def test_header_exports_constants_and_prototypes():
    returns = dict((n, t) for t, n in re.findall(r"^(int|size_t)\s+(pvnet_[a-z0-9_]+)\s*\(", HDR, re.M))
    assert set(returns) == EXPORTS and set(returns.values()) == {"int"}
    decl = re.search(r"^int pvnet_class_split\s*\((.*?)\);", HDR, re.M | re.S).group(1).split(",")
    args = _abi.CLASSES_PROTOTYPES["pvnet_class_split"][1]
    assert "uint64_t seed" in decl[8] and args[8] is C.c_uint64 and "num_classes" in decl[3] and "max_num" in decl[7]
    assert "bits" in decl[10] and "seg0" in decl[11] and "cum" in decl[12] and "stream" in decl[13]
    consts = dict((n, int(v)) for n, v in re.findall(r"^#define\s+PVNET_CLASSES_(\w+)\s+(\d+)", HDR, re.M))
    assert consts.pop("ABI_VERSION") == _abi.CLASSES_ABI_VERSION == 1
    assert consts.pop("MAX") == _abi.CLASSES_MAX >= 22   # 21 objects and the background
    assert len(consts) == 3
    for name, value in consts.items():
        assert getattr(_abi, "CLASSES_" + name) == value, name
    # the voting header declares the second half and no longer misstates the histogram length
    assert "pvnet_vote_v3_prepared" in _abi.PROTOTYPES and re.search(r"^int pvnet_vote_v3_prepared\(", VOTE_HDR, re.M)
    assert "[b][nseg][1024]" not in VOTE_HDR and "[b][nseg][%d]" % RS.THIN_BINS in VOTE_HDR
    v3, prep = _abi.PROTOTYPES["pvnet_vote_v3"][1], _abi.PROTOTYPES["pvnet_vote_v3_prepared"][1]
    assert prep == v3[3:6] + [C.c_int] + v3[6:]   # v3 without its mask part, src_div behind b


def test_libraries_are_built_and_the_vote_library_keeps_its_abi_and_kernel_count(libs):
    clib, vlib = libs
    raw = C.CDLL(_abi.CLASSES_LIB_PATH)
    assert clib.pvnet_classes_abi_version() == 1
    assert b"class_split_kernel" in open(_abi.CLASSES_LIB_PATH, "rb").read()
    assert build.SIDE_LIBRARIES["classes"][:2] == (["class_split.hip"], "pvnet_classes.h")
    # it links nothing from the vote library, and neither exports the other's functions
    assert not hasattr(raw, "pvnet_vote_v3") and not hasattr(raw, "pvnet_vote_v3_prepared") and not hasattr(raw, "pvnet_vote_layout")
    for path in (_abi.LIB_PATH, _abi.DEV_LIB_PATH):
        other = C.CDLL(path)
        assert hasattr(other, "pvnet_vote_v3_prepared")
        assert b"class_split_kernel" not in open(path, "rb").read()
    assert vlib.pvnet_vote_abi_version() == _abi.ABI_VERSION == 9
    info = C.CDLL(_abi.LIB_PATH).pvnet_vote_build_info
    info.restype = C.c_char_p
    assert 0 < int(re.search(r"(\d+) kernels", info().decode()).group(1)) <= 55   # no new kernel in the release vote library


def test_bad_arguments_are_rejected_without_a_device(libs):
    clib, vlib = libs
    p, q = C.c_void_p(0x1000), C.c_void_p(0x2000)   # never dereferenced: validation returns before any HIP call
    s3, s4, s5 = (C.c_int64 * 3)(7200, 100, 1), (C.c_int64 * 4)(28800, 7200, 100, 1), (C.c_int64 * 5)(1, 1, 1, 1, 1)

    def split(labels=p, dt=_abi.MASK_I64, st=s3, nc=4, b=3, h=72, w=100, max_num=200, bits=q, seg0=q, cum=q, fn=clib.pvnet_class_split):
        return fn(labels, dt, st, nc, b, h, w, max_num, 3, 0, bits, seg0, cum, None)

    for fn, st, good, types in ((clib.pvnet_class_split, s3, _abi.MASK_I64, (-1, 5, 99)),
                                (clib.pvnet_class_split_logits, s4, _abi.CLASSES_LOGITS_BF16, (-1, 3))):
        def call(**kw):
            return split(**{**dict(fn=fn, st=st, dt=good), **kw})

        for name in ("labels", "st", "bits", "seg0"):
            assert call(**{name: None}) == BADARG, name
        assert call(cum=None) == BADARG                # max_num < h w needs the histograms ...
        assert call(nc=1) == BADARG and call(nc=0) == BADARG and call(nc=-3) == BADARG
        assert call(nc=_abi.CLASSES_MAX + 1) == BADARG
        for dt in types:
            assert call(dt=dt) == BADARG, dt
        assert call(b=0) == BADARG and call(h=0) == BADARG and call(w=-1) == BADARG and call(max_num=-1) == BADARG
        assert call(bits=C.c_void_p(0x2004)) == BADARG and call(cum=C.c_void_p(0x2002)) == BADARG
        assert call(h=32768, w=32769) == UNSUPPORTED and call(b=21846, nc=4) == UNSUPPORTED

    from pvnet_amd import voting
    L = voting.vote_layout(9, 72, 100, 9, 128, 200)

    def prepared(vertex=p, vs=s5, b=9, div=3, out=p, ws=q, nbytes=L.total_bytes, hn=128):
        return vlib.pvnet_vote_v3_prepared(vertex, vs, b, div, 72, 100, 9, hn, 0.99, 5, 200, 3, 0, None, 0, out, None, ws, nbytes, None)

    for name in ("vertex", "vs", "out", "ws"):
        assert prepared(**{name: None}) == BADARG, name
    assert prepared(b=9, div=2) == BADARG and prepared(b=10, div=3) == BADARG       # B % src_div
    assert prepared(div=0) == BADARG and prepared(div=-3) == BADARG and prepared(b=0) == BADARG
    assert prepared(nbytes=L.total_bytes - 1) == WORKSPACE and prepared(nbytes=0) == WORKSPACE   # a short workspace
    assert prepared(ws=C.c_void_p(0x2010)) == BADARG                                # misaligned workspace
    assert prepared(hn=0) == BADARG


def test_front_end_checks_need_no_device():
    import torch
    from pvnet_amd import voting
    m, v = torch.zeros(1, 8, 8, dtype=torch.int64), torch.zeros(1, 8, 8, 2, 2)
    with pytest.raises(RuntimeError, match="CUDA"):
        voting.ransac_voting_layer_v2(m, v, 3, 64)           # no CPU fallback
    with pytest.raises(RuntimeError, match="CUDA"):
        voting.ransac_voting_layer_v2_from_logits(torch.zeros(1, 3, 8, 8), v, 64)
    sig = inspect.signature(voting.ransac_voting_layer_v2)
    assert [n for n, q in sig.parameters.items() if q.kind is q.POSITIONAL_OR_KEYWORD] == V2_POSITIONAL
    assert [n for n, q in sig.parameters.items() if q.kind is q.KEYWORD_ONLY] == [
        "idxs", "seed", "image_offset", "literal", "approx", "refine", "return_status", "return_debug", "workspace", "out"]
    lsig = inspect.signature(voting.ransac_voting_layer_v2_from_logits)
    assert [n for n, q in lsig.parameters.items() if q.kind is q.POSITIONAL_OR_KEYWORD] == \
        ["seg_pred", "vertex"] + V2_POSITIONAL[3:]


def test_overlay_exports_v2_under_the_reference_signature():
    path = os.path.join(ROOT, "lib", "ransac_voting_gpu_layer", "ransac_voting_gpu.py")
    code = ("import sys, inspect; sys.path.insert(0, %r); import importlib.util as u; s = u.spec_from_file_location('ov', %r); "
            "m = u.module_from_spec(s); s.loader.exec_module(m); f = m.ransac_voting_layer_v2; "
            "from pvnet_amd import voting; assert f is voting.ransac_voting_layer_v2 and 'ransac_voting_layer_v2' in m._NATIVE; "
            "ps = inspect.signature(f).parameters.values(); "
            "print([q.name for q in ps if q.kind is q.POSITIONAL_OR_KEYWORD]); "
            "print([q.default for q in ps if q.kind is q.POSITIONAL_OR_KEYWORD and q.default is not q.empty])") % (ROOT, path)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    names, defaults = (ast.literal_eval(line) for line in r.stdout.strip().splitlines()[-2:])
    assert names == V2_POSITIONAL and defaults == V2_DEFAULTS
    ref = os.path.join(REFERENCE, "lib", "ransac_voting_gpu_layer", "ransac_voting_gpu.py")
    if os.path.isfile(ref):   # the reference's own definition, where a checkout is at hand: the same names and defaults, in order
        fn = next(n for n in ast.parse(open(ref).read()).body if isinstance(n, ast.FunctionDef) and n.name == "ransac_voting_layer_v2")
        assert [a.arg for a in fn.args.args] == names and not fn.args.kwonlyargs and fn.args.vararg is None
        assert [ast.literal_eval(d) for d in fn.args.defaults] == defaults


def test_register_rule_holds_for_the_new_kernels():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_resources.py"), "--classes"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [l for l in r.stdout.splitlines() if "class_split_kernel" in l]
    assert len(rows) == 7 and all("8 waves/SIMD" in l and "scratch   0 B" in l for l in rows)   # five types, the pair load, the logits


# ---- the restatement against hand-made label images ---------------------------------------------------------------------------------
def test_restatement_bits_and_counts_of_a_hand_made_image():
    lab = np.zeros((1, 2, 70), np.int64)        # 140 pixels: words 0, 1 and a third of 12 pixels
    lab[0, 0, 0:3] = 1                          # pixels 0, 1, 2
    lab[0, 0, 62:66] = 2                        # pixels 62 .. 65: across the boundary of words 0 and 1
    lab[0, 1, 58:70] = 1                        # pixels 128 .. 139: the partial last word
    lab[0, 0, 10], lab[0, 0, 11], lab[0, 0, 12], lab[0, 0, 13] = 3, 255, 257, -1   # 3 = num_classes and beyond: nobody's
    bits, seg0, cum, has = RS.split(lab, 3, 10 ** 6, seed=1)
    assert cum is None and bits.shape == (2, 3) and seg0.shape == (2, 1)
    assert [int(x) for x in bits[0]] == [0b111, 0, (1 << 12) - 1] and [int(x) for x in bits[1]] == [0b11 << 62, 0b11, 0]
    assert seg0.tolist() == [[15], [4]] and has.all()
    # labels are compared on their full value, not on their low byte; a bool image is class 1
    assert RS.class_of(np.array([256 + 1, -255, 1, 2, 0]), 3).tolist() == [0, 0, 1, 2, 0]
    assert RS.class_of(np.array([True, False]), 2).tolist() == [1, 0]
    assert RS.class_of(np.array([1.0, 1.5, 2.0, np.nan, -1.0, 3.0], np.float32), 3).tolist() == [1, 0, 2, 0, 0, 0]
    # two images: virtual image v = i (num_classes - 1) + k
    lab2 = np.stack([lab[0], np.full((2, 70), 2, np.int64)])
    bits2, seg2, _, has2 = RS.split(lab2, 3, 10 ** 6, seed=1)
    assert (bits2[:2] == bits).all() and seg2[2:].tolist() == [[0], [140]] and has2.tolist() == [[True], [True], [False], [True]]
    assert int(bits2[3, 2]) == (1 << 12) - 1 and int(bits2[3, 0]) == 2 ** 64 - 1


def test_restatement_argmax_rules():
    seg = np.zeros((1, 3, 1, 5), np.float32)
    seg[0, :, 0, 0] = (1, 1, 1)                  # a tie: the first maximum
    seg[0, :, 0, 1] = (0, 2, 2)
    seg[0, :, 0, 2] = (5, np.nan, 7)             # a NaN counts as the maximum
    seg[0, :, 0, 3] = (np.nan, np.nan, 9)        # the first NaN wins
    seg[0, :, 0, 4] = (-1, -2, -0.5)
    assert RS.argmax_first(seg)[0, 0].tolist() == [0, 1, 1, 0, 2]


def test_restatement_histograms_agree_with_the_oracles_thinning():
    rng = np.random.default_rng(5)
    h, w, nc, max_num, seed, base = 72, 100, 4, 200, 11, 5
    lab = rng.integers(0, nc + 1, (2, h, w))                 # label 4 is nobody's
    lab[1][lab[1] == 2] = 0                                  # class 2 absent from image 1
    lab[0, :41][lab[0, :41] == 3] = 0                        # class 3 of image 0 lives in the second segment only
    bits, seg0, cum, has = RS.split(lab, nc, max_num, seed, base)
    assert cum.shape == (6, 2, RS.THIN_BINS) and RS.THIN_BINS == 1536 and seg0.shape == (6, 2)
    assert not has[4].any() and has[2].tolist() == [False, True] and (cum[4] == 0).all()
    for r in (0, 1, 5, 1 << 4, (1 << 26) - 1, 1 << 26, 2 ** 32 - 1, 123456789):
        assert RS.thin_bins(np.array([r], np.uint32))[0] == O.thin_bin(r)
    for v in range(6):
        i, k = divmod(v, nc - 1)
        m = (lab[i] == k + 1).reshape(-1)
        tn0 = int(m.sum())
        per_word = np.add.reduceat(np.pad(m, (0, 113 * 64 - m.size)).astype(int), np.arange(0, 113 * 64, 64))   # 112.5 words
        assert seg0[v].sum() == tn0 and [bin(int(x)).count("1") for x in bits[v]] == per_word.tolist()
        if tn0 == 0:
            continue
        for s in range(2):
            if has[v, s]:
                assert cum[v, s, -1] == seg0[v, s] and (np.diff(cum[v, s].astype(int)) >= 0).all()   # every bin kept: every pixel
        assert tn0 > max_num
        keep = O.subsample_keep(seed, base + v, h * w, max_num, tn0) & m    # the oracle's own thinning of this mask, this stream
        for s in range(2):
            want = int(keep[s * 4096:(s + 1) * 4096].sum())
            assert (RS.kept_before(cum[v, s], max_num, tn0) if has[v, s] else 0) == want
