"""CPU-only checks of the C-ABI library and its host wrapper: it builds, loads, exports every symbol that
include/pvnet_vote.h declares, validates arguments, and never falls back to a CPU path."""
import ctypes as C
import os
import sys
import re

import pytest
import torch

from pvnet_amd import _abi, build, voting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return voting.load_library()


def test_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "pvnet_vote.h")).read()
    names = set(re.findall(r"\b(pvnet_[a-z0-9_]+)\s*\(", hdr))
    assert {"pvnet_vote_v3", "pvnet_vote_v3_profiled", "pvnet_generate_hypothesis", "pvnet_voting_for_hypothesis",
            "pvnet_vote_workspace_bytes", "pvnet_vote_layout", "pvnet_vote_abi_version", "pvnet_vote_tuning_reload",
            "pvnet_vote_v3_stage_repeat", "pvnet_generate_hypothesis_vanishing_point",
            "pvnet_voting_for_hypothesis_vanishing_point", "pvnet_vote_build_info"} <= names
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/pvnet_vote.h but not exported"
    assert lib.pvnet_vote_abi_version() == 9
    assert b"gfx950" in lib.pvnet_vote_build_info()


def test_release_and_development_builds(monkeypatch):
    """two libraries of ONE ABI: libpvnet_vote.so -- the knobs are constants, the kernels the defaults reach -- and the development
    build with the environment knobs and every kernel variant; the Python front end takes the second only when a knob is set"""
    build.build()
    hdr = open(os.path.join(ROOT, "include", "pvnet_vote.h")).read()
    names = set(re.findall(r"\b(pvnet_[a-z0-9_]+)\s*\(", hdr))
    info = {}
    for path in (voting.LIB_PATH, voting.DEV_LIB_PATH):
        lib = C.CDLL(path)
        for n in names:
            assert hasattr(lib, n), f"{n} declared in include/pvnet_vote.h but not exported by {os.path.basename(path)}"
        lib.pvnet_vote_build_info.restype = C.c_char_p
        info[path] = lib.pvnet_vote_build_info().decode()
        assert lib.pvnet_vote_abi_version() == 9
    rel, dev = info[voting.LIB_PATH], info[voting.DEV_LIB_PATH]
    assert "release build" in rel and "development build" in dev
    nrel, ndev = (int(re.search(r"(\d+) kernels", t).group(1)) for t in (rel, dev))
    assert 0 < nrel <= 55 < ndev   # the shipped library holds the kernels its defaults reach (the count is in build_info)
    for k in voting.TUNING_KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("PVNET_VOTE_LIB", raising=False)
    assert voting._wanted_library() == voting.LIB_PATH
    monkeypatch.setenv("PVNET_SCORE_CHUNK", "64")
    assert voting._wanted_library() == voting.DEV_LIB_PATH
    monkeypatch.delenv("PVNET_SCORE_CHUNK")
    # the release build reads no environment: a knob changes ITS layout nothing, the development build's it does
    L = voting.Layout()
    lrel, ldev = C.CDLL(voting.LIB_PATH), C.CDLL(voting.DEV_LIB_PATH)
    monkeypatch.setenv("PVNET_SCORE_CHUNK", "64")
    for lib in (lrel, ldev):
        lib.pvnet_vote_tuning_reload()
    assert lrel.pvnet_vote_layout(32, 480, 640, 9, 1024, 30000, C.byref(L)) == 0 and L.chunk == 128
    assert ldev.pvnet_vote_layout(32, 480, 640, 9, 1024, 30000, C.byref(L)) == 0 and L.chunk == 64
    monkeypatch.delenv("PVNET_SCORE_CHUNK")
    ldev.pvnet_vote_tuning_reload()
    voting.reload_tuning()


def test_host_pnp_library_exports_every_declared_symbol():
    """include/pvnet_pnp.h: the host-side pose refinement, incl. the reference's own `uncertainty_pnp` symbol"""
    from pvnet_amd import pnp
    build.build()
    plib = pnp.load_pnp_library()
    hdr = open(os.path.join(ROOT, "include", "pvnet_pnp.h")).read()
    body = hdr[hdr.index('extern "C"'):]
    names = set(re.findall(r"^(?:void|int)\s+([a-z0-9_]+)\s*\(", body, flags=re.M))
    assert {"uncertainty_pnp", "pvnet_pnp_refine", "pvnet_pnp_evaluate", "pvnet_pnp_solve", "pvnet_pnp_solve_batch", "pvnet_pnp_poses_from_rt",
            "pvnet_angle_axis_to_matrix", "pvnet_matrix_to_angle_axis", "farthest_point_sampling",
            "farthest_point_sampling_init_center"} == names
    for n in names:
        assert hasattr(plib, n), f"{n} declared in include/pvnet_pnp.h but not exported"


def test_library_contains_gfx950_code_object():
    blob = open(voting.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"score_kernel" in blob and b"score_mfma_kernel" in blob and b"score_exact_kernel" in blob


def test_layout_baseline_config(lib):
    L = voting.vote_layout(32, 480, 640, 9, 1024, 30000)
    assert (L.b, L.vn, L.hn, L.words) == (32, 9, 1024, 4800)
    assert L.cap % 8 == 0 and 30000 < L.cap < 32000  # max_num + 8 sigma of the Bernoulli subsample
    assert L.hn_pad == L.hgroups * 64 * L.hpl >= 1024 and L.max_chunks == -(-L.cap // L.chunk)
    offs = [L.off_ctrl, L.off_seg, L.off_items, L.off_bits, L.off_pix, L.off_rec, L.off_hyp, L.off_partial,
            L.off_counts, L.off_win, L.total_bytes]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    assert lib.pvnet_vote_workspace_bytes(32, 480, 640, 9, 1024, 30000) == L.total_bytes
    full = voting.vote_layout(1, 480, 640, 9, 512, 10 ** 9)
    assert full.cap == 480 * 640 + 8  # no subsampling possible -> every pixel may be foreground


def test_argument_validation_without_a_gpu(lib):
    assert lib.pvnet_vote_workspace_bytes(0, 480, 640, 9, 1024, 30000) == 0
    L = voting.Layout()
    assert lib.pvnet_vote_layout(1, 4, 4, 1, 0, 10, C.byref(L)) == -1  # PVNET_E_BADARG
    ms = (C.c_int64 * 3)(16, 4, 1)
    vs = (C.c_int64 * 5)(64, 16, 4, 2, 1)
    rc = lib.pvnet_vote_v3(None, 3, ms, None, vs, 1, 4, 4, 2, 8, C.c_float(0.99), 5, 100, 0, 0, None, 0, None, None,
                           None, 0, None)
    assert rc == -1
    rc = lib.pvnet_generate_hypothesis(None, None, None, None, 1, 1, 1, None)
    assert rc == -1


def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="CUDA"):
        voting.ransac_voting_layer_v3(torch.zeros((1, 8, 8), dtype=torch.int64), torch.zeros((1, 8, 8, 2, 2)), 16)
    with pytest.raises(RuntimeError, match="CUDA"):
        voting.generate_hypothesis(torch.zeros(4, 1, 2), torch.zeros(4, 2), torch.zeros(2, 1, 2, dtype=torch.int32))
    for f in os.listdir(os.path.join(ROOT, "pvnet_amd")):  # the product never imports the checker
        if f.endswith(".py"):
            src = open(os.path.join(ROOT, "pvnet_amd", f)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_abi, "_lib", None)
    monkeypatch.setattr(_abi, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        voting.load_library()


def test_reference_import_path_resolves_to_hip_layer():
    import importlib
    m = importlib.import_module("lib.ransac_voting_gpu_layer.ransac_voting_gpu")
    assert m.ransac_voting_layer_v3 is voting.ransac_voting_layer_v3
    import inspect
    sig = inspect.signature(m.ransac_voting_layer_v3)
    names = list(sig.parameters)[:8]
    assert names == ["mask", "vertex", "round_hyp_num", "inlier_thresh", "confidence", "max_iter", "min_num",
                     "max_num"]  # ransac_voting_gpu.py:514-515
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["inlier_thresh"], d["confidence"], d["max_iter"], d["min_num"], d["max_num"]) == \
           (0.999, 0.99, 20, 5, 30000)
    ops = importlib.import_module("lib.ransac_voting_gpu_layer.ransac_voting")
    for n in ("generate_hypothesis", "voting_for_hypothesis", "generate_hypothesis_vanishing_point",
              "voting_for_hypothesis_vanishing_point"):  # ransac_voting.cpp:102-107
        assert callable(getattr(ops, n))


def test_compiled_ransac_voting_module_loads_without_a_gpu():
    """pvnet_amd/csrc/ransac_voting_ext.cpp: the reference's compiled extension module (src/ransac_voting.cpp:102-107) on
    libpvnet_vote.so.  No compute here: it must build, import from the reference's module path ahead of the Python
    stand-in, expose the four functions with the reference's doc strings and refuse CPU tensors as CHECK_CUDA does."""
    import importlib
    import subprocess
    out = build.build_ext()
    if out is None:
        pytest.skip("torch headers / C++ compiler not available: the Python stand-in serves the module")
    code = ("import sys; sys.path.insert(0, %r); import torch; "
            "import lib.ransac_voting_gpu_layer.ransac_voting as m; "
            "assert m.__file__ == %r, m.__file__; "
            "docs = {n: getattr(m, n).__doc__.strip().splitlines()[-1] for n in ('generate_hypothesis', 'voting_for_hypothesis', "
            "'generate_hypothesis_vanishing_point', 'voting_for_hypothesis_vanishing_point')}; "
            "assert docs == {'generate_hypothesis': 'generate hypothesis', 'voting_for_hypothesis': 'voting for hypothesis', "
            "'generate_hypothesis_vanishing_point': 'generate hypothesis vanishing point', "
            "'voting_for_hypothesis_vanishing_point': 'voting for hypothesis vanishing point'}, docs\n"
            "try:\n    m.generate_hypothesis(torch.zeros(4, 9, 2), torch.zeros(4, 2), torch.zeros(3, 9, 2, dtype=torch.int32))\n"
            "except RuntimeError as e:\n    assert 'must be a CUDA tensor' in str(e)\nelse:\n    raise SystemExit('no error')\n"
            "print('ok')") % (ROOT, out)
    r = subprocess.run([sys.executable, "-c", code], cwd="/tmp", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    # the pybind signatures are the reference's (three / five positional arguments)
    importlib.invalidate_caches()


def test_motion_voting_workspace_and_argument_checks(lib):
    lib.pvnet_motion_workspace_bytes.restype = C.c_size_t
    n = lib.pvnet_motion_workspace_bytes(32, 480, 640, 9)
    assert 32 * 4800 * 8 < n < 8 * 1024 * 1024 and n % 256 == 0  # bit mask + segment counts + per-segment sums
    assert lib.pvnet_motion_workspace_bytes(0, 480, 640, 9) == 0
    z3, z5 = (C.c_int64 * 3)(), (C.c_int64 * 5)()
    assert lib.pvnet_motion_voting(None, 3, z3, None, z5, 1, 4, 4, 1, None, None, 0, None) == -1  # PVNET_E_BADARG


def test_oversized_matrix_pipe_items_are_refused(monkeypatch):
    """the wrapped vote accumulators of the matrix-pipe kernel hold < 512 votes: a work item of >= 1024 pixels is
    refused by pvnet_vote_layout instead of miscounting"""
    monkeypatch.setenv("PVNET_SCORE_CHUNK", "256")
    voting.reload_tuning()  # knobs are read once, at the library's first call; re-read them explicitly
    try:
        with pytest.raises(RuntimeError, match="PVNET_E_UNSUPPORTED"):
            voting.vote_layout(2, 120, 160, 9, 100, 30000)  # 100 hypotheses: 4 chunks per work item
    finally:
        monkeypatch.delenv("PVNET_SCORE_CHUNK")
        voting.reload_tuning()
    voting.vote_layout(2, 120, 160, 9, 100, 30000)  # and an environment change alone does nothing until reloaded


@pytest.fixture(scope="module")
def chk():
    """tools/check_kernel_resources.py -- its assembly of both builds is compiled once for the tests that read it"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_kernel_resources", os.path.join(ROOT, "tools", "check_kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_kernel_keeps_a_spare_vgpr_granule(tmp_path, chk):
    """round 2's compaction flake: identical code failed in 98 % of the runs when it used its VGPR allocation to the top
    and never with one granule more (profiles/r02_compaction_flake_investigation.txt).  Every kernel of both sources must
    allocate at least 8 VGPRs beyond the highest one an instruction names (PVNET_SPARE_VGPRS); the checker is checked on
    a hand-made violation."""
    assert chk.main([]) == 0
    body = ("kern:\n\tv_add_u32_e32 v23, v0, v1\n\ts_endpgm\n.Lfunc_end0:\n"
            "\t.amdhsa_kernel kern\n\t\t.amdhsa_next_free_vgpr %d\n\t.end_amdhsa_kernel\n")
    tight, roomy = tmp_path / "tight.s", tmp_path / "roomy.s"
    tight.write_text(body % 24)
    roomy.write_text(body % 32)
    assert chk.main([str(tight)]) == 1 and chk.main([str(roomy)]) == 0


def test_vote_epilogue_keeps_mfma_hazard_distance(tmp_path):
    """vote8 reads MFMA results from inline asm, where LLVM inserts no XDL-write -> VALU-read wait states: the generated
    assembly of every matrix-pipe scoring kernel is re-checked (tools/check_mfma_hazard.py), and the checker itself is
    checked on a hand-made violation."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_mfma_hazard", os.path.join(ROOT, "tools", "check_mfma_hazard.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    assert chk.main([]) == 0  # compiles the library's translation units to assembly with the product's flags
    bad = tmp_path / "bad.s"
    bad.write_text("_Z17score_mfma_kernelILi9EEv:\n"
                   "\tv_mfma_f32_32x32x16_bf16 v[2:17], v[144:147], v[82:85], 0\n"
                   "\ts_nop 3\n"
                   "\tv_sub_f32_e64 v50, v18, |v9| clamp\n"
                   "\ts_endpgm\n.Lfunc_end0:\n")
    assert chk.main([str(bad)]) == 1  # 4 wait states < 11
    ok = tmp_path / "ok.s"
    ok.write_text(bad.read_text().replace("s_nop 3", "s_nop 7\n\ts_nop 2"))
    assert chk.main([str(ok)]) == 0  # 8 + 3 = 11


def test_concurrency_hint_follows_stream_alternation(monkeypatch):
    """host logic of the PVNET_F_CONCURRENT hint (voting.concurrent_hint): explicit values win; with None the flag is set
    exactly when a call's stream differs from the previous call's on that device (no GPU needed: the stream query is faked)."""
    class FakeStream:
        def __init__(self, h):
            self.cuda_stream = h
    cur = {"h": 11}
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: FakeStream(cur["h"]))
    monkeypatch.setattr(voting, "_last_stream", {})
    dev0, dev1 = torch.device("cuda", 0), torch.device("cuda", 1)
    assert voting.concurrent_hint(dev0, True) == voting.F_CONCURRENT and voting.concurrent_hint(dev0, False) == 0
    assert voting._last_stream == {}                      # explicit values do not touch the history
    seen = []
    for h in (11, 11, 12, 11, 11, 11):
        cur["h"] = h
        seen.append(voting.concurrent_hint(dev0, None) != 0)
    assert seen == [False, False, True, True, False, False]
    cur["h"] = 99                                          # another device has its own history
    assert voting.concurrent_hint(dev1, None) == 0 and voting.concurrent_hint(dev1, None) == 0
    cur["h"] = 11
    assert voting.concurrent_hint(dev0, None) == 0
    assert voting.F_CONCURRENT == 256   # (equal to the header's PVNET_F_CONCURRENT: tests/test_abi_mirror.py, with every other constant)


def test_release_kernels_equal_the_development_builds(chk):
    """the knob tests and the fuzz matrix run the DEVELOPMENT build (a PVNET_* knob loads it): their green speaks for the shipped
    kernels only if every kernel of the release build is the same-named development kernel -- the same instruction stream (comments
    stripped, local labels renumbered) and the same descriptor (.amdhsa_* fields).  A `#ifdef PVNET_DEV` inside a kernel body breaks
    that.  The comparison is checked on hand-made differences."""
    texts = {}
    for src, dev, text in chk.assembly():
        texts.setdefault(src, {})[dev] = text
    pairs = [(t[False], t[True]) for t in texts.values()]
    released = [n for rel, _ in pairs for n in chk.kernel_code(rel)]
    assert len(released) >= 45 and any("score_exact_kernel_both" in n for n in released)
    assert chk.release_differs_from_dev(pairs) == []
    rel = next(t[False] for src, t in texts.items() if src.endswith("k4_score_cull.hip"))
    name = next(n for n in chk.kernel_code(rel) if "score_exact_kernel_both_0_0" in n)
    i = rel.index("\n" + name + ":")
    j = rel.index("v_sub_f32_e64", i)
    k = rel.index(".amdhsa_next_free_sgpr", rel.index(".amdhsa_kernel " + name))
    one_op = rel[:j] + "v_add_f32_e64" + rel[j + len("v_sub_f32_e64"):]
    one_field = rel[:k] + ".amdhsa_next_free_sgpr 7\n;" + rel[k:]
    labels = re.sub(r"\.LBB(\d+)_", r".LBB9\1_", rel)   # other label numbers only
    assert chk.release_differs_from_dev([(rel, one_op)]) == [name]
    assert chk.release_differs_from_dev([(rel, one_field)]) == [name]
    assert chk.release_differs_from_dev([(rel, labels)]) == []


def release_layout(b, h, w, vn, hn, max_num=30000):
    """pvnet_vote_layout of the RELEASE library, whatever the environment holds"""
    L = voting.Layout()
    assert C.CDLL(voting.LIB_PATH).pvnet_vote_layout(b, h, w, vn, hn, max_num, C.byref(L)) == 0
    return L


def test_release_layout_gives_the_gpu_tests_their_culling_path(lib):
    """the release library builds culling buffers (L.cull: the merged scoring launch) only for hn_pad 1 024, 256-pixel items and
    vn <= 32.  tests/test_release_scoring.py needs that path for its shapes and for half its fuzz cases; a layout change that would
    turn them into plain dense calls fails here, without a GPU"""
    from tests import fuzz_cases as F
    from tests.test_release_scoring import CULLING_SHAPES, MANY_KP_SHAPES, RELEASE_BLOCK, RELEASE_BLOCKS
    for shape in CULLING_SHAPES:
        assert release_layout(*shape).cull == 1, shape
    for shape in [(7, 240, 320, 9, 1024), (1, 240, 320, 32, 1024), (2, 240, 320, 9, 1024),   # b * vn < 64 at hn 1 024
                  (8, 240, 320, 9, 256), (8, 240, 320, 9, 2048), (8, 240, 320, 9, 767), (8, 240, 320, 9, 1025),
                  MANY_KP_SHAPES[33], MANY_KP_SHAPES[40]]:
        assert release_layout(*shape).cull == 0, shape
    capable = 0
    for case in range(F.RELEASE_FIRST, F.RELEASE_FIRST + RELEASE_BLOCKS * RELEASE_BLOCK):
        p = F.release_case_params(case)
        want = 768 <= p["hn"] <= 1024 and p["b"] * p["vn"] >= 64 and p["vn"] <= 32
        assert release_layout(p["b"], p["h"], p["w"], p["vn"], p["hn"], p["max_num"]).cull == want, p
        assert want == (p["stratum"] in (0, 1) or (p["stratum"] == 3 and want))
        capable += want
    assert 2 * capable >= RELEASE_BLOCKS * RELEASE_BLOCK
