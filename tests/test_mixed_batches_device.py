"""GPU tests of the merged scoring launch (score_exact_kernel_both_*) on the batches the other modules never build: live, empty,
below-min_num and few-pixel images side by side at layouts with culling buffers (768 <= hn <= 1024, b * vn >= 64, vn <= 32), reused
workspaces whose images change kind, ties under the Hilbert permutation, and the per-class vote (ransac_voting_layer_v2) at these layouts.
Inputs: tests/mixed_cases.py; tests/test_mixed_batches_cpu.py pins their layouts and holds the reference side to its own conditions.

The claim under test: no selection and no workspace history ever changes a count.  EVERY call goes through `check`: hypotheses, all hn
counts and the winners torch.equal to literal mode's; literal mode's winners and winner counts equal to the C oracle's (oracle/cref.py);
key-points within 1e-3 px of literal's and literal's within 1e-4 px of the oracle's; status 0 on every live image; exact zeros, S_SKIPPED
and no culling mark on every dead one.

Knob-free, on the RELEASE library, selections through voting.set_cull_selection only, every workspace explicitly zeroed unless the
test is about history."""
import ctypes as C
import os
from typing import NamedTuple

import numpy as np
import pytest
import torch

from oracle import cref, ransac_voting_oracle as O, refkernels
from pvnet_amd import synth, voting
from tests import mixed_cases as M
from tests.test_class_vote_device import assert_equals_definition, materialised

pytestmark = pytest.mark.gpu

HN, THRESH, MIN_NUM = 1024, 0.99, M.MIN_NUM
V2_SEED = 31


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def release_library():
    if any(os.environ.get(k) for k in voting.TUNING_KNOBS):
        pytest.skip("a PVNET_* knob is set in the environment: the front end loads the development build")
    voting.reload_tuning()
    assert b"release build" in voting.load_library().pvnet_vote_build_info()
    voting.set_cull_selection(None)
    yield
    voting.set_cull_selection(None)


def zeroed(b, vn, hn, max_num):
    return torch.zeros(voting.vote_layout(b, M.H, M.W, vn, hn, max_num).total_bytes, dtype=torch.uint8, device=dev())


class Reference(NamedTuple):
    """literal mode on a fresh zeroed workspace and the C oracle, computed once per input and left unchanged"""
    out: np.ndarray
    counts: torch.Tensor
    win: torch.Tensor
    hyp: bytes
    status: np.ndarray
    out_c: np.ndarray
    wi: np.ndarray
    wc: np.ndarray


_REFERENCES = {}


def reference(key, m, v, hn, thresh, max_num, seed, idxs, mask_np, vertex_np) -> Reference:
    """`m`, `v`, `idxs`: the device inputs of the call; `mask_np`, `vertex_np` [b,h,w,vn,2] float32: the same values for the oracle"""
    if key not in _REFERENCES:
        b, vn = v.shape[0], v.shape[3]
        out, d = voting.ransac_voting_layer_v3(m, v, hn, thresh, min_num=MIN_NUM, max_num=max_num, idxs=idxs, seed=seed, literal=True,
                                               return_debug=True, workspace=zeroed(b, vn, hn, max_num), concurrent=False)
        assert d["mode"] == "literal"
        out_c, wi, wc = cref.vote_v3(O.foreground(mask_np), vertex_np, hn, thresh, min_num=MIN_NUM, max_num=max_num, seed=seed,
                                     idxs=None if idxs is None else idxs.cpu().numpy(), return_winners=True)
        _REFERENCES[key] = Reference(out.cpu().numpy().copy(), d["counts"].clone(), d["win"].clone(), d["hyp"].cpu().numpy().tobytes(),
                                     d["status"].cpu().numpy().copy(), out_c, wi, wc)
    return _REFERENCES[key]


def check(out, d, ref: Reference, kinds) -> np.ndarray:
    """the assertions every call of this module must pass; `out` [B,vn,2].  Returns the culling marks [B,vn]."""
    live = np.array([k not in M.DEAD_KINDS for k in kinds])
    dead = ~live
    assert d["mode"] == "exact" and d["layout"].cull == 1
    torch.cuda.synchronize()
    assert d["hyp"].cpu().numpy().tobytes() == ref.hyp, "hypotheses"
    bad = d["counts"] != ref.counts
    assert not bool(bad.any()), f"{int(bad.sum())} counts differ from literal mode's, images {sorted(set(bad.nonzero()[:, 0].tolist()))}"
    assert torch.equal(d["win"], ref.win), "winners"
    wl = ref.win.cpu().numpy()
    assert np.array_equal(wl[live, :, 0], ref.wi[live]) and np.array_equal(wl[live, :, 1], ref.wc[live]), "literal mode against the C oracle"
    o, st, bits = out.cpu().numpy(), d["status"].cpu().numpy(), d["cull_bits"].cpu().numpy()
    assert (st[live] == 0).all() and (ref.status[live] == 0).all(), (st, kinds)
    if live.any():
        px, px_c = float(np.abs(o[live] - ref.out[live]).max()), float(np.abs(ref.out[live] - ref.out_c[live]).max())
        assert px < 1e-3 and px_c < 1e-4, (px, px_c)
    assert (st[dead] == voting.S_SKIPPED).all() and (ref.status[dead] == voting.S_SKIPPED).all()
    assert not o[dead].any() and not ref.out[dead].any() and not bits[dead].any()
    dd = torch.from_numpy(dead).to(out.device)
    assert not bool(d["counts"][dd].any()) and not bool(d["win"][dd].any())
    return bits


# ------------------------------------------------------------------------------------------------------------------------------ v3
class DeviceBatch(NamedTuple):
    bt: M.MixedBatch
    m: torch.Tensor
    v: torch.Tensor       # the planar field's strided view, read in place
    idxs: object


_BATCHES = {}


def device_batch(order, seed, hn=HN) -> DeviceBatch:
    key = (tuple(order), seed, hn)
    if key not in _BATCHES:
        bt = M.mixed_batch(order, M.V3_VN, seed, hn)
        _BATCHES[key] = DeviceBatch(bt, torch.from_numpy(bt.mask).to(dev()), synth.planar_to_vertex_view(torch.from_numpy(bt.planar).to(dev())),
                                    None if bt.idxs is None else torch.from_numpy(bt.idxs).to(dev()))
    return _BATCHES[key]


def on_device(bt: M.MixedBatch) -> DeviceBatch:
    return DeviceBatch(bt, torch.from_numpy(bt.mask).to(dev()), synth.planar_to_vertex_view(torch.from_numpy(bt.planar).to(dev())), None)


def vote(db: DeviceBatch, hn=HN, thresh=THRESH, ws=None, concurrent=False):
    bt = db.bt
    ws = zeroed(len(bt.kinds), M.V3_VN, hn, bt.max_num) if ws is None else ws
    return voting.ransac_voting_layer_v3(db.m, db.v, hn, thresh, min_num=MIN_NUM, max_num=bt.max_num, idxs=db.idxs, seed=bt.call_seed,
                                         return_debug=True, workspace=ws, concurrent=concurrent)


def v3_reference(db: DeviceBatch, key, hn=HN, thresh=THRESH) -> Reference:
    bt = db.bt
    return reference(("v3", key, hn, thresh), db.m, db.v, hn, thresh, bt.max_num, bt.call_seed, db.idxs, bt.mask,
                     synth.planar_to_vertex_view(bt.planar))


def under_every_selection(db: DeviceBatch, key, hn=HN, thresh=THRESH):
    ref = v3_reference(db, key, hn, thresh)
    live = np.array([k not in M.DEAD_KINDS for k in db.bt.kinds])
    try:
        for sel in (None, "all", "none"):
            voting.set_cull_selection(sel)
            for conc in (False, True):
                out, d = vote(db, hn, thresh, concurrent=conc)
                assert d["concurrent"] == conc
                bits = check(out, d, ref, db.bt.kinds)
                if sel == "all":
                    assert (bits[live] == 1).all(), (sel, conc, bits)      # exactly the live images (check: none of the dead)
                elif sel == "none":
                    assert not bits.any()
    finally:
        voting.set_cull_selection(None)


@pytest.mark.parametrize("index", range(M.N_PERMUTATIONS))
def test_v3_mixed_batch_under_every_selection(index):
    """1. eight of the eleven kinds in a seeded order, `empty` and `below_min` always among them (index 0 starts with a dead image, index
    1 ends with one): selections None / "all" / "none", alone and with the in-flight hint"""
    under_every_selection(device_batch(M.permutation(index), index), index)


@pytest.mark.parametrize("index", M.HN_PERMUTATIONS)
def test_v3_mixed_batch_with_padding_hypotheses(index):
    """1. hn = 1000: padding columns inside the last tile of 32"""
    under_every_selection(device_batch(M.permutation(index), index, M.HN_PADDED), index, hn=M.HN_PADDED)


@pytest.mark.parametrize("thresh", [0.9, 0.999])
@pytest.mark.parametrize("index", M.THRESH_PERMUTATIONS)
def test_v3_mixed_batch_at_other_thresholds(index, thresh):
    under_every_selection(device_batch(M.permutation(index), index), index, thresh=thresh)


def snapshot(out, d):
    torch.cuda.synchronize()
    return out.clone(), d["counts"].clone(), d["win"].clone(), d["status"].clone(), d["cull_bits"].clone()


def test_workspace_history_never_changes_a_result():
    """2. ONE workspace through batches whose every slot changes kind -- live to dead, culled to dense, a batch of empty images between --
    each call equal to the same call on a fresh zeroed workspace: stale perm / cnts / hyps / hypc, culling marks and band origins of images
    that are dead now, the batch gate decided by the call before"""
    index = M.HISTORY_PERMUTATION
    x = device_batch(M.permutation(index), index)
    xr = on_device(M.rolled(x.bt))
    empty = on_device(M.mixed_batch(("empty",) * M.V3_B, M.V3_VN, 99))
    assert empty.bt.max_num == 30000 and x.bt.max_num == M.THIN_MAX_NUM
    ws = zeroed(M.V3_B, M.V3_VN, HN, x.bt.max_num)
    # (the empty batch is voted with the workspace's max_num, so that the layout -- and with it the gate's fingerprint -- stays)
    empty = DeviceBatch(empty.bt._replace(max_num=x.bt.max_num), empty.m, empty.v, None)
    refs = {id(x): v3_reference(x, index), id(xr): v3_reference(xr, ("rolled", index)), id(empty): v3_reference(empty, "empty")}
    steps = [(x, "all"), (xr, "all"), (xr, None), (empty, None), (x, None), (xr, "all"), (x, "none"), (x, None), (x, None)]
    marks = []
    try:
        for db, sel in steps:
            voting.set_cull_selection(sel)
            out, d = vote(db, ws=ws)
            check(out, d, refs[id(db)], db.bt.kinds)
            got = snapshot(out, d)
            fresh = snapshot(*vote(db))
            for a, c, what in zip(got[:4], fresh[:4], ("key-points", "counts", "winners", "status")):
                assert torch.equal(a, c), (what, db.bt.kinds, sel)
            if db is empty:
                assert not got[0].any() and not got[1].any() and (got[3] == voting.S_SKIPPED).all() and not got[4].any()
            marks.append((int(got[4].sum()), int(fresh[4].sum())))
    finally:
        voting.set_cull_selection(None)
    print("culling marks per step (history workspace, fresh workspace):", marks)
    live = sum(k not in M.DEAD_KINDS for k in x.bt.kinds) * M.V3_VN
    assert marks[0] == (live, live) and marks[1] == (live, live) and marks[6][0] == 0


def test_ties_first_caller_index_wins_under_the_hilbert_permutation():
    """3. a clean disc whose hypotheses nearly all collect every pixel, 40 of them identical: K5 returns a culled key-point's counts from
    Hilbert order to caller order and the smallest tied CALLER index must win, as in the C oracle"""
    db = device_batch(M.TIES_ORDER, M.TIES_SEED)
    ref = v3_reference(db, "ties")
    t = db.bt.kinds.index("ties")
    slots = M.tie_slots(HN)
    assert (ref.wi[t] == M.TIE_FIRST).all() and (ref.wc[t] == int((db.bt.mask[t] != 0).sum())).all()
    try:
        for sel in ("all", "none", None):
            voting.set_cull_selection(sel)
            out, d = vote(db)
            bits = check(out, d, ref, db.bt.kinds)
            win, counts = d["win"][t].cpu().numpy(), d["counts"][t].cpu().numpy()
            assert np.array_equal(win[:, 0], ref.wi[t]) and np.array_equal(win[:, 1], ref.wc[t])
            assert (counts[:, slots] == ref.wc[t][:, None]).all() and (counts[:, :M.TIE_FIRST] < ref.wc[t][:, None]).all()
            if sel == "all":
                assert bits[t].all()
                perm = d["perm"][t].cpu().numpy()
                scrambled = 0
                for k in range(M.V3_VN):
                    tied = np.flatnonzero(counts[k] == counts[k].max())
                    first_sorted = perm[k][np.isin(perm[k], tied)][0]
                    scrambled += int(first_sorted != tied.min())
                # the inputs bite: "the first tied hypothesis in sorted order wins" would name another winner (the draws are fixed: 9 of 9)
                print(f"key-points whose first tied hypothesis in Hilbert order is not the smallest caller index: {scrambled} of {M.V3_VN}")
                assert scrambled > 0
            elif sel == "none":
                assert not bits.any()
    finally:
        voting.set_cull_selection(None)


# ------------------------------------------------------------------------------------------------------------------------------ v2
_LABELS = {}


def label_case(case, changed=False):
    key = (case, changed)
    if key not in _LABELS:
        b, cn, vn = case
        _LABELS[key] = M.label_batch(b, cn, vn, M.v2_present_changed() if changed else M.v2_present(case), seed=cn)
    return _LABELS[key]


def v2_reference(key, labels_t, field_t, cn) -> Reference:
    """literal v3 and the C oracle on the materialised batch; a half field is read by the oracle widened to float32"""
    masks, rep = materialised(labels_t, field_t, cn)
    masks = masks.to(torch.uint8)
    return reference(("v2",) + key, masks, rep, HN, THRESH, 30000, V2_SEED, None, masks.cpu().numpy(), rep.float().cpu().numpy())


def v2_checked(case, lb, labels_t, field_t, key, selections=(None, "all")):
    b, cn, vn = case
    kinds = lb.kinds.reshape(-1)
    live = np.array([k not in M.DEAD_KINDS for k in kinds])
    ref = v2_reference(key, labels_t, field_t, cn)
    try:
        for sel in selections:
            voting.set_cull_selection(sel)
            out, dbg = assert_equals_definition(labels_t, field_t, cn, HN, max_num=30000, thresh=THRESH, seed=V2_SEED)
            bits = check(out.view(b * (cn - 1), vn, 2), dbg, ref, kinds)
            if sel == "all":
                assert (bits[live] == 1).all()
    finally:
        voting.set_cull_selection(None)


@pytest.mark.parametrize("case", M.V2_CASES)
def test_v2_at_culling_layouts_against_its_definition_and_the_oracle(case):
    """4. classes of label images as virtual images, most of them absent and between the present ones: equal to v3 on the materialised
    batch (tests/test_class_vote_device.py's comparison) AND held to literal mode and the C oracle, under the library's selection and "all" """
    lb = label_case(case)
    labels = torch.from_numpy(lb.labels).to(dev())
    field = torch.from_numpy(lb.field).to(dev())
    v2_checked(case, lb, labels, field, (case, "float32"))


@pytest.mark.parametrize("ldt", [torch.uint8, torch.int32])
def test_v2_other_label_types(ldt):
    case = M.V2_CASES[0]
    lb = label_case(case)
    labels = torch.from_numpy(lb.labels).to(dev()).to(ldt)    # uint8: -1 wraps to 255, still nobody's
    assert bool((labels == (255 if ldt == torch.uint8 else -1)).any())
    v2_checked(case, lb, labels, torch.from_numpy(lb.field).to(dev()), (case, "float32"))


@pytest.mark.parametrize("fdt", [torch.bfloat16, torch.float16])
def test_v2_half_precision_fields(fdt):
    case = M.V2_CASES[0]
    lb = label_case(case)
    field = torch.from_numpy(lb.field).to(dev()).to(fdt)
    v2_checked(case, lb, torch.from_numpy(lb.labels).to(dev()), field, (case, str(fdt)))


def test_v2_second_call_on_a_workspace_equals_the_first():
    """4. the batch gate divides the images that voted for culling by ALL images of the call, dead ones included: with ten of thirteen
    classes absent it closes behind the first call on a workspace, so the second call scores densely what the first culled.  Bit for bit
    the same result.  Recorded, not asserted: the sum of cull_bits over the 26 x 3 key-points was 15 in the first call
    (the five clean live classes) and 0 in the second."""
    case = M.V2_CASES[0]
    b, cn, vn = case
    lb = label_case(case)
    labels, field = torch.from_numpy(lb.labels).to(dev()), torch.from_numpy(lb.field).to(dev())
    ref = v2_reference((case, "float32"), labels, field, cn)
    ws = zeroed(b * (cn - 1), vn, HN, 30000)
    got = []
    for _ in range(2):
        out, d = voting.ransac_voting_layer_v2(labels, field, cn, HN, THRESH, min_num=MIN_NUM, max_num=30000, seed=V2_SEED, return_debug=True,
                                               workspace=ws)
        check(out.view(-1, vn, 2), d, ref, lb.kinds.reshape(-1))
        got.append(snapshot(out, d) + (d["hyp"].clone(),))
    for a, c in zip(got[0][:4] + got[0][5:], got[1][:4] + got[1][5:]):
        assert torch.equal(a, c)
    print(f"cull_bits sum: first call {int(got[0][4].sum())}, second call {int(got[1][4].sum())} of {b * (cn - 1) * vn} key-points")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_v2_from_logits_at_a_culling_layout(dt):
    """5. the fused arg-max, logits with ties and a NaN: the two-step call's result, and through `check` as well"""
    case = M.V2_CASES[0]
    b, cn, vn = case
    lb = label_case(case)
    rng = np.random.default_rng(5)
    seg = rng.standard_normal((b, cn, M.H, M.W)).astype(np.float32)
    lab = np.where((lb.labels >= 1) & (lb.labels < cn), lb.labels, 0)
    np.put_along_axis(seg, lab[:, None], 10.0, axis=1)
    r = M.STRAY_ROW                                    # nobody's pixels: the classes keep their kinds
    seg[0, :, r, 20] = 0.25                            # a tie of all classes: the background
    seg[0, :, r, 21] = 0.0
    seg[0, 1:3, r, 21] = 3.0                           # a two-way tie: class 1 (absent from image 0: one pixel, below min_num)
    seg[0, :, r, 22] = 0.0
    seg[0, 2, r, 22], seg[0, 9, r, 22] = np.nan, 9.0   # a NaN counts as the maximum: class 2
    s = torch.from_numpy(seg).to(dev()).to(dt)
    labels = torch.argmax(s, 1)
    assert labels[0, r, 20:23].tolist() == [0, 1, 2]
    field = torch.from_numpy(lb.field).to(dev())
    kw = dict(min_num=MIN_NUM, max_num=30000, seed=V2_SEED, return_debug=True)
    a, da = voting.ransac_voting_layer_v2_from_logits(s, field, HN, THRESH, workspace=zeroed(b * (cn - 1), vn, HN, 30000), **kw)
    c, dc = voting.ransac_voting_layer_v2(labels, field, cn, HN, THRESH, workspace=zeroed(b * (cn - 1), vn, HN, 30000), **kw)
    torch.cuda.synchronize()
    assert torch.equal(a, c) and torch.equal(da["status"], dc["status"]) and torch.equal(da["counts"], dc["counts"])
    assert torch.equal(da["win"], dc["win"]) and torch.equal(da["hyp"], dc["hyp"]) and torch.equal(da["bits"], dc["bits"])
    ref = v2_reference((case, "logits", str(dt)), labels, field, cn)
    check(a.view(-1, vn, 2), da, ref, lb.kinds.reshape(-1))


def test_epilogues_per_class_at_a_culling_layout():
    """6. vote_confidence and pvnet_vote_distribution on the per-class debug dict, culled key-points present, against the numpy oracle
    on the materialised masks; dead virtual images: confidence 0 and the reference's substitute covariance (zero hypotheses, ratio one)"""
    case = M.V2_CASES[0]
    b, cn, vn = case
    B = b * (cn - 1)
    lb = label_case(case)
    kinds = lb.kinds.reshape(-1)
    live = np.array([k not in M.DEAD_KINDS for k in kinds])
    labels, field = torch.from_numpy(lb.labels).to(dev()), torch.from_numpy(lb.field).to(dev())
    try:
        voting.set_cull_selection("all")
        out, dbg = voting.ransac_voting_layer_v2(labels, field, cn, HN, THRESH, min_num=MIN_NUM, max_num=30000, seed=V2_SEED, return_debug=True,
                                                 workspace=zeroed(B, vn, HN, 30000))
    finally:
        voting.set_cull_selection(None)
    check(out.view(B, vn, 2), dbg, v2_reference((case, "float32"), labels, field, cn), kinds)
    assert bool(dbg["cull_bits"].any())
    masks = M.materialised_masks(lb.labels, cn)
    rep = np.repeat(lb.field, cn - 1, axis=0)
    pts = out.view(B, vn, 2)
    conf = voting.vote_confidence(dbg, pts, 0.999).cpu().numpy()
    want = O.vote_confidence(masks, rep, pts.cpu().numpy(), 0.999, dtype=np.float32)
    np.testing.assert_allclose(conf[live], want[live], atol=1e-6)
    assert (conf[live] > 0.05).all() and (conf[~live] == 0).all()
    mean = pts.clone()
    mean[torch.from_numpy(~live).to(dev())] = torch.tensor([3.0, -2.0], device=dev())     # the substitute covariance is not zero
    cov = torch.empty((B, vn, 2, 2), dtype=torch.float32, device=dev())
    voting._check(voting.load_library().pvnet_vote_distribution(C.c_void_p(mean.data_ptr()), C.c_void_p(cov.data_ptr()),
                                                                *voting._ws_tail(dbg["layout"], 30000, dbg["workspace"])), "distribution")
    torch.cuda.synchronize()
    ref = O.estimate_voting_distribution_with_mean(masks, rep, mean.cpu().numpy(), HN, THRESH, min_num=MIN_NUM, seed=V2_SEED, dtype=np.float32)
    np.testing.assert_allclose(cov.cpu().numpy(), ref, rtol=1e-4, atol=1e-5)
    assert np.abs(ref[~live]).min() > 1.0


@pytest.mark.skipif(not refkernels.available("off"), reason="oracle/_ref (the reference's kernels compiled for gfx950) not built")
def test_mixed_batch_counts_equal_the_references_own_kernel():
    """7. the reference's voting_for_hypothesis_kernel itself on every live image's compacted records and hypotheses, every key-point culled"""
    index = M.REF_KERNEL_PERMUTATION
    db = device_batch(M.permutation(index), index)
    try:
        voting.set_cull_selection("all")
        out, d = vote(db)
    finally:
        voting.set_cull_selection(None)
    check(out, d, v3_reference(db, index), db.bt.kinds)
    for bi, kind in enumerate(db.bt.kinds):
        if kind in M.DEAD_KINDS:
            continue
        assert bool(d["cull_bits"][bi].all())
        tn = int(d["tn"][bi])
        rec = d["rec"][bi, :, :tn]
        inl = refkernels.voting_for_hypothesis(rec[:, :, 2:4].permute(1, 0, 2).contiguous(), rec[0, :, 0:2].contiguous(),
                                               d["hyp"][bi].permute(1, 0, 2).contiguous(), THRESH)
        assert torch.equal(d["counts"][bi].T, inl.sum(2, dtype=torch.int32)), (bi, kind)


def test_v2_graph_capture_at_a_culling_layout():
    """8. the per-class call captured on a caller-owned workspace with static label and field tensors (a linear graph): three replays,
    another label batch copied in before the third (one class appears, one vanishes), each bitwise equal to the eager call on the same
    inputs on a fresh workspace"""
    case = M.V2_CASES[0]
    b, cn, vn = case
    B = b * (cn - 1)
    first, second = label_case(case), label_case(case, changed=True)
    assert not np.array_equal(first.labels, second.labels)
    labels = torch.from_numpy(first.labels).to(dev())
    field = torch.from_numpy(first.field).to(dev())
    L = voting.vote_layout(B, M.H, M.W, vn, HN, 30000)
    ws = zeroed(B, vn, HN, 30000)
    out = torch.zeros((b, cn - 1, vn, 2), dtype=torch.float32, device=dev())
    kw = dict(min_num=MIN_NUM, max_num=30000, seed=V2_SEED)

    def eager(lab):
        o, d = voting.ransac_voting_layer_v2(lab, field, cn, HN, THRESH, return_debug=True, workspace=zeroed(B, vn, HN, 30000), **kw)
        torch.cuda.synchronize()
        return o.clone(), d["counts"].clone(), d["win"].clone()

    def enqueue():
        voting.ransac_voting_layer_v2(labels, field, cn, HN, THRESH, workspace=ws, out=out, **kw)

    want_first, want_second = eager(labels), eager(torch.from_numpy(second.labels).to(dev()))
    assert not torch.equal(want_first[0], want_second[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enqueue()   # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    out.zero_()
    ws.zero_()
    views = voting._debug_views(ws, L)
    for replay, want in enumerate((want_first, want_first, want_second)):
        if replay == 2:
            labels.copy_(torch.from_numpy(second.labels).to(dev()))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[0]), replay
        assert torch.equal(views["counts"], want[1]) and torch.equal(views["win"], want[2]), replay
