"""The oracle and the HIP path against fixtures G6L / G7L = the reference's OWN ransac_voting_layer_v3 and its siblings, executed line by
line by oracle/ref_driver.py (tests/golden/make_golden.py) at the shapes where the RELEASE library does something else than at G6's:

  A  b 8, vn 9, hn 1024, 96 x 128, clean and noisy images alternating -- a disc-culling layout, both scoring bodies in one call, ties
  B  b 6, vn 12, hn 800, 72 x 96, one image of three pixels          -- vn != 9, padding hypotheses through the sort, a dead image
  C  b 8, vn 8, hn 768, thinned by max_num                            -- b * vn == 64, the lower edge of the hn range
  D  b 2, 480 x 640, radius 40, hn 1024                               -- BASELINE configs[2]'s shape, scored densely
  E  the demo's cat mask, hn 512, b 1                                 -- the reference's tools/demo.py:55

The fixtures hold the reference's key-points, its draws, its first-index winners with their counts, and a sha256 per image of its
hypotheses and of its inlier counts.  CPU tests: the numpy oracle (float32 arithmetic, float64 least squares) fed the recorded draws
reproduces all of that, so its ARRAYS stand for the reference's; GPU tests: the device arrays equal the oracle's, in every scoring mode and
under every culling selection, and the key-points lie within 1e-3 px of the reference's."""
import ctypes as C
import functools
import hashlib
import importlib.util
import os
from typing import NamedTuple

import numpy as np
import pytest

from oracle import ransac_voting_oracle as O
from oracle import ref_driver, refkernels

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

# as tests/test_reference_driver.py: the reference's float32 un-centred normal equations carry ~1e-4..2e-3 px of rounding noise
TOL_REF_PX = 1e-3
# input condition: the reference alone may use half of the bar (its distance to the float64 oracle); the device keeps the other half
HALF_BAR_PX = 0.5e-3
CASES = tuple(MG.REF_DRIVER_LAYOUT_CASES)
CULL_CASES = ("A", "B", "C")
SIZE_CAP = 515588   # bytes: the largest fixture committed before these (head_metrics.npz); no new file may exceed it
CONF_EDGE_PIXELS = 2.0   # as tests/test_reference_driver.py: pixels of ~100 whose vote may differ 1e-3 px from the reference's point


def sha(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).digest()


class CaseData(NamedTuple):
    name: str
    case: dict
    mask: np.ndarray      # [b,h,w] int64, as the reference run got it
    vertex: np.ndarray    # [b,h,w,vn,2] strided view
    keep: np.ndarray      # [b,h,w] bool: the pixels the reference kept (all foreground where it did not thin)
    idxs: np.ndarray      # [b,hn,vn,2] int32, zeros on dead images
    live: list
    fix: dict


@functools.lru_cache(maxsize=None)
def case_data(name) -> CaseData:
    case = MG.REF_DRIVER_LAYOUT_CASES[name]
    fix = dict(np.load(MG.layout_fixture_path(name)))
    mask, vertex, _ = MG.ref_driver_layout_inputs(case)
    b, h, w = mask.shape
    keep = np.unpackbits(fix["keep_bits"])[:b * h * w].reshape(b, h, w).astype(bool)
    live = fix["live"].tolist()
    idxs = np.zeros((b, case["hn"], case["vn"], 2), np.int32)
    idxs[live] = fix["idxs"]
    return CaseData(name, case, mask, vertex, keep, idxs, live, fix)


class Oracle(NamedTuple):
    out32: np.ndarray     # float32 arithmetic, float64 least squares
    out64: np.ndarray     # float64 throughout
    out32_lsq32: np.ndarray   # float32 arithmetic and the reference's un-centred float32 sums
    hyp: np.ndarray       # [b,hn,vn,2] float32 (oracle32), zeros on dead images
    counts: np.ndarray    # [b,hn,vn] int32
    win64: np.ndarray     # [b,vn] the float64 oracle's winners


@functools.lru_cache(maxsize=None)
def oracle(name) -> Oracle:
    """computed once per case and left unchanged"""
    cd = case_data(name)
    kw = dict(cd.case["kw"])
    thresh = kw.pop("inlier_thresh")
    b, hn, vn = cd.mask.shape[0], cd.case["hn"], cd.case["vn"]
    run = functools.partial(O.ransac_voting_layer_v3, cd.mask, cd.vertex, hn, inlier_thresh=thresh, idxs=cd.idxs, keep=cd.keep,
                            return_debug=True, **kw)
    out32, d32 = run(dtype=np.float32, lsq_dtype=np.float64)
    out64, d64 = run(dtype=np.float64, lsq_dtype=np.float64)
    hyp, counts = np.zeros((b, hn, vn, 2), np.float32), np.zeros((b, hn, vn), np.int32)
    win64, lsq32 = np.zeros((b, vn), np.int64), np.zeros((b, vn, 2), np.float32)
    for bi in cd.live:
        d = d32[bi]
        assert d["hyp"].dtype == np.float32
        hyp[bi], counts[bi], win64[bi] = d["hyp"], d["counts"], d64[bi]["win_idx"]
        lsq32[bi] = O.refine(d["direct"], d["coords"], d["win_pts"], thresh, np.float32, np.float32)[0]
    assert [d["tn"] for d in d32 if d["tn"] > 0] == cd.fix["tn"].tolist()
    return Oracle(out32, out64, lsq32, hyp, counts, win64)


# ------------------------------------------------------------------------------------------------------------------ the comparers
def first_index_winners(counts):
    """counts [b,hn,vn] -> winners in the device's layout [b,vn,2] = (index, count), the smallest index among ties"""
    return np.stack([counts.argmax(axis=1), counts.max(axis=1)], axis=-1).astype(np.int32)


def compare_integers(name, hyp, counts, win):
    """numpy arrays in the device's layout -- hyp [b,vn,hn,2] float32, counts [b,vn,hn], win [b,vn,2] -- against the oracle32 arrays
    (which the digests tie to the reference's own, see the CPU test below) and the reference's recorded winners"""
    cd, orc = case_data(name), oracle(name)
    for j, bi in enumerate(cd.live):
        assert np.ascontiguousarray(hyp[bi].transpose(1, 0, 2)).tobytes() == orc.hyp[bi].tobytes(), (name, bi, "hypotheses")
        bad = counts[bi].T != orc.counts[bi]
        assert not bad.any(), (name, bi, f"{int(bad.sum())} of {bad.size} counts differ")
        assert np.array_equal(win[bi, :, 0], cd.fix["win_idx"][j]), (name, bi, "winners", win[bi, :, 0], cd.fix["win_idx"][j])
        assert np.array_equal(win[bi, :, 1], cd.fix["win_cnt"][j]), (name, bi, "winner counts")
    dead = [bi for bi in range(cd.mask.shape[0]) if bi not in cd.live]
    assert not counts[dead].any() and not win[dead].any(), (name, "dead images")


def compare_keypoints(name, out, bar=TOL_REF_PX):
    """key-points [b,vn,2] against the reference's; returns the distance"""
    cd = case_data(name)
    dead = [bi for bi in range(cd.mask.shape[0]) if bi not in cd.live]
    assert not out[dead].any() and not cd.fix["out"][dead].any()          # fewer than min_num pixels: zeros (:531-534)
    px = float(np.abs(out[cd.live] - cd.fix["out"][cd.live]).max())
    assert px < bar, (name, px)
    return px


def oracle_in_device_layout(name):
    orc = oracle(name)
    return orc.hyp.transpose(0, 2, 1, 3).copy(), orc.counts.transpose(0, 2, 1).copy(), first_index_winners(orc.counts)


# ------------------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_executed_reference_driver(name):
    cd, orc = case_data(name), oracle(name)
    px32, px64 = compare_keypoints(name, orc.out32), compare_keypoints(name, orc.out64)
    hyp, counts, win = oracle_in_device_layout(name)
    compare_integers(name, hyp, counts, win)
    for j, bi in enumerate(cd.live):                      # the oracle's arrays ARE the reference's: the same bytes
        assert sha(orc.hyp[bi], np.float32) == cd.fix["hyp_sha"][j].tobytes(), (name, bi)
        assert sha(orc.counts[bi], np.int32) == cd.fix["cnt_sha"][j].tobytes(), (name, bi)
        assert np.array_equal(orc.win64[bi], cd.fix["win_idx"][j]), (name, bi, "float64 oracle's winners")
    assert cd.fix["rounds"].tolist() == [1] * len(cd.live)
    # recorded, not asserted: with the reference's un-centred float32 sums the oracle shares the reference's noise floor
    lsq32 = float(np.abs(orc.out32_lsq32[cd.live] - cd.fix["out"][cd.live]).max())
    print(f"case {name}: |reference - oracle32/float64 LSQ| {px32:.2e} px, |reference - oracle64| {px64:.2e} px, "
          f"|reference - oracle32/float32 LSQ| {lsq32:.2e} px")
    assert px64 <= HALF_BAR_PX, (name, px64)              # the input condition


def test_case_contents_are_what_the_table_says():
    a, b, c = case_data("A"), case_data("B"), case_data("C")
    ties = []
    for bi in a.live:                                     # clean images: many hypotheses collect every pixel
        cnt = oracle("A").counts[bi]
        ties.append(int((cnt == cnt.max(axis=0)).sum(axis=0).min()))
    assert all(t > 1 for t in ties[0::2]), ties
    assert b.live == [0, 1, 3, 4, 5] and int((b.mask[2] != 0).sum()) == 3
    assert b.case["hn"] % 32 == 0 and b.case["hn"] < 1024 and b.case["vn"] != 9
    assert c.case["b"] * c.case["vn"] == 64 and c.case["hn"] == 768
    tn0 = (c.mask != 0).sum(axis=(1, 2))
    assert (c.fix["tn"] < 0.6 * tn0).all() and (c.fix["tn"] > 0.4 * tn0).all()      # thinned to about half (:537-540)
    d, e = case_data("D"), case_data("E")
    assert d.mask.shape == (2, 480, 640) and d.case["hn"] == 1024 and e.mask.shape == (1, 480, 640) and e.case["hn"] == 512


def release_layout(b, h, w, vn, hn, max_num=30000):
    """pvnet_vote_layout of the RELEASE library, whatever the environment holds (as tests/test_library_cpu.py)"""
    from pvnet_amd import voting
    L = voting.Layout()
    assert C.CDLL(voting.LIB_PATH).pvnet_vote_layout(b, h, w, vn, hn, max_num, C.byref(L)) == 0
    return L


@pytest.mark.parametrize("name", CASES)
def test_release_layout_of_every_case(name):
    cd = case_data(name)
    b, h, w = cd.mask.shape
    L = release_layout(b, h, w, cd.case["vn"], cd.case["hn"])
    assert L.cull == (1 if name in CULL_CASES else 0), name
    if name in CULL_CASES:
        assert L.hn_pad == 1024


def expect_failure(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return
    raise AssertionError("the comparer accepted a wrong kernel's output")


def test_comparers_reject_counts_left_in_sorted_order():
    """a culled key-point's counts come back in the order of its sorted hypotheses: `perm` not undone"""
    hyp, counts, win = oracle_in_device_layout("A")
    bi, k = 0, 3
    perm = np.lexsort((hyp[bi, k, :, 1], hyp[bi, k, :, 0]))         # a spatial order of the hypotheses
    assert not np.array_equal(perm, np.arange(perm.size))
    counts[bi, k] = counts[bi, k][perm]
    expect_failure(compare_integers, "A", hyp, counts, win)


def test_comparers_reject_a_last_index_tie_break():
    hyp, counts, win = oracle_in_device_layout("A")
    hn = counts.shape[2]
    win[..., 0] = hn - 1 - counts[:, :, ::-1].argmax(axis=2)
    assert (win[0::2, :, 0] != first_index_winners(oracle("A").counts)[0::2, :, 0]).all()    # every clean key-point is tied
    expect_failure(compare_integers, "A", hyp, counts, win)
    compare_integers("A", *oracle_in_device_layout("A"))


def test_comparers_reject_a_winning_padding_hypothesis():
    """B has hn 800 of hn_pad 1024: the arg-max must never look at the 224 padding columns"""
    cd = case_data("B")
    hyp, counts, win = oracle_in_device_layout("B")
    bi, k = cd.live[-1], cd.case["vn"] - 1
    padded = np.zeros(1024, np.int32)
    padded[:cd.case["hn"]] = counts[bi, k]
    padded[900] = counts[bi, k].max() + 1
    win[bi, k] = (padded.argmax(), padded.max())
    expect_failure(compare_integers, "B", hyp, counts, win)


def test_comparers_reject_a_shifted_keypoint_and_a_live_dead_image():
    cd = case_data("B")
    out = cd.fix["out"].copy()
    out[0, 0, 0] += 2 * TOL_REF_PX
    expect_failure(compare_keypoints, "B", out)
    out = cd.fix["out"].copy()
    out[2, 0, 0] = 1e-6
    expect_failure(compare_keypoints, "B", out)


# --- G7L
@functools.lru_cache(maxsize=None)
def sibling_data():
    a = case_data("A")
    sib = {s: dict(np.load(MG.layout_fixture_path("sib_" + s))) for s in MG.LAYOUT_SIBLINGS}
    b, h, w = a.mask.shape
    keep5 = np.unpackbits(sib["v5"]["keep_bits"])[:b * h * w].reshape(b, h, w).astype(bool)
    idxs = {s: sib[s]["idxs"].astype(np.int32) for s in sib}
    _, dbg = O.ransac_voting_layer_v3(a.mask, a.vertex, a.case["hn"], inlier_thresh=0.99, idxs=idxs["gh"], dtype=np.float32,
                                      return_debug=True)
    gh_hyp = np.stack([d["hyp"].astype(np.float32) for d in dbg])
    gh_counts = np.stack([d["counts"] for d in dbg]).astype(np.int64)
    return sib, keep5, idxs, gh_hyp, gh_counts


def test_oracle_reproduces_the_reference_siblings_at_hn_1024():
    a = case_data("A")
    sib, keep5, idxs, gh_hyp, gh_counts = sibling_data()
    b, hn, vn = a.mask.shape[0], a.case["hn"], a.case["vn"]
    v5, dist, gh = sib["v5"], sib["dist"], sib["gh"]
    # v5 (:763-858): thinned to ~max_num=100 pixels by the reference's own draw; points and confidence at 0.999
    assert (v5["tn"] < 160).all() and (v5["tn"] > 50).all()
    pts = O.ransac_voting_layer_v3(a.mask * keep5, a.vertex, hn, inlier_thresh=0.99, idxs=idxs["v5"], dtype=np.float32)
    px = float(np.abs(pts - v5["pts"]).max())
    assert px < TOL_REF_PX
    conf = O.vote_confidence(a.mask * keep5, a.vertex, v5["pts"], 0.999, dtype=np.float32)
    assert np.abs(conf - v5["conf"]).max() < 1e-6
    # distribution about a given mean (:333-406): 4 rounds of 256 independent pairs = one draw of 1024
    assert int(dist["rounds"]) == 4 and idxs["dist"].shape == (b, 1024, vn, 2)
    cov = O.estimate_voting_distribution_with_mean(a.mask, a.vertex, dist["mean"], 1024, inlier_thresh=0.99, idxs=idxs["dist"],
                                                   dtype=np.float32)
    cov_err = float(np.abs(cov - dist["cov"]).max())
    assert cov_err < 1e-3 * max(1.0, np.abs(dist["cov"]).max())
    # Python-level generate_hypothesis (:983-1034): every hypothesis and its inlier count, through their digests
    for bi in range(b):
        assert sha(gh_hyp[bi], np.float32) == gh["hyp_sha"][bi].tobytes()
        assert sha(gh_counts[bi], np.int32) == gh["cnt_sha"][bi].tobytes()
    print(f"siblings on A: v5 tn {v5['tn'].tolist()} |pts - reference| {px:.2e} px, |cov - reference| {cov_err:.2e}")


@pytest.mark.skipif(not ref_driver.available(), reason="needs the reference tree (build container only)")
def test_fixture_is_what_the_reference_driver_returns_today():
    rec, fix = MG.layout_case_record("A"), case_data("A").fix
    assert sorted(rec) == sorted(fix)
    for k in rec:
        assert rec[k].dtype == fix[k].dtype and np.array_equal(rec[k], fix[k]), k


def test_every_new_fixture_is_within_the_size_cap():
    for n in list(CASES) + ["sib_" + s for s in MG.LAYOUT_SIBLINGS]:
        assert os.path.getsize(MG.layout_fixture_path(n)) <= SIZE_CAP, n
    assert all(case_data(n).fix["idxs"].dtype == np.uint16 for n in CASES)


# ------------------------------------------------------------------------------------------------------------------------ GPU tests
def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def release_library():
    from pvnet_amd import voting
    if any(os.environ.get(k) for k in voting.TUNING_KNOBS):
        pytest.skip("a PVNET_* knob is set in the environment: the front end loads the development build")
    voting.reload_tuning()
    assert b"release build" in voting.load_library().pvnet_vote_build_info()
    voting.set_cull_selection(None)
    yield voting
    voting.set_cull_selection(None)


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    """the reference's own thinning decisions are applied to the mask (as G6 case 2): max_num stays at the default"""
    import torch
    cd = case_data(name)
    return (torch.from_numpy(cd.mask * cd.keep).to(dev()), torch.from_numpy(np.ascontiguousarray(cd.vertex)).to(dev()),
            torch.from_numpy(cd.idxs).to(dev()))


def vote(voting, name, ws=None, literal=False):
    import torch
    cd = case_data(name)
    m, v, idxs = device_inputs(name)
    b, h, w = cd.mask.shape
    if ws is None:
        ws = torch.zeros(voting.vote_layout(b, h, w, cd.case["vn"], cd.case["hn"], 30000).total_bytes, dtype=torch.uint8, device=dev())
    out, d = voting.ransac_voting_layer_v3(m, v, cd.case["hn"], inlier_thresh=cd.case["kw"]["inlier_thresh"], idxs=idxs, literal=literal,
                                           return_debug=True, workspace=ws, concurrent=False)
    assert d["mode"] == ("literal" if literal else "exact")
    torch.cuda.synchronize()
    return out, d, ws


def check_call(name, out, d):
    """every assertion of test 1 on one call; returns (px to the reference, culled key-points)"""
    cd = case_data(name)
    compare_integers(name, d["hyp"].cpu().numpy(), d["counts"].cpu().numpy(), d["win"].cpu().numpy())
    px = compare_keypoints(name, out.cpu().numpy())
    bits = d["cull_bits"].cpu().numpy()
    dead = [bi for bi in range(cd.mask.shape[0]) if bi not in cd.live]
    assert not bits[dead].any()
    assert d["layout"].cull == (1 if name in CULL_CASES else 0)
    return px, bits


def own_selection_twice(voting, name):
    """exact mode under the library's own selection, twice on ONE zeroed workspace: the second call follows the first call's history"""
    voting.set_cull_selection(None)
    got, ws = [], None
    for _ in range(2):
        out, d, ws = vote(voting, name, ws)
        got.append(check_call(name, out, d))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_path_reproduces_the_executed_reference_driver_in_every_mode(name, release_library):
    voting = release_library
    cd = case_data(name)
    nlive = len(cd.live) * cd.case["vn"]
    figures, sorted_away = {}, 0
    try:
        out, d, _ = vote(voting, name, literal=True)
        px, bits = check_call(name, out, d)
        assert not bits.any()
        figures["literal"] = (px, 0)
        for sel in ("none", "all"):
            voting.set_cull_selection(sel)
            out, d, _ = vote(voting, name)
            px, bits = check_call(name, out, d)
            if sel == "all" and name in CULL_CASES:
                assert (bits[cd.live] == 1).all(), bits
                # the hand-back is really exercised: a noisy image's hypotheses are hn scattered points, whose spatial sort is not the
                # identity.  (A clean image's may all coincide in the key-point itself: equal keys, and a stable sort leaves them be.)
                noisy = [bi for bi in cd.live if name != "A" or bi % 2]
                moved = (d["perm"].cpu().numpy() != np.arange(d["layout"].hn_pad)).any(axis=-1)
                assert moved[noisy].all(), moved
                sorted_away = int(moved[cd.live].sum())
            else:
                assert not bits.any(), (sel, bits)            # "none"; D and E have no culling layout to begin with
            figures[sel] = (px, int(bits.sum()))
        for i, (px, bits) in enumerate(own_selection_twice(voting, name)):
            if name not in CULL_CASES:
                assert not bits.any()
            figures[f"own selection, call {i + 1}"] = (px, int(bits.sum()))
    finally:
        voting.set_cull_selection(None)
    print(f"case {name} ({nlive} live key-points): " + "; ".join(f"{k}: {px:.2e} px, {c} culled" for k, (px, c) in figures.items()) +
          (f"; under \"all\" {sorted_away} key-points' sort is not the identity" if name in CULL_CASES else ""))


@pytest.mark.gpu
def test_the_culling_cases_reach_both_scoring_bodies_in_one_call(release_library):
    """under the library's own selection at least one call over A, B and C must cull some live key-points and score the others
    densely: the merged launch's two bodies in one call.  If none does, the case set has to change."""
    voting = release_library
    mixed, seen = 0, {}
    for name in CULL_CASES:
        cd = case_data(name)
        nlive = len(cd.live) * cd.case["vn"]
        seen[name] = [int(bits.sum()) for _, bits in own_selection_twice(voting, name)]
        mixed += sum(0 < c < nlive for c in seen[name])
        seen[name].append(nlive)
    print("culled key-points under the library's own selection (first call, second call, live):", seen)
    assert mixed > 0, seen


@pytest.mark.gpu
def test_hip_siblings_reproduce_the_executed_reference_at_a_culling_layout(release_library):
    import torch
    voting = release_library
    a = case_data("A")
    sib, keep5, idxs, gh_hyp, gh_counts = sibling_data()
    v5, dist = sib["v5"], sib["dist"]
    hn = a.case["hn"]
    v = device_inputs("A")[1]
    m = torch.from_numpy(a.mask).to(dev())
    m5 = torch.from_numpy(a.mask * keep5).to(dev())
    ix = {s: torch.from_numpy(idxs[s]).to(dev()) for s in idxs}
    ref_pts = torch.from_numpy(v5["pts"]).to(dev())
    mean = torch.from_numpy(dist["mean"]).to(dev())
    worst = dict(pts=0.0, conf=0.0, cov=0.0)
    culled = {}
    try:
        for sel in ("all", "none", None):
            for literal in (False, True):
                voting.set_cull_selection(sel)
                pts, conf = voting.ransac_voting_layer_v5(m5, v, hn, inlier_thresh=0.99, max_num=30000, literal=literal, idxs=ix["v5"])
                worst["pts"] = max(worst["pts"], float(np.abs(pts.cpu().numpy() - v5["pts"]).max()))
                assert np.abs(pts.cpu().numpy() - v5["pts"]).max() < TOL_REF_PX
                # the confidence (:846-850) at the REFERENCE'S OWN refined points on this call's pixel list: the same integers over the same tn
                _, dbg5 = voting.ransac_voting_layer_v3(m5, v, hn, inlier_thresh=0.99, max_num=30000, literal=literal, idxs=ix["v5"],
                                                        return_debug=True)
                assert dbg5["layout"].cull == 1
                conf_ref = voting.vote_confidence(dbg5, ref_pts, 0.999)
                assert np.abs(conf_ref.cpu().numpy() - v5["conf"]).max() <= 1e-6
                conf_err = float(np.abs(conf.cpu().numpy() - v5["conf"]).max())
                worst["conf"] = max(worst["conf"], conf_err)
                if np.array_equal(pts.cpu().numpy(), v5["pts"]):
                    assert conf_err <= 1e-6
                else:
                    assert conf_err <= CONF_EDGE_PIXELS / v5["tn"].min() + 1e-6
                _, cov = voting.estimate_voting_distribution_with_mean(m, v, mean, inlier_thresh=0.99, literal=literal, idxs=ix["dist"],
                                                                       **MG.LAYOUT_DIST)
                cov_err = float(np.abs(cov.cpu().numpy() - dist["cov"]).max())
                worst["cov"] = max(worst["cov"], cov_err)
                assert cov_err < 1e-3 * max(1.0, np.abs(dist["cov"]).max())
                hyp, counts = voting.generate_hypothesis_counts(m, v, hn, inlier_thresh=0.99, literal=literal, idxs=ix["gh"])
                assert hyp.cpu().numpy().tobytes() == gh_hyp.tobytes()
                np.testing.assert_array_equal(counts.cpu().numpy(), gh_counts)
                if not literal:
                    culled[str(sel)] = int(dbg5["cull_bits"].sum())
                    if sel == "all":
                        assert bool(dbg5["cull_bits"].all())
                    elif sel == "none":
                        assert not bool(dbg5["cull_bits"].any())
    finally:
        voting.set_cull_selection(None)
    print(f"siblings on A: max |pts - reference| {worst['pts']:.2e} px, |conf - reference| {worst['conf']:.2e}, "
          f"|cov - reference| {worst['cov']:.2e}; v5 key-points culled per selection: {culled}")


def lsq64(direct, coords, inl):
    """the refinement (:579-594) in float64 on given inlier flags [vn,tn]: per key-point (sum n n^T) x = sum n (n.c)"""
    out = np.zeros((inl.shape[0], 2))
    for k in range(inl.shape[0]):
        sel = inl[k] != 0
        n = np.stack([direct[sel, k, 1], -direct[sel, k, 0]], axis=1).astype(np.float64)
        rhs = (n * coords[sel].astype(np.float64)).sum(axis=1)
        out[k] = np.linalg.solve(n.T @ n, (n * rhs[:, None]).sum(axis=0))
    return out


@pytest.mark.gpu
@pytest.mark.skipif(not (refkernels.available("fast") and refkernels.available("off")),
                    reason="oracle/_ref (the reference's kernels compiled for gfx950, both contraction readings) not built")
def test_reference_kernels_in_both_contraction_readings_on_case_a(release_library):
    """a measurement: the reference's device code on A's compacted inputs, compiled without contraction (what every parity claim of
    this repository means) and with it (what nvcc's default --fmad=true may give).  Asserted: the product equals the `off` reading's
    integers.  Printed: how far the `fast` reading lies from it -- nobody has a bar for that."""
    import torch
    voting = release_library
    a = case_data("A")
    out, d, _ = vote(voting, "A")
    check_call("A", out, d)
    idxs = device_inputs("A")[2]
    ncounts = nwin = total = 0
    px = 0.0
    for bi in a.live:
        tn = int(d["tn"][bi])
        rec = d["rec"][bi, :, :tn]
        direct, coords = rec[:, :, 2:4].permute(1, 0, 2).contiguous(), rec[0, :, 0:2].contiguous()
        reading = {}
        for contract in ("off", "fast"):
            hyp = refkernels.generate_hypothesis(direct, coords, idxs[bi].contiguous(), contract)
            counts = refkernels.voting_for_hypothesis(direct, coords, hyp, 0.99, contract).sum(2, dtype=torch.int32).cpu().numpy()
            wi = counts.argmax(axis=0)
            win_pts = hyp.cpu().numpy()[wi, np.arange(a.case["vn"])]
            inl = refkernels.voting_for_hypothesis(direct, coords, torch.from_numpy(win_pts[None]).to(dev()), 0.99, contract)
            reading[contract] = (hyp.cpu().numpy(), counts, wi, lsq64(direct.cpu().numpy(), coords.cpu().numpy(), inl[0].cpu().numpy()))
        hyp, counts, wi, _ = reading["off"]
        assert d["hyp"][bi].permute(1, 0, 2).contiguous().cpu().numpy().tobytes() == hyp.tobytes()
        assert np.array_equal(d["counts"][bi].T.cpu().numpy(), counts)
        assert np.array_equal(d["win"][bi, :, 0].cpu().numpy(), wi)
        ncounts += int((reading["fast"][1] != counts).sum())
        nwin += int((reading["fast"][2] != wi).sum())
        total += counts.size
        px = max(px, float(np.abs(reading["fast"][3] - reading["off"][3]).max()))
    print(f"reference kernels on A, contraction fast against off: {ncounts} of {total} counts differ, {nwin} of "
          f"{len(a.live) * a.case['vn']} winners differ, refined key-points (float64 LSQ) up to {px:.2e} px apart")
