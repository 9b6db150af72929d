"""CPU checks behind tests/test_mixed_batches_device.py: its shapes get culling buffers from the release library, the builder
(tests/mixed_cases.py) makes the images its table names, and the reference side alone -- the C oracle against the numpy float32 oracle
-- stays within its own conditions on these inputs."""
import numpy as np
import pytest

from oracle import cref, ransac_voting_oracle as O
from pvnet_amd import build, synth
from tests import mixed_cases as M
from tests.test_library_cpu import release_layout

THRESH = 0.99


@pytest.fixture(scope="module")
def lib():
    build.build()


def test_every_device_shape_gets_culling_buffers_from_the_release_library(lib):
    """a layout change that would turn the device module's calls into plain dense ones fails here, without a GPU"""
    shapes = M.v3_shapes() + M.v2_shapes()
    assert len(shapes) == 7
    for b, h, w, vn, hn, max_num in shapes:
        assert (h, w) == (M.H, M.W) and 768 <= hn <= 1024 and b * vn >= 64 and vn <= 32
        assert release_layout(b, h, w, vn, hn, max_num).cull == 1, (b, h, w, vn, hn, max_num)
    assert release_layout(7, M.H, M.W, 9, 1024).cull == 0   # (the helper does tell the layouts apart)


def test_permutations_hold_the_dead_images_where_the_tests_need_them():
    orders = [M.permutation(i) for i in range(M.N_PERMUTATIONS)]
    assert len(set(orders)) == M.N_PERMUTATIONS
    for o in orders:
        assert len(o) == M.V3_B == len(set(o)) and "empty" in o and "below_min" in o and set(o) <= set(M.KINDS)
    assert orders[0][0] in M.DEAD_KINDS and orders[1][-1] in M.DEAD_KINDS
    assert {k for o in orders for k in o} == set(M.KINDS)
    assert any(0 < o.index("empty") < M.V3_B - 1 for o in orders)          # a dead image between live ones
    hist = orders[M.HISTORY_PERMUTATION]
    assert "ties" not in hist and all(a != b for a, b in zip(hist, M.rolled(M.mixed_batch(hist, seed=M.HISTORY_PERMUTATION)).kinds))
    for i in M.HN_PERMUTATIONS + M.THRESH_PERMUTATIONS + (M.REF_KERNEL_PERMUTATION,):
        assert 0 <= i < M.N_PERMUTATIONS
    assert any("ties" in orders[i] for i in M.HN_PERMUTATIONS) and any("thinned" in orders[i] for i in M.HN_PERMUTATIONS)
    assert "ties" in M.TIES_ORDER and "thinned" not in M.TIES_ORDER and len(M.TIES_ORDER) == M.V3_B


def test_images_are_what_the_table_says():
    counts = dict(M.PIXELS, clean=None, noisy=None, ties=None, thinned=M.H * M.W)
    seen = set()
    for i in range(M.N_PERMUTATIONS):
        bt = M.mixed_batch(M.permutation(i), seed=i)
        assert bt.mask.shape == (M.V3_B, M.H, M.W) and bt.planar.shape == (M.V3_B, 2 * M.V3_VN, M.H, M.W) and bt.planar.dtype == np.float32
        assert bt.max_num == (M.THIN_MAX_NUM if "thinned" in bt.kinds else 30000)
        for j, kind in enumerate(bt.kinds):
            fg = bt.mask[j] != 0
            n = int(fg.sum())
            seen.add(kind)
            if kind in M.DISC_KINDS:
                ys, xs = np.nonzero(fg)
                assert 2700 < n < 2900 and ys.max() - ys.min() == 2 * M.RADIUS == xs.max() - xs.min()   # a whole disc of radius 30
            else:
                assert n == counts[kind], (kind, n)
            if kind == "thinned":
                tn = M.kept_pixels(fg, bt.call_seed, j, bt.max_num)
                assert n > bt.max_num and 0.9 * bt.max_num < tn < 1.15 * bt.max_num   # (a Bernoulli draw about max_num .. max_num 17 / 16)
            v = bt.planar[j].reshape(M.V3_VN, 2, M.H, M.W)
            if kind in M.CLEAN_KINDS:      # unit vectors at the key-points on the foreground, zeros elsewhere
                assert not v[:, :, ~fg].any()
                ys, xs = np.nonzero(fg)
                d = bt.kpts[j][:, None, :] - np.stack([xs, ys], 1)[None]
                d /= np.linalg.norm(d, axis=2, keepdims=True)
                assert np.abs(v[:, :, fg] - d.transpose(0, 2, 1)).max() < 1e-6
            elif kind in ("empty", "below_min"):
                assert np.isnan(bt.kpts[j]).all() == (kind == "empty") and v.std() > 0.5
            if kind == "ties":
                assert (bt.kpts[j] == np.round(bt.kpts[j])).all() and not fg[bt.kpts[j][:, 1].astype(int), bt.kpts[j][:, 0].astype(int)].any()
        if "ties" in bt.kinds:
            j = bt.kinds.index("ties")
            ix = bt.idxs[j]
            tn = M.kept_pixels(bt.mask[j] != 0, bt.call_seed, j, bt.max_num)
            slots = M.tie_slots(1024)
            assert len(set(slots.tolist())) == M.TIE_SLOTS and slots[0] == M.TIE_FIRST and slots[-1] > 1000
            assert (ix >= 0).all() and (ix < tn).all() and (ix[slots] == ix[slots[0]]).all() and (ix[:M.TIE_FIRST, :, 0] == ix[:M.TIE_FIRST, :, 1]).all()
            for jj, kind in enumerate(bt.kinds):   # every other live image gets the layer's own draws
                if kind not in M.DEAD_KINDS + ("ties",):
                    tnj = M.kept_pixels(bt.mask[jj] != 0, bt.call_seed, jj, bt.max_num)
                    assert np.array_equal(bt.idxs[jj], O.draw_idxs(bt.call_seed, jj, 1024, M.V3_VN, tnj))
        else:
            assert bt.idxs is None
    assert seen == set(M.KINDS)


def test_label_batches_hold_empty_classes_between_live_ones():
    for case in M.V2_CASES:
        b, cn, vn = case
        lb = M.label_batch(b, cn, vn, M.v2_present(case), seed=cn)
        masks = M.materialised_masks(lb.labels, cn)
        n = masks.reshape(b, cn - 1, -1).sum(2)
        for i in range(b):
            for k in range(cn - 1):
                kind = lb.kinds[i, k]
                if kind in ("clean", "noisy"):
                    assert 2700 < n[i, k] < 2900
                else:
                    assert n[i, k] == M.PIXELS[kind], (i, k, kind)
        live = (n >= M.MIN_NUM).reshape(-1)
        dead_kinds = np.isin(lb.kinds.reshape(-1), M.DEAD_KINDS)
        assert np.array_equal(~live, dead_kinds)
        if case == (8, 4, 3):
            assert live.all()
        else:
            first, last = np.flatnonzero(live)[[0, -1]]
            assert (~live[first:last]).sum() >= 5                      # dead ones between the live, not only at the ends
            assert (lb.kinds == "below_min").any() and (n == 0).sum() > (n > 0).sum()
        # nobody's labels are there and belong to nobody
        lab = lb.labels
        assert (lab == -1).any() and (lab == cn).any() and (lab == 255).any() and (lab[:, M.STRAY_ROW, 0:4] != 0).sum() == 3 * b
        assert masks.sum() == ((lab >= 1) & (lab < cn)).sum()
        assert lb.field.shape == (b, M.H, M.W, vn, 2) and lb.field.flags.c_contiguous
    a, c = M.v2_present((2, 14, 3)), M.v2_present_changed()
    assert set(a[0]) - set(c[0]) == {6} and set(c[0]) - set(a[0]) == {3} and a[1] == c[1]


def reference_side(mask, vertex, hn, max_num, seed, idxs, kinds, kpts):
    """the C oracle against the numpy float32 oracle on every live image; clean tiny images against their key-points"""
    out_c, wi, wc = cref.vote_v3(O.foreground(mask), vertex, hn, THRESH, min_num=M.MIN_NUM, max_num=max_num, seed=seed, idxs=idxs,
                                 return_winners=True)
    out_o, dbg = O.ransac_voting_layer_v3(mask, vertex, hn, inlier_thresh=THRESH, min_num=M.MIN_NUM, max_num=max_num, seed=seed, idxs=idxs,
                                          dtype=np.float32, return_debug=True)
    for i, kind in enumerate(kinds):
        if kind in M.DEAD_KINDS:
            assert dbg[i]["skipped"] and not out_c[i].any() and not out_o[i].any()
            continue
        assert np.array_equal(wi[i], dbg[i]["win_idx"]) and np.array_equal(wc[i], dbg[i]["win_cnt"]), (i, kind)
        err = float(np.abs(out_c[i] - out_o[i]).max())
        assert err < 1e-4, (i, kind, err)
        if kind in ("at_min", "tile", "item_m1", "item", "item_p1"):
            far = float(np.abs(out_c[i] - kpts[i]).max())
            assert far < 5e-3, (i, kind, far)
            assert (wc[i] == dbg[i]["tn"]).all()
    return dbg


def test_the_reference_side_on_a_mixed_batch_and_its_ties():
    bt = M.mixed_batch(M.TIES_ORDER, seed=M.TIES_SEED)
    dbg = reference_side(bt.mask, synth.planar_to_vertex_view(bt.planar), 1024, bt.max_num, bt.call_seed, bt.idxs, bt.kinds, bt.kpts)
    d = dbg[bt.kinds.index("ties")]
    slots = M.tie_slots(1024)
    for k in range(M.V3_VN):
        c = d["counts"][:, k]
        tied = np.flatnonzero(c == c.max())
        assert len(tied) >= M.TIE_SLOTS and set(slots.tolist()) <= set(tied.tolist())       # a real tie for the maximum
        assert d["win_idx"][k] == tied.min() == M.TIE_FIRST                                 # and the smallest tied index wins
        assert (c[:M.TIE_FIRST] < c.max()).all()
        assert d["hyp"][slots, k].astype(np.float32).tobytes() == d["hyp"][slots[:1], k].astype(np.float32).tobytes() * M.TIE_SLOTS


def test_the_reference_side_on_a_label_batch():
    case = M.V2_CASES[0]
    b, cn, vn = case
    lb = M.label_batch(b, cn, vn, M.v2_present(case), seed=cn)
    masks = M.materialised_masks(lb.labels, cn)
    reference_side(masks, np.repeat(lb.field, cn - 1, axis=0), 1024, 30000, 31, None, lb.kinds.reshape(-1), lb.kpts.reshape(-1, vn, 2))
