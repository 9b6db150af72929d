"""GPU tests of the band origin worked out ONCE per image (the origin block of the compaction launch, k2_compact.hip) and of the
hypothesis launch that reads it with one key-point per block (k3_hypotheses.hip).

a. `band_origin` and the per-key-point culled marks EQUAL a float32 numpy restatement of kp_origin_vote() (vote_common.h) on the
   records the call itself returns: one rounding per operation, median by rank, rint.  The restatement reads `rec` -- what the
   compaction blocks wrote -- while the origin block reads the mask's bits and the field: the equality also says that the block
   found the same 17 pixels and the same directions.
b. a mixed batch (live, below min_num, empty, thinned: the thinned image takes the per-block fallback) under both culling
   selections: counts, winners and key-points torch.equal to literal mode and to every image voted alone.
c. the hypotheses of the one-key-point-per-block grid: bit-equal to literal mode's and to the reference kernel's; the padding
   columns' counts are zero.

Every call runs on an explicitly zeroed workspace: the batch gate CF_BATCH_OK otherwise follows recycled memory."""
import numpy as np
import pytest
import torch

from oracle import ransac_voting_oracle as O
from oracle import refkernels
from pvnet_amd import synth, voting

pytestmark = pytest.mark.gpu

F = np.float32
KF1E6 = F(float.fromhex("0x1.0c6f7ap-20"))
NCAND, KP_MAX = 8, 32
CULL_Q = F(F(1e-3) * F(1000.0))   # fill_params: 1e-3f * PVNET_CULL_Q_MILLI of the release library
MANY_KP_CULLING_SHAPE = (2, 240, 320, 32, 1024)   # pinned as a culling layout by tests/test_library_cpu.py


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def default_selection():
    yield
    voting.set_cull_selection(None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def band_rho(tn):
    r = F(0.6) * np.sqrt(F(0.3183) * F(tn))
    return F(8.0) if r < F(8.0) else F(r)


def origin_slots(tn):
    ta = [((2 * j + 1) * tn) >> 4 for j in range(NCAND)]
    tb = [(t + tn // 2) - tn if t + tn // 2 >= tn else t + tn // 2 for t in ta]
    return ta, tb


def intersect(q0, q1):
    """hyp_intersect() of vote_common.h on float32 arrays [..., 4] = (x, y, ux, uy): one rounding per operation"""
    cx0, cy0, ux0, uy0 = (q0[..., i] for i in range(4))
    cx1, cy1, ux1, uy1 = (q1[..., i] for i in range(4))
    nx0, ny0, nx1, ny1 = uy0, -ux0, uy1, -ux1
    with np.errstate(all="ignore"):
        dety = nx1 * ny0 - nx0 * ny1
        detx = ny1 * nx0 - ny0 * nx1
        b0 = nx0 * cx0 + ny0 * cy0
        b1 = nx1 * cx1 + ny1 * cy1
        oy = (nx1 * b0 - nx0 * b1) / dety
        ox = (ny1 * b0 - ny0 * b1) / detx
    gate = (np.abs(dety) <= KF1E6) | (np.abs(detx) <= KF1E6)
    return np.where(gate, F(0), ox).astype(F), np.where(gate, F(0), oy).astype(F)


def restate_image(rec, tn, tn0, w, thresh, cull, min_num):
    """(origins int [vn, 2], votes int [vn]) of one image from its records float32 [vn, cap, 4]"""
    vn = rec.shape[0]
    org = np.zeros((vn, 2), np.int64)
    vote = np.zeros(vn, np.int64)
    live = tn0 >= min_num and tn > 0
    if not live:
        return org, vote
    pmx, pmy = int(rec[0, tn // 2, 0]), int(rec[0, tn // 2, 1])
    ta, tb = origin_slots(tn)
    hx, hy = intersect(rec[:, ta], rec[:, tb])
    with np.errstate(all="ignore"):
        ok = ((hx != 0) | (hy != 0)) & (np.abs(hx) < F(1048576.0)) & (np.abs(hy) < F(1048576.0))
    rho = band_rho(tn)
    ro = F(rho * (F(1.0) / F(0.6)))
    t32 = F(thresh)
    tau = F(np.sqrt(1.0 - float(t32) * float(t32)) / float(t32))
    for k in range(vn):
        xs, ys = hx[k][ok[k]], hy[k][ok[k]]
        n = len(xs)
        if n < 3:
            org[k] = (pmx, pmy)
            vote[k] = 1 if cull == 1 else 0
            continue
        mx, my = np.sort(xs, kind="stable")[n // 2], np.sort(ys, kind="stable")[n // 2]
        d = np.sort(np.maximum(np.abs(xs - mx), np.abs(ys - my)), kind="stable")
        dj = d[n // 2]
        dist = max(abs(F(mx - F(pmx))), abs(F(my - F(pmy))))
        lhs = F(dj + rho) * F(F(1.0) + F(F(dist + ro) / rho))
        rhs = F(F(dist + dj) + rho) * F(F(1.0) + F(ro / rho))
        org[k] = (int(np.rint(mx)), int(np.rint(my))) if lhs < rhs else (pmx, pmy)
        dv = d[max(n // 2, n - 2)]
        vote[k] = 1 if cull == 1 or (cull == 2 and dv <= F(F(CULL_Q * rho) * tau)) else 0
    return org, vote


def check_origins(dbg, thresh, selection, min_num=5):
    """band_origin and cull_bits of an exact-mode call on a zeroed workspace against the restatement; returns the marks"""
    L = dbg["layout"]
    assert dbg["mode"] == "exact"
    rec = dbg["rec"].cpu().numpy()
    tn, tn0 = dbg["tn"].cpu().numpy(), dbg["tn0"].cpu().numpy()
    got_org, got_marks = dbg["band_origin"].cpu().numpy(), dbg["cull_bits"].cpu().numpy()
    cull = 0 if not L.cull or selection == "none" else (1 if selection == "all" else 2)
    for bi in range(L.b):
        if L.vn > KP_MAX:   # the image's median pixel for every key-point, never culled
            live = tn0[bi] >= min_num and tn[bi] > 0
            pm = rec[bi, 0, tn[bi] // 2, :2].astype(np.int64) if live else np.zeros(2, np.int64)
            org, marks = np.tile(pm, (L.vn, 1)), np.zeros(L.vn, np.int64)
        else:
            org, vote = restate_image(rec[bi], int(tn[bi]), int(tn0[bi]), L.w, thresh, cull, min_num)
            marks = np.full(L.vn, 1 if (cull and 2 * int(vote.sum()) > L.vn) else 0)
        assert (got_org[bi] == org).all(), f"image {bi}: origins {got_org[bi].tolist()} != restated {org.tolist()}"
        assert (got_marks[bi] == marks).all(), f"image {bi}: culled marks {got_marks[bi].tolist()} != restated {marks.tolist()}"
    return got_marks


def zeroed_ws(b, h, w, vn, hn, max_num=30000):
    return torch.zeros(voting.vote_layout(b, h, w, vn, hn, max_num).total_bytes, dtype=torch.uint8, device=dev())


def vote(m, v, hn, thresh=0.99, seed=11, **kw):
    b, h, w, vn = v.shape[:4]
    ws = zeroed_ws(b, h, w, vn, hn, kw.get("max_num", 30000))
    return voting.ransac_voting_layer_v3(m, v, hn, inlier_thresh=thresh, seed=seed, return_debug=True, workspace=ws, **kw)


def disc_batch(b, h, w, vn=9, radius=14, noise=True, first=300, mask_dtype=np.int64):
    mask, planar, _ = synth.make_batch(b, first_index=first, h=h, w=w, vn=vn, radius=radius, noise=noise, background="normal",
                                       mask_dtype=mask_dtype)
    return torch.from_numpy(mask).to(dev()), synth.planar_to_vertex_view(torch.from_numpy(planar).to(dev()))


def field_for(mask_np, vn, seed, kind="points"):
    """a float32 planar field [b, 2 vn, h, w] for arbitrary masks: directions towards vn random points, or nearly parallel ones"""
    rng = np.random.default_rng(seed)
    b, h, w = mask_np.shape
    planar = rng.standard_normal((b, 2 * vn, h, w)).astype(np.float32)
    if kind == "parallel":   # every determinant of two directions is ~1e-8: below the 1e-6 gate, no usable candidate
        planar[:, 0::2] = 1.0
        planar[:, 1::2] = (1e-8 * rng.standard_normal((b, vn, h, w))).astype(np.float32)
        return planar
    ys, xs = np.mgrid[0:h, 0:w]
    for bi in range(b):
        for k in range(vn):
            px, py = rng.uniform(0, w), rng.uniform(0, h)
            dx, dy = px - xs, py - ys
            nrm = np.maximum(np.hypot(dx, dy), 1e-3)
            noise = rng.normal(0, 0.03, (h, w))
            planar[bi, 2 * k] = (dx / nrm * np.cos(noise) - dy / nrm * np.sin(noise)).astype(np.float32)
            planar[bi, 2 * k + 1] = (dx / nrm * np.sin(noise) + dy / nrm * np.cos(noise)).astype(np.float32)
    return planar


def to_dev(mask_np, planar_np):
    return torch.from_numpy(mask_np).to(dev()), synth.planar_to_vertex_view(torch.from_numpy(planar_np).to(dev()))


# ---------------------------------------------------------------------------------------------------------------------------------
# a. origin and vote against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("selection", [None, "all"], ids=["library_selects", "every_keypoint_culled"])
def test_discs_at_a_culling_layout(noise, selection):
    """vn = 32 at the pinned culling layout: the vote decides something here (the clean field's key-points vote to cull)"""
    b, h, w, vn, hn = MANY_KP_CULLING_SHAPE
    m, v = disc_batch(b, h, w, vn=vn, radius=25, noise=noise)
    voting.set_cull_selection(selection)
    _, dbg = vote(m, v, hn)
    assert dbg["layout"].cull == 1
    marks = check_origins(dbg, 0.99, selection)
    if selection == "all" or not noise:
        assert marks.all()


@pytest.mark.parametrize("noise", [False, True], ids=["clean", "noisy"])
@pytest.mark.parametrize("vn", [1, 9, 33])
def test_discs_by_key_point_count(noise, vn):
    m, v = disc_batch(3, 96, 128, vn=vn, noise=noise)
    _, dbg = vote(m, v, 128)
    check_origins(dbg, 0.99, None)


def test_nearly_parallel_field_takes_the_median_pixel():
    mask = np.stack([synth.disk_mask(96, 128, 60 + 5 * i, 40 + 3 * i, 13) for i in range(2)]).astype(np.int64)
    m, v = to_dev(mask, field_for(mask, 9, 5, "parallel"))
    _, dbg = vote(m, v, 128)
    check_origins(dbg, 0.99, None)
    pm = dbg["rec"][:, 0].cpu().numpy()
    for bi in range(2):
        t = int(dbg["tn"][bi]) // 2
        assert (dbg["band_origin"][bi].cpu().numpy() == pm[bi, t, :2].astype(np.int64)).all()


@pytest.mark.parametrize("tn", [1, 2, 5, 17])
def test_tiny_lists_where_slots_collide(tn):
    rng = np.random.default_rng(tn)
    mask = np.zeros((2, 64, 96), np.int64)
    for bi in range(2):
        mask[bi].reshape(-1)[rng.choice(64 * 96, tn, replace=False)] = 1
    m, v = to_dev(mask, field_for(mask, 9, 40 + tn))
    _, dbg = vote(m, v, 128, min_num=1)
    assert dbg["tn"].tolist() == [tn, tn]
    check_origins(dbg, 0.99, None, min_num=1)


@pytest.mark.parametrize("h,w,cx,cy", [(96, 128, 64, 32), (64, 100, 50, 41), (72, 96, 63, 42)],
                         ids=["segment_and_word_boundary", "width_100", "segment_boundary_inside_a_row"])
def test_foreground_across_segment_and_word_boundaries(h, w, cx, cy):
    """a segment is 4 096 pixels (32 rows of 128; row 40.96 of width 100; row 42.67 of 96), a word 64: the disc lies across both"""
    mask = np.stack([synth.disk_mask(h, w, cx + i, cy, 11) for i in range(2)]).astype(np.int64)
    flat = np.flatnonzero(mask[0].reshape(-1))
    assert flat.min() < 4096 <= flat.max() and len({int(p) // 64 for p in flat}) > 1
    m, v = to_dev(mask, field_for(mask, 9, 7))
    _, dbg = vote(m, v, 128)
    check_origins(dbg, 0.99, None)


@pytest.mark.parametrize("mdt", [np.uint8, np.int64], ids=["uint8", "int64"])
def test_mask_types(mdt):
    m, v = disc_batch(2, 64, 96, mask_dtype=mdt, radius=10)
    assert m.dtype == {np.uint8: torch.uint8, np.int64: torch.int64}[mdt]
    _, dbg = vote(m, v, 128)
    check_origins(dbg, 0.99, None)


@pytest.mark.parametrize("fdt", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_half_precision_fields_read_in_place(fdt):
    mask, planar, _ = synth.make_batch(2, first_index=310, h=64, w=96, radius=10, noise=True, background="normal")
    m = torch.from_numpy(mask).to(dev())
    v = synth.planar_to_vertex_view(torch.from_numpy(planar).to(dev()).to(fdt))
    assert v.dtype == fdt
    _, dbg = vote(m, v, 128)
    check_origins(dbg, 0.99, None)
    tn = int(dbg["tn"][0])   # the records are the half-precision values, widened
    assert torch.equal(dbg["rec"][0, :, :tn, 2:4].to(fdt).float(), dbg["rec"][0, :, :tn, 2:4])


def test_strided_field():
    """the field is a window of a larger planar tensor: every stride differs from the packed one"""
    mask, planar, _ = synth.make_batch(2, first_index=320, h=64, w=96, radius=10, noise=True, background="normal")
    big = torch.zeros((2, 18, 70, 2 * 96 + 5), device=dev())
    window = big[:, :, 3:67, 2:2 + 2 * 96:2]
    window.copy_(torch.from_numpy(planar).to(dev()))
    v = synth.planar_to_vertex_view(window)
    assert not v.is_contiguous() and v.stride(2) == 2
    _, dbg = vote(torch.from_numpy(mask).to(dev()), v, 128)
    check_origins(dbg, 0.99, None)
    _, dense = vote(torch.from_numpy(mask).to(dev()), synth.planar_to_vertex_view(torch.from_numpy(planar).to(dev())), 128)
    assert torch.equal(dbg["band_origin"], dense["band_origin"])


def test_per_class_entry_reads_the_source_image():
    """two classes per image (src_div = 2): virtual image i * 2 + k gathers from field i"""
    b, h, w, cn = 2, 64, 96, 3
    labels = np.zeros((b, h, w), np.int64)
    for i in range(b):
        labels[i][synth.disk_mask(h, w, 30 + 4 * i, 30, 10)] = 1
        labels[i][synth.disk_mask(h, w, 66, 36 - 3 * i, 9)] = 2
    planar = field_for(labels, 9, 21)
    lab, v = to_dev(labels, planar)
    ws = zeroed_ws(b * (cn - 1), h, w, 9, 128)
    _, dbg = voting.ransac_voting_layer_v2(lab, v, cn, 128, inlier_thresh=0.99, seed=11, return_debug=True, workspace=ws)
    assert dbg["layout"].b == b * (cn - 1) and (dbg["tn"] > 100).all()
    check_origins(dbg, 0.99, None)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. mixed batch
# ---------------------------------------------------------------------------------------------------------------------------------
MIXED_MAX_NUM = 400


@pytest.fixture(scope="module")
def mixed():
    """(live, below min_num, empty, thinned) at a shape whose layout has culling buffers"""
    b, h, w, vn = 4, 96, 128, 16
    mask = np.zeros((b, h, w), np.int64)
    mask[0] = synth.disk_mask(h, w, 40, 50, 9)          # ~250 pixels: live, kept whole
    mask[1, 10, 10:13] = 1                               # 3 pixels: below min_num = 5
    mask[3] = synth.disk_mask(h, w, 70, 40, 16)         # ~800 pixels > max_num: thinned, the per-block fallback
    assert mask[0].sum() < MIXED_MAX_NUM < mask[3].sum()
    planar = field_for(mask, vn, 77)
    m, v = to_dev(mask, planar)
    kw = dict(inlier_thresh=0.99, seed=5, max_num=MIXED_MAX_NUM, return_debug=True)
    out_l, lit = voting.ransac_voting_layer_v3(m, v, 1024, literal=True, workspace=zeroed_ws(b, h, w, vn, 1024, MIXED_MAX_NUM), **kw)
    out_l = out_l.clone()
    lit = {k: lit[k].clone() for k in ("counts", "win", "tn", "hyp")}
    alone = []
    for i in range(b):
        o, d = voting.ransac_voting_layer_v3(m[i:i + 1], v[i:i + 1], 1024, image_offset=i,
                                             workspace=zeroed_ws(1, h, w, vn, 1024, MIXED_MAX_NUM), **kw)
        alone.append((o.clone(), d["counts"].clone(), d["win"].clone()))
    return m, v, kw, out_l, lit, alone


@pytest.mark.parametrize("selection", [None, "all"], ids=["library_selects", "every_keypoint_culled"])
def test_mixed_batch(mixed, selection):
    m, v, kw, out_l, lit, alone = mixed
    b, h, w, vn = v.shape[:4]
    voting.set_cull_selection(selection)
    out, dbg = voting.ransac_voting_layer_v3(m, v, 1024, workspace=zeroed_ws(b, h, w, vn, 1024, MIXED_MAX_NUM), **kw)
    voting.set_cull_selection(None)
    assert dbg["mode"] == "exact" and dbg["layout"].cull == 1
    # (thinning keeps about max_num pixels, not at most: a pixel stays when the bin of its random word is below k)
    assert int(dbg["tn0"][3]) > MIXED_MAX_NUM and int(dbg["tn0"][3]) > int(dbg["tn"][3]) > 0
    assert MIXED_MAX_NUM > int(dbg["tn"][0]) == int(dbg["tn0"][0]) and dbg["tn0"][1:3].tolist() == [3, 0]
    marks = check_origins(dbg, 0.99, selection)
    if selection == "all":
        assert marks[0].all() and marks[3].all() and not marks[1].any() and not marks[2].any()
    assert torch.equal(dbg["tn"], lit["tn"])
    assert dbg["hyp"].cpu().numpy().tobytes() == lit["hyp"].cpu().numpy().tobytes()
    assert torch.equal(dbg["counts"], lit["counts"])
    assert torch.equal(dbg["win"], lit["win"])
    assert torch.equal(out, out_l)
    for i, (o, c, wn) in enumerate(alone):
        assert torch.equal(dbg["counts"][i:i + 1], c), f"image {i}: counts differ from the image voted alone"
        assert torch.equal(dbg["win"][i:i + 1], wn)
        assert torch.equal(out[i:i + 1], o)


# ---------------------------------------------------------------------------------------------------------------------------------
# c. hypothesis order
# ---------------------------------------------------------------------------------------------------------------------------------
_HYP = {}


def hyp_case(hn, vn):
    if (hn, vn) not in _HYP:
        m, v = disc_batch(2, 64, 96, vn=vn, radius=10, first=330 + vn)
        _, lit = vote(m, v, hn, literal=True)
        lit_hyp = lit["hyp"].clone()
        _, dbg = vote(m, v, hn)
        _HYP[(hn, vn)] = (lit_hyp, dbg)
    return _HYP[(hn, vn)]


@pytest.mark.parametrize("vn", [1, 9, 32])
@pytest.mark.parametrize("hn", [100, 256, 257, 1000])
def test_hypotheses_equal_literal_mode_and_padding_counts_are_zero(hn, vn):
    lit_hyp, dbg = hyp_case(hn, vn)
    L = dbg["layout"]
    assert dbg["mode"] == "exact" and L.hn == hn and L.hn_pad >= hn
    assert dbg["hyp"].cpu().numpy().tobytes() == lit_hyp.cpu().numpy().tobytes()
    counts = dbg["workspace"][L.off_counts:L.off_counts + 4 * L.b * L.vn * L.hn_pad].view(torch.int32).view(L.b, L.vn, L.hn_pad)
    assert int(counts[:, :, :hn].max()) > 0
    assert not bool(counts[:, :, hn:].any()), f"{int((counts[:, :, hn:] != 0).sum())} padding counts are not zero"


@pytest.mark.skipif(not refkernels.available("off"), reason="oracle/_ref not built (needs the reference tree)")
@pytest.mark.parametrize("vn", [1, 9, 32])
@pytest.mark.parametrize("hn", [100, 256, 257, 1000])
def test_hypotheses_equal_the_reference_kernel(hn, vn):
    _, dbg = hyp_case(hn, vn)
    for bi in range(2):
        tn = int(dbg["tn"][bi])
        rec = dbg["rec"][bi, :, :tn]
        coords = rec[0, :, 0:2].contiguous()
        direct = rec[:, :, 2:4].permute(1, 0, 2).contiguous()
        idxs = torch.from_numpy(O.draw_idxs(dbg["seed"], bi, hn, vn, tn)).to(dev())
        hyp_ref = refkernels.generate_hypothesis(direct, coords, idxs)
        assert dbg["hyp"][bi].permute(1, 0, 2).contiguous().cpu().numpy().tobytes() == hyp_ref.cpu().numpy().tobytes()
