"""GPU tests of the per-class vote: ``voting.ransac_voting_layer_v2`` (libpvnet_classes.so's class split, then
``pvnet_vote_v3_prepared``) against its definition -- ``ransac_voting_layer_v3`` called ONCE on the materialised batch of
B = b (class_num - 1) images: masks ``mask[i] == k + 1`` in the order (i, k), the field of image i repeated class_num - 1 times, the same
seed, image_offset, flags and hn.  ``torch.equal`` on key-points, status, tn0 / tn, the pixel lists and the inlier counts; the split
itself against the numpy restatement (tests/class_split_restatement.py).

Shapes: 72 x 100 = 7200 pixels -- two 4096-pixel segments, the second partial; 112.5 words of 64 pixels, so the last word is half --
b = 3, class_num = 4, (vn, hn) = (9, 128) and (2, 64), max_num = 200 so that the thinning histograms of both segments are used."""
import numpy as np
import pytest
import torch

from oracle import ransac_voting_oracle as O
from pvnet_amd import synth, voting
from tests import class_split_restatement as RS

pytestmark = pytest.mark.gpu

H, W, B0, CN = 72, 100, 3, 4
NK = CN - 1
MIN_NUM, MAX_NUM, THRESH = 5, 200, 0.99


def dev():
    return torch.device("cuda:0")


def make_labels() -> np.ndarray:
    """int64 [3,72,100]; see the assertions of test_label_images_hold_the_cases"""
    lab = np.zeros((B0, H, W), np.int64)
    # image 0: class 1 is large (3050 px > max_num, both segments), its edges at columns 10 and 60 fall inside 64-pixel words
    lab[0, 5:66, 10:60] = 1
    lab[0, 10:16, 60:90] = 2                       # 180 px
    lab[0, 50:61, 70:80] = 3                       # 110 px
    lab[0, 20, 60:70], lab[0, 20, 90:94] = 2, 3    # word 32 (row 20 from column 48, row 21 to column 11): classes 1, 2, 3 and background
    lab[0, 0, 0:4] = (4, 255, 256 + 1, -1)         # nobody's
    lab[0, 71, 96:100] = (-1, 4, 255, 256 + 1)     # ... in the half last word too
    # image 1: class 1 absent, class 2 below min_num, class 3 large
    lab[1, 30, 40:43] = 2
    lab[1, 25:55, 30:60] = 3                       # 900 px
    lab[1, 30, 40:43] = 2
    # image 2: class 1 from the first pixel, class 2 to the last (the half word), class 3 across the segment boundary (pixel 4096)
    lab[2, 0:3, :] = 1
    lab[2, 69:72, :] = 2
    lab[2, 39:43, 20:95] = 3
    return lab


def make_field(lab: np.ndarray, vn: int, seed: int = 7) -> np.ndarray:
    """[b,h,w,vn,2] float32: every class's pixels point at that class's key-points, rotated by a little noise; background N(0,1)"""
    rng = np.random.default_rng(seed)
    out = rng.standard_normal((B0, H, W, vn, 2)).astype(np.float32)
    for i in range(B0):
        for k in range(NK):
            fg = lab[i] == k + 1
            if not fg.any():
                continue
            ys, xs = np.nonzero(fg)
            kp = np.stack([rng.uniform(xs.mean() - 15, xs.mean() + 15, vn), rng.uniform(ys.mean() - 15, ys.mean() + 15, vn)], 1)
            planar = synth.add_noise(synth.field_from_keypoints(fg, kp), fg, rng, sigma_rad=0.03, outlier_frac=0.1)
            out[i][fg] = planar.reshape(vn, 2, H, W).transpose(2, 3, 0, 1)[fg]
    return out


LABELS = make_labels()
FIELDS = {}


def field(vn):
    if vn not in FIELDS:
        FIELDS[vn] = make_field(LABELS, vn)
    return FIELDS[vn]


def materialised(labels: torch.Tensor, vertex: torch.Tensor, cn: int):
    """the definition's batch: masks [B,h,w] in the order (i, k), the field of image i repeated cn - 1 times"""
    masks = torch.stack([labels[i] == k + 1 for i in range(labels.shape[0]) for k in range(cn - 1)])
    return masks, vertex.repeat_interleave(cn - 1, dim=0)


def zero_ws(b, vn, hn, max_num=MAX_NUM, h=H, w=W):
    """a zeroed workspace: what neither call writes compares equal"""
    return torch.zeros(voting.vote_layout(b, h, w, vn, hn, max_num).total_bytes, dtype=torch.uint8, device=dev())


def assert_equals_definition(labels, vertex, cn, hn, *, max_num=MAX_NUM, thresh=THRESH, **kw):
    b, h, w, vn = vertex.shape[:4]
    B = b * (cn - 1)
    out, dbg = voting.ransac_voting_layer_v2(labels, vertex, cn, hn, thresh, min_num=MIN_NUM, max_num=max_num, return_debug=True,
                                             workspace=zero_ws(B, vn, hn, max_num, h, w), **kw)
    masks, rep = materialised(labels, vertex, cn)
    if kw.get("idxs") is not None and kw["idxs"].dim() == 5:
        kw = dict(kw, idxs=kw["idxs"].reshape(B, *kw["idxs"].shape[2:]))
    ref, rdbg = voting.ransac_voting_layer_v3(masks, rep, hn, thresh, min_num=MIN_NUM, max_num=max_num, return_debug=True,
                                              workspace=zero_ws(B, vn, hn, max_num, h, w), concurrent=False, **kw)
    torch.cuda.synchronize()
    assert out.shape == (b, cn - 1, vn, 2) and out.dtype == torch.float32
    assert dbg["mode"] == rdbg["mode"] and dbg["layout"].total_bytes == rdbg["layout"].total_bytes
    assert torch.equal(out.view(B, vn, 2), ref), "key-points"
    assert torch.equal(dbg["status"], rdbg["status"]), "status"
    assert torch.equal(dbg["ctrl"][:B, :2], rdbg["ctrl"][:B, :2]), "tn0 / tn"
    assert torch.equal(dbg["pix"], rdbg["pix"]), "pixel lists"
    assert torch.equal(dbg["counts"], rdbg["counts"]), "inlier counts"
    assert torch.equal(dbg["bits"], rdbg["bits"]) and torch.equal(dbg["hyp"], rdbg["hyp"]) and torch.equal(dbg["win"], rdbg["win"])
    return out, dbg


def test_label_images_hold_the_cases():
    """(no device needed, but it speaks for the device tests only) the label images are what the module's docstring says"""
    cls = RS.class_of(LABELS, CN)
    cnt = np.array([[(cls[i] == k + 1).sum() for k in range(NK)] for i in range(B0)])
    assert cnt[1, 0] == 0 and 0 < cnt[1, 1] < MIN_NUM and cnt[0, 0] > MAX_NUM and cnt[1, 2] > MAX_NUM and (cnt[0, 1:] < MAX_NUM).all()
    bits, seg0, _, has = RS.split(LABELS, CN, MAX_NUM, 1)
    assert has[0].all() and seg0[0].min() > 0                                  # the large class has pixels in both segments
    assert all(int(bits[k, 32]) != 0 for k in range(NK)) and int(bits[0, 32] | bits[1, 32] | bits[2, 32]) != 2 ** 64 - 1   # word 32
    assert not any(int(bits[k, 0]) & 0xF for k in range(NK)) and int(bits[7, 112]) == 2 ** 32 - 1   # nobody's labels; the half word
    assert (LABELS == 4).any() and (LABELS == 255).any() and (LABELS == 257).any() and (LABELS == -1).any()
    edges = np.flatnonzero(np.diff(cls[0].reshape(-1)) != 0) + 1
    assert (edges % 64 != 0).sum() > 100                                       # class boundaries of image 0 inside words
    assert seg0[8].tolist() == [150, 150]                                      # image 2's class 3 lies on both sides of pixel 4096


def split_on_device(src, cn, max_num=MAX_NUM, seed=11, image_base=5, logits=False):
    """the split alone, into a zeroed workspace laid out for B images: (bits, seg0, cum) as numpy"""
    import ctypes as C
    from pvnet_amd import _abi
    clib = _abi.load_classes_library()
    b, h, w = (src.shape[0], *src.shape[-2:])
    B = b * (cn - 1)
    L = voting.vote_layout(B, h, w, 1, 64, max_num)
    ws = torch.zeros(L.total_bytes, dtype=torch.uint8, device=dev())
    base = ws.data_ptr()
    off_seg0 = L.off_seg + 4 * B * L.nseg
    off_cum = L.off_seg + (8 * B * L.nseg + 15) // 16 * 16
    tail = [cn, b, h, w, max_num, C.c_uint64(seed), image_base, C.c_void_p(base + L.off_bits), C.c_void_p(base + off_seg0),
            C.c_void_p(base + off_cum), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    if logits:
        rc = clib.pvnet_class_split_logits(C.c_void_p(src.data_ptr()), voting._CLASS_LOGITS_CODES[src.dtype], voting._strides(src, 4), *tail)
    else:
        rc = clib.pvnet_class_split(*voting._mask_part(src), *tail)
    assert rc == 0
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    bits = raw[L.off_bits:L.off_bits + 8 * B * L.words].view(np.uint64).reshape(B, L.words)
    seg0 = raw[off_seg0:off_seg0 + 4 * B * L.nseg].view(np.int32).reshape(B, L.nseg)
    cum = raw[off_cum:off_cum + 2 * B * L.nseg * RS.THIN_BINS].view(np.uint16).reshape(B, L.nseg, RS.THIN_BINS) if max_num < h * w else None
    return bits, seg0, cum


def assert_split_equals_restatement(src, host_labels, cn, **kw):
    bits, seg0, cum = split_on_device(src, cn, **kw)
    rb, rs, rc, has = RS.split(host_labels, cn, kw.get("max_num", MAX_NUM), 11, 5)
    assert np.array_equal(bits, rb), "bit words"
    assert np.array_equal(seg0, rs), "segment counts"
    # rows of segments without pixels of the class are not written: zero in the zeroed workspace, zero in the restatement
    assert np.array_equal(cum, rc), "thinning histograms"
    assert has.any() and not has.all()


@pytest.mark.parametrize("case", ["uint8", "bool", "int16", "int32", "int64_pair", "int64_odd_offset", "int64_strided", "float32"])
def test_split_equals_the_restatement(case):
    lab = LABELS
    if case == "uint8":          # 255 stays nobody's, 257 and -1 wrap to 1 and 255 BEFORE the kernel sees them: the restatement gets the same bytes
        host = lab.astype(np.uint8)
        assert_split_equals_restatement(torch.from_numpy(host).to(dev()), host, CN)
    elif case == "bool":
        host = lab == 1
        host[1] = lab[1] == 3    # (an image without a pixel stays: image 2 is all False below)
        host[2] = False
        assert_split_equals_restatement(torch.from_numpy(host).to(dev()), host, 2)
    elif case in ("int16", "int32", "float32"):
        host = lab.astype(getattr(np, case))
        if case == "float32":
            host[2, 10, 10:14] = (1.5, np.nan, 2.0, -0.0)
        assert_split_equals_restatement(torch.from_numpy(host).to(dev()), host, CN)
    elif case == "int64_pair":   # contiguous, 16-byte aligned, an even pixel count: the two-pixel load
        t = torch.from_numpy(lab).to(dev())
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        assert_split_equals_restatement(t, lab, CN)
    elif case == "int64_odd_offset":   # the same labels one element further: 8-byte aligned only, the generic path
        buf = torch.zeros(lab.size + 1, dtype=torch.int64, device=dev())
        buf[1:] = torch.from_numpy(lab).to(dev()).reshape(-1)
        t = buf[1:].view(B0, H, W)
        assert t.data_ptr() % 16 == 8
        assert_split_equals_restatement(t, lab, CN)
    else:                        # a strided slice: every second column of a wider image, every second image of a longer batch
        wide = torch.full((2 * B0, H, 2 * W), 2, dtype=torch.int64, device=dev())
        wide[::2, :, ::2] = torch.from_numpy(lab).to(dev())
        t = wide[::2, :, ::2]
        assert not t.is_contiguous()
        assert_split_equals_restatement(t, lab, CN)


def test_split_of_logits_equals_the_restatement():
    rng = np.random.default_rng(3)
    seg = rng.standard_normal((B0, CN, H, W)).astype(np.float32)
    seg[0, :, 10, 10] = 0.25
    seg[0, :, 11, 11] = (0.0, 3.0, 3.0, -1.0)
    seg[0, :, 12, 12] = (0.0, 1.0, np.nan, 9.0)
    seg[1, 1] = -10.0                                          # class 1 absent from image 1
    host = RS.argmax_first(seg)
    t = torch.from_numpy(seg).to(dev())
    assert torch.equal(torch.argmax(t, 1).cpu(), torch.from_numpy(host))   # the restatement's arg-max is torch's
    assert_split_equals_restatement(t, host, CN, logits=True)
    # channels-last logits: strides, not a copy
    assert_split_equals_restatement(t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), host, CN, logits=True)


@pytest.mark.parametrize("mode", ["exact", "literal", "approx"])
@pytest.mark.parametrize("vn,hn", [(9, 128), (2, 64)])
def test_full_call_equals_v3_on_the_materialised_batch(mode, vn, hn):
    labels = torch.from_numpy(LABELS).to(dev())
    v32 = torch.from_numpy(field(vn)).to(dev())
    kw = dict(literal=mode == "literal", approx=mode == "approx")
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        out, dbg = assert_equals_definition(labels, v32.to(dt), CN, hn, seed=21, **kw)
        assert dbg["mode"] == mode
    st = dbg["status"].view(B0, NK, vn).cpu()
    skipped = (st & voting.S_SKIPPED) != 0
    assert skipped[1, 0].all() and skipped[1, 1].all() and (out[1, :2] == 0).all()   # absent / fewer than min_num pixels: zeros
    assert not skipped[0].any() and not skipped[2].any() and not skipped[1, 2].any() and not (st & voting.S_OVERFLOW).any()
    tn0, tn = dbg["tn0"].cpu(), dbg["tn"].cpu()
    assert tn0.tolist() == [int((RS.class_of(LABELS, CN)[i] == k + 1).sum()) for i in range(B0) for k in range(NK)]
    assert 0 < tn[0] < tn0[0] and tn[1] == tn0[1] and tn[3] == 0            # the large class is thinned, the small one kept whole


def test_full_call_with_image_offset_explicit_idxs_and_a_planar_field():
    labels = torch.from_numpy(LABELS).to(dev())
    vn, hn = 9, 128
    v = torch.from_numpy(field(vn)).to(dev())
    _, dbg = assert_equals_definition(labels, v, CN, hn, seed=4, image_offset=5)
    _, dbg0 = assert_equals_definition(labels, v, CN, hn, seed=4)
    assert torch.equal(dbg["tn0"], dbg0["tn0"]) and not torch.equal(dbg["pix"], dbg0["pix"])   # another stream thins other pixels
    # the backbone's planar layout, read in place
    planar = v.permute(0, 3, 4, 1, 2).reshape(B0, 2 * vn, H, W).contiguous()
    pv = synth.planar_to_vertex_view(planar)
    assert not pv.is_contiguous() and torch.equal(pv, v)
    out_p, _ = assert_equals_definition(labels, pv, CN, hn, seed=4, image_offset=5)
    # explicit pixel pairs per (image, class), below every virtual image's tn
    tn = dbg["tn"].cpu().numpy().astype(np.int64)
    rng = np.random.default_rng(9)
    idxs = (rng.random((B0 * NK, hn, vn, 2)) * np.maximum(tn, 1)[:, None, None, None]).astype(np.int32)
    idxs = torch.from_numpy(idxs).to(dev()).view(B0, NK, hn, vn, 2)
    for kw in (dict(), dict(literal=True), dict(approx=True)):
        assert_equals_definition(labels, v, CN, hn, seed=4, image_offset=5, idxs=idxs, **kw)
    shared = torch.zeros((hn, vn, 2), dtype=torch.int32, device=dev())    # [hn,vn,2]: one draw for all
    shared[:, :, 1] = 2
    assert_equals_definition(labels, v, CN, hn, seed=4, idxs=shared)
    # other label dtypes give the same call
    a = voting.ransac_voting_layer_v2(labels, v, CN, hn, THRESH, min_num=MIN_NUM, max_num=MAX_NUM, seed=4)
    c = voting.ransac_voting_layer_v2(labels.to(torch.int32), v, CN, hn, THRESH, min_num=MIN_NUM, max_num=MAX_NUM, seed=4)
    assert torch.equal(a, c)
    with pytest.raises(NotImplementedError):
        voting.ransac_voting_layer_v2(labels, v, CN, hn, refine_iter_num=2)
    with pytest.raises(RuntimeError, match="class_num"):
        voting.ransac_voting_layer_v2(labels, v, 1, hn)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_from_logits_equals_the_two_step_call(dt):
    rng = np.random.default_rng(3)
    seg = rng.standard_normal((B0, CN, H, W)).astype(np.float32)
    seg[0, :, 10, 10] = 0.25                     # a four-way tie
    seg[0, :, 11, 11] = (0.0, 3.0, 3.0, -1.0)    # a two-way tie
    seg[0, :, 12, 12] = (0.0, 1.0, np.nan, 9.0)  # a NaN
    seg[1, 1] = -10.0
    s = torch.from_numpy(seg).to(dev()).to(dt)
    labels = torch.argmax(s, 1)
    assert int(labels[0, 10, 10]) == 0 and int(labels[0, 11, 11]) == 1 and int(labels[0, 12, 12]) == 2
    vn, hn = 9, 128
    v = torch.from_numpy(field(vn)).to(dev())
    kw = dict(min_num=MIN_NUM, max_num=MAX_NUM, seed=8, image_offset=2, return_status=True)
    a, sa = voting.ransac_voting_layer_v2_from_logits(s, v, hn, THRESH, **kw)
    c, sc = voting.ransac_voting_layer_v2(labels, v, CN, hn, THRESH, **kw)
    assert a.shape == (B0, NK, vn, 2) and torch.equal(a, c) and torch.equal(sa, sc)
    assert ((sa[1, 0] & voting.S_SKIPPED) != 0).all() and ((sa[0] & voting.S_SKIPPED) == 0).all()


def test_clean_discs_against_the_float64_oracle():
    """three discs, one per class, each pointing at its own key-points without noise: every class's key-points within the
    project's 1e-3 px of the float64 oracle run on `mask == k + 1` with the virtual image's RNG stream"""
    vn, hn, cn = 9, 128, 4
    rng = np.random.default_rng(12)
    centres = [(22, 20), (72, 30), (45, 54)]
    lab = np.zeros((1, H, W), np.int64)
    planar = np.zeros((2 * vn, H, W), np.float32)
    kps = []
    for k, (cx, cy) in enumerate(centres):
        fg = synth.disk_mask(H, W, cx, cy, 11)
        lab[0][fg] = k + 1
        kp = np.stack([rng.uniform(cx - 16, cx + 16, vn), rng.uniform(cy - 16, cy + 16, vn)], 1)
        planar += synth.field_from_keypoints(fg, kp)
        kps.append(kp)
    vnp = synth.planar_to_vertex_view(planar[None])
    out, st = voting.ransac_voting_layer_v2(torch.from_numpy(lab).to(dev()), synth.planar_to_vertex_view(torch.from_numpy(planar[None]).to(dev())),
                                            cn, hn, THRESH, seed=3, image_offset=1, return_status=True)
    got = out.cpu().numpy()
    assert (st == 0).all()
    for k in range(cn - 1):
        ref = O.ransac_voting_layer_v3((lab == k + 1).astype(np.uint8), vnp, hn, inlier_thresh=THRESH, seed=3, image_offset=1 + k)
        err = float(np.abs(got[0, k] - ref[0]).max())
        print(f"class {k + 1}: {err:.3e} px from the float64 oracle, {float(np.abs(got[0, k] - kps[k]).max()):.3e} px from the key-points")
        assert err < 1e-3, (k, err)


def test_two_classes_equal_v3_on_the_binary_mask():
    vn, hn = 9, 128
    v = torch.from_numpy(field(vn)).to(dev())
    m = torch.from_numpy((LABELS == 3).astype(np.int64)).to(dev())
    for kw in (dict(), dict(approx=True)):
        a, sa = voting.ransac_voting_layer_v2(m, v, 2, hn, THRESH, min_num=MIN_NUM, max_num=MAX_NUM, seed=6, return_status=True, **kw)
        c, sc = voting.ransac_voting_layer_v3(m, v, hn, THRESH, min_num=MIN_NUM, max_num=MAX_NUM, seed=6, return_status=True,
                                              concurrent=False, **kw)
        assert a.shape == (B0, 1, vn, 2) and torch.equal(a[:, 0], c) and torch.equal(sa[:, 0], sc)
    kw = dict(min_num=MIN_NUM, max_num=MAX_NUM, seed=6)
    assert torch.equal(voting.ransac_voting_layer_v2(m.bool(), v, 2, hn, THRESH, **kw), voting.ransac_voting_layer_v2(m, v, 2, hn, THRESH, **kw))


def test_workspace_reuse_leaves_no_stale_bits():
    vn, hn = 2, 64
    v = torch.from_numpy(field(vn)).to(dev())
    first = torch.from_numpy(LABELS).to(dev())
    other = torch.from_numpy(np.ascontiguousarray(np.roll(LABELS[::-1], 17, axis=2))).to(dev())   # other images, other places
    ws = torch.full((voting.vote_layout(B0 * NK, H, W, vn, hn, MAX_NUM).total_bytes,), 0xFF, dtype=torch.uint8, device=dev())
    kw = dict(min_num=MIN_NUM, max_num=MAX_NUM, seed=13, return_debug=True)
    voting.ransac_voting_layer_v2(first, v, CN, hn, THRESH, workspace=ws, **kw)
    again, dbg = voting.ransac_voting_layer_v2(other, v, CN, hn, THRESH, workspace=ws, **kw)
    fresh, fdbg = voting.ransac_voting_layer_v2(other, v, CN, hn, THRESH, **kw)
    torch.cuda.synchronize()
    want = RS.split(other.cpu().numpy(), CN, MAX_NUM, 13)[0]
    assert np.array_equal(dbg["bits"].cpu().numpy().view(np.uint64), want)      # every word written, zero words included
    assert torch.equal(again, fresh) and torch.equal(dbg["status"], fdbg["status"]) and torch.equal(dbg["ctrl"][:B0 * NK, :2], fdbg["ctrl"][:B0 * NK, :2])


def test_graph_capture_with_a_caller_owned_workspace():
    vn, hn = 9, 128
    labels = torch.from_numpy(LABELS).to(dev())
    v = torch.from_numpy(field(vn)).to(dev())
    ws = zero_ws(B0 * NK, vn, hn)
    out = torch.zeros((B0, NK, vn, 2), dtype=torch.float32, device=dev())
    kw = dict(min_num=MIN_NUM, max_num=MAX_NUM, seed=17, image_offset=3)
    ref = voting.ransac_voting_layer_v2(labels, v, CN, hn, THRESH, **kw)

    def enqueue():
        voting.ransac_voting_layer_v2(labels, v, CN, hn, THRESH, workspace=ws, out=out, **kw)

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
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_per_class_confidence_and_distribution_on_the_debug_dict():
    vn, hn = 9, 128
    labels = torch.from_numpy(LABELS).to(dev())
    v = torch.from_numpy(field(vn)).to(dev())
    out, dbg = assert_equals_definition(labels, v, CN, hn, seed=19)
    masks, rep = materialised(labels, v, CN)
    ref, rdbg = voting.ransac_voting_layer_v3(masks, rep, hn, THRESH, min_num=MIN_NUM, max_num=MAX_NUM, seed=19, return_debug=True,
                                              concurrent=False)
    B = B0 * NK
    conf = voting.vote_confidence(dbg, out.view(B, vn, 2), 0.999)
    assert conf.shape == (B, vn) and torch.equal(conf, voting.vote_confidence(rdbg, ref, 0.999))
    live = ((dbg["status"] & voting.S_SKIPPED) == 0).all(1)
    assert live.sum() == 7 and (conf[live] > 0.2).all() and (conf[~live] == 0).all()
    # the device part of estimate_voting_distribution_with_mean: pvnet_vote_distribution on either workspace
    import ctypes as C
    covs = []
    for d, mean in ((dbg, out.view(B, vn, 2).contiguous()), (rdbg, ref)):
        cov = torch.empty((B, vn, 2, 2), dtype=torch.float32, device=dev())
        voting._check(voting.load_library().pvnet_vote_distribution(C.c_void_p(mean.data_ptr()), C.c_void_p(cov.data_ptr()),
                                                                    *voting._ws_tail(d["layout"], MAX_NUM, d["workspace"])), "distribution")
        covs.append(cov)
    torch.cuda.synchronize()
    assert torch.equal(covs[0], covs[1]) and torch.isfinite(covs[0][live]).all()
