"""GPU tests of the targets of several objects (pvnet_amd/validation.py, pvnet_amd/csrc/class_targets.hip, libpvnet_class_targets.so).

The bar is EQUALITY everywhere but the two bars of the chain test, as in tests/test_targets_device.py:

* the materialised targets against the float64 numpy restatement (tests/class_targets_restatement.py) and against the per-class
  SELECTION of ``vertex_targets_device`` calls, ``torch.equal`` and on the float32 bit patterns (a ``-0.0`` is seen);
* the fused head against the existing head on the materialised class targets: the same float32 targets enter the same float64 sums in
  the same order.

Shapes are the smallest at which the kernels can go wrong: 48 x 64 (fast path, three segments), 37 x 53 (h w no multiple of 8: the
general path), 1 x 1, 3 x 1024 (a lane's eight pixels never wrap) and 8 x 1 (they wrap at every pixel); class counts 2, 4, 14, 64 and
a table of 3 x 17 key-points; 120 x 160 for the chain through the renderer, the per-class vote and the per-class pose solve."""
import numpy as np
import pytest
import torch

from pvnet_amd import synth
from pvnet_amd import validation as V
from tests import class_targets_cases as CASES
from tests.class_targets_restatement import vertex_targets_classes_f64

pytestmark = pytest.mark.gpu

SHAPES = [(48, 64), (37, 53), (1, 1), (3, 1024), (8, 1)]
CLASSES = [(2, 9), (4, 4), (14, 9), (64, 2), (3, 17)]
NP_DTYPES = {torch.uint8: np.uint8, torch.bool: np.bool_, torch.int32: np.int32, torch.int64: np.int64}


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def same(a, b):
    """torch.equal with NaN == NaN (a NaN key-point gives NaN targets on both sides)"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def same_bits(a, b):
    """the float32 bit patterns are equal (-0.0 is not +0.0) wherever the values are no NaN, and the NaNs sit at the same places"""
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.contiguous().view(torch.int32)[~nan], b.contiguous().view(torch.int32)[~nan])


def stored(labels):
    """the labels as integers, as the device reads them"""
    return labels.cpu().numpy().astype(np.int64)


def scales(kind, b, nk):
    """None, [b] or [b,nk] with a zero and a negative entry"""
    if kind == 0:
        return None
    ws = np.linspace(-0.75, 1.5, b * nk).astype(np.float32).reshape(b, nk)
    ws[0, 0], ws[-1, -1] = 0.0, -0.375
    return ws[:, 0].copy() if kind == 1 else ws


def selection_of_single_class_calls(labels, hc, ws, motion):
    """what the feature replaces, combined by selection: one ``vertex_targets_device`` call per class on ``labels == k + 1``"""
    b, nk = hc.shape[0], hc.shape[1]
    full = None if ws is None else (ws[:, None].expand(b, nk) if ws.dim() == 1 else ws)
    lab = labels.to(torch.int64)
    vertex = torch.zeros((b, 2 * hc.shape[2]) + tuple(labels.shape[1:]), dtype=torch.float32, device=labels.device)
    weights = torch.zeros((b, 1) + tuple(labels.shape[1:]), dtype=torch.float32, device=labels.device)
    for k in range(nk):
        own = (lab == k + 1)
        v, wgt = V.vertex_targets_device(own.to(torch.uint8), hc[:, k].contiguous(), None if full is None else full[:, k].contiguous(),
                                         use_motion=motion)
        vertex = torch.where(own[:, None], v, vertex)
        weights = torch.where(own[:, None], wgt, weights)
    return vertex, weights


def check_targets(labels, hc_np, ws_np=None, motion=False, out=None, what="", single=True):
    """device against the restatement and against the selection of single-class calls; returns the device's outputs"""
    hc = cuda(hc_np)
    ws = None if ws_np is None else cuda(ws_np)
    vertex, weights = V.vertex_targets_classes_device(labels, hc, ws, use_motion=motion, out=out)
    torch.cuda.synchronize()
    want_v, want_w = vertex_targets_classes_f64(stored(labels), hc_np, ws_np, motion)
    got_v, got_w = vertex.cpu(), weights.cpu()
    diff = int((~((got_v == torch.from_numpy(want_v)) | (torch.isnan(got_v) & torch.from_numpy(np.isnan(want_v))))).sum())
    print(f"{what}: {got_v.numel()} target elements, {int((got_v != 0).sum())} non-zero, {diff} differ from the restatement")
    assert same(got_v, torch.from_numpy(want_v)) and same_bits(got_v, torch.from_numpy(want_v)), what
    assert torch.equal(got_w, torch.from_numpy(want_w)) and same_bits(got_w, torch.from_numpy(want_w)), what
    if single:
        sel_v, sel_w = selection_of_single_class_calls(labels, hc, ws, motion)
        assert same(vertex, sel_v) and same_bits(vertex, sel_v) and torch.equal(weights, sel_w) and same_bits(weights, sel_w), what
    return vertex, weights


# ---- 1. the materialised outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("class_num,vn", CLASSES)
def test_materialised_targets_equal_the_restatement_and_the_selection(h, w, class_num, vn):
    """every label dtype, both motion modes, every label builder, the three forms of weight_scale -- on one shape and class count"""
    b, nk, run = 2, class_num - 1, 0
    for builder in sorted(CASES.BUILDERS):
        base = CASES.BUILDERS[builder](b, h, w, class_num)
        hc = CASES.class_keypoints(base, class_num, vn, seed=h + w + class_num, minus_zero=True)
        for dt in (torch.uint8, torch.bool, torch.int32, torch.int64):
            labels = cuda(CASES.as_dtype(base, NP_DTYPES[dt]))
            assert labels.dtype == dt
            for motion in (False, True):
                run += 1
                got = check_targets(labels, hc, scales(run % 3, b, nk), motion, what=f"{builder} {dt} {h}x{w} C={class_num} vn={vn} motion={motion}",
                                    single=nk <= 13 or run % 8 == 0)   # (63 launches a comparison: one run in eight at 64 classes)
                if builder.startswith("stripes") and dt == torch.int64 and w >= 8 and (labels[0] == 1).any():
                    assert (got[0][0, 2 * vn - 2][labels[0] == 1].view(torch.int32) == -2 ** 31).all()   # class 1's planted -0.0


def test_strided_labels_strided_and_misaligned_outputs_one_output_only():
    d = dev()
    b, h, w, class_num, vn = 2, 40, 56, 4, 3
    base = CASES.planted(b, h, w, class_num)
    hc = CASES.class_keypoints(base, class_num, vn, seed=9)
    ws = scales(2, b, class_num - 1)
    labels = cuda(base)
    want = check_targets(labels, hc, ws, what="contiguous")
    # a window of a wider tensor, and channels-last storage
    wide = torch.full((b, 2 * vn, 48, 72), -7.0, device=d)
    wcl = torch.full((b, h, w, 1), -7.0, device=d).permute(0, 3, 1, 2)
    got = check_targets(labels, hc, ws, out=(wide[:, :, 3:43, 9:65], wcl), what="window / channels-last")
    assert got[0].data_ptr() == wide[:, :, 3:43, 9:65].data_ptr() and same_bits(got[0], want[0]) and same_bits(wcl, want[1])
    frame = wide.clone()
    frame[:, :, 3:43, 9:65] = -7.0
    assert (frame == -7.0).all()   # nothing outside the window was written

    def shifted(shape, k=1):
        flat = torch.full((int(np.prod(shape)) + k,), -7.0, device=d)
        out = flat[k:].view(shape)
        assert out.data_ptr() % 16 != 0
        return flat, out

    fv, ov = shifted((b, 2 * vn, h, w))
    fw, ow = shifted((b, 1, h, w), 3)
    check_targets(labels, hc, ws, out=(ov, ow), what="misaligned outputs")
    assert same_bits(ov, want[0]) and same_bits(ow, want[1]) and fv[0] == -7.0 and (fw[:3] == -7.0).all()
    # strided labels (every second column of a wider image), misaligned uint8 labels
    lab_wide = torch.zeros((b, h, 2 * w), dtype=torch.int64, device=d)
    lab_wide[:, :, ::2] = labels
    got = check_targets(lab_wide[:, :, ::2], hc, ws, what="strided labels")
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    l8 = torch.zeros(labels.numel() + 3, dtype=torch.uint8, device=d)
    l8[3:] = cuda(CASES.as_dtype(base, np.uint8)).reshape(-1)
    got = check_targets(l8[3:].view(labels.shape), hc, ws, what="misaligned labels")
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])   # (-1 stored as 255: outside the classes either way)
    # one output only: the other is not made
    hcd, wsd = cuda(hc), cuda(ws)
    only_v = V.vertex_targets_classes_device(labels, hcd, wsd, out=(torch.empty_like(want[0]), None))
    only_w = V.vertex_targets_classes_device(labels, hcd, wsd, out=(None, torch.empty_like(want[1])))
    torch.cuda.synchronize()
    assert only_v[1] is None and only_w[0] is None and same_bits(only_v[0], want[0]) and same_bits(only_w[1], want[1])
    with pytest.raises(RuntimeError, match="out"):
        V.vertex_targets_classes_device(labels, hcd, out=(None, None))
    with pytest.raises(RuntimeError, match=r"\[b,C-1,vn,3\]"):
        V.vertex_targets_classes_device(labels, hcd[:, 0])
    with pytest.raises(RuntimeError, match=r"\[b,C-1,vn,3\]"):
        V.vertex_targets_classes_device(labels, hcd[:1])
    with pytest.raises(RuntimeError, match="weight_scale"):
        V.vertex_targets_classes_device(labels, hcd, wsd[:, :2])
    with pytest.raises(RuntimeError, match=r"\[b,C-1,vn,3\]"):
        V.vertex_targets_classes_device(labels, torch.zeros((b, 64, 2, 3), dtype=torch.float64, device=d))   # 65 classes
    empty = V.vertex_targets_classes_device(labels[:0], hcd[:0])
    assert empty[0].shape == (0, 2 * vn, h, w) and empty[1].shape == (0, 1, h, w)
    # float32 key-points widen exactly, and [b,nk,vn,2] is hz = 1
    hc1 = hc.astype(np.float32).astype(np.float64)
    hc1[..., 2] = 1.0
    a, _ = V.vertex_targets_classes_device(labels, cuda(hc1))
    c, _ = V.vertex_targets_classes_device(labels, cuda(hc1.astype(np.float32)))
    e, _ = V.vertex_targets_classes_device(labels, cuda(hc1[..., :2]))
    assert same_bits(a, c) and same_bits(a, e)


# ---- 2. one class on 0/1 masks is the single-class library ---------------------------------------------------------------------------
def upstream_for(b, d):
    return torch.from_numpy(np.stack([np.linspace(0.5, 1.5, b), np.linspace(2.0, 0.25, b)], 1)).to(d)


def predictions(b, class_num, vn, h, w, seed, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    seg = torch.randn((b, class_num, h, w), generator=g) * 3.0
    vp = torch.randn((b, 2 * vn, h, w), generator=g)
    return seg.to(dtype).to(dev()), vp.to(dtype).to(dev())


@pytest.mark.parametrize("h,w", [(48, 64), (37, 53)])
@pytest.mark.parametrize("dt", [torch.uint8, torch.bool, torch.int64])
def test_one_class_on_binary_masks_equals_the_single_class_entries(h, w, dt):
    d = dev()
    b, vn = 3, 4
    base = CASES.three_discs(b, h, w, 2)
    mask = cuda(CASES.as_dtype(base, NP_DTYPES[dt]))
    hc = cuda(CASES.class_keypoints(base, 2, vn, seed=h))
    seg, vp = predictions(b, 2, vn, h, w, seed=w)
    up = upstream_for(b, d)
    # a negative scale: the background weighs 0 * scale = -0.0 there and 0.0f here -- equal as numbers, and so is everything after
    neg = torch.tensor([0.0, 1.0, -0.625], device=d)
    one, many = V.vertex_targets_device(mask, hc[:, 0].contiguous(), neg), V.vertex_targets_classes_device(mask, hc, neg)
    assert torch.equal(many[0], one[0]) and same_bits(many[0], one[0]) and torch.equal(many[1], one[1])
    assert same_bits(many[1][:2], one[1][:2]) and (one[1][2].view(torch.int32) == -2 ** 31).any() and not (many[1].view(torch.int32) == -2 ** 31).any()
    m1, mc = V.head_metrics_from_keypoints(seg, vp, mask, hc[:, 0].contiguous(), neg), V.head_metrics_from_class_keypoints(seg, vp, mask, hc, neg)
    g1, gc = V.head_grad_from_keypoints(seg, vp, mask, hc[:, 0].contiguous(), up, neg), V.head_grad_from_class_keypoints(seg, vp, mask, hc, up, neg)
    assert all(torch.equal(a, c) for a, c in zip(mc + gc, m1 + g1))
    for ws in (None, torch.tensor([0.0, 1.0, 0.625], device=d)):
        for motion in (False, True):
            one = V.vertex_targets_device(mask, hc[:, 0].contiguous(), ws, use_motion=motion)
            many = V.vertex_targets_classes_device(mask, hc, ws, use_motion=motion)
            assert torch.equal(many[0], one[0]) and same_bits(many[0], one[0]) and torch.equal(many[1], one[1]) and same_bits(many[1], one[1])
            m1 = V.head_metrics_from_keypoints(seg, vp, mask, hc[:, 0].contiguous(), ws, sigma=0.8, use_motion=motion)
            mc = V.head_metrics_from_class_keypoints(seg, vp, mask, hc, ws, sigma=0.8, use_motion=motion)
            g1 = V.head_grad_from_keypoints(seg, vp, mask, hc[:, 0].contiguous(), up, ws, sigma=0.8, use_motion=motion)
            gc = V.head_grad_from_class_keypoints(seg, vp, mask, hc, up, ws, sigma=0.8, use_motion=motion)
            torch.cuda.synchronize()
            assert all(torch.equal(a, c) for a, c in zip(mc + gc, m1 + g1))
    if dt != torch.bool:   # the one deliberate difference: a mask VALUE of 2 is no target pixel in either, weighs 2 there and 0 here
        mask[0, 1, 1] = 2
        one = V.vertex_targets_device(mask, hc[:, 0].contiguous())
        many = V.vertex_targets_classes_device(mask, hc)
        assert torch.equal(many[0], one[0]) and float(one[1][0, 0, 1, 1]) == 2.0 and float(many[1][0, 0, 1, 1]) == 0.0


# ---- 3. the fused forward and backward ----------------------------------------------------------------------------------------------
def check_fused(seg, vp, labels, hc, ws=None, sigma=1.0, motion=False, what="", need=(True, True), out=None):
    """the fused forward and backward against the existing head on the materialised class targets: equality"""
    b = seg.shape[0]
    vt, vw = V.vertex_targets_classes_device(labels, hc, ws, use_motion=motion)
    want = V.head_metrics_device(seg, vp, labels, vt, vw, sigma=sigma)
    got = V.head_metrics_from_class_keypoints(seg, vp, labels, hc, ws, sigma=sigma, use_motion=motion)
    up = upstream_for(b, seg.device)
    gwant = V.head_grad_device(seg, vp, labels, vt, vw, up, sigma=sigma, need=need)
    ggot = V.head_grad_from_class_keypoints(seg, vp, labels, hc, up, ws, sigma=sigma, use_motion=motion, need=need, out=out)
    torch.cuda.synchronize()
    assert got[0].dtype == torch.float64 and same(got[0], want[0]), (what, got[0], want[0])
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), what
    for k in range(2):
        assert (ggot[k] is None) == (not need[k]) and (gwant[k] is None) == (not need[k])
        if need[k]:
            assert ggot[k].dtype == (seg, vp)[k].dtype and same(ggot[k], gwant[k]), (what, k)
    assert torch.equal(ggot[2], gwant[2]), what
    return got, ggot


@pytest.mark.parametrize("pred_dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("h,w", [(48, 64), (37, 53)])
def test_fused_equals_materialised(pred_dtype, h, w):
    """fast and general path, every prediction type, every label builder at four classes; then 14 and 64 classes, a scale per class,
    sigma other than 1, motion, one gradient half only"""
    d = dev()
    b, class_num, vn = 2, 4, 4
    seg, vp = predictions(b, class_num, vn, h, w, seed=h + 7, dtype=pred_dtype)
    for builder in ("discs", "stripes3", "stripes5", "absent", "empty"):
        base = CASES.BUILDERS[builder](b, h, w, class_num)
        labels, hc = cuda(base), cuda(CASES.class_keypoints(base, class_num, vn, seed=11, minus_zero=True))
        got, ggot = check_fused(seg, vp, labels, hc, what=f"{builder} {pred_dtype} {h}x{w}")
        assert torch.isfinite(got[0]).all() and float(got[0][0, 1]) > 0.0 and float(ggot[1].float().abs().max()) > 0.0   # (image 1 may be empty)
        assert got[2].tolist() == [0, 0]
    ws = cuda(scales(2, b, class_num - 1))
    check_fused(seg, vp, labels, hc, ws, sigma=0.6, what="a scale per class, sigma 0.6")
    check_fused(seg, vp, labels, hc, ws[:, 0].contiguous(), motion=True, what="a scale per image, motion")
    check_fused(seg.float(), vp, labels, hc, what="float32 logits")
    check_fused(seg, vp.float(), labels, hc, sigma=2.0, what="float32 field")
    for need in ((True, False), (False, True)):
        check_fused(seg, vp, labels, hc, ws, need=need, what=f"need={need}")
    for class_num, vn in ((14, 9), (64, 2), (3, 17)):
        seg, vp = predictions(b, class_num, vn, h, w, seed=class_num, dtype=pred_dtype)
        for builder in ("discs", "stripes3"):
            base = CASES.BUILDERS[builder](b, h, w, class_num)
            check_fused(seg, vp, cuda(CASES.as_dtype(base, np.uint8)), cuda(CASES.class_keypoints(base, class_num, vn, seed=3)),
                        cuda(scales(2, b, class_num - 1)), what=f"{builder} C={class_num} vn={vn}")


@pytest.mark.parametrize("h,w", [(48, 64), (37, 53)])
def test_fused_bad_labels_and_a_nan_keypoint_in_one_class(h, w):
    d = dev()
    b, class_num, vn = 2, 4, 3
    seg, vp = predictions(b, class_num, vn, h, w, seed=5)
    base = CASES.stripes(b, h, w, class_num, 5)
    hc_np = CASES.class_keypoints(base, class_num, vn, seed=13)
    # labels outside 0 .. C-1 in image 1: the status bit and a NaN loss_seg; no target and weight 0 for the field, which stays finite
    bad = base.copy()
    bad[1, 2, 3], bad[1, h // 2, w // 2], bad[1, h - 1, w - 1] = class_num, -1, 255
    for dt in (torch.int64, torch.int32, torch.uint8):
        got, ggot = check_fused(seg, vp, cuda(CASES.as_dtype(bad, NP_DTYPES[dt])), cuda(hc_np), what=f"bad labels {dt}")
        assert got[2].tolist() == [0, V.HEAD_S_BAD_LABEL] and ggot[2].tolist() == [0, V.HEAD_S_BAD_LABEL]
        assert torch.isnan(got[0][1, 0]) and torch.isfinite(got[0][1, 1]) and torch.isfinite(got[0][0]).all()
        assert int(torch.isnan(ggot[0]).sum()) == 3 * class_num and torch.isfinite(ggot[1]).all()
    only_v = V.head_grad_from_class_keypoints(seg, vp, cuda(bad), cuda(hc_np), upstream_for(b, d), need=(False, True))
    assert only_v[2].tolist() == [0, 0]   # without the logits' half no label is judged
    # a NaN key-point of class 2 in image 1: NaN targets on that class's pixels of that key-point only, whatever the class weighs
    hc_np[1, 1, 2, 0] = np.nan
    labels = cuda(base)
    for ws in (None, np.array([[1.0, 1.0, 1.0], [1.0, 0.0, 1.0]], np.float32)):
        vt, _ = check_targets(labels, hc_np, ws, what="NaN key-point")
        nan = torch.isnan(vt)
        want = torch.zeros_like(nan)
        want[1, 4:6] = (labels[1] == 2)[None]
        assert torch.equal(nan, want) and int(nan.sum()) > 0
        got, ggot = check_fused(seg, vp, labels, cuda(hc_np), None if ws is None else cuda(ws), what="NaN key-point")
        assert torch.isnan(got[0][1, 1]) and torch.isfinite(got[0][0, 1]) and torch.isfinite(got[0][:, 0]).all()
        assert torch.equal(torch.isnan(ggot[1]), want)
    # a NaN prediction at a background pixel reaches the loss and the gradient as 0 * NaN: the predictions are read at every pixel
    hc_np[1, 1, 2, 0] = 7.0
    bg = (labels[0] == 0).nonzero()[0]
    vp[0, 2, bg[0], bg[1]] = float("nan")
    got, ggot = check_fused(seg, vp, labels, cuda(hc_np), what="NaN at a background pixel")
    assert torch.isnan(got[0][0, 1]) and torch.isfinite(got[0][1, 1])
    assert torch.isnan(ggot[1][0, 2, bg[0], bg[1]]) and int(torch.isnan(ggot[1]).sum()) == 1


def test_fused_strided_predictions_and_the_packed_form():
    d = dev()
    b, h, w, class_num, vn = 2, 40, 56, 4, 4
    seg, vp = predictions(b, class_num, vn, h, w, seed=5)
    base = CASES.stripes(b, h, w, class_num, 3)
    labels, hc = cuda(base), cuda(CASES.class_keypoints(base, class_num, vn, seed=2))
    want, gwant = check_fused(seg, vp, labels, hc, what="contiguous")
    seg_cl = seg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    vp_cl = vp.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    lab_wide = torch.zeros((b, h, 2 * w), dtype=torch.int64, device=d)
    lab_wide[:, :, ::2] = labels
    got, ggot = check_fused(seg_cl, vp_cl, lab_wide[:, :, ::2], hc, what="channels-last / strided labels")
    # (the general path sums a segment's pixels in another order than the fast path: the losses agree to rounding, the gradients --
    # one element each -- bit for bit; check_fused held each path to the head on the materialised targets on the SAME path)
    assert torch.allclose(got[0], want[0], rtol=1e-12, atol=0.0) and torch.equal(got[1], want[1])
    assert torch.equal(ggot[0], gwant[0]) and torch.equal(ggot[1], gwant[1])
    assert ggot[0].stride() == seg_cl.stride()
    # the two channel slices of one tensor (the network's output), gradients into the slices of one tensor
    head_out = torch.cat([seg, vp], 1)
    grad = torch.full_like(head_out, -7.0)
    got, ggot = check_fused(head_out[:, :class_num], head_out[:, class_num:], labels, hc, out=(grad[:, :class_num], grad[:, class_num:]),
                            what="packed slices")
    assert torch.equal(got[0], want[0]) and torch.equal(grad[:, :class_num], gwant[0]) and torch.equal(grad[:, class_num:], gwant[1])
    # misaligned predictions
    flat = torch.zeros(vp.numel() + 1, device=d)
    flat[1:] = vp.reshape(-1)
    got, ggot = check_fused(seg, flat[1:].view(vp.shape), labels, hc, what="misaligned field")
    assert torch.allclose(got[0], want[0], rtol=1e-12, atol=0.0) and torch.equal(ggot[1], gwant[1])
    # the modules: HeadLoss.from_class_keypoints and packed_from_class_keypoints against HeadLoss on the materialised class targets
    ws = cuda(scales(2, b, class_num - 1))
    vt, vw = V.vertex_targets_classes_device(labels, hc, ws)
    loss = V.HeadLoss(sigma=2.0)
    seg1, vp1 = seg.clone().requires_grad_(True), vp.clone().requires_grad_(True)
    hcg = hc.clone().requires_grad_(True)
    out = loss.from_class_keypoints(seg1, vp1, labels, hcg, ws)
    (out[0].mean() + 0.5 * out[1].mean()).backward()
    seg2, vp2 = seg.clone().requires_grad_(True), vp.clone().requires_grad_(True)
    ref = loss(seg2, vp2, labels, vt, vw)
    (ref[0].mean() + 0.5 * ref[1].mean()).backward()
    torch.cuda.synchronize()
    assert len(out) == 4 and all(a.dtype == torch.float32 and torch.equal(a, c) for a, c in zip(out, ref))
    assert all(torch.equal(a, c) for a, c in zip(V.HeadMetrics(sigma=2.0).from_class_keypoints(seg, vp, labels, hc, ws), ref))
    assert out[0].grad_fn is not None and out[1].grad_fn is not None and not out[2].requires_grad and not out[3].requires_grad
    assert torch.equal(seg1.grad, seg2.grad) and torch.equal(vp1.grad, vp2.grad) and hcg.grad is None
    vp3 = vp.clone().requires_grad_(True)   # needs_input_grad is honoured: one half alone gives the same bits
    loss.from_class_keypoints(seg, vp3, labels, hc, ws)[1].mean().mul(0.5).backward()
    assert torch.equal(vp3.grad, vp2.grad)
    packed_in = torch.cat([seg, vp], 1).requires_grad_(True)
    packed = loss.packed_from_class_keypoints(packed_in, class_num, labels, hc, ws)
    (packed[0].mean() + 0.5 * packed[1].mean()).backward()
    torch.cuda.synchronize()
    assert all(torch.equal(a, c) for a, c in zip(packed, ref))
    assert torch.equal(packed_in.grad[:, :class_num], seg2.grad) and torch.equal(packed_in.grad[:, class_num:], vp2.grad)
    # the autograd function saves the predictions, the labels, the key-points and the scale: nothing of the size of the target field
    seg4 = seg.clone().requires_grad_(True)
    fresh = loss.from_class_keypoints(seg4, vp, labels, hc, ws)
    saved = fresh[0].grad_fn.saved_tensors
    assert len(saved) == 5 and sorted(t.numel() for t in saved) == sorted(t.numel() for t in (seg, vp, labels, hc, ws))
    with pytest.raises(RuntimeError, match=r"\[b,C-1,vn,3\] with C-1=3"):
        V.head_metrics_from_class_keypoints(seg, vp, labels, hc[:, :2])   # the logits' class count is the targets'
    with pytest.raises(RuntimeError, match="vertex_pred"):
        V.head_metrics_from_class_keypoints(seg, vp[:, :6], labels, hc)


# ---- 4. workspace and measurement flags ---------------------------------------------------------------------------------------------
def test_two_calls_on_a_dirty_workspace_agree_and_the_measurement_flags_change_nothing():
    d = dev()
    b, h, w, class_num, vn = 3, 96, 128, 5, 9
    seg, vp = predictions(b, class_num, vn, h, w, seed=17)
    base = CASES.three_discs(b, h, w, class_num)
    base[2] = CASES.stripes(1, h, w, class_num, 3)[0]
    labels, hc = cuda(base), cuda(CASES.class_keypoints(base, class_num, vn, seed=4))
    up = upstream_for(b, d)
    lib = V.load_class_targets_library()
    nm, ng = lib.pvnet_head_metrics_ckp_workspace_bytes(b, h, w), lib.pvnet_head_grad_ckp_workspace_bytes(b, h, w)
    res = []
    for fill in (0xFF, 0x7F):   # NaN patterns / set flags if anything of a workspace were read before it is written
        out = (torch.full((b, 4), -1.0, dtype=torch.float64, device=d), torch.full((b, 3), -1, dtype=torch.int64, device=d),
               torch.full((b,), -1, dtype=torch.int32, device=d))
        m = V.head_metrics_from_class_keypoints(seg, vp, labels, hc, out=out, workspace=torch.full((nm,), fill, dtype=torch.uint8, device=d))
        g = V.head_grad_from_class_keypoints(seg, vp, labels, hc, up, workspace=torch.full((ng,), fill, dtype=torch.uint8, device=d))
        torch.cuda.synchronize()
        assert m[0] is out[0] and m[1] is out[1] and m[2] is out[2]
        res.append([t.clone() for t in m + g])
    assert all(torch.equal(a, c) for a, c in zip(*res)) and torch.isfinite(res[0][0]).all()
    for flags in (V.HEAD_F_NT_NONE, V.HEAD_F_NT_ALL):
        m = V.head_metrics_from_class_keypoints(seg, vp, labels, hc, flags=flags)
        g = V.head_grad_from_class_keypoints(seg, vp, labels, hc, up, flags=flags)
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(m + g, res[0]))
    with pytest.raises(RuntimeError, match="PVNET_E_WORKSPACE"):
        V.head_metrics_from_class_keypoints(seg, vp, labels, hc, workspace=torch.empty(nm - 256, dtype=torch.uint8, device=d))
    with pytest.raises(RuntimeError, match="PVNET_E_WORKSPACE"):
        V.head_grad_from_class_keypoints(seg, vp, labels, hc, up, workspace=torch.empty(ng - 256, dtype=torch.uint8, device=d))
    with pytest.raises(RuntimeError, match="need"):
        V.head_grad_from_class_keypoints(seg, vp, labels, hc, up, need=(False, False))
    empty = V.head_grad_from_class_keypoints(seg[:0], vp[:0], labels[:0], hc[:0], up[:0])
    assert empty[0].shape == (0, class_num, h, w) and empty[1].shape == (0, 2 * vn, h, w) and empty[2].shape == (0,)


# ---- 5. graph replay -----------------------------------------------------------------------------------------------------------------
def test_graph_of_forward_and_backward_replays_on_changed_labels_and_keypoints():
    """a forward + backward through HeadLoss.from_class_keypoints captured in a torch.cuda.graph with the process's default queue
    count, replayed after the labels and the key-points changed in place: the replay equals an eager step on the new inputs bit for bit
    (PyTorch's rules for capturing a backward as in tests/test_targets_device.py: a warm-up on a side stream, detached results only)"""
    b, h, w, class_num, vn = 4, 96, 128, 4, 9
    seg0, vp0 = predictions(b, class_num, vn, h, w, seed=37)
    first_np, second_np = CASES.three_discs(b, h, w, class_num, seed=5), CASES.stripes(b, h, w, class_num, 5)
    hc_a, hc_b = CASES.class_keypoints(first_np, class_num, vn, seed=1), CASES.class_keypoints(second_np, class_num, vn, seed=2)
    seg, vp = seg0.clone().requires_grad_(True), vp0.clone().requires_grad_(True)
    labels_in, hc_in = cuda(first_np), cuda(hc_a)
    loss = V.HeadLoss()

    def step():
        seg.grad = vp.grad = None
        ls, lv, pr, rc = loss.from_class_keypoints(seg, vp, labels_in, hc_in)
        total = ls.mean() + 0.5 * lv.mean()
        total.backward()
        return [t.detach() for t in (total, ls, lv, pr, rc, seg.grad, vp.grad)]

    def eager():
        out = step()
        torch.cuda.synchronize()
        return [t.clone() for t in out]

    first = eager()
    assert all(torch.equal(a, c) for a, c in zip(first, eager()))   # two calls agree bitwise
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    seg.grad = vp.grad = None
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    names = ("total", "loss_seg", "loss_vertex", "precision", "recall", "grad_seg", "grad_vertex")
    for name, a, c in zip(names, captured, first):
        assert torch.equal(a, c), name
    with torch.no_grad():   # new labels and key-points in the captured tensors
        labels_in.copy_(cuda(second_np))
        hc_in.copy_(cuda(hc_b))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    del captured, graph
    second = eager()
    for name, a, c in zip(names, replayed, second):
        assert torch.equal(a, c), name
    assert not torch.equal(second[6], first[6]) and torch.isfinite(second[6]).all() and float(second[6].abs().max()) > 0.0


# ---- 6. the chain the feature exists for ---------------------------------------------------------------------------------------------
# twice the measured share of differing label pixels: 0 of 19 200 from render_labels' image; 3 of 19 200 from render_visible_labels'
# image, which is compared with render_labels' image of the solved poses -- the two renderers' images of the INPUT poses differ there
CLASS_HAND_OVER_BAR = {"render_labels": 2 * 0.0, "render_visible_labels": 2 * (3 / 19200.0)}


@pytest.mark.parametrize("renderer", ["render_labels", "render_visible_labels"])
def test_labels_to_targets_to_the_class_vote_to_the_class_poses(renderer):
    """render_labels / render_visible_labels -> ONE vertex_targets_classes_device call -> ransac_voting_layer_v2 -> pnp_classes_device ->
    render_labels of the solved poses, at 120 x 160 with the three meshes and poses of tests/test_raster_device.py::
    test_label_image_is_a_valid_input_of_the_class_vote; the key-points of a class are its bounding box's corners and its origin (the
    pose solve takes six or more).

    MEASURED on one MI355X (19 200 pixels, three classes): the one call's field equals that test's loop-and-add field; the voted
    key-points lie within the printed distance of the projected ones (bar: 1e-3 px, that of the existing hand-over test and of
    smoke()): measured 0.0 px for every class; render_labels' image of the solved poses differs from render_labels' input image in 0 of
    19 200 pixels and from render_visible_labels' input image in 3 (1.5625e-4).  The bar is twice the measured share."""
    from pvnet_amd import depth, pnp, render, voting
    from tests import raster_restatement as RS
    from tests.render_cases import camera, pose
    d = dev()
    h, w = 120, 160
    K = camera(h, w)
    meshes = [render.icosphere(2, 0.07), render.box_mesh(0.12, 0.09, 0.1), render.l_prism_mesh(0.16, 0.07)]
    table = render.DeviceMeshes(meshes)
    poses = np.stack([pose((1, 2, 3), 0.8, (-0.12, -0.05, 0.6)), pose((2, -1, 1), 2.0, (0.10, -0.04, 0.55)),
                      pose((0, 1, 1), 0.6, (0.0, 0.08, 0.5))])[None]
    draw = render.render_labels if renderer == "render_labels" else depth.render_visible_labels
    labels = draw(table, [0, 1, 2], [1, 2, 3], cuda(poses), K, h, w)
    assert set(torch.unique(labels).cpu().tolist()) == {0, 1, 2, 3}
    kp3 = []
    for v, _ in meshes:
        lo, hi = v.min(0), v.max(0)
        kp3.append(np.array([(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])] + [(0.0, 0.0, 0.0)]))
    kp3 = np.stack(kp3)                                                                                    # [3,9,3]
    vn = kp3.shape[1]
    proj = np.stack([np.stack(RS.project_points(kp3[k], poses[0, k], K)[:2], -1).astype(np.float64) for k in range(3)])   # [3,9,2]
    hcoords = cuda(np.concatenate([proj, np.ones((3, vn, 1))], -1)[None])                                   # [1,3,9,3]
    field, weights = V.vertex_targets_classes_device(labels, hcoords)
    # that test's loop: a binary mask, a call and an add per class (torch.equal holds -0 == +0: this comparison may use addition)
    added = torch.zeros((1, 2 * vn, h, w), dtype=torch.float32, device=d)
    for k in range(3):
        vert, _ = V.vertex_targets_device((labels == k + 1).to(torch.uint8), hcoords[:, k].contiguous())
        added += vert
    assert torch.equal(field, added) and torch.equal(weights[:, 0], (labels > 0).float())
    view = synth.planar_to_vertex_view(field)
    voted, vstatus = voting.ransac_voting_layer_v2(labels, view, 4, 128, inlier_thresh=0.99, seed=5, return_status=True)
    assert tuple(voted.shape) == (1, 3, vn, 2)
    err = (voted[0].double().cpu() - torch.from_numpy(proj)).abs().amax((1, 2))
    print(f"chain ({renderer}): voted key-points within {[f'{float(e):.3e}' for e in err]} px of the projected ones, per class")
    assert float(err.max()) < 1e-3, err
    solved, status = pnp.pnp_classes_device(kp3, voted, K, vote_status=vstatus)
    assert (status.cpu() >= 0).all() and tuple(solved.shape) == (1, 3, 3, 4)
    again = render.render_labels(table, [0, 1, 2], [1, 2, 3], solved, K, h, w)
    differ = int((again != labels).sum())
    share = differ / float(labels.numel())
    print(f"chain ({renderer}): the solved poses' label image differs from the input one in {share:.6e} of the pixels ({differ} of "
          f"{labels.numel()})")
    own = int((draw(table, [0, 1, 2], [1, 2, 3], solved, K, h, w) != labels).sum())
    print(f"chain ({renderer}): {renderer} of the solved poses differs from its own input image in {own} pixels")
    assert share <= CLASS_HAND_OVER_BAR[renderer], (share, CLASS_HAND_OVER_BAR[renderer])
