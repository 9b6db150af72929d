"""GPU tests of the targets from key-points (pvnet_amd/validation.py, pvnet_amd/csrc/head_targets.hip, libpvnet_targets.so).

The bar is EQUALITY everywhere, not a tolerance:

* the materialised targets against the float64 numpy restatement (tests/targets_restatement.py) and against what the reference's own
  compute_vertex_hcoords returned (tests/golden/vertex_targets.npz): every float64 operation of the formula (multiply, subtract, add,
  square root, divide) is correctly rounded on both sides, nothing is contracted, the float32 rounding happens once;
* the fused head against the existing head on the materialised targets: the same float32 targets enter the same float64 sums in the
  same order.
"""
import os

import numpy as np
import pytest
import torch

from pvnet_amd import evaluation as E
from pvnet_amd import pnp as P
from pvnet_amd import synth
from pvnet_amd import validation as V
from tests.targets_restatement import vertex_targets_f64
from tests.test_head_metrics_device import dev, random_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "vertex_targets.npz"))
CASES = [str(n) for n in GOLDEN["cases"]]


def same(a, b):
    """torch.equal with NaN == NaN (a NaN key-point gives NaN targets on both sides); bit patterns of everything else"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def keypoints_for(mask, vn, seed, planted=True):
    """[b,vn,3] float64 key-points around each image's foreground, hz in [0.5, 2]; with `planted`, key-point 0 exactly on a foreground
    pixel (n = 0), key-point 1 5e-4 beside one (0 < n < 1e-3) -- both with hz = 1 -- and key-point 2 with hz = 0"""
    rng = np.random.default_rng(seed)
    m = mask.cpu().numpy()
    b, h, w = m.shape
    hz = rng.uniform(0.5, 2.0, (b, vn, 1))
    hc = np.concatenate([rng.uniform(-0.5 * w, 1.5 * w, (b, vn, 1)) * hz, rng.uniform(-0.5 * h, 1.5 * h, (b, vn, 1)) * hz, hz], 2)
    if planted:
        for i in range(b):
            ys, xs = np.nonzero(m[i] == 1)
            if len(ys) == 0:
                continue
            j = rng.integers(len(ys), size=2)
            hc[i, 0] = (xs[j[0]], ys[j[0]], 1.0)
            if vn > 1:
                hc[i, 1] = (xs[j[1]] + 5e-4, ys[j[1]], 1.0)
            if vn > 2:
                hc[i, 2, 2] = 0.0
    return hc


def check_targets(mask, hc, weight_scale=None, use_motion=False, out=None, what=""):
    """device against the restatement; returns the device's (vertex, vertex_weights)"""
    d = mask.device
    ws = None if weight_scale is None else torch.from_numpy(np.asarray(weight_scale, np.float32)).to(d)
    vertex, weights = V.vertex_targets_device(mask, torch.from_numpy(hc).to(d), ws, use_motion=use_motion, out=out)
    torch.cuda.synchronize()
    want_v, want_w = vertex_targets_f64(mask.cpu().numpy().astype(np.int64), hc, weight_scale, use_motion)
    got_v, got_w = vertex.cpu(), weights.cpu()
    diff = int((~((got_v == torch.from_numpy(want_v)) | (torch.isnan(got_v) & torch.from_numpy(np.isnan(want_v))))).sum())
    print(f"{what}: {got_v.numel()} target elements, {int((got_v != 0).sum())} non-zero, {diff} differ from the restatement")
    assert same(got_v, torch.from_numpy(want_v)), what
    assert torch.equal(got_w, torch.from_numpy(want_w)), what
    return vertex, weights


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.int32, torch.int64])
def test_fixture_cases_equal_the_reference_and_the_restatement(name, mask_dtype):
    d = dev()
    mask = torch.from_numpy(GOLDEN[name + ".mask"].astype(np.int64))[None].to(mask_dtype).to(d)
    hc = GOLDEN[name + ".hcoords"][None]
    for key, motion in (("ref", False), ("ref_motion", True)):
        vertex, weights = check_targets(mask, hc.astype(np.float64), use_motion=motion, what=f"{name} {key} {mask_dtype}")
        ref = torch.from_numpy(np.ascontiguousarray(np.transpose(GOLDEN[f"{name}.{key}"], (2, 0, 1))))[None]
        assert torch.equal(vertex.cpu(), ref), (name, key)
        assert torch.equal(weights.cpu()[0, 0], torch.from_numpy(GOLDEN[name + ".mask"].astype(np.float32)))
        # the key-points in the dtype the fixture stores them in (float32 widens exactly), and [vn,2] where hz = 1
        again, _ = V.vertex_targets_device(mask, torch.from_numpy(hc).to(d), use_motion=motion)
        assert torch.equal(again, vertex)
        if np.all(hc[..., 2] == 1):
            two, _ = V.vertex_targets_device(mask, torch.from_numpy(hc[..., :2].copy()).to(d), use_motion=motion)
            assert torch.equal(two, vertex)


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.bool, torch.int32, torch.int64])
@pytest.mark.parametrize("h,w", [(48, 64), (37, 53), (1, 1), (3, 1024), (8, 1), (24, 3)])
@pytest.mark.parametrize("motion", [False, True])
def test_every_mask_dtype_size_and_mode(mask_dtype, h, w, motion):
    """h w a multiple of 8 (fast path, rows shorter than a lane's eight pixels included) and not (general path)"""
    d = dev()
    _, _, mask, _, _ = random_inputs(3, h, w, 1, d, seed=h * w + 1, C=3 if mask_dtype != torch.bool else 2, mask_dtype=mask_dtype)
    if h * w == 1:
        mask[:] = 1
    hc = keypoints_for(mask.to(torch.int64), 4, seed=h + w)
    check_targets(mask, hc, use_motion=motion, what=f"{mask_dtype} {h}x{w} motion={motion}")
    check_targets(mask, hc, weight_scale=[0.0, 1.0, 0.625], use_motion=motion, what=f"{mask_dtype} {h}x{w} scaled")


def test_benchmark_size_with_planted_keypoints():
    """480 x 640 x 9 on synth.make_batch masks: key-points ON a foreground pixel, 5e-4 beside one, hz = 0, and the generator's own"""
    d = dev()
    mask_np, _, kpts = synth.make_batch(4, first_index=40)
    mask = torch.from_numpy(np.ascontiguousarray(mask_np)).to(d)
    hc = keypoints_for(mask, 9, seed=5)
    vertex, weights = check_targets(mask, hc, what="480x640 vn=9 planted")
    assert vertex.shape == (4, 18, 480, 640) and weights.shape == (4, 1, 480, 640)
    own = np.concatenate([kpts, np.ones_like(kpts[:, :, :1])], 2)
    check_targets(mask, own, use_motion=True, what="480x640 vn=9 generator key-points, motion")
    vertex, _ = check_targets(mask, own, what="480x640 vn=9 generator key-points")
    # the project's own generator follows the same definition (synth.field_from_keypoints)
    _, planar, _ = synth.make_batch(4, first_index=40)
    assert torch.equal(vertex.cpu(), torch.from_numpy(planar))


def test_strided_and_misaligned_outputs_take_the_general_path():
    d = dev()
    _, _, mask, _, _ = random_inputs(2, 40, 56, 1, d, seed=3)
    mask[0, :2, :7] = 2
    hc = keypoints_for(mask, 3, seed=9)
    base = check_targets(mask, hc, what="contiguous")
    # a window of a wider tensor, and channels-last storage
    wide = torch.full((2, 6, 48, 72), -7.0, device=d)
    wcl = torch.full((2, 40, 56, 1), -7.0, device=d).permute(0, 3, 1, 2)
    got = check_targets(mask, hc, out=(wide[:, :, 3:43, 9:65], wcl), what="window / channels-last")
    assert got[0].data_ptr() == wide[:, :, 3:43, 9:65].data_ptr() and torch.equal(got[0], base[0]) and torch.equal(wcl, base[1])
    frame = wide.clone()
    frame[:, :, 3:43, 9:65] = -7.0
    assert (frame == -7.0).all()   # nothing outside the window was written

    def shifted(shape, k=1):
        flat = torch.full((int(np.prod(shape)) + k,), -7.0, device=d)
        out = flat[k:].view(shape)
        assert out.data_ptr() % 16 != 0
        return flat, out

    fv, ov = shifted((2, 6, 40, 56))
    fw, ow = shifted((2, 1, 40, 56), 3)
    check_targets(mask, hc, out=(ov, ow), what="misaligned outputs")
    assert torch.equal(ov, base[0]) and torch.equal(ow, base[1]) and fv[0] == -7.0 and (fw[:3] == -7.0).all()
    # a strided mask (every second column of a wider one), a misaligned uint8 mask
    mask_wide = torch.zeros((2, 40, 112), dtype=torch.int64, device=d)
    mask_wide[:, :, ::2] = mask
    got = check_targets(mask_wide[:, :, ::2], hc, what="strided mask")
    assert torch.equal(got[0], base[0])
    m8 = torch.zeros(mask.numel() + 3, dtype=torch.uint8, device=d)
    m8[3:] = mask.reshape(-1).to(torch.uint8)
    got = check_targets(m8[3:].view(mask.shape), hc, what="misaligned mask")
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    # one output only: the other is not made
    only_v = V.vertex_targets_device(mask, torch.from_numpy(hc).to(d), out=(torch.empty_like(base[0]), None))
    only_w = V.vertex_targets_device(mask, torch.from_numpy(hc).to(d), out=(None, torch.empty_like(base[1])))
    torch.cuda.synchronize()
    assert only_v[1] is None and only_w[0] is None and torch.equal(only_v[0], base[0]) and torch.equal(only_w[1], base[1])
    with pytest.raises(RuntimeError, match="out"):
        V.vertex_targets_device(mask, torch.from_numpy(hc).to(d), out=(None, None))
    with pytest.raises(RuntimeError, match="hcoords"):
        V.vertex_targets_device(mask, torch.from_numpy(hc[:1]).to(d))
    empty = V.vertex_targets_device(mask[:0], torch.from_numpy(hc[:0]).to(d))
    assert empty[0].shape == (0, 6, 40, 56) and empty[1].shape == (0, 1, 40, 56)


def head_case(b, h, w, vn, d, seed, pred_dtype=torch.float32, mask_dtype=torch.int64, C=2):
    seg, vp, mask, _, _ = random_inputs(b, h, w, vn, d, seed=seed, C=C, pred_dtype=pred_dtype, mask_dtype=mask_dtype)
    hc = torch.from_numpy(keypoints_for(mask.to(torch.int64), vn, seed=seed + 100)).to(d)
    return seg, vp, mask, hc


def upstream_for(b, d):
    return torch.from_numpy(np.stack([np.linspace(0.5, 1.5, b), np.linspace(2.0, 0.25, b)], 1)).to(d)


def check_fused(seg, vp, mask, hc, weight_scale=None, sigma=1.0, use_motion=False, what="", need=(True, True), out=None):
    """the fused forward and backward against the existing head on the materialised targets: equality"""
    b = seg.shape[0]
    vt, vw = V.vertex_targets_device(mask, hc, weight_scale, use_motion=use_motion)
    want = V.head_metrics_device(seg, vp, mask, vt, vw, sigma=sigma)
    got = V.head_metrics_from_keypoints(seg, vp, mask, hc, weight_scale, sigma=sigma, use_motion=use_motion)
    up = upstream_for(b, seg.device)
    gwant = V.head_grad_device(seg, vp, mask, vt, vw, up, sigma=sigma, need=need)
    ggot = V.head_grad_from_keypoints(seg, vp, mask, hc, up, weight_scale, sigma=sigma, use_motion=use_motion, need=need, out=out)
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
    """fast and general path, every prediction type, sigma other than 1, a scale, motion, three classes"""
    d = dev()
    seg, vp, mask, hc = head_case(3, h, w, 4, d, seed=h + 7, pred_dtype=pred_dtype)
    got, ggot = check_fused(seg, vp, mask, hc, what=f"{pred_dtype} {h}x{w}")
    assert torch.isfinite(got[0]).all() and float(got[0][:, 1].min()) > 0.0 and float(ggot[1].float().abs().max()) > 0.0
    ws = torch.tensor([0.0, 1.0, 0.375], device=d)
    check_fused(seg, vp, mask, hc, ws, sigma=0.6, what="scaled, sigma 0.6")
    check_fused(seg, vp, mask, hc, use_motion=True, what="motion")
    check_fused(seg.float(), vp, mask, hc, what="float32 logits")
    check_fused(seg, vp.float(), mask, hc, sigma=2.0, what="float32 field")
    for need in ((True, False), (False, True)):
        check_fused(seg, vp, mask, hc, ws, need=need, what=f"need={need}")
    seg3, vp3, mask3, hc3 = head_case(2, h, w, 2, d, seed=h + 8, pred_dtype=pred_dtype, C=3)   # labels 0 / 1 / 2: weight 2, no target
    assert (mask3 == 2).any() and (mask3 == 1).any()
    check_fused(seg3, vp3, mask3, hc3, what="three classes")


@pytest.mark.parametrize("h,w", [(48, 64), (37, 53)])
def test_fused_one_half_equals_that_half_of_both(h, w):
    """one body serves both halves: a half asked for alone is bit for bit the same half of the two-half call, fast and general path;
    without the logits' half no label is judged -- status 0 even with a label outside 0..C-1"""
    d = dev()
    seg, vp, mask, hc = head_case(2, h, w, 3, d, seed=h + 21)
    mask[1, h // 2, w // 3] = 2   # outside 0..1
    up = upstream_for(2, d)
    both = V.head_grad_from_keypoints(seg, vp, mask, hc, up)
    only_s = V.head_grad_from_keypoints(seg, vp, mask, hc, up, need=(True, False))
    only_v = V.head_grad_from_keypoints(seg, vp, mask, hc, up, need=(False, True))
    torch.cuda.synchronize()
    assert only_s[1] is None and only_v[0] is None
    assert same(only_s[0], both[0]) and int(torch.isnan(both[0]).sum()) == 2   # the bad pixel's C gradients are NaN in either call
    assert torch.equal(only_v[1], both[1]) and float(both[1].abs().max()) > 0.0
    assert both[2].tolist() == [0, V.HEAD_S_BAD_LABEL] and only_s[2].tolist() == [0, V.HEAD_S_BAD_LABEL]
    assert only_v[2].tolist() == [0, 0]


@pytest.mark.parametrize("h,w", [(1, 1), (3, 1024), (8, 1)])
def test_fused_degenerate_sizes(h, w):
    """one pixel (general path); three rows of one segment each, where a lane's eight pixels never wrap to the next row; a column,
    where they wrap at every pixel (fast path)"""
    d = dev()
    seg, vp, mask, hc = head_case(2, h, w, 3, d, seed=h + w)
    mask[:, 0, 0] = 1   # a target pixel in every image, the 1 x 1 one included
    hc = torch.from_numpy(keypoints_for(mask, 3, seed=h * w)).to(d)
    got, ggot = check_fused(seg, vp, mask, hc, what=f"{h}x{w}")
    assert torch.isfinite(got[0]).all() and float(ggot[1].abs().max()) > 0.0
    check_fused(seg.bfloat16(), vp.bfloat16(), mask, hc, use_motion=True, what=f"{h}x{w} bfloat16, motion")


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.bool, torch.int32])
def test_fused_every_mask_dtype_and_bad_labels(mask_dtype):
    d = dev()
    for h, w in ((48, 64), (37, 53)):
        seg, vp, mask, hc = head_case(2, h, w, 3, d, seed=11, mask_dtype=mask_dtype)
        check_fused(seg, vp, mask, hc, what=f"{mask_dtype} {h}x{w}")
        if mask_dtype != torch.bool:
            mask[1, 2, 3] = 2   # outside 0..1: a bad label for the logits, weight 2 and no target for the field
            got, ggot = check_fused(seg, vp, mask, hc, what=f"{mask_dtype} bad label")
            assert got[2].tolist() == [0, V.HEAD_S_BAD_LABEL] and ggot[2].tolist() == [0, V.HEAD_S_BAD_LABEL]
            assert torch.isnan(got[0][1, 0]) and torch.isfinite(got[0][1, 1])


def test_fused_strided_inputs_outputs_and_packed_slices():
    d = dev()
    seg, vp, mask, hc = head_case(2, 40, 56, 4, d, seed=5)
    base, gbase = check_fused(seg, vp, mask, hc, what="contiguous")
    seg_cl = seg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    vp_cl = vp.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    mask_wide = torch.zeros((2, 40, 112), dtype=torch.int64, device=d)
    mask_wide[:, :, ::2] = mask
    got, ggot = check_fused(seg_cl, vp_cl, mask_wide[:, :, ::2], hc, what="channels-last / strided mask")
    assert torch.equal(got[0], base[0]) and torch.equal(ggot[0], gbase[0]) and torch.equal(ggot[1], gbase[1])
    assert ggot[0].stride() == seg_cl.stride()
    # the two channel slices of one tensor (the network's output), gradients into the slices of one tensor: fast path, plane stride kept
    head_out = torch.cat([seg, vp], 1)
    grad = torch.full_like(head_out, -7.0)
    got, ggot = check_fused(head_out[:, :2], head_out[:, 2:], mask, hc, out=(grad[:, :2], grad[:, 2:]), what="packed slices")
    assert torch.equal(got[0], base[0]) and torch.equal(grad[:, :2], gbase[0]) and torch.equal(grad[:, 2:], gbase[1])
    # misaligned predictions
    flat = torch.zeros(vp.numel() + 1, device=d)
    flat[1:] = vp.reshape(-1)
    got, ggot = check_fused(seg, flat[1:].view(vp.shape), mask, hc, what="misaligned field")
    assert torch.equal(got[0], base[0]) and torch.equal(ggot[1], gbase[1])


def test_benchmark_size_fused():
    d = dev()
    mask_np, planar, kpts = synth.make_batch(2, first_index=11, noise=True)
    mask = torch.from_numpy(np.ascontiguousarray(mask_np)).to(d)
    vp = torch.from_numpy(planar).to(d)
    g = torch.Generator(device="cpu").manual_seed(3)
    seg = (torch.randn((2, 2, 480, 640), generator=g) * 2.0).to(d)
    seg[:, 1] += (mask > 0).float() * 4.0 - 2.0
    hc = torch.from_numpy(keypoints_for(mask, 9, seed=2)).to(d)
    check_fused(seg, vp, mask, hc, what="480x640 vn=9")
    check_fused(seg.bfloat16(), vp.bfloat16(), mask, hc, what="480x640 vn=9 bfloat16")


def test_semantics_of_bad_values():
    d = dev()
    for h, w in ((48, 64), (37, 53)):   # fast and general path
        seg, vp, mask, hc = head_case(3, h, w, 3, d, seed=13)
        bg = (mask[0] == 0).nonzero()[0]
        vp[0, 2, bg[0], bg[1]] = float("nan")   # a NaN prediction at a BACKGROUND pixel: 0 * NaN reaches the loss and the gradient
        got, ggot = check_fused(seg, vp, mask, hc, what=f"NaN at a background pixel {h}x{w}")
        assert torch.isnan(got[0][0, 1]) and torch.isfinite(got[0][1:, 1]).all() and torch.isfinite(got[0][:, 0]).all()
        assert torch.isnan(ggot[1][0, 2, bg[0], bg[1]]) and int(torch.isnan(ggot[1]).sum()) == 1
        # a NaN key-point: NaN targets on that image's mask == 1 pixels of that key-point, nowhere else
        seg, vp, mask, hc = head_case(3, h, w, 3, d, seed=14)
        hc[1, 2, 0] = float("nan")
        vt, _ = V.vertex_targets_device(mask, hc)
        torch.cuda.synchronize()
        nan = torch.isnan(vt)
        want = torch.zeros_like(nan)
        want[1, 4:6] = (mask[1] == 1)[None]
        assert torch.equal(nan, want) and int(nan.sum()) > 0
        check_targets(mask, hc.cpu().numpy(), what="NaN key-point")
        got, _ = check_fused(seg, vp, mask, hc, what="NaN key-point")
        assert torch.isnan(got[0][1, 1]) and torch.isfinite(got[0][0, 1]) and torch.isfinite(got[0][2, 1])


def test_workspace_out_tensors_two_calls_bitwise_and_measurement_flags():
    d = dev()
    seg, vp, mask, hc = head_case(3, 96, 128, 9, d, seed=17)
    up = upstream_for(3, d)
    nm, ng = V.load_targets_library().pvnet_head_metrics_kp_workspace_bytes(3, 96, 128), V.load_targets_library().pvnet_head_grad_kp_workspace_bytes(3, 96, 128)
    res = []
    for fill in (0xFF, 0x7F):   # NaN patterns / set flags if anything of a workspace were read before it is written
        out = (torch.full((3, 4), -1.0, dtype=torch.float64, device=d), torch.full((3, 3), -1, dtype=torch.int64, device=d),
               torch.full((3,), -1, dtype=torch.int32, device=d))
        m = V.head_metrics_from_keypoints(seg, vp, mask, hc, out=out, workspace=torch.full((nm,), fill, dtype=torch.uint8, device=d))
        g = V.head_grad_from_keypoints(seg, vp, mask, hc, up, workspace=torch.full((ng,), fill, dtype=torch.uint8, device=d))
        torch.cuda.synchronize()
        assert m[0] is out[0] and m[1] is out[1] and m[2] is out[2]
        res.append([t.clone() for t in m + g])
    assert all(torch.equal(a, c) for a, c in zip(*res))
    for flags in (V.HEAD_F_NT_NONE, V.HEAD_F_NT_ALL):
        m = V.head_metrics_from_keypoints(seg, vp, mask, hc, flags=flags)
        g = V.head_grad_from_keypoints(seg, vp, mask, hc, up, flags=flags)
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(m + g, res[0]))
    with pytest.raises(RuntimeError, match="PVNET_E_WORKSPACE"):
        V.head_metrics_from_keypoints(seg, vp, mask, hc, workspace=torch.empty(nm - 256, dtype=torch.uint8, device=d))
    with pytest.raises(RuntimeError, match="PVNET_E_WORKSPACE"):
        V.head_grad_from_keypoints(seg, vp, mask, hc, up, workspace=torch.empty(ng - 256, dtype=torch.uint8, device=d))
    with pytest.raises(RuntimeError, match="need"):
        V.head_grad_from_keypoints(seg, vp, mask, hc, up, need=(False, False))
    with pytest.raises(RuntimeError, match="vertex_pred"):
        V.head_metrics_from_keypoints(seg, vp[:, :16], mask, hc)
    empty = V.head_grad_from_keypoints(seg[:0], vp[:0], mask[:0], hc[:0], up[:0])
    assert empty[0].shape == (0, 2, 96, 128) and empty[1].shape == (0, 18, 96, 128) and empty[2].shape == (0,)


def test_modules_from_keypoints():
    d = dev()
    seg0, vp0, mask, hc = head_case(3, 48, 64, 9, d, seed=23)
    ws = torch.tensor([1.0, 0.0, 0.5], device=d)
    for scale in (None, ws):
        vt, vw = V.vertex_targets_device(mask, hc, scale)
        loss = V.HeadLoss(sigma=2.0)
        seg, vp = seg0.clone().requires_grad_(True), vp0.clone().requires_grad_(True)
        hcg = hc.clone().requires_grad_(True)
        got = loss.from_keypoints(seg, vp, mask, hcg, scale)
        (got[0].mean() + 0.5 * got[1].mean()).backward()
        seg2, vp2 = seg0.clone().requires_grad_(True), vp0.clone().requires_grad_(True)
        want = loss(seg2, vp2, mask, vt, vw)
        (want[0].mean() + 0.5 * want[1].mean()).backward()
        torch.cuda.synchronize()
        assert len(got) == 4
        for k, (a, c) in enumerate(zip(got, want)):
            assert a.dtype == torch.float32 and tuple(a.shape) == (3,) and torch.equal(a, c), k
        assert all(torch.equal(a, c) for a, c in zip(V.HeadMetrics(sigma=2.0).from_keypoints(seg0, vp0, mask, hc, scale), want))
        assert got[0].grad_fn is not None and got[1].grad_fn is not None
        assert not got[2].requires_grad and not got[3].requires_grad and got[2].grad_fn is None and got[3].grad_fn is None
        assert torch.equal(seg.grad, seg2.grad) and torch.equal(vp.grad, vp2.grad)
        assert hcg.grad is None   # no gradient for the key-points (nor, an integer tensor, for the mask)
        # needs_input_grad is honoured: one half alone gives the same bits
        seg3 = seg0.clone().requires_grad_(True)
        out = loss.from_keypoints(seg3, vp0, mask, hc, scale)
        (out[0].mean() + 0.5 * out[1].mean()).backward()
        assert torch.equal(seg3.grad, seg2.grad)
        vp3 = vp0.clone().requires_grad_(True)
        out = loss.from_keypoints(seg0, vp3, mask, hc, scale)
        out[1].mean().mul(0.5).backward()
        assert torch.equal(vp3.grad, vp2.grad)
        assert all(not t.requires_grad for t in loss.from_keypoints(seg0, vp0, mask, hc, scale))
        # packed: the network's output before it is sliced
        head_out = torch.cat([seg0, vp0], 1).requires_grad_(True)
        packed = loss.packed_from_keypoints(head_out, 2, mask, hc, scale)
        (packed[0].mean() + 0.5 * packed[1].mean()).backward()
        parent = torch.cat([seg0, vp0], 1).requires_grad_(True)
        pw = loss.packed(parent, 2, mask, vt, vw)
        (pw[0].mean() + 0.5 * pw[1].mean()).backward()
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(packed, pw)) and all(torch.equal(a, c) for a, c in zip(packed, want))
        assert packed[0].grad_fn is not None and not packed[2].requires_grad and not packed[3].requires_grad
        assert torch.equal(head_out.grad, parent.grad) and torch.equal(head_out.grad[:, :2], seg2.grad)
    # the autograd functions save the predictions, the mask and the key-points only: nothing of the size of the target field but them
    seg = seg0.clone().requires_grad_(True)
    out = V.HeadLoss().from_keypoints(seg, vp0, mask, hc)
    saved = out[0].grad_fn.saved_tensors
    assert len(saved) == 4 and sorted(t.numel() for t in saved) == sorted(t.numel() for t in (seg, vp0, mask, hc))
    with pytest.raises(RuntimeError, match="seg_dim"):
        V.HeadLoss().packed_from_keypoints(torch.cat([seg0, vp0], 1), 1, mask, hc)
    motion = V.HeadLoss().from_keypoints(seg0, vp0, mask, hc, use_motion=True)
    vt, vw = V.vertex_targets_device(mask, hc, use_motion=True)
    assert all(torch.equal(a, c) for a, c in zip(motion, V.HeadLoss()(seg0, vp0, mask, vt, vw)))


def test_graph_of_forward_and_backward_replays_on_changed_inputs():
    """a forward + backward through HeadLoss.packed_from_keypoints captured in a torch.cuda.graph with the process's default queue
    count, replayed after the inputs changed in place: the replay equals an eager step on the new inputs bit for bit (PyTorch's
    rules for capturing a backward as in tests/test_head_grad_device.py: a warm-up on a side stream, detached results only)"""
    d = dev()
    b = 4
    seg, vp, mask, hc = head_case(b, 96, 128, 9, d, seed=37)
    seg_b, vp_b, mask_b, hc_b = head_case(b, 96, 128, 9, d, seed=38)
    head_out = torch.cat([seg, vp], 1).requires_grad_(True)
    mask_in, hc_in = mask.clone(), hc.clone()
    loss = V.HeadLoss()

    def step():
        head_out.grad = None
        ls, lv, pr, rc = loss.packed_from_keypoints(head_out, 2, mask_in, hc_in)
        total = ls.mean() + 0.5 * lv.mean()
        total.backward()
        return [t.detach() for t in (total, ls, lv, pr, rc, head_out.grad)]

    def eager():
        out = step()
        torch.cuda.synchronize()
        return [t.clone() for t in out]

    first = eager()
    again = eager()
    assert all(torch.equal(a, c) for a, c in zip(first, again))   # two calls agree bitwise
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    head_out.grad = None
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    names = ("total", "loss_seg", "loss_vertex", "precision", "recall", "gradient")
    for name, a, c in zip(names, captured, first):
        assert torch.equal(a, c), name
    with torch.no_grad():   # new predictions, mask and key-points in the captured tensors
        head_out.copy_(torch.cat([seg_b, vp_b], 1))
        mask_in.copy_(mask_b)
        hc_in.copy_(hc_b)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in captured]
    del captured, graph
    head_out.grad = None
    second = eager()
    for name, a, c in zip(names, replayed, second):
        assert torch.equal(a, c), name
    assert not torch.equal(second[5], first[5]) and torch.isfinite(second[5]).all() and float(second[5].abs().max()) > 0.0


def test_val_step_from_keypoints_equals_the_step_on_materialised_targets():
    d = dev()
    b, h, w = 4, 96, 128
    mask_np, planar, kpts = synth.make_batch(b, first_index=700, h=h, w=w, radius=14, noise=True)
    mask = torch.from_numpy(np.ascontiguousarray(mask_np)).to(d).to(torch.int64)
    vertex_pred = torch.from_numpy(planar).to(d).contiguous()
    vn = vertex_pred.shape[1] // 2
    g = torch.Generator(device="cpu").manual_seed(31)
    seg_pred = (torch.randn((b, 2, h, w), generator=g) * 0.5).to(d)
    seg_pred[:, 1] += (mask > 0).float() * 6.0 - 3.0
    hc = torch.from_numpy(np.concatenate([kpts, np.ones_like(kpts[:, :, :1])], 2)).to(d)
    rng = np.random.default_rng(1)
    ev = E.Evaluator(models={"cat": rng.uniform(-0.1, 0.1, size=(700, 3))}, diameters={"cat": 0.2},
                     points_3d={"cat": rng.uniform(-0.08, 0.08, size=(vn, 3))}, K=P.LINEMOD_K.copy())
    targets = torch.from_numpy(np.stack([np.concatenate([np.eye(3), [[0.0], [0.0], [0.8]]], 1) for _ in range(b)])).to(d)
    step = V.ValStep(ev, "cat", round_hyp_num=64)
    vt, vw = V.vertex_targets_device(mask, hc)
    torch.default_generator.manual_seed(21)   # the vote draws its seed from torch's CPU generator
    want = step.enqueue(seg_pred, vertex_pred, mask, vt, vw, targets)
    torch.default_generator.manual_seed(21)
    got = step.enqueue_from_keypoints(seg_pred, vertex_pred, mask, hc, targets)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 8
    for name, a, c in zip(("losses", "counts", "head status", "poses", "pose status", "errors", "passed", "metric status"), got, want):
        assert torch.equal(a, c), name
    assert torch.isfinite(got[0]).all()
