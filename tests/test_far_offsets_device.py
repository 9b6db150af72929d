"""Every strided entry point with ONE stride of every strided operand beyond 2^31 elements or 2^32 bytes (tests/far_cases.py lays the
operands into one uninitialised arena; tests/test_far_offsets_cpu.py checks the geometry of exactly these calls).

The bar is the same everywhere and involves no tolerance: the call on the far views and the call on their near twins -- the same shapes,
base alignments and strides but for the one far stride -- take the same code path, so every output must be bit-equal (``torch.equal``),
and every sentinel round the far outputs and in the windows a truncated offset would land in must survive.  The inputs' landing windows
hold decoys (different seeded data), so a kernel that truncated an offset would read them and fail the comparison instead of faulting.

The Python front ends hand ``data_ptr()`` and ``stride()`` of these tensors through unchanged (voting._mask_part / _v3_args,
validation's ``_ptr`` / ``_strides`` calls, augment's, the network wrappers' ``triple``, pnp's ``points_2d.stride()``): none copies a
supported dtype, so the tests go through them."""
import numpy as np
import pytest
import torch

from pvnet_amd import synth
from pvnet_amd import validation as V
from pvnet_amd import voting
from tests import far_cases as F
from tests.test_head_metrics_device import random_inputs

pytestmark = pytest.mark.gpu
H, W, VN, HN = F.H, F.W, F.VN, F.HN


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def arena():
    a = F.Arena(dev())   # once per module; a failed allocation raises with the free-memory figure
    yield a
    a.free()


def cases(*calls):
    return pytest.mark.parametrize("case", [(c, *k) for c in calls for k in F.cases(c)], ids=F.case_id)


def session(arena, case):
    call, kind, which, odd = case
    return F.Session(arena, call, kind, which, odd)


def same(far, near, what):
    assert far.dtype == near.dtype and far.shape == near.shape, what
    assert torch.equal(far.contiguous().view(torch.uint8), near.contiguous().view(torch.uint8)), f"{what}: far differs from near"


# ---- voting ------------------------------------------------------------------------------------------------------------------------
MASK_DTYPES = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
FIELD_DTYPES = {4: torch.float32, 2: torch.bfloat16}
_batch = {}


def vote_batch():
    """(mask [2,h,w] int64, planar [2,18,h,w] float32) on the host, made once"""
    if not _batch:
        mask, planar, _ = synth.make_batch(2, first_index=3, h=H, w=W, radius=10, noise=True, background="normal")
        _batch["v"] = (torch.from_numpy(mask).to(torch.int64), torch.from_numpy(planar))
    return _batch["v"]


def lay_field(s, planar):
    """the field of the call's table, far and near, as the [b,h,w,vn,2] the layer takes: the planar storage through the reference's
    permuted view, or the contiguous one"""
    spec = s.expect[0]
    planar = planar.to(FIELD_DTYPES[spec[2]])
    if len(spec[1]) == 4:
        return tuple(synth.planar_to_vertex_view(v) for v in s.input("field", planar))
    return s.input("field", synth.planar_to_vertex_view(planar).contiguous())


def pair_kernel_runs(mask):
    """launch_mask_bits' condition for mask_bits_pair_kernel, restated (pvnet_amd/csrc/k1_mask.hip): an int64 mask with contiguous
    images, a 16-byte aligned base, an even image stride and an even pixel count"""
    return (mask.dtype == torch.int64 and mask.stride(1) == mask.shape[2] and mask.stride(2) == 1 and mask.data_ptr() % 16 == 0 and
            mask.stride(0) % 2 == 0 and (mask.shape[1] * mask.shape[2]) % 2 == 0)


def same_debug(far, near, what):
    (of, df), (on, dn) = far, near
    torch.cuda.synchronize()
    same(of, on, what + " key-points")
    same(df["tn"], dn["tn"], what + " tn")
    same(df["counts"], dn["counts"], what + " counts")
    same(df["status"], dn["status"], what + " status")
    assert int(df["tn"].min()) >= 5, what   # (every image votes)
    for i, tn in enumerate(df["tn"].tolist()):
        same(df["pix"][i, :tn], dn["pix"][i, :tn], what + f" pixel list {i}")


@cases("vote_v3-u8-f32-planar", "vote_v3-i32-bf16-planar", "vote_v3-i64-f32-contiguous", "vote_v3-u8-bf16-contiguous")
def test_ransac_voting_layer_v3(arena, case):
    s = session(arena, case)
    mask, planar = vote_batch()
    mf, mn = s.input("mask", mask.to(MASK_DTYPES[s.expect[0][2]]))
    ff, fn = lay_field(s, planar)
    if mf.dtype == torch.int64:
        # the int64 far-batch placement reaches mask_bits_pair_kernel (ms0 even, base 16-byte aligned); its odd placement and the
        # far-rows one reach mask_bits_kernel<I64>; the twin takes the same kernel
        assert pair_kernel_runs(mf) == pair_kernel_runs(mn) == (case[1] != "far_rows" and not case[3])
    for kw in (dict(), dict(literal=True)):
        far = voting.ransac_voting_layer_v3(mf, ff, HN, inlier_thresh=0.99, seed=3, return_debug=True, **kw)
        near = voting.ransac_voting_layer_v3(mn, fn, HN, inlier_thresh=0.99, seed=3, return_debug=True, **kw)
        same_debug(far, near, F.case_id(case) + str(kw))
    s.check()


def logits_of(mask, nc, seed):
    g = torch.Generator().manual_seed(seed)
    seg = torch.randn((mask.shape[0], nc, H, W), generator=g) * 3.0
    return seg + 6.0 * torch.nn.functional.one_hot(mask, nc).permute(0, 3, 1, 2).float()


@cases("vote_v3_logits-f32", "vote_v3_logits-bf16")
def test_ransac_voting_layer_v3_from_logits(arena, case):
    """the class stride of the logits far (far_planes) as well as the batch and the row stride"""
    s = session(arena, case)
    mask, planar = vote_batch()
    seg = logits_of(mask, 3, 11).to(FIELD_DTYPES[s.expect[0][2]])
    sf, sn = s.input("seg_pred", seg)
    ff, fn = lay_field(s, planar)
    far = voting.ransac_voting_layer_v3_from_logits(sf, ff, HN, inlier_thresh=0.99, seed=3)
    near = voting.ransac_voting_layer_v3_from_logits(sn, fn, HN, inlier_thresh=0.99, seed=3)
    two_step = voting.ransac_voting_layer_v3(torch.argmax(seg.to(dev()), 1), fn, HN, inlier_thresh=0.99, seed=3)
    torch.cuda.synchronize()
    same(far, near, F.case_id(case))
    same(far, two_step, F.case_id(case) + " against arg-max then vote")
    assert bool((far != 0).any())
    s.check()


@cases("motion_voting")
def test_ransac_motion_voting(arena, case):
    s = session(arena, case)
    mask, planar = vote_batch()
    mf, mn = s.input("mask", mask.to(torch.uint8))
    ff, fn = lay_field(s, planar)
    far, near = voting.ransac_motion_voting(mf, ff), voting.ransac_motion_voting(mn, fn)
    torch.cuda.synchronize()
    same(far, near, F.case_id(case))
    assert bool((far != 0).any())
    s.check()


@cases("vote_v2-i64", "vote_v2-u8")
def test_ransac_voting_layer_v2(arena, case):
    """the label source far: the upper half of every disc is class 1, the lower class 2"""
    s = session(arena, case)
    mask, planar = vote_batch()
    labels = mask.clone()
    for i in range(labels.shape[0]):
        rows = torch.nonzero(mask[i].any(1)).flatten()
        labels[i, int(rows.float().mean()):] *= 2
    assert all(int((labels == k).sum(dim=(1, 2)).min()) >= 20 for k in (1, 2))
    lf, ln = s.input("mask", labels.to(MASK_DTYPES[s.expect[0][2]]))
    ff, fn = lay_field(s, planar)
    far = voting.ransac_voting_layer_v2(lf, ff, 3, HN, inlier_thresh=0.99, seed=3, return_debug=True)
    near = voting.ransac_voting_layer_v2(ln, fn, 3, HN, inlier_thresh=0.99, seed=3, return_debug=True)
    same_debug(far, near, F.case_id(case))
    s.check()


# ---- head --------------------------------------------------------------------------------------------------------------------------
PRED_DTYPES = {4: torch.float32, 2: torch.bfloat16}
HEAD_MASKS = {1: torch.uint8, 4: torch.int32, 8: torch.int64}


def head_inputs(s, targets=True):
    """the head's inputs of the call's table laid far and near -> (far tuple, near tuple)"""
    pe, me = s.expect[0][2], s.expect[2][2]
    host = [t.cpu() for t in random_inputs(2, H, W, 4, "cpu", seed=5, C=3, pred_dtype=PRED_DTYPES[pe], mask_dtype=HEAD_MASKS[me])]
    names = ("seg_pred", "vertex_pred", "mask", "vertex", "vertex_weights")[:5 if targets else 3]
    pairs = [s.input(n, t) for n, t in zip(names, host)]
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs), host


def hcoords_of(b, vn, seed):
    g = torch.Generator().manual_seed(seed)
    hz = 0.5 + 1.5 * torch.rand((b, vn, 1), generator=g, dtype=torch.float64)
    xy = torch.rand((b, vn, 2), generator=g, dtype=torch.float64) * torch.tensor([W, H], dtype=torch.float64)
    return torch.cat([xy * hz, hz], 2)


def grad_outputs(s, far_in):
    pairs = [s.output(n, tuple(far_in[k].shape), far_in[k].dtype) for k, n in enumerate(("grad_seg", "grad_vertex"))]
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)


def upstream():
    return torch.tensor([[0.7, 1.3], [1.1, 0.4]], dtype=torch.float64, device=dev())


@cases("head_metrics-f32-i64", "head_metrics-bf16-u8")
def test_head_metrics_device(arena, case):
    s = session(arena, case)
    far_in, near_in, _ = head_inputs(s)
    far, near = V.head_metrics_device(*far_in), V.head_metrics_device(*near_in)
    torch.cuda.synchronize()
    for f, n, what in zip(far, near, ("losses", "counts", "status")):
        same(f, n, f"{F.case_id(case)} {what}")
    assert bool((far[1][:, 0] > 0).all())   # true positives in every image: the mask and the logits were read
    s.check()


@cases("head_grad-f32-i64", "head_grad-bf16-u8")
def test_head_grad_device(arena, case):
    """both gradient outputs far as well"""
    s = session(arena, case)
    far_in, near_in, _ = head_inputs(s)
    far_out, near_out = grad_outputs(s, far_in)
    far = V.head_grad_device(*far_in, upstream(), out=far_out)
    near = V.head_grad_device(*near_in, upstream(), out=near_out)
    torch.cuda.synchronize()
    same(far[2], near[2], F.case_id(case) + " status")
    assert far[0] is far_out[0] and far[1] is far_out[1]
    assert bool((far_out[0] != 0).any()) and bool((far_out[1] != 0).any())
    s.check()   # (the two gradients bit-equal to their twins, the sentinels intact)


@cases("vertex_targets")
def test_vertex_targets_device(arena, case):
    """both outputs far"""
    s = session(arena, case)
    mask = random_inputs(2, H, W, 4, "cpu", seed=5, C=2)[2]
    mf, mn = s.input("mask", mask)
    vf, vn_ = s.output("vertex", (2, 8, H, W), torch.float32)
    wf, wn = s.output("vertex_weights", (2, 1, H, W), torch.float32)
    hc = hcoords_of(2, 4, 7).to(dev())
    V.vertex_targets_device(mf, hc, out=(vf, wf))
    V.vertex_targets_device(mn, hc, out=(vn_, wn))
    torch.cuda.synchronize()
    assert bool((vf != 0).any()) and bool((wf != 0).any())
    s.check()


@cases("head_metrics_kp")
def test_head_metrics_from_keypoints(arena, case):
    s = session(arena, case)
    far_in, near_in, _ = head_inputs(s, targets=False)
    hc = hcoords_of(2, 4, 7).to(dev())
    far, near = V.head_metrics_from_keypoints(*far_in, hc), V.head_metrics_from_keypoints(*near_in, hc)
    torch.cuda.synchronize()
    for f, n, what in zip(far, near, ("losses", "counts", "status")):
        same(f, n, f"{F.case_id(case)} {what}")
    s.check()


@cases("head_grad_kp")
def test_head_grad_from_keypoints(arena, case):
    s = session(arena, case)
    far_in, near_in, _ = head_inputs(s, targets=False)
    far_out, near_out = grad_outputs(s, far_in)
    hc = hcoords_of(2, 4, 7).to(dev())
    far = V.head_grad_from_keypoints(*far_in, hc, upstream(), out=far_out)
    near = V.head_grad_from_keypoints(*near_in, hc, upstream(), out=near_out)
    torch.cuda.synchronize()
    same(far[2], near[2], F.case_id(case) + " status")
    assert bool((far_out[0] != 0).any()) and bool((far_out[1] != 0).any())
    s.check()


# ---- augmentation and colour jitter -----------------------------------------------------------------------------------------------
AUG_MASKS = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
WIDE = dict(brightness=0.6, contrast=0.7, saturation=0.8, hue=0.5)


def aug_inputs(s, with_mask=True):
    """the uint8 picture and the mask of the call's table (tests/augment_cases.py's sweep draws: masks of values 1 .. 3) laid far and
    near, and the host-side arguments: key-points, uniforms"""
    from tests import augment_cases as AC
    rng = np.random.default_rng(20250120)
    h, w = F.AH, F.AW
    rgb = torch.from_numpy(rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8))
    mask = torch.from_numpy(np.stack([AC.sweep_mask(rng, i, h, w) for i in (4, 5)]))
    hc = np.concatenate([rng.uniform(-10.0, w + 10.0, (2, 3, 2)), rng.uniform(0.5, 2.0, (2, 3, 1))], 2)
    U = rng.uniform(0.0, 1.0, (2, 12))
    JU = rng.uniform(0.0, 1.0, (2, 5))
    assert int(mask[0].sum()) > 0 and int(mask[1].sum()) > 0
    rf, rn = s.input("rgb", rgb)
    mf = mn = None
    if with_mask:
        mf, mn = s.input("mask", mask.to(AUG_MASKS[s.expect[0][2]]))
    return (rf, mf), (rn, mn), torch.from_numpy(hc).to(dev()), torch.from_numpy(U), torch.from_numpy(JU)


def same_all(far, near, what):
    torch.cuda.synchronize()
    for k, (f, n) in enumerate(zip(far, near)):
        same(f, n, f"{what} output {k}")


@cases("augment_batch")
def test_augment_batch(arena, case):
    from pvnet_amd import augment as A
    from tests import augment_cases as AC
    s = session(arena, case)
    (rf, mf), (rn, mn), hc, U, _ = aug_inputs(s)
    cfg = A.AugmentConfig(**dict(AC.MIXED, use_mask_out=True))
    far = A.augment_batch(rf, mf, hc, 32, 40, cfg, U, 500, mask_dtype=torch.int64)
    near = A.augment_batch(rn, mn, hc, 32, 40, cfg, U, 500, mask_dtype=torch.int64)
    same_all(far, near, F.case_id(case))
    assert int(far[1].sum()) > 0
    s.check()


@cases("normalize_batch")
def test_normalize_batch(arena, case):
    from pvnet_amd import augment as A
    s = session(arena, case)
    (rf, _), (rn, _), _, _, _ = aug_inputs(s, with_mask=False)
    for dt in (torch.float32, torch.bfloat16):
        same_all([A.normalize_batch(rf, out_dtype=dt)], [A.normalize_batch(rn, out_dtype=dt)], F.case_id(case))
    s.check()


@cases("jitter_batch")
def test_jitter_batch(arena, case):
    from pvnet_amd import color as K
    s = session(arena, case)
    (rf, mf), (rn, mn), _, _, JU = aug_inputs(s)
    cfg = K.ColorJitterConfig(**WIDE)
    far = K.jitter_batch(rf, cfg, JU, mask=mf, maskmul=[1, 1])
    near = K.jitter_batch(rn, cfg, JU, mask=mn, maskmul=[1, 1])
    same_all([far], [near], F.case_id(case))
    assert bool((far != 0).any())
    s.check()


@cases("augment_jitter_batch")
def test_augment_jitter_batch(arena, case):
    from pvnet_amd import augment as A
    from pvnet_amd import color as K
    from tests import augment_cases as AC
    s = session(arena, case)
    (rf, mf), (rn, mn), hc, U, JU = aug_inputs(s)
    cfg, jcfg = A.AugmentConfig(**dict(AC.MIXED, use_mask_out=True)), K.ColorJitterConfig(**WIDE)
    far = K.augment_jitter_batch(rf, mf, hc, 32, 40, cfg, jcfg, U, JU, 500)
    near = K.augment_jitter_batch(rn, mn, hc, 32, 40, cfg, jcfg, U, JU, 500)
    same_all(far, near, F.case_id(case))
    s.check()


# ---- the network launches --------------------------------------------------------------------------------------------------------
NET_DTYPES = {4: torch.float32, 2: torch.bfloat16}


def near_loader_runs(t):
    """trunk.hip's near_ok, restated: the 32-bit loader serves a source whose strides inside an image are non-negative and whose image
    spans less than 2^31 bytes; every other source takes the loader with a 64-bit address per load"""
    c, h, w = t.shape[1:]
    st = t.stride()
    return min(st[1:]) >= 0 and ((c - 1) * st[1] + (h - 1) * st[2] + (w - 1) * st[3] + 1) * t.element_size() < 2 ** 31


def lay(s, named, dtypes=None):
    """the named host tensors of the call's table, laid far and near in order (each in the type its table entry has)"""
    far, near = [], []
    for name, t in named:
        dt = (dtypes or NET_DTYPES)[s.expect[0][2]]
        f, n = s.input(name, t.to(dt))
        far.append(f), near.append(n)
    return far, near


@cases("conv3x3-32-0-32-bf16", "conv3x3-64-32-96-f32", "conv3x3-stride2-f16")
def test_fused_conv3x3(arena, case):
    """src1, src2 and the residual far.  far_batch keeps the 32-bit loader; far_planes and far_rows make near_ok false and so reach the
    loader with 64-bit addresses, while their near twins stay on the 32-bit one: the two loaders must give the same bits."""
    from pvnet_amd import trunk as T
    from tests import trunk_cases as TC
    s = session(arena, case)
    call = case[0]
    triple = tuple(int(x) for x in call.split("-")[1:4]) if "stride2" not in call else (32, 0, 32)
    stride = 2 if "stride2" in call else 1
    src1, src2, res, (wt, bias) = TC.seeded(2, 19, 27, triple, stride, 31)
    named = [("src1", src1)] + ([("src2", src2)] if src2 is not None else []) + [("residual", res)]
    far, near = lay(s, named, {4: torch.float32, 2: torch.float16 if "f16" in call else torch.bfloat16})
    params = T.ConvParams(wt, bias, stride=stride, dilation=1, act="relu")
    for t in far[:-1]:
        assert near_loader_runs(t) == (case[1] == "far_batch"), "the far source takes the loader the placement is meant for"
    assert all(near_loader_runs(t) for t in near[:-1])
    kw = lambda v: dict(src2=v[1] if src2 is not None else None, residual=v[-1])   # noqa: E731
    got_far, got_near = T.fused_conv3x3(far[0], params, **kw(far)), T.fused_conv3x3(near[0], params, **kw(near))
    same_all([got_far], [got_near], F.case_id(case))
    assert bool((got_far != 0).any())
    s.check()


@cases("fused_stage")
def test_fused_stage(arena, case):
    from pvnet_amd import decoder as D
    from tests import decoder_cases as DC
    s = session(arena, case)
    lo, skip, (wt, bias) = DC.seeded(2, 20, 36, (64, 64, 32), 41)
    far, near = lay(s, [("lo", lo), ("skip", skip)])
    params = D.StageParams(wt, bias)
    same_all([D.fused_stage(far[0], far[1], params)], [D.fused_stage(near[0], near[1], params)], F.case_id(case))
    s.check()


@cases("fused_stem", "fused_stem-bf16")
def test_fused_stem(arena, case):
    from pvnet_amd import stem as S
    from tests import stem_cases as SC
    s = session(arena, case)
    image, (wt, bias) = SC.seeded(2, 37, 53, 51)
    far, near = lay(s, [("image", image)])
    params = S.StemParams(wt, bias)
    same_all(S.fused_stem(far[0], params), S.fused_stem(near[0], params), F.case_id(case))
    s.check()


@cases("fused_tail")
def test_fused_tail(arena, case):
    from pvnet_amd import tail as TL
    from tests import tail_cases as TLC
    s = session(arena, case)
    fm, image, weights = TLC.seeded(2, 40, 56, 20, 61)
    far, near = lay(s, [("fm", fm), ("image", image)])
    params = TL.TailParams(*weights)
    for precision in ("bf16", "f32"):
        same_all([TL.fused_tail(far[0], far[1], params, precision=precision, out_dtype=torch.float32)],
                 [TL.fused_tail(near[0], near[1], params, precision=precision, out_dtype=torch.float32)], F.case_id(case) + precision)
    s.check()


# ---- the pose solves ---------------------------------------------------------------------------------------------------------------
POSE_DTYPES = {4: torch.float32, 8: torch.float64}


@cases("pnp_batch-f32", "pnp_batch-f64")
def test_pnp_batch_device(arena, case):
    from pvnet_amd import pnp as P
    from tests import pose_cases as PC
    s = session(arena, case)
    X, x2, _ = PC.problems(2, 11, 9)
    far, near = lay(s, [("points_2d", torch.from_numpy(np.ascontiguousarray(x2)))], POSE_DTYPES)
    got_far, got_near = P.pnp_batch_device(X, far[0], P.LINEMOD_K), P.pnp_batch_device(X, near[0], P.LINEMOD_K)
    same_all(got_far, got_near, F.case_id(case))
    assert bool((got_far[1] >= 0).all())   # both images solved
    s.check()


@cases("pnp_classes-f32", "pnp_classes-f64")
def test_pnp_classes_device(arena, case):
    from pvnet_amd import pnp as P
    from tests import pose_classes_cases as PCC
    s = session(arena, case)
    X, x2, _ = PCC.case(2, 3, 9, noise=PCC.NOISE)
    far, near = lay(s, [("points_2d", torch.from_numpy(np.ascontiguousarray(x2)))], POSE_DTYPES)
    got_far, got_near = P.pnp_classes_device(X, far[0], P.LINEMOD_K), P.pnp_classes_device(X, near[0], P.LINEMOD_K)
    same_all(got_far, got_near, F.case_id(case))
    assert bool((got_far[1] >= 0).all())
    s.check()


# ---- contiguous outputs beyond 2^31 elements --------------------------------------------------------------------------------------
# The network launches write a dense [b,co,ho,wo] with no strides to pass, so the placements above cannot reach their store index.
# Here ONE image has a plane of more than 2^26 pixels, so a 32-channel output has more than 2^31 elements (more than 2^32 bytes in
# bfloat16).  Inputs and output are slices of the arena, the output from its middle.  Only two bands of input rows -- the first and the
# last -- hold seeded data; the kernel runs over everything between them, whatever the memory holds.
BIG_W, BIG_H, BAND_IN, BAND_OUT = 8192, 8192 + 13, 24, 16   # (BIG_H is no multiple of the tiles' 8 rows: the last tile is cut)


def arena_tensor(arena, byte0, shape, dtype):
    es = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape))
    assert byte0 % 256 == 0 and 0 <= byte0 and byte0 + n * es <= F.ARENA_BYTES
    return arena.bytes[byte0:byte0 + n * es].view(dtype).view(shape), byte0 + n * es


def decoys_differ(arena, base, rows, what):
    """``rows``: [(element offset of a row in the bfloat16 output at arena byte ``base``, the expected row)].  Wherever a modelled
    mistake moves the row's address, the truncated address lies inside the arena and must not hold the row's values.  Which mistakes
    move a row follows from its offset alone: the signed byte truncation from byte 2^31, the signed element truncation and the
    unsigned byte truncation from element 2^31 = byte 2^32 (no offset here reaches element 2^32).  Returns the rows beyond element
    2^31."""
    beyond = 0
    for at, row in rows:
        moved = {m for m in F.MISTAKES if F.mistaken_bytes(m, at, 2) != 2 * at}
        assert moved == ({"i32_byte"} if 2 * at >= 2 ** 31 else set()) | ({"i32_elem", "u32_byte"} if at >= 2 ** 31 else set()), (what, at)
        beyond += at >= 2 ** 31
        for m in moved:
            s = base + F.mistaken_bytes(m, at, 2)
            assert 0 <= s and s + 2 * row.numel() <= F.ARENA_BYTES, "a truncated store stays inside the arena"
            there = arena.bytes[s:s + 2 * row.numel()].view(torch.int16)
            assert not torch.equal(there, row.contiguous().view(torch.int16)), (what, at, m)
    return beyond


def bf16_sentinel():
    return torch.tensor([F.SENTINEL * 257], dtype=torch.int32).to(torch.int16).view(torch.bfloat16).item()


def test_conv3x3_output_beyond_2_31_elements(arena):
    """The trunk convolution, 32 -> 32 channels, bfloat16 in and out, stride 1, on one image of 8205 x 8192 pixels: the output has
    2^31 + 3 407 872 elements, so the last 416 rows of channel 31 lie beyond element 2^31 and byte 2^32, channels 16 .. 31 beyond byte 2^31.

    The output rows of the two bands must be bit-equal to the same launch on the cropped bands.  That is exact because an output
    pixel's summation order does not depend on where its tile lies (pvnet_amd/csrc/trunk.hip, conv3x3_kernel): its accumulator starts
    from the bias and takes the same sequence of MFMAs (chunk, tap row, k-step) whatever the tile, the row y of the tile (an
    accumulator block of its own per row) and the lane; the source takes the 64-bit loader here (its image spans more than 2^31
    bytes) and the 32-bit one in the cropped launch, which load the same values.  The output's true band is filled with a sentinel
    before the launch, and the addresses where an offset truncated to 32 bits (elements or bytes, sign- or zero-extended) would put
    the last band must not hold its values afterwards."""
    from pvnet_amd import trunk as T
    from tests import trunk_cases as TC
    H, W = BIG_H, BIG_W
    plane = H * W
    assert plane >= 2 ** 26 and 32 * plane > 2 ** 31 and 31 * plane + (H - BAND_OUT) * W >= 2 ** 31
    src, end = arena_tensor(arena, 0, (1, 32, H, W), torch.bfloat16)
    assert end + F.GUARD <= F.MID
    out, out_end = arena_tensor(arena, F.MID, (1, 32, H, W), torch.bfloat16)
    assert out.data_ptr() - arena.bytes.data_ptr() >= 2 ** 33 and out_end + F.GUARD <= F.ARENA_BYTES
    assert not near_loader_runs(src)
    g = torch.Generator().manual_seed(71)
    bands = [torch.relu(torch.randn(1, 32, BAND_IN, W, generator=g)).to(torch.bfloat16).to(dev()) for _ in range(2)]
    src[:, :, :BAND_IN] = bands[0]
    src[:, :, H - BAND_IN:] = bands[1]
    assert torch.equal(src[:, :, :BAND_IN], bands[0]) and torch.equal(src[:, :, H - BAND_IN:], bands[1])
    _, _, _, (wt, bias) = TC.seeded(1, 1, 1, (32, 0, 32), 1, 72)
    params = T.ConvParams(wt, bias, stride=1, dilation=1, act="relu")
    # sentinels: the true bands of the output, and a guard on both sides of it
    sent = bf16_sentinel()
    out[:, :, :BAND_OUT] = sent
    out[:, :, H - BAND_OUT:] = sent
    arena.bytes[F.MID - F.GUARD:F.MID] = F.SENTINEL
    arena.bytes[out_end:out_end + F.GUARD] = F.SENTINEL
    got = T.fused_conv3x3(src, params, out=out)
    want = [T.fused_conv3x3(band, params) for band in bands]
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    same(out[:, :, :BAND_OUT], want[0][:, :, :BAND_OUT], "the first band")
    same(out[:, :, H - BAND_OUT:], want[1][:, :, BAND_IN - BAND_OUT:], "the last band")
    last = want[1][0, :, BAND_IN - BAND_OUT:]   # [32, BAND_OUT, W]
    assert bool((last != 0).any()) and bool((want[0] != 0).any())
    assert bool((arena.bytes[F.MID - F.GUARD:F.MID] == F.SENTINEL).all()) and bool((arena.bytes[out_end:out_end + F.GUARD] == F.SENTINEL).all())
    rows = [(c * plane + (H - BAND_OUT + y) * W, last[c, y]) for c in range(32) for y in range(BAND_OUT)]
    # (channels 16 .. 31 lie beyond byte 2^31, the band of channel 31 beyond element 2^31 and byte 2^32)
    assert decoys_differ(arena, F.MID, rows, "the convolution's output") == BAND_OUT

def test_stem_output_beyond_2_31_elements(arena):
    """The stem on one float32 image of 8202 x 16384 pixels, bfloat16 out: x2s [1,64,4101,8192] has 2^31 + 2 621 440 elements; the
    pooled tensor (2^29 elements) rides along.  The bands' x2s and pooled rows must be bit-equal to the launch on the cropped bands:
    a pixel is one column of the matrix product whatever lane and tile it is on (pvnet_amd/csrc/stem.hip says so of the halo pixels
    it recomputes), and the bands start at image rows that are multiples of 4, so the stride-2 windows of the convolution and of the
    pool fall on the same rows in both launches."""
    from pvnet_amd import stem as S
    from tests import stem_cases as SC
    H, W, BAND = 8202, 16384, 26
    ho, wo, hp, wp = S.out_sizes(H, W)
    plane = ho * wo
    assert 64 * plane > 2 ** 31 and 63 * plane + (ho - 8) * wo >= 2 ** 31 and (H - BAND) % 4 == 0
    image, end = arena_tensor(arena, 0, (1, 3, H, W), torch.float32)
    assert end <= F.MID - F.GUARD
    x2s, x_end = arena_tensor(arena, F.MID, (1, 64, ho, wo), torch.bfloat16)
    pooled, p_end = arena_tensor(arena, F.round_up(x_end + F.GUARD, 4096), (1, 64, hp, wp), torch.bfloat16)
    assert p_end + F.GUARD <= F.ARENA_BYTES
    g = torch.Generator().manual_seed(81)
    bands = [torch.randn(1, 3, BAND, W, generator=g).to(dev()) for _ in range(2)]
    image[:, :, :BAND] = bands[0]
    image[:, :, H - BAND:] = bands[1]
    assert torch.equal(image[:, :, H - BAND:], bands[1])
    _, (wt, bias) = SC.seeded(1, 1, 1, 82)
    params = S.StemParams(wt, bias)
    sent = bf16_sentinel()
    x2s[:, :, :8] = sent
    x2s[:, :, ho - 8:] = sent
    pooled[:, :, :3] = sent
    pooled[:, :, hp - 4:] = sent
    for s in (F.MID - F.GUARD, x_end, p_end):
        arena.bytes[s:s + F.GUARD] = F.SENTINEL
    S.fused_stem(image, params, out=(x2s, pooled))
    want = [S.fused_stem(band, params, out_dtype=torch.bfloat16) for band in bands]
    torch.cuda.synchronize()
    ch, cp = want[1][0].shape[2], want[1][1].shape[2]
    assert (ch, cp) == (13, 7) and ho - ch == (H - BAND) // 2 and hp - cp == (H - BAND) // 4
    same(x2s[:, :, :8], want[0][0][:, :, :8], "x2s, the first band")
    same(pooled[:, :, :3], want[0][1][:, :, :3], "pooled, the first band")
    same(x2s[:, :, ho - 8:], want[1][0][:, :, ch - 8:], "x2s, the last band")
    same(pooled[:, :, hp - 4:], want[1][1][:, :, cp - 4:], "pooled, the last band")
    assert bool((want[1][0][:, :, ch - 8:] != 0).any())
    for s in (F.MID - F.GUARD, x_end, p_end):
        assert bool((arena.bytes[s:s + F.GUARD] == F.SENTINEL).all())
    rows = [(c * plane + (ho - 8 + y) * wo, want[1][0][0, c, ch - 8 + y]) for c in range(64) for y in range(8)]
    assert decoys_differ(arena, F.MID, rows, "x2s") == 8   # the band of channel 63 lies beyond element 2^31


def test_tail_output_beyond_2_31_elements(arena):
    """The tail (bfloat16 tier, cout = 32, bfloat16 out) on one image of 8206 x 8192 pixels: the output has 2^31 + 3 670 016
    elements.  The upsample's coordinates depend on the whole image's height, so a cropped launch sees other interpolation weights;
    the features are therefore constant planes of powers of two over the bands (tests/tail_cases.py: those the float32 upsample
    reproduces exactly whatever the weights), and the seeded per-pixel data is the image's, which is not upsampled.  With that, an
    output pixel's value depends on its neighbourhood alone and its summation order on nothing else (pvnet_amd/csrc/tail.hip: the
    same 18 + 2 MFMAs for every pixel, pixels on the lanes), so the bands must be bit-equal to the launch on the cropped bands."""
    from pvnet_amd import tail as TL
    from tests import tail_cases as TLC
    hin, win, BAND = 4103, 4096, 16
    h, w = 2 * hin, 2 * win
    plane = h * w
    assert 32 * plane > 2 ** 31 and 31 * plane + (h - BAND) * w >= 2 ** 31
    fm, end = arena_tensor(arena, 0, (1, 32, hin, win), torch.bfloat16)
    image, end = arena_tensor(arena, F.round_up(end, 4096), (1, 3, h, w), torch.float32)
    assert end <= F.MID - F.GUARD
    out, out_end = arena_tensor(arena, F.MID, (1, 32, h, w), torch.bfloat16)
    assert out_end + F.GUARD <= F.ARENA_BYTES
    g = torch.Generator().manual_seed(91)
    values = torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0])[torch.randint(0, 7, (32,), generator=g)]
    fm_band = values.view(1, 32, 1, 1).expand(1, 32, BAND, win).to(torch.bfloat16).contiguous().to(dev())
    bands = [torch.randn(1, 3, 2 * BAND, w, generator=g).to(dev()) for _ in range(2)]
    fm[:, :, :BAND] = fm_band
    fm[:, :, hin - BAND:] = fm_band
    image[:, :, :2 * BAND] = bands[0]
    image[:, :, h - 2 * BAND:] = bands[1]
    assert torch.equal(image[:, :, h - 2 * BAND:], bands[1]) and torch.equal(fm[:, :, hin - BAND:], fm_band)
    params = TL.TailParams(*TLC.seeded(1, 2, 2, 32, 92)[2])
    sent = bf16_sentinel()
    out[:, :, :BAND] = sent
    out[:, :, h - BAND:] = sent
    for s in (F.MID - F.GUARD, out_end):
        arena.bytes[s:s + F.GUARD] = F.SENTINEL
    TL.fused_tail(fm, image, params, out=out)
    want = [TL.fused_tail(fm_band, band, params, out_dtype=torch.bfloat16) for band in bands]
    torch.cuda.synchronize()
    same(out[:, :, :BAND], want[0][:, :, :BAND], "the first band")
    same(out[:, :, h - BAND:], want[1][:, :, BAND:], "the last band")
    assert bool((want[1] != 0).any())
    for s in (F.MID - F.GUARD, out_end):
        assert bool((arena.bytes[s:s + F.GUARD] == F.SENTINEL).all())
    rows = [(c * plane + (h - BAND + y) * w, want[1][0, c, BAND + y]) for c in range(32) for y in range(BAND)]
    assert decoys_differ(arena, F.MID, rows, "the tail's output") == BAND   # the band of channel 31 lies beyond element 2^31


def test_decoder_stage_output_beyond_2_31_elements(arena):
    """conv2s' stage (64 + 64 -> 32 channels, bfloat16 everywhere) on one image of 8206 x 8192 pixels.  Its three tensors -- the skip
    features of 8 GiB, the output of 4 GiB and the low-resolution input of 2 GiB -- fit in the arena with the output behind the skip
    features, so its base still lies beyond byte 2^33.  As for the tail, the upsampled input is constant planes of powers of two over
    the bands and the seeded data is the skip features'; the kernel (pvnet_amd/csrc/decoder.hip) accumulates a pixel over the chunks
    of 32 channels and their 18 k-steps in one order whatever its tile."""
    from pvnet_amd import decoder as D
    from tests import decoder_cases as DC
    hin, win, BAND = 4103, 4096, 16
    h, w = 2 * hin, 2 * win
    plane = h * w
    assert 32 * plane > 2 ** 31 and 31 * plane + (h - BAND) * w >= 2 ** 31
    skip, end = arena_tensor(arena, 0, (1, 64, h, w), torch.bfloat16)
    base = F.round_up(end + F.GUARD, 4096)
    out, out_end = arena_tensor(arena, base, (1, 32, h, w), torch.bfloat16)
    lo, end = arena_tensor(arena, F.round_up(out_end + F.GUARD, 4096), (1, 64, hin, win), torch.bfloat16)
    assert base >= F.MID and end <= F.ARENA_BYTES
    g = torch.Generator().manual_seed(95)
    values = torch.tensor([0.0, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0])[torch.randint(0, 7, (64,), generator=g)]
    lo_band = values.view(1, 64, 1, 1).expand(1, 64, BAND, win).to(torch.bfloat16).contiguous().to(dev())
    bands = [torch.relu(torch.randn(1, 64, 2 * BAND, w, generator=g)).to(torch.bfloat16).to(dev()) for _ in range(2)]
    lo[:, :, :BAND] = lo_band
    lo[:, :, hin - BAND:] = lo_band
    skip[:, :, :2 * BAND] = bands[0]
    skip[:, :, h - 2 * BAND:] = bands[1]
    assert torch.equal(skip[:, :, h - 2 * BAND:], bands[1]) and torch.equal(lo[:, :, hin - BAND:], lo_band)
    params = D.StageParams(*DC.seeded(1, 2, 2, (64, 64, 32), 96)[2])
    sent = bf16_sentinel()
    out[:, :, :BAND] = sent
    out[:, :, h - BAND:] = sent
    for s in (base - F.GUARD, out_end):
        arena.bytes[s:s + F.GUARD] = F.SENTINEL
    D.fused_stage(lo, skip, params, out=out)
    want = [D.fused_stage(lo_band, band, params) for band in bands]
    torch.cuda.synchronize()
    same(out[:, :, :BAND], want[0][:, :, :BAND], "the first band")
    same(out[:, :, h - BAND:], want[1][:, :, BAND:], "the last band")
    assert bool((want[1] != 0).any())
    for s in (base - F.GUARD, out_end):
        assert bool((arena.bytes[s:s + F.GUARD] == F.SENTINEL).all())
    rows = [(c * plane + (h - BAND + y) * w, want[1][0, c, BAND + y]) for c in range(32) for y in range(BAND)]
    assert decoys_differ(arena, base, rows, "the stage's output") == BAND
