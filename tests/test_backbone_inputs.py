"""GPU tests of the input contract of the fused arg-max entry (``ransac_voting_layer_v3_from_logits``, what ``EvalWrapper`` and
tools/e2e_amd.py run) and of half-precision fields at a culling layout.

The spec is the reference's own two-step operation (tools/demo.py:47-55): ``torch.argmax(seg_pred, 1)``, then ``.byte() != 0``, then
the voting layer on the field widened to float32.  So:

* A -- K1's mask stage, bit for bit against the device's ``torch.argmax``: every logits dtype, the layouts a backbone hands over (the
  ``y[:, :C]`` slice of one output tensor, channels-last, a batch-strided view), 1 .. 300 classes, ties, signed zeros, infinities and
  NaNs (torch counts a NaN as the maximum; the first one wins);
* B -- key-points, counts, winners and compacted pixel lists of the fused entry ``torch.equal`` to the two-step call;
* C -- bf16 / f16 fields at a culling layout: exact-mode counts equal to literal mode, to the float32 call on ``.float()`` of the
  field and to the reference's own kernel, under both culling selections; v5's confidence and the voting distribution as well.

Like tests/test_release_scoring.py: knob-free on the release library, explicitly zeroed workspaces, and the layout / culling marks
each test relies on are asserted."""
import math
import os

import pytest
import torch

from pvnet_amd import synth, voting
from tests.test_release_scoring import HEAVY_SHAPE, assert_counts_equal_the_references_kernel, assert_equal_to_literal

pytestmark = pytest.mark.gpu

NAN, INF = math.nan, math.inf
LOW = -1000.0        # every class a pattern below does not name
HN, THRESH, SEED = 32, 0.99, 21

# (leading class values, {class: value}, the arg-max torch returns, value of every other class): planted pixels of the A tests.
# The smallest class count a pattern applies to follows from the classes it names and its answer.
FLOAT_PATTERNS = [
    ((0.0, 0.0), {}, 0, LOW),                 # exact tie: the first maximum
    ((-0.0, 0.0), {}, 0, LOW),                # -0.0 == +0.0: a tie, not an order
    ((0.0, -0.0), {}, 0, LOW),
    ((-1.0, -0.0, 0.0), {}, 1, LOW),
    ((), {}, 0, -INF),                        # every class -inf
    ((INF, 1.0), {}, 0, LOW),
    ((1.0, INF), {}, 1, LOW),
    ((INF, INF), {}, 0, LOW),
    ((-INF, 5.0), {}, 1, LOW),
    ((NAN,), {}, 0, LOW),                     # NaN in class 0
    ((1.0, NAN), {}, 1, LOW),                 # NaN in class 1
    ((NAN, NAN), {}, 0, LOW),                 # NaN in both: the first
    ((5.0, NAN), {}, 1, LOW),                 # NaN after a larger finite value
    ((5.0, 1.0, NAN), {}, 2, LOW),
    ((0.0, NAN, 1.0), {}, 1, LOW),
    ((NAN, 2.0, NAN), {}, 0, LOW),
    ((1.0, INF, NAN), {}, 2, LOW),
    ((INF, NAN), {}, 1, LOW),
    ((-INF, NAN, INF), {}, 1, LOW),
    ((NAN, -INF), {}, 0, LOW),
    ((), {20: 100.0}, 20, LOW),               # the last of 21 classes
    ((), {255: 100.0}, 255, LOW),
    ((), {256: 100.0}, 256, LOW),             # .byte() wraps 256 to background
    ((), {257: 100.0}, 257, LOW),
    ((), {256: 100.0, 257: 100.0}, 256, LOW),
    ((), {256: NAN, 257: 100.0}, 256, LOW),
    ((), {257: NAN, 256: 100.0}, 257, LOW),
    ((), {299: INF}, 299, LOW),
]
# logits that float32 cannot tell apart: narrowing them first would make ties where torch.argmax sees an order
WIDE_FLOAT_PATTERNS = [
    ((1.0, 1.0 + 1e-12), {}, 1, LOW),
    ((1.0 + 2e-12, 1.0, 1.0 + 3e-12), {}, 2, LOW),
    ((1.0 + 1e-12, 1.0), {}, 0, LOW),
]
INT_PATTERNS = [
    ((7, 7), {}, 0, LOW),
    ((2 ** 30, 2 ** 30 + 1), {}, 1, LOW),
    ((2 ** 30 + 1, 2 ** 30, 2 ** 30 + 2), {}, 2, LOW),
    ((2 ** 31 - 2, 2 ** 31 - 1), {}, 1, LOW),
    ((), {}, 0, -2 ** 31),
    ((), {256: 2 ** 31 - 1}, 256, LOW),
    ((), {257: 2 ** 30 + 1, 258: 2 ** 30}, 257, LOW),
]
PATTERNS = {torch.float32: FLOAT_PATTERNS, torch.float16: FLOAT_PATTERNS, torch.bfloat16: FLOAT_PATTERNS,
            torch.float64: FLOAT_PATTERNS + WIDE_FLOAT_PATTERNS, torch.int32: INT_PATTERNS}
DTYPES = list(PATTERNS)
LAYOUTS = ("contiguous", "backbone_slice", "channels_last", "batch_strided")
CLASSES = (1, 2, 3, 21, 300)
SHAPES = ((1, 64), (37, 53), (480, 640))     # 37 x 53: odd width, odd pixel count
BACKBONE_VN = 9                              # tools/e2e_amd.py: [b, 2 + 2 * 9, h, w] for two classes


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


def zeroed(b, h, w, vn, hn, max_num=30000):
    L = voting.vote_layout(b, h, w, vn, hn, max_num)
    return torch.zeros(L.total_bytes, dtype=torch.uint8, device=dev()), L


def patterns_for(dt, nc):
    return [p for p in PATTERNS[dt] if max([len(p[0]) - 1, p[2], *p[1]]) < nc]


def planted(dt, nc):
    """[K, nc] float64 (int64 for integer dtypes): one row per pattern that fits nc classes, and its expected arg-max [K]"""
    pats = patterns_for(dt, nc)
    wide = torch.int64 if not dt.is_floating_point else torch.float64
    rows = torch.empty((len(pats), nc), dtype=wide)
    for i, (lead, extra, _, fill) in enumerate(pats):
        rows[i] = fill
        if lead:
            rows[i, :len(lead)] = torch.tensor(lead, dtype=wide)
        for c, x in extra.items():
            rows[i, c] = x
    return rows, torch.tensor([p[2] for p in pats], dtype=torch.int64)


def logits(dt, b, nc, h, w, seed):
    """[b, nc, h, w] of dtype dt on the GPU, logically contiguous: half the pixels from a coarse grid (ties are common at every
    precision, half precision included), half continuous (large integers for int32); the patterns planted at the first pixels of
    image 0 and the last pixels of image b - 1"""
    g = torch.Generator(device=dev()).manual_seed(seed)
    npix = h * w
    if dt.is_floating_point:
        grid = torch.randint(-4, 5, (b, nc, npix), generator=g, device=dev()).double() * 0.5
        cont = torch.randn((b, nc, npix), generator=g, device=dev(), dtype=torch.float64)
    else:
        grid = torch.randint(-8, 9, (b, nc, npix), generator=g, device=dev())
        cont = torch.randint(-2 ** 31, 2 ** 31, (b, nc, npix), generator=g, device=dev())
    x = torch.where(torch.rand((b, 1, npix), generator=g, device=dev()) < 0.5, grid, cont)
    rows, _ = planted(dt, nc)
    k = rows.shape[0]
    assert k <= npix
    x[0, :, :k] = rows.T.to(dev())
    x[b - 1, :, npix - k:] = rows.T.to(dev())
    return x.view(b, nc, h, w).to(dt)


def lay_out(x, layout, seed):
    """(seg_pred, vertex view) with seg_pred holding x's values in the given memory layout"""
    b, nc, h, w = x.shape
    g = torch.Generator(device=dev()).manual_seed(seed + 1)
    if layout == "backbone_slice":   # model_repository.py:77: seg_pred = y[:, :seg_dim] of one [b, seg_dim + 2 vn, h, w] output
        y = torch.empty((b, nc + 2 * BACKBONE_VN, h, w), dtype=x.dtype, device=dev())
        y[:, :nc] = x
        y[:, nc:] = torch.randn((b, 2 * BACKBONE_VN, h, w), generator=g, device=dev()).to(x.dtype)
        return y[:, :nc], synth.planar_to_vertex_view(y[:, nc:])
    planar = torch.randn((b, 2, h, w), generator=g, device=dev())
    if layout == "contiguous":
        seg = x.contiguous()
    elif layout == "channels_last":
        seg = x.contiguous(memory_format=torch.channels_last)
        assert nc == 1 or (seg.stride(1) == 1 and seg.stride(3) == nc)   # (torch keeps one class planar)
    else:   # every other image of a batch twice the size; the skipped images hold values that would change the answer
        z = torch.full((2 * b, nc, h, w), NAN if x.dtype.is_floating_point else 2 ** 31 - 1, dtype=x.dtype, device=dev())
        z[::2] = x
        seg = z[::2]
        assert seg.stride(0) == 2 * nc * h * w
    return seg, synth.planar_to_vertex_view(planar)


def unpack(bits, npix):
    """[b, words] int64 bit words -> [b, npix] bool (pixel p at bit p % 64 of word p // 64); asserts the tail bits are clear"""
    b, words = bits.shape
    shifts = torch.arange(64, device=bits.device)
    u = ((bits.unsqueeze(-1) >> shifts) & 1).bool().view(b, words * 64)
    assert not bool(u[:, npix:].any()), "bits set past the last pixel"
    return u[:, :npix]


def reference_mask(seg):
    """the reference's mask (tools/demo.py:52, ransac_voting_gpu.py:527): torch.argmax(seg_pred, 1), .byte() != 0"""
    return torch.argmax(seg, 1).to(torch.uint8) != 0


def test_special_value_fixture_is_the_same_spec_on_cpu_and_gpu():
    """the planted patterns' arg-max as written in this module -- torch on the CPU and on the GPU agree with it, so the spec the A
    tests compare against is not a property of one device"""
    for dt in DTYPES:
        for nc in (3, 21, 300):
            rows, want = planted(dt, nc)
            x = rows.to(dt).T.reshape(1, nc, -1, 1)
            cpu = torch.argmax(x, 1).flatten()
            gpu = torch.argmax(x.to(dev()), 1).flatten().cpu()
            assert torch.equal(cpu, want), (dt, nc, (cpu != want).nonzero().flatten().tolist())
            assert torch.equal(gpu, want), (dt, nc, (gpu != want).nonzero().flatten().tolist())


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("nc", CLASSES, ids=lambda c: f"{c}cls")
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTYPES, ids=str)
def test_mask_stage_equals_torch_argmax(dt, layout, nc, hw):
    """K1's fused arg-max (or, for float64 / int32, the two-step call the entry falls back to): the bit mask and the foreground
    count of every image equal torch.argmax(seg_pred, 1).byte() != 0 on the same device"""
    h, w = hw
    b = 2
    seed = 1000 * DTYPES.index(dt) + 100 * LAYOUTS.index(layout) + 10 * CLASSES.index(nc) + SHAPES.index(hw)
    seg, v = lay_out(logits(dt, b, nc, h, w, seed), layout, seed)
    assert seg.dtype == dt and tuple(seg.shape) == (b, nc, h, w)
    vn = v.shape[3]
    ws, L = zeroed(b, h, w, vn, HN)
    out = voting.ransac_voting_layer_v3_from_logits(seg, v, HN, inlier_thresh=THRESH, seed=SEED, workspace=ws)
    d = voting._debug_views(ws, L)
    want = reference_mask(seg).view(b, h * w)
    got = unpack(d["bits"], h * w)
    bad = got != want
    assert not bool(bad.any()), \
        f"{int(bad.sum())} of {bad.numel()} mask pixels differ from torch.argmax (first at (image, pixel) {bad.nonzero()[0].tolist()})"
    assert torch.equal(d["tn0"].long(), want.sum(1)), (d["tn0"].tolist(), want.sum(1).tolist())
    if nc == 1:   # every pixel background: every image skipped, key-points zero
        assert not bool(want.any()) and not bool(out.any())
    else:
        assert bool(want.all(1).logical_not().all()) and bool(want.any(1).all())   # both kinds of pixel in every image


# ---------------------------------------------------------------------------------------------------------------------------------
# B: the whole call, fused entry against the two-step call
# ---------------------------------------------------------------------------------------------------------------------------------
def fused_call(seg, v, hn, max_num=30000, **kw):
    b, _, h, w = seg.shape
    ws, L = zeroed(b, h, w, v.shape[3], hn, max_num)
    out = voting.ransac_voting_layer_v3_from_logits(seg, v, hn, inlier_thresh=THRESH, max_num=max_num, seed=SEED, workspace=ws,
                                                    **kw)
    return out, voting._debug_views(ws, L)


def two_step_call(seg, v, hn, max_num=30000, **kw):
    """the reference's EvalWrapper: torch.argmax, then the layer on the field widened to float32"""
    b, _, h, w = seg.shape
    ws, L = zeroed(b, h, w, v.shape[3], hn, max_num)
    vf = v.float()
    out = voting.ransac_voting_layer_v3(torch.argmax(seg, 1), vf, hn, inlier_thresh=THRESH, max_num=max_num, seed=SEED,
                                        workspace=ws, **kw)
    return out, voting._debug_views(ws, L)


def assert_same_call(a, b):
    (oa, da), (ob, db) = a, b
    tn = da["tn"].cpu()
    assert torch.equal(da["tn0"], db["tn0"]), f"foreground pixels per image {da['tn0'].tolist()} against {db['tn0'].tolist()}"
    assert torch.equal(tn, db["tn"].cpu())
    assert torch.equal(da["bits"], db["bits"])
    for bi in range(tn.numel()):
        assert torch.equal(da["pix"][bi, :int(tn[bi])], db["pix"][bi, :int(tn[bi])]), f"image {bi}: compacted pixel lists differ"
    assert torch.equal(da["hyp"], db["hyp"])
    bad = da["counts"] != db["counts"]
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} counts differ"
    assert torch.equal(da["win"], db["win"])
    assert torch.equal(da["cull_bits"], db["cull_bits"])
    assert torch.equal(oa, ob)


def backbone_output(b, h, w, first, noise, dt, logit_noise, vn=BACKBONE_VN, radius=40):
    """a synthetic backbone output [b, 2 + 2 vn, h, w] of dtype dt: two-class logits (foreground +1 / background -1 apart, plus
    Gaussian noise of the given sigma) ahead of the planar field, as model_repository.py:76-78 returns them"""
    mask, planar, _ = synth.make_batch(b, first_index=first, h=h, w=w, vn=vn, radius=radius, noise=noise,
                                       background="normal" if noise else "zeros")
    m = torch.from_numpy(mask).to(dev()).float()
    g = torch.Generator(device=dev()).manual_seed(first)
    y = torch.empty((b, 2 + 2 * vn, h, w), dtype=dt, device=dev())
    y[:, 0] = (1.0 - m + logit_noise * torch.randn(m.shape, generator=g, device=dev())).to(dt)
    y[:, 1] = (m + logit_noise * torch.randn(m.shape, generator=g, device=dev())).to(dt)
    y[:, 2:] = torch.from_numpy(planar).to(dev()).to(dt)
    return y


def test_eval_wrapper_on_backbone_output_in_place():
    """tools/e2e_amd.py's configuration: EvalWrapper(512, 0.99) on a bf16 [32, 20, 480, 640] output, logits and field read in
    place -- key-points torch.equal to the two-step call; then counts, winners and pixel lists of the same call with a fixed seed"""
    b, h, w = 32, 480, 640
    y = backbone_output(b, h, w, 4400, noise=True, dt=torch.bfloat16, logit_noise=0.4)
    seg, field = y[:, :2], y[:, 2:]
    v = synth.planar_to_vertex_view(field)
    wrap = voting.EvalWrapper(512, 0.99)
    torch.manual_seed(11)
    a = wrap(seg, field).clone()
    torch.manual_seed(11)
    ref = voting.ransac_voting_layer_v3(torch.argmax(seg, 1), v.float(), 512, inlier_thresh=0.99)
    assert torch.equal(a, ref)
    f, t = fused_call(seg, v, 512), two_step_call(seg, v, 512)
    assert f[1]["layout"].cull == 0   # hn 512: the dense scoring launch
    assert_same_call(f, t)


# the two inputs on which the fused entry once disagreed with torch.argmax: (foreground logits, background logits) per dtype
DISAGREEING = {torch.float32: ((0.0, NAN), (NAN, 0.0)), torch.float16: ((5.0, NAN), (NAN, NAN)),
               torch.bfloat16: ((-INF, NAN), (NAN, 1.0)),                                  # NaN is the maximum, the first wins
               torch.float64: ((1.0, 1.0 + 1e-12), (1.0 + 1e-12, 1.0)),                      # one float32, two float64 values
               torch.int32: ((2 ** 30, 2 ** 30 + 1), (2 ** 30 + 1, 2 ** 30))}


@pytest.mark.parametrize("dt", list(DISAGREEING), ids=str)
def test_nan_logits_and_wide_ties_through_the_entry_point(dt):
    """every foreground pixel's logits are NaN-carrying (half and single precision) or differ only below float32's resolution
    (float64, int32): the whole call equals the two-step call"""
    b, h, w, vn = 2, 96, 128, 9
    mask, planar, _ = synth.make_batch(b, first_index=4800, h=h, w=w, vn=vn, radius=20, noise=True, background="normal")
    m = torch.from_numpy(mask).to(dev())
    fg, bg = (torch.tensor(x, dtype=torch.float64 if dt.is_floating_point else torch.int64, device=dev()) for x in DISAGREEING[dt])
    seg = torch.where(m.bool().unsqueeze(-1), fg, bg).permute(0, 3, 1, 2).to(dt)
    assert torch.equal(torch.argmax(seg, 1), m)
    v = synth.planar_to_vertex_view(torch.from_numpy(planar).to(dev()))
    assert_same_call(fused_call(seg, v, 128), two_step_call(seg, v, 128))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=str)
def test_fused_entry_at_a_culling_layout(dt):
    """clean fields at test_release_scoring's culling shape: the fused entry's call disc-culls, and equals the two-step call"""
    b, h, w, vn, hn = HEAVY_SHAPE
    y = backbone_output(b, h, w, 4500, noise=False, dt=dt, logit_noise=0.05, vn=vn, radius=30)
    seg, v = y[:, :2], synth.planar_to_vertex_view(y[:, 2:])
    f = fused_call(seg, v, hn)
    assert f[1]["layout"].cull == 1 and bool(f[1]["cull_bits"].any())
    assert_same_call(f, two_step_call(seg, v, hn))


@pytest.mark.parametrize("dt", [torch.float32, torch.float16], ids=str)
def test_fused_entry_feeds_the_thinning(dt):
    """a foreground of ~5 000 pixels against max_num 1 000: the fused K1 builds the thinning histograms, and the compacted pixel
    lists equal the two-step call's"""
    y = backbone_output(4, 120, 160, 4600, noise=True, dt=dt, logit_noise=0.3)
    seg, v = y[:, :2], synth.planar_to_vertex_view(y[:, 2:])
    f = fused_call(seg, v, 256, max_num=1000)
    tn0, tn = f[1]["tn0"].cpu(), f[1]["tn"].cpu()
    assert bool((tn0 > 2000).all()) and bool((tn < tn0).all()) and bool((tn > 0).all()), (tn0.tolist(), tn.tolist())
    assert_same_call(f, two_step_call(seg, v, 256, max_num=1000))


# ---------------------------------------------------------------------------------------------------------------------------------
# C: half-precision fields through the culling path
# ---------------------------------------------------------------------------------------------------------------------------------
def vote(m, v, literal=False, **kw):
    ws, L = zeroed(*HEAVY_SHAPE)
    out, d = voting.ransac_voting_layer_v3(m, v, HEAVY_SHAPE[4], inlier_thresh=THRESH, seed=SEED, literal=literal, return_debug=True,
                                           workspace=ws, **kw)
    assert d["mode"] == ("literal" if literal else "exact")
    return out.clone(), d["counts"].clone(), d["win"].clone(), d["hyp"].cpu().numpy().tobytes(), d


@pytest.mark.parametrize("sel", [None, "all"], ids=["library_selects", "every_keypoint_culled"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=str)
def test_half_precision_fields_at_a_culling_layout(dt, sel):
    """even images clean, odd images noisy, the planar field in bf16 / f16 read in place: exact-mode counts equal literal mode's,
    the float32 call's on .float() of the field and the reference kernel's; v5's confidence and the voting distribution equal
    their float32 calls"""
    b, h, w, vn, hn = HEAVY_SHAPE
    mask, planar, _ = synth.make_batch(b, first_index=4700, h=h, w=w, vn=vn, radius=30, noise=False, background="zeros")
    mn, pn, _ = synth.make_batch(b, first_index=4700, h=h, w=w, vn=vn, radius=30, noise=True, background="normal")
    mask[1::2], planar[1::2] = mn[1::2], pn[1::2]
    m = torch.from_numpy(mask).to(dev())
    p16 = torch.from_numpy(planar).to(dev()).to(dt)
    v16, v32 = synth.planar_to_vertex_view(p16), synth.planar_to_vertex_view(p16.float())
    assert v16.dtype == dt and not v16.is_contiguous()
    voting.set_cull_selection(sel)
    lit = vote(m, v16, literal=True)
    ex = vote(m, v16)
    ex32 = vote(m, v32)
    d = ex[4]
    bits = d["cull_bits"]
    assert d["layout"].cull == 1
    assert bool(bits.all()) if sel == "all" else bool(bits[0::2].any(1).all()), bits.tolist()
    assert_equal_to_literal(ex, lit)
    assert ex[3] == ex32[3] and torch.equal(ex[1], ex32[1]) and torch.equal(ex[2], ex32[2]) and torch.equal(ex[0], ex32[0])
    assert torch.equal(bits, ex32[4]["cull_bits"])
    assert_counts_equal_the_references_kernel(d, b)

    def culled(ws, L):   # the culling marks a wrapper's own v3 call left on its workspace
        return voting._debug_views(ws, L)["cull_bits"]

    res = {}
    for name, v in (("half", v16), ("float", v32)):
        ws5, L5 = zeroed(*HEAVY_SHAPE)
        kp, conf = voting.ransac_voting_layer_v5(m, v, hn, THRESH, max_num=30000, seed=SEED, workspace=ws5)
        wsd, Ld = zeroed(*HEAVY_SHAPE)
        mean, cov = voting.estimate_voting_distribution_with_mean(m, v, ex[0], round_hyp_num=256, min_hyp_num=hn, max_num=30000,
                                                                  seed=SEED, workspace=wsd)
        assert L5.cull == 1 and Ld.cull == 1
        assert torch.equal(culled(ws5, L5), bits)
        assert bool(culled(wsd, Ld).all()) if sel == "all" else bool(culled(wsd, Ld)[0::2].any(1).all())
        res[name] = (kp, conf, cov)
    assert torch.equal(res["half"][0], ex[0])
    for x, y in zip(res["half"], res["float"]):
        assert torch.equal(x, y)
