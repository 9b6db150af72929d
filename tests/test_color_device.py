"""GPU tests of the colour jitter on the device (pvnet_amd/color.py, pvnet_amd/csrc/color_jitter.hip, libpvnet_color.so).

The bar is equality: the device against the numpy restatement of include/pvnet_color.h (tests/color_restatement.py), ``torch.equal``
on the output tensor for float32, bfloat16 and float16 (the restatement's float32 rounded once); the fused path against
``augment_batch`` (mask, key-points, status) and against ``jitter_batch`` run on the warped uint8 image that ``augment_batch`` made.
The restatement is held to Pillow on the CPU (tests/test_color_cpu.py); here the device is held to the bytes recorded from Pillow
(tests/golden/color_pillow.npz, no Pillow needed) and to the restatement on every colour where a float32-only hue is not Pillow's."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import augment_cases as AC  # noqa: E402
from tests import augment_restatement as ARS  # noqa: E402
from tests import color_restatement as RS  # noqa: E402

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
WIDE = dict(brightness=0.6, contrast=0.7, saturation=0.8, hue=0.5)   # wide ranges: the clips and the hue wrap are reached
ZERO = dict(brightness=0, contrast=0, saturation=0, hue=0)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvnet_amd import color
    return color


@pytest.fixture(scope="module")
def A():
    from pvnet_amd import augment
    return augment


def dev():
    return torch.device("cuda:0")


def check(K, rgb, cfg, U, mask=None, maskmul=None, t_rgb=None, dtypes=DTYPES):
    """jitter_batch against the restatement, for every output type; returns the float32 result"""
    want = torch.from_numpy(RS.jitter_batch(rgb, cfg, U, mask, maskmul))
    t_rgb = torch.from_numpy(rgb).to(dev()) if t_rgb is None else t_rgb
    t_mask = None if mask is None else torch.from_numpy(mask).to(dev())
    t_mul = None if maskmul is None else torch.tensor(maskmul, dtype=torch.int32)
    first = None
    for dt in dtypes:
        got = K.jitter_batch(t_rgb, K.ColorJitterConfig(**{**RS.DEFAULTS, **cfg}), torch.from_numpy(np.asarray(U, np.float64)), out_dtype=dt,
                             mask=t_mask, maskmul=t_mul)
        torch.cuda.synchronize()
        assert got.dtype == dt and tuple(got.shape) == (len(rgb), 3) + rgb.shape[1:3] and got.is_contiguous()
        assert torch.equal(got.cpu(), want.to(dt)), dt
        first = got if first is None else first
    return first


def uniforms(b, seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (b, 5))


def test_all_orders(K):
    """b = 24, one order per image, under the reference's ranges and under wide ones"""
    rgb = np.random.default_rng(1).integers(0, 256, (24, 16, 24, 3), dtype=np.uint8)
    U = uniforms(24, 2)
    U[:, 4] = (np.arange(24) + 0.5) / 24
    assert len({tuple(RS.chain({}, u)[4]) for u in U}) == 24
    check(K, rgb, {}, U)
    check(K, rgb, WIDE, U)


def test_vector_and_scalar_stores_and_a_strided_view(K):
    rng = np.random.default_rng(3)
    U = uniforms(3, 4)
    U[:, 4] = (0.5 / 24, 9.5 / 24, 23.5 / 24)
    rgb = rng.integers(0, 256, (3, 32, 48, 3), dtype=np.uint8)          # the vector stores, the packed loads
    check(K, rgb, WIDE, U)
    odd = rng.integers(0, 256, (3, 37, 43, 3), dtype=np.uint8)          # the scalar stores, a tail lane per row, two blocks per image
    check(K, odd, WIDE, U)
    # a strided view: rows longer than the image, a gap between the images, pixels 4 bytes apart
    big = torch.full((3, 40, 50, 4), 77, dtype=torch.uint8, device=dev())
    big[:, :37, :43, :3] = torch.from_numpy(odd).to(dev())
    view = big[:, :37, :43, :3]
    assert not view.is_contiguous() and view.stride(3) == 1 and view.stride(2) == 4
    check(K, odd, WIDE, U, t_rgb=view)
    big = torch.full((3, 35, 56, 3), 77, dtype=torch.uint8, device=dev())
    big[:, :32, 3:51] = torch.from_numpy(rgb).to(dev())
    view = big[:, :32, 3:51]                                             # packed pixels whose rows begin off a dword boundary
    assert not view.is_contiguous() and view.stride(2) == 3
    check(K, rgb, WIDE, U, t_rgb=view)


def test_constructed_images(K):
    """all black, all 255, a grey ramp, pure primaries and secondaries (maxc ties two channels), every order"""
    h, w = 8, 24
    black, white = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    ramp = np.repeat((np.arange(h * w) * 255 // (h * w - 1)).astype(np.uint8).reshape(h, w, 1), 3, axis=2)
    colours = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [200, 200, 10], [9, 130, 130]],
                       np.uint8)
    prim = np.ascontiguousarray(np.broadcast_to(colours[None, np.arange(w) % 8], (h, w, 3)))
    rgb = np.stack([black, white, ramp, prim] * 6)
    U = uniforms(24, 5)
    U[:, 4] = (np.arange(24) + 0.5) / 24
    check(K, rgb, WIDE, U)
    check(K, rgb, {}, U, dtypes=(torch.float32,))
    out = RS.jitter_uint8(ramp, dict(ZERO, saturation=0.8, hue=0.5), U[2])[0]
    assert np.array_equal(out, ramp)                                     # grey stays grey under S and H


def test_reproducible_whatever_the_workspace_holds(K):
    rgb = np.random.default_rng(6).integers(0, 256, (3, 37, 43, 3), dtype=np.uint8)
    U = torch.from_numpy(uniforms(3, 7))
    cfg = K.ColorJitterConfig(**WIDE)
    t = torch.from_numpy(rgb).to(dev())
    n = K.color_workspace_bytes(3)
    dirty = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev())
    clean = torch.zeros((n,), dtype=torch.uint8, device=dev())
    a = K.jitter_batch(t, cfg, U, workspace=dirty)
    b = K.jitter_batch(t, cfg, U, workspace=clean)
    c = K.jitter_batch(t, cfg, U, workspace=dirty)       # the sums of the first call are still in it
    d = K.jitter_batch(t, cfg, U)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    assert torch.equal(a.cpu(), torch.from_numpy(RS.jitter_batch(rgb, WIDE, U.numpy())))


def test_subsets_of_steps(K):
    rgb = np.random.default_rng(8).integers(0, 256, (4, 16, 40, 3), dtype=np.uint8)
    U = uniforms(4, 9)
    U[:, 4] = (1.5 / 24, 8.5 / 24, 14.5 / 24, 22.5 / 24)
    c_only = check(K, rgb, dict(ZERO, contrast=0.7), U)
    plain = check(K, rgb, ZERO, U, dtypes=(torch.float32,))
    assert not torch.equal(c_only, plain)
    # no C: no statistics launch, and the workspace is not touched
    no_c = dict(WIDE, contrast=0)
    check(K, rgb, no_c, U)
    ws = torch.full((K.color_workspace_bytes(4),), 0xA5, dtype=torch.uint8, device=dev())
    K.jitter_batch(torch.from_numpy(rgb).to(dev()), K.ColorJitterConfig(**no_c), torch.from_numpy(U), workspace=ws)
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all())
    check(K, rgb, dict(ZERO, hue=0.5), U)
    check(K, rgb, dict(ZERO, brightness=0.9), U, dtypes=(torch.float32,))
    check(K, rgb, dict(ZERO, saturation=0.9), U, dtypes=(torch.float32,))


def test_maskmul_per_image(K):
    rng = np.random.default_rng(10)
    rgb = rng.integers(0, 256, (4, 16, 24, 3), dtype=np.uint8)
    mask = (rng.uniform(size=(4, 16, 24)) < 0.5).astype(np.uint8)
    mask[2] *= 3                                                       # a mask value other than 1 multiplies
    U = uniforms(4, 11)
    on = check(K, rgb, {}, U, mask=mask, maskmul=[1, 0, 1, 0])
    off = check(K, rgb, {}, U, dtypes=(torch.float32,))
    assert torch.equal(on[1], off[1]) and torch.equal(on[3], off[3]) and not torch.equal(on[0], off[0])
    assert bool((on[0].cpu()[:, mask[0] == 0] == 0).all())
    odd = rng.integers(0, 256, (2, 9, 13, 3), dtype=np.uint8)           # the tail lanes read no mask beyond the row
    check(K, odd, WIDE, U[:2], mask=np.ones((2, 9, 13), np.int64) * 2, maskmul=[0, 1])


def fused_inputs():
    """b = 4, source 40 x 56 -> 32 x 48, every geometric step on, use_mask_out on: image 0 takes the no-foreground path, image 1 the
    mask-out, image 2 the pad (a resize below the output's size), image 3 the multiply"""
    rng = np.random.default_rng(12)
    b, H, W = 4, 40, 56
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = rng.integers(0, 256, (b, H, W, 3), dtype=np.uint8)
    mask = np.zeros((b, H, W), np.uint8)
    for i, (cy, cx, r) in enumerate(((0, 0, 0), (18, 26, 12), (20, 30, 11), (22, 24, 10))):
        mask[i] = ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r)
    hc = np.concatenate([rng.uniform(0.0, 56.0, (b, 5, 2)), rng.uniform(0.5, 2.0, (b, 5, 1))], 2)
    U = rng.uniform(0.55, 0.75, (b, 12))                                 # every gate closed, no resize ...
    U[:, 6] = 0.9
    U[1, [0, 1, 2, 3, 4]] = 0.2, 0.9, 0.9, 0.5, 0.5                      # ... but: the mask-out,
    U[2, [6, 7, 10]] = 0.1, 0.02, 0.2                                    # a resize to about a third, which is padded, and a flip,
    U[3, 11] = 0.05                                                      # the multiply
    cfg = dict(resize_hmin=8, resize_wmin=8, resize_hmax=44, resize_wmax=44, use_mask_out=True)
    return rgb, mask, hc, U, cfg


def test_fused_path_equals_augment_then_jitter(K, A):
    rgb, mask, hc, U, cfg = fused_inputs()
    seed, size = 77, (32, 48)
    # the four paths are taken (the float64 restatement of the augmentation says so)
    _, wm, _, wstatus, plans = ARS.augment_batch(rgb, mask, hc, *size, cfg, U, seed)
    assert wstatus[0] & ARS.S_NO_FOREGROUND and not any(wstatus[1:] & ARS.S_NO_FOREGROUND)
    unmasked = ARS.augment_one(rgb[1], mask[1], hc[1], *size, cfg, np.concatenate([[0.9], U[1, 1:]]), seed, 1)[1]
    assert 0 < wm[1].sum() < unmasked.sum()
    assert plans[2]["resized"] and plans[2]["hoff"] > 0 and plans[2]["woff"] > 0 and plans[2]["flip"]
    assert [p["maskmul"] for p in plans] == [False, False, False, True] and wm[3].sum() > 0
    config, plain = A.AugmentConfig(**cfg), A.AugmentConfig(**dict(cfg, use_mask_out=False))
    args = (torch.from_numpy(rgb).to(dev()), torch.from_numpy(mask).to(dev()), torch.from_numpy(hc).to(dev()), *size)
    tU, JU = torch.from_numpy(U), torch.from_numpy(uniforms(4, 13))
    base = A.augment_batch(*args, config, tU, seed)
    # the warped uint8 image, recovered exactly from the float32 output without the multiply
    x = A.augment_batch(*args, plain, tU, seed)[0]
    mean, std = (torch.tensor(v, dtype=torch.float32, device=dev()).view(1, 3, 1, 1) for v in (A.MEAN, A.STD))
    warped = torch.round((x * std + mean) * 255.0)
    assert float(warped.min()) >= 0 and float(warped.max()) <= 255
    warped = warped.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(A.normalize_batch(warped), x)                    # it round-trips
    maskmul = torch.tensor([int(p["maskmul"]) for p in plans], dtype=torch.int32)
    for jcfg in (K.ColorJitterConfig(**WIDE), K.ColorJitterConfig()):
        for dt in DTYPES:
            for mdt in (torch.uint8, torch.int64):
                got = K.augment_jitter_batch(*args, config, jcfg, tU, JU, seed, out_dtype=dt, mask_dtype=mdt)
                torch.cuda.synchronize()
                assert got[0].dtype == dt and got[1].dtype == mdt
                assert torch.equal(got[1], base[1].to(mdt)) and torch.equal(got[2], base[2]) and torch.equal(got[3], base[3])
                want = K.jitter_batch(warped, jcfg, JU, out_dtype=dt, mask=base[1], maskmul=maskmul)
                assert torch.equal(got[0], want), (dt, mdt)
    # against the restatement too, once
    got = K.augment_jitter_batch(*args, config, K.ColorJitterConfig(**WIDE), tU, JU, seed)
    want = RS.jitter_batch(warped.cpu().numpy(), WIDE, JU.numpy(), wm, maskmul.tolist())
    assert torch.equal(got[0].cpu(), torch.from_numpy(want))
    # with all ranges 0 the image is augment_batch's own
    for dt in DTYPES:
        got = K.augment_jitter_batch(*args, config, K.ColorJitterConfig(**ZERO), tU, JU, seed, out_dtype=dt)
        assert torch.equal(got[0], A.augment_batch(*args, config, tU, seed, out_dtype=dt)[0]) and torch.equal(got[1], base[1])
    # an output the vector stores do not fit (width 43), and a dirty workspace
    odd = (31, 43)
    ws = torch.full((K.color_workspace_bytes(4, *odd),), 0xFF, dtype=torch.uint8, device=dev())
    args = args[:3] + odd
    got = K.augment_jitter_batch(*args, config, K.ColorJitterConfig(**WIDE), tU, JU, seed, workspace=ws)
    base = A.augment_batch(*args, config, tU, seed)
    x = A.augment_batch(*args, plain, tU, seed)[0]
    warped = torch.round((x * std + mean) * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    plans = ARS.augment_batch(rgb, mask, hc, *odd, cfg, U, seed)[4]
    maskmul = torch.tensor([int(p["maskmul"]) for p in plans], dtype=torch.int32)
    assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]) and torch.equal(got[3], base[3])
    assert torch.equal(got[0], K.jitter_batch(warped, K.ColorJitterConfig(**WIDE), JU, mask=base[1], maskmul=maskmul))


def test_fused_path_under_the_warps_own_oracles(K, A):
    """``augment_jitter_batch`` compiles the same warp (pvnet_amd/csrc/augment_warp.h) into another library.  With all four ranges
    0 its image satisfies the ramp's closed form (tests/augment_cases.py: the inverse of the composed forward maps, bar 0.5 + 1e-6)
    on one batch of the ramp set per store path, and its mask is the one the reference's own chain gave for the recorded ramp cases
    (tests/golden/augment.npz), whose image it meets to 1 grey level 2 px inside the source."""
    import json
    zero = K.ColorJitterConfig(**ZERO)
    for g in [x for x in AC.ramp_set() if x["name"] in ("mixed->(32, 40)", "mixed->(31, 37)")]:
        n = len(g["rgb"])
        got = K.augment_jitter_batch(torch.from_numpy(g["rgb"]).to(dev()), torch.from_numpy(g["mask"]).to(dev()), torch.from_numpy(g["hc"]).to(dev()),
                                     *g["size"], A.AugmentConfig(**g["cfg"]), zero, torch.from_numpy(g["U"]), torch.from_numpy(uniforms(n, 15)),
                                     g["seed"])
        torch.cuda.synchronize()
        assert got[3].tolist() == [0] * n and got[0].dtype == torch.float32
        worst, counts, _ = AC.ramp_check(got[0].cpu().numpy(), g)
        print(f"fused, {g['name']}: worst |v - I(sx, sy)| = {worst:.8f} on {sum(counts)} interior pixels")
        assert worst <= AC.RAMP_BAR and min(counts) >= AC.RAMP_MIN_INTERIOR_PER_SAMPLE and sum(counts) >= 15000, (worst, counts)
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz"))
    names = [str(x) for x in golden["ramp_cases"]]
    assert len(names) == 5
    for name in names:
        rgb, mask, hc, U = AC.golden_rgb(golden, name), golden[name + ".mask"], golden[name + ".hcoords"], golden[name + ".uniforms"]
        size, cfg, seed = tuple(int(v) for v in golden[name + ".size"]), json.loads(str(golden[name + ".cfg"])), int(golden[name + ".seed"])
        got = K.augment_jitter_batch(torch.from_numpy(rgb[None]).to(dev()), torch.from_numpy(mask[None]).to(dev()),
                                     torch.from_numpy(hc[None]).to(dev()), *size, A.AugmentConfig(**cfg), zero, torch.from_numpy(U[None]),
                                     torch.from_numpy(uniforms(1, 16)), seed)
        torch.cuda.synchronize()
        assert np.array_equal(got[1].cpu().numpy()[0], golden[name + ".ref_mask"]) and golden[name + ".ref_mask"].sum() > 0, name
        assert np.array_equal(got[2].cpu().numpy()[0], golden[name + ".ref_hcoords"]), name
        plan = ARS.augment_one(rgb, mask, hc, *size, cfg, U, seed)[4]
        worst, pixels, _ = AC.two_pass_difference(AC.recover_uint8(got[0].cpu().numpy())[0], golden[name + ".ref_image"], plan, 48, 64)
        assert worst <= 1 and pixels >= 200, (name, worst, pixels)


def test_fused_multiply_with_mask_values_above_255(K, A):
    """The fused multiply reads ``mask_out``: an int64 ``mask_out`` holds the source's values, so the image with all ranges 0 is
    ``augment_batch``'s; a uint8 ``mask_out`` keeps their low 8 bits, the restriction include/pvnet_color.h documents."""
    rgb, mask, hc, U, cfg = fused_inputs()
    wide = mask.astype(np.int64) * 300                                  # 300 = 256 + 44
    config, size, seed = A.AugmentConfig(**cfg), (32, 48), 77
    args = (torch.from_numpy(rgb).to(dev()), torch.from_numpy(wide).to(dev()), torch.from_numpy(hc).to(dev()), *size)
    tU, JU = torch.from_numpy(U), torch.from_numpy(uniforms(4, 13))
    zero = K.ColorJitterConfig(**ZERO)
    base = A.augment_batch(*args, config, tU, seed, mask_dtype=torch.int64)
    assert int(base[1][3].max()) == 300                                 # image 3 takes the multiply
    got = K.augment_jitter_batch(*args, config, zero, tU, JU, seed, mask_dtype=torch.int64)
    assert all(torch.equal(g, w) for g, w in zip(got, base))
    # uint8 out: mask_out is augment_batch's, the image is multiplied by what mask_out holds
    base8 = A.augment_batch(*args, config, tU, seed)
    got8 = K.augment_jitter_batch(*args, config, zero, tU, JU, seed)
    assert int(base8[1][3].max()) == 44 and torch.equal(got8[1], base8[1])
    low = A.augment_batch(args[0], torch.from_numpy((mask * 44).astype(np.uint8)).to(dev()), *args[2:], config, tU, seed)
    assert torch.equal(low[1], base8[1]) and torch.equal(got8[0], low[0]) and torch.equal(got8[0][:3], base8[0][:3])
    assert not torch.equal(got8[0][3], base8[0][3])


def test_graph_capture_replays_with_changed_uniforms(K, A):
    rgb, mask, hc, U, cfg = fused_inputs()
    config, jcfg = A.AugmentConfig(**cfg), K.ColorJitterConfig(**WIDE)
    args = (torch.from_numpy(rgb).to(dev()), torch.from_numpy(mask).to(dev()), torch.from_numpy(hc).to(dev()), 32, 48, config, jcfg)
    rng = np.random.default_rng(14)
    rounds = [(A.pack_uniforms(torch.from_numpy(rng.uniform(0.05, 0.95, (4, 12))), config, dev()),
               torch.from_numpy(rng.uniform(0.0, 1.0, (4, 5))).to(dev())) for _ in range(3)]
    eager = [tuple(t.clone() for t in K.augment_jitter_batch(*args, u, ju, 5)) for u, ju in rounds]
    torch.cuda.synchronize()
    assert not torch.equal(eager[0][0], eager[1][0])
    u, ju = rounds[0][0].clone(), rounds[0][1].clone()
    out = tuple(torch.empty_like(t) for t in eager[0])
    ws = torch.empty(K.color_workspace_bytes(4, 32, 48), dtype=torch.uint8, device=dev())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.augment_jitter_batch(*args, u, ju, 5, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.augment_jitter_batch(*args, u, ju, 5, out=out, workspace=ws)
    for k in (1, 2):
        u.copy_(rounds[k][0])
        ju.copy_(rounds[k][1])
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[k], out):
            assert torch.equal(a, b), k


def test_output_feeds_the_head_loss(K, A):
    """augment_jitter_batch -> HeadLoss.from_keypoints, forward and backward, once"""
    from pvnet_amd.validation import HeadLoss
    rgb, mask, hc, U, cfg = fused_inputs()
    config = A.AugmentConfig(**dict(cfg, use_mask_out=False))
    image, m, k, status = K.augment_jitter_batch(torch.from_numpy(rgb).to(dev()), torch.from_numpy(mask).to(dev()), torch.from_numpy(hc).to(dev()),
                                                 32, 48, config, K.ColorJitterConfig(), torch.from_numpy(U), K.draw_jitter_uniforms(4), 3)
    b, vn = hc.shape[:2]
    gen = torch.Generator().manual_seed(3)
    seg = torch.randn((b, 2, 32, 48), generator=gen).to(dev()).requires_grad_(True)
    vp = torch.randn((b, 2 * vn, 32, 48), generator=gen).to(dev()).requires_grad_(True)
    loss_seg, loss_vertex, precision, recall = HeadLoss().from_keypoints(seg, vp, m, k)
    (loss_seg.sum() + loss_vertex.sum()).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(image).all()) and float(loss_vertex.detach().sum()) > 0 and bool(torch.isfinite(vp.grad).all())
    assert bool(torch.isfinite(seg.grad).all()) and status.tolist()[0] == ARS.S_NO_FOREGROUND


# ---- the device against the bytes recorded from Pillow, and on the colours where a float32-only hue is not Pillow's ----------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_pillow.npz")
KEYS = ("brightness", "contrast", "saturation", "hue")


def golden_groups():
    """the fixture's 48 cases x 2 draws, grouped by configuration: (cfg, rgb [n,32,40,3], uniforms [n,5], Pillow's bytes [n,32,40,3])"""
    z = np.load(GOLDEN)
    image, ranges, U, want = z["image"], z["ranges"], z["uniforms"], z["want"]
    groups = {}
    for c in range(48):
        groups.setdefault(tuple(ranges[c].tolist()), []).append(c)
    assert len(groups) == 5 and sum(len(v) for v in groups.values()) == 48
    for key, cases in groups.items():
        n = 2 * len(cases)
        yield (dict(zip(KEYS, key)), np.ascontiguousarray(np.broadcast_to(image, (n,) + image.shape)), U[cases].reshape(n, 5),
               want[cases].reshape((n,) + image.shape), str(z["pil_version"]))


def normalized(want):
    return torch.from_numpy(np.stack([RS.normalize(w.astype(np.int64)) for w in want]))


def test_jitter_batch_gives_the_bytes_recorded_from_pillow(K):
    for cfg, rgb, U, want, version in golden_groups():
        ref = normalized(want)
        t_rgb, t_U = torch.from_numpy(rgb).to(dev()), torch.from_numpy(U)
        for dt in DTYPES:
            got = K.jitter_batch(t_rgb, K.ColorJitterConfig(**cfg), t_U, out_dtype=dt)
            torch.cuda.synchronize()
            bad = (got.cpu() != ref.to(dt)).flatten(1).any(1).nonzero().flatten().tolist()
            assert torch.equal(got.cpu(), ref.to(dt)), f"{cfg}, {dt}: images {bad} differ from what Pillow {version} gave"


def test_fused_path_gives_the_bytes_recorded_from_pillow(K, A):
    """``augment_jitter_batch`` under the identity geometric plan: nothing masked, rotated, cropped, resized or flipped"""
    identity = A.AugmentConfig(mask=False, rotation=False, crop=False, flip=False, use_mask_out=False)
    for cfg, rgb, U, want, version in golden_groups():
        n, h, w = rgb.shape[:3]
        ref = normalized(want)
        mask = np.zeros((n, h, w), np.uint8)
        mask[:, 8:20, 10:30] = 1
        hc = np.tile(np.array([[5.0, 7.0, 1.0], [30.0, 20.0, 2.0]]), (n, 1, 1))
        args = (torch.from_numpy(rgb).to(dev()), torch.from_numpy(mask).to(dev()), torch.from_numpy(hc).to(dev()), h, w, identity)
        tU = torch.from_numpy(np.random.default_rng(31).uniform(0.0, 1.0, (n, 12)))
        plain = A.augment_batch(*args, tU, 3)
        assert torch.equal(plain[0], A.normalize_batch(args[0])) and torch.equal(plain[1].cpu(), torch.from_numpy(mask))   # the identity
        for dt in DTYPES:
            got = K.augment_jitter_batch(*args, K.ColorJitterConfig(**cfg), tU, torch.from_numpy(U), 3, out_dtype=dt)
            torch.cuda.synchronize()
            assert torch.equal(got[0].cpu(), ref.to(dt)), f"{cfg}, {dt}: differs from what Pillow {version} gave"
            assert torch.equal(got[1], plain[1]) and torch.equal(got[2], plain[2]) and torch.equal(got[3], plain[3])


@pytest.fixture(scope="module")
def hard_image():
    """[1,282,256,3] uint8: every colour on which the hue computed in float32 throughout and the definition's differ (72 036 of the
    2^24, found here from the two numpy formulas), shuffled, the last row filled up with the first colours again"""
    found = []
    for r0 in range(0, 256, 16):
        r, g, b = np.meshgrid(np.arange(r0, r0 + 16), np.arange(256), np.arange(256), indexing="ij")
        img = np.stack([r, g, b], -1).reshape(-1, 3).astype(np.uint8)
        found.append(img[RS.rgb_to_hsv(img)[0] != RS.rgb_to_hsv(img, float32_only=True)[0]])
    hard = np.random.default_rng(40).permutation(np.concatenate(found))
    assert len(hard) == 72036
    w = 256
    h = -(-len(hard) // w)
    return np.concatenate([hard, hard[:h * w - len(hard)]]).reshape(1, h, w, 3)


def branches(rgb):
    """how many pixels take the r, g and b branch of the forward hue"""
    c = rgb.reshape(-1, 3).astype(np.int64)
    m = c.max(1)
    return [int((c[:, 0] == m).sum()), int(((c[:, 0] != m) & (c[:, 1] == m)).sum()), int(((c[:, 0] != m) & (c[:, 1] != m)).sum())]


HUE_ONLY = dict(ZERO, hue=0.5)
HUE_U = np.array([[0.3, 0.3, 0.3, u3, 0.5] for u3 in (0.5, 0.6, 0.4)])   # fh = 0, 0.1, -0.1: shifts 0, +25, -25


def check_hard(K, rgb):
    assert [RS.hue_shift(RS.chain(HUE_ONLY, u)[3]) for u in HUE_U] == [0, 25, 256 - 25]
    assert all(RS.chain(HUE_ONLY, u)[4] == [RS.H] for u in HUE_U) and min(branches(rgb)) > 0
    batch = np.ascontiguousarray(np.broadcast_to(rgb, (3,) + rgb.shape[1:]))
    check(K, batch, HUE_ONLY, HUE_U)
    # these are the colours the float32-only hue gets wrong: with it every pixel's h is another, and the images differ
    old = np.stack([RS.hsv_to_rgb((h + RS.hue_shift(RS.chain(HUE_ONLY, u)[3])) % 256, s, v)
                    for u in HUE_U for h, s, v in [RS.rgb_to_hsv(rgb[0], float32_only=True)]])
    new = np.stack([RS.jitter_uint8(rgb[0], HUE_ONLY, u)[0] for u in HUE_U])
    assert all(bool((o != n).any()) for o, n in zip(old, new))


def test_hard_colours_on_the_vector_path(K, hard_image):
    assert hard_image.shape[2] % 8 == 0
    check_hard(K, hard_image)


def test_hard_colours_on_the_element_path(K, hard_image):
    check_hard(K, np.ascontiguousarray(hard_image[:, :33, :47]))
