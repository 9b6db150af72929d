"""GPU tests of the augmentation on the device (pvnet_amd/augment.py, pvnet_amd/csrc/augment.hip, libpvnet_augment.so).

The bar is equality: the device against the numpy restatement of include/pvnet_augment.h (tests/augment_restatement.py), bit for bit,
and its key-points and masks against what the reference's own ``augmentation`` returned (tests/golden/augment.npz).  Two oracles
that do not descend from the header hold the image of rotated and resized samples: the closed form of a ramp source under the
inverse of the composed forward maps (tests/augment_cases.py, bar 0.5 + 1e-6), and the reference's own chain over stand-in
samplers, recorded in the fixture (ramp pictures, at most 1 grey level 2 px inside the source)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import augment_cases as AC  # noqa: E402
from tests import augment_restatement as RS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "augment.npz")
GROW = dict(resize_hmin=24, resize_hmax=44, resize_wmin=24, resize_wmax=44)


@pytest.fixture(scope="module")
def A():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from pvnet_amd import augment
    return augment


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def bits(t):
    """the bit pattern of a float tensor (host)"""
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def run(A, rgb, mask, hc, size, cfg, U, seed, out_dtype=torch.float32, mask_dtype=torch.uint8, pad_strides=False, mask_in=torch.uint8,
        by_value=False, want=None):
    """one device call against the restatement (``want``: its output where a caller has it already); returns both sides"""
    dev = torch.device("cuda:0")
    config = A.AugmentConfig(**cfg)
    if want is None:
        want = RS.augment_batch(rgb, mask, hc, size[0], size[1], cfg, U, seed)
    t_rgb, t_mask = torch.from_numpy(rgb).to(dev), torch.from_numpy(mask).to(dev).to(mask_in)
    if pad_strides:   # rows longer than the image, a gap between the images: any strides with the channel stride 1
        b, h, w = mask.shape
        big = torch.full((b, h + 3, w + 5, 3), 77, dtype=torch.uint8, device=dev)
        big[:, :h, :w] = t_rgb
        t_rgb = big[:, :h, :w]
        bigm = torch.full((b, h + 1, 2 * w + 3), 9, dtype=mask_in, device=dev)
        bigm[:, :h, 0:2 * w:2] = t_mask
        t_mask = bigm[:, :h, 0:2 * w:2]
        assert not t_rgb.is_contiguous() and t_mask.stride(2) == 2
    got = A.augment_batch(t_rgb, t_mask, torch.from_numpy(hc).to(dev), size[0], size[1], config, torch.from_numpy(np.asarray(U, np.float64)),
                          seed, out_dtype=out_dtype, mask_dtype=mask_dtype)
    torch.cuda.synchronize()
    image, m, hco, status = got
    assert image.dtype == out_dtype and m.dtype == mask_dtype and hco.dtype == torch.float64 and status.dtype == torch.int32
    assert tuple(image.shape) == (len(rgb), 3) + tuple(size) and image.is_contiguous() and hco.is_contiguous()
    assert np.array_equal(status.cpu().numpy(), want[3]), (status.cpu().numpy(), want[3])
    assert np.array_equal(hco.cpu().numpy(), want[2])
    assert np.array_equal(m.cpu().numpy().astype(np.int64), want[1])
    ref_image = torch.from_numpy(want[0]).to(out_dtype)   # rounded once from the float32 definition
    if by_value:
        assert bool((image.cpu() == ref_image).all())     # (use_mask_out: a product with 0 may be -0)
    else:
        assert torch.equal(bits(image), bits(ref_image))
    return got, want


def case(g, n):
    return (AC.golden_rgb(g, n)[None], g[n + ".mask"][None], g[n + ".hcoords"][None], tuple(int(v) for v in g[n + ".size"]),
            json.loads(str(g[n + ".cfg"])), g[n + ".uniforms"][None], int(g[n + ".seed"]))


def test_identity_plan_equals_the_torch_composition(A, golden):
    rgb = np.stack([golden[n + ".rgb"] for n in ("all_open", "all_closed", "pad_both")])
    mask = np.stack([golden[n + ".mask"] for n in ("all_open", "all_closed", "pad_both")])
    hc = np.stack([golden["all_open.hcoords"]] * 3)
    x = torch.from_numpy(rgb)
    mean, std = torch.tensor(A.MEAN, dtype=torch.float32).view(1, 3, 1, 1), torch.tensor(A.STD, dtype=torch.float32).view(1, 3, 1, 1)
    want = x.permute(0, 3, 1, 2).float().div(255).sub(mean).div(std)
    dev = torch.device("cuda:0")
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert torch.equal(A.normalize_batch(x.to(dev), dt).cpu(), want.to(dt))
    odd = x[:, :45, :61]   # a view: rows of 61 pixels, the element path
    assert torch.equal(A.normalize_batch(odd.to(dev)[:, :, :, :], torch.float32).cpu(), want[:, :, :45, :61])
    image, m, hco, status = A.augment_batch(x.to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(hc).to(dev), 48, 64,
                                            A.AugmentConfig.identity(), A.draw_uniforms(3, torch.Generator().manual_seed(1)), 0)
    assert torch.equal(image.cpu(), want) and np.array_equal(m.cpu().numpy(), mask) and np.array_equal(hco.cpu().numpy(), hc)
    assert status.tolist() == [0, 0, 0]


def test_device_equals_restatement_and_reference_keypoints(A, golden):
    """every recorded case: (48,64) -> (32,40) the vector path, -> (31,37) the element path, the padded sizes; the device's
    key-points equal the REFERENCE's recorded float64 ones, and its mask the REFERENCE's recorded one, rotated and resized cases
    included"""
    seen = set()
    assert len(golden["cases"]) >= 16
    for n in (str(x) for x in golden["cases"]):
        rgb, mask, hc, size, cfg, U, seed = case(golden, n)
        got, want = run(A, rgb, mask, hc, size, cfg, U, seed)
        assert np.array_equal(got[2].cpu().numpy()[0], golden[n + ".ref_hcoords"]), n
        assert np.array_equal(got[1].cpu().numpy()[0], golden[n + ".ref_mask"]), n
        seen.add(size)
    assert {(32, 40), (31, 37), (56, 72), (48, 64)} <= seen


def test_device_image_against_the_references_chain(A, golden):
    """The device's image against the image the reference's own code chains together (rotate_instance, crop_resize_instance_v2, crop
    or pad, flip) over the stand-in samplers.  Without rotation and resize: ``==``.  Ramp pictures, rotated and resized: at most 1
    grey level wherever the source point is 2 px inside the source and the canvas point inside the canvas -- against the exact ramp
    two passes are off by at most 0.5 + 0.5, one pass by at most 0.5, so the integers differ by less than 2.  The noisy pictures:
    printed, not asserted (the deviation the header names)."""
    dev = torch.device("cuda:0")
    ramps = {str(x) for x in golden["ramp_cases"]}
    checked = 0
    for n in (str(x) for x in golden["cases"]):
        rgb, mask, hc, size, cfg, U, seed = case(golden, n)
        image, m, _, status = A.augment_batch(torch.from_numpy(rgb).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(hc).to(dev),
                                              size[0], size[1], A.AugmentConfig(**cfg), torch.from_numpy(U), seed)
        torch.cuda.synchronize()
        v = AC.recover_uint8(image.cpu().numpy())[0]
        ref = golden[n + ".ref_image"]
        plan = RS.augment_one(rgb[0], mask[0], hc[0], size[0], size[1], cfg, U[0], seed)[4]
        assert np.array_equal(m.cpu().numpy()[0], golden[n + ".ref_mask"]), n
        if not plan["rotated"] and not plan["resized"]:
            assert np.array_equal(v, ref.astype(np.int64).transpose(2, 0, 1)), n
            continue
        worst, pixels, anywhere = AC.two_pass_difference(v, ref, plan, 48, 64)
        print(f"{n}: device against the reference's two passes: at most {worst} on {pixels} pixels 2 px inside, {anywhere} anywhere")
        if n in ramps:
            assert worst <= 1 and pixels >= 200, (n, worst, pixels)
            checked += 1
    assert checked == 5


def device_images(A, group, out_dtype=torch.float32):
    """the device's output for one group of tests/augment_cases.py"""
    dev = torch.device("cuda:0")
    got = A.augment_batch(torch.from_numpy(group["rgb"]).to(dev), torch.from_numpy(group["mask"]).to(dev), torch.from_numpy(group["hc"]).to(dev),
                          group["size"][0], group["size"][1], A.AugmentConfig(**group["cfg"]), torch.from_numpy(group["U"]), group["seed"],
                          out_dtype=out_dtype)
    torch.cuda.synchronize()
    return got


def test_device_image_equals_the_ramp_closed_form(A):
    """The device's float32 image, directly (not through the restatement), against ``rint(I(sx, sy))`` of a ramp source: the source
    point is the inverse of the composed forward maps R, S, C, F in float64 (tests/augment_cases.py), the bar 0.5 (the one rint) +
    1e-6.  300 samples of status 0 over three resize ranges and four targets, 503 372 interior pixels; one group with the mask-out
    gate open (pixels with a tap in the rectangle left out); a 37 x 53 source.  bfloat16 and float16 are the float32 result rounded
    once, on the vector path (32,40) and the element path (31,37)."""
    worst, counts = 0.0, []
    groups = AC.ramp_set()
    for g in groups + (AC.ramp_maskout_case(),) + AC.ramp_odd_source():
        main = any(g is x for x in groups)
        image, m, _, status = device_images(A, g)
        assert image.dtype == torch.float32 and status.tolist() == [0] * len(g["rgb"])
        w, c, left = AC.ramp_check(image.cpu().numpy(), g)
        print(f"{g['name']}: worst {w:.8f} on {sum(c)} interior pixels, {sum(left)} left out")
        assert w <= AC.RAMP_BAR, (g["name"], w)
        assert min(c) >= (AC.RAMP_MIN_INTERIOR_PER_SAMPLE if main else 500) and (sum(left) >= 500) == bool(g["maskout"])
        if main:
            worst, counts = max(worst, w), counts + c
        if g["size"] in ((32, 40), (31, 37)) and (g["name"].startswith("mixed") or g["name"].startswith("37x53")):
            for dt in (torch.bfloat16, torch.float16):
                half = device_images(A, g, dt)[0]
                assert half.dtype == dt and torch.equal(bits(half), bits(image.to(dt))), (g["name"], dt)
    print(f"ramp closed form, device: worst |v - I(sx, sy)| = {worst:.8f} on {sum(counts)} interior pixels of {len(counts)} samples")
    assert len(counts) >= 250 and sum(counts) >= AC.RAMP_MIN_INTERIOR_TOTAL


def test_seeded_sweep_equals_restatement(A):
    """280 seeded samples in seven calls of 40, all twelve uniforms over [0, 1): empty, one-row, one-column, border and interior
    blobs, two source sizes, five targets, three resize ranges, the three output types, use_mask_out on and off, the three mask
    input types, padded strides.  What they cover is asserted on the CPU (tests/test_augment_cpu.py)."""
    cover = AC.sweep_coverage(AC.sweep_calls())
    assert cover["samples"] >= 192 and all(cover[f"status_{b}"] >= 1 for b in (1, 2, 4, 8))
    for c in AC.sweep_calls():
        run(A, c["rgb"], c["mask"], c["hc"], c["size"], c["cfg"], c["U"], c["seed"], out_dtype=getattr(torch, c["out_dtype"]),
            mask_dtype=getattr(torch, c["mask_dtype"]), pad_strides=c["pad_strides"], mask_in=getattr(torch, c["mask_in"]),
            by_value=bool(c["cfg"].get("use_mask_out")), want=c["want"])


def test_element_path_padded_strides_int64_masks_and_half_types(A, golden):
    rgb, mask, hc, size, cfg, U, seed = case(golden, "odd_target")
    assert size == (31, 37)
    run(A, rgb, mask, hc, size, cfg, U, seed, pad_strides=True, mask_in=torch.int64, mask_dtype=torch.int64)
    run(A, rgb, mask, hc, size, cfg, U, seed, pad_strides=True, mask_in=torch.int32, out_dtype=torch.bfloat16)
    rgb, mask, hc, size, cfg, U, seed = case(golden, "all_open")
    run(A, rgb, mask, hc, size, cfg, U, seed, out_dtype=torch.bfloat16, mask_dtype=torch.int64)   # the vector path's 2-byte stores
    run(A, rgb, mask, hc, size, cfg, U, seed, out_dtype=torch.float16, mask_in=torch.int64)


def extras(golden):
    """what the reference cannot run, in one batch under one configuration: an empty mask with the mask-out gate open, a mask that
    mask-out empties, a single pixel (hi <= lo, a bbox without extent), a rectangle with a negative start, two ordinary samples
    with every gate open / closed and use_mask_out, and a rectangle whose negative start wraps below its stop (sides above w / 2)"""
    rng = np.random.default_rng(7)
    H, W = 48, 64
    rgb = np.stack([golden[n + ".rgb"] for n in ("all_open", "all_closed", "odd_target", "negative_start", "same_size", "pad_both", "flip_crop_only")])
    mask = np.zeros((7, H, W), np.uint8)
    mask[1, 20:25, 30:35] = 1
    mask[2, 20, 30] = 1
    mask[3] = golden["negative_start.mask"]
    mask[4] = golden["all_open.mask"]
    mask[5] = golden["all_closed.mask"] * 3     # a mask value other than 1 multiplies the image under use_mask_out
    hc = np.concatenate([rng.uniform(-10.0, 70.0, (6, 4, 2)), rng.uniform(0.5, 2.0, (6, 4, 1))], 2)
    U = rng.uniform(0.05, 0.95, (6, 12))
    mask[6, 10:31, :] = 1                         # a band over the whole width: x_side = floor(63 * 1.981 / 2) = 62 about x_loc = 0
    hc = np.concatenate([hc, rng.uniform(0.0, 60.0, (1, 4, 3))])
    U = np.concatenate([U, rng.uniform(0.05, 0.95, (1, 12))])
    U[6, [0, 1, 2, 3, 4]] = 0.1, 0.99, 0.2, 0.001, 0.5   # columns [-62, 62) are numpy's [2, 62): not empty
    U[0, 0] = 0.1                                 # empty mask, gate open
    U[1, [0, 1, 2, 3, 4]] = 0.1, 0.9, 0.9, 0.99, 0.99   # emptied: sides floor(4 * 1.81 / 2) = 3 about the bbox's last-but-one pixel
    U[2, [0, 6]] = 0.2, 0.1                       # the single pixel: S_RANGE twice, S_DEGENERATE
    U[3, [0, 1, 2, 3]] = 0.3, 0.5, 0.5, 0.01      # negative start: x_loc = 0, x_side > 0
    U[4, [0, 1, 2, 6, 10, 11]] = 0.1, 0.1, 0.1, 0.1, 0.1, 0.01    # every gate open (a rectangle of sides 2 inside the blob)
    U[5, [0, 6, 10, 11]] = 0.9, 0.9, 0.9, 0.5     # every gate closed
    cfg = dict(GROW, min_mask=0.1, max_mask=2.0, use_mask_out=True)
    return rgb, mask, hc, cfg, U


def test_extensions_gates_and_use_mask_out(A, golden):
    rgb, mask, hc, cfg, U = extras(golden)
    got, want = run(A, rgb, mask, hc, (32, 40), cfg, U, 99, by_value=True)
    status = want[3]
    assert status[0] == RS.S_NO_FOREGROUND and status[1] & RS.S_EMPTIED and status[2] & RS.S_RANGE and status[2] & RS.S_DEGENERATE
    assert status[4] == 0 and status[5] == 0 and status[6] == 0
    plans = want[4]
    assert plans[4]["rotated"] and plans[4]["resized"] and plans[4]["flip"] and plans[4]["maskmul"]
    assert plans[5]["rotated"] and not plans[5]["resized"] and not plans[5]["flip"] and not plans[5]["maskmul"]
    assert want[1][1].sum() == 0 and want[1][4].sum() > 0 and set(np.unique(want[1][5])) == {0, 3}
    # the image of the sample under use_mask_out is 0 outside its mask
    assert bool((got[0][4].cpu()[:, want[1][4] == 0] == 0).all())
    run(A, rgb, mask, hc, (32, 40), cfg, U, 99, out_dtype=torch.bfloat16, mask_dtype=torch.int64, by_value=True)
    # padding after a resize: ratios below 0.45 make the resized image smaller than the target
    small = dict(resize_hmin=5, resize_hmax=8, resize_wmin=5, resize_wmax=8)
    got, want = run(A, rgb[4:], mask[4:], hc[4:], (32, 40), small, U[4:], 5)
    assert want[4][0]["resized"] and want[4][0]["hoff"] > 0 and want[4][0]["woff"] > 0


def test_wrapped_rectangle_is_numpys_slice(golden):
    """the seventh sample of `extras`: the reference's img[y0:y1, x0:x1] = ... with x0 = -62 writes columns 2 .. 61"""
    rgb, mask, hc, cfg, U = extras(golden)
    _, m, _, status, plan = RS.augment_one(rgb[6], mask[6], hc[6], 48, 64, dict(cfg, rotation=False, crop=False, flip=False), U[6], 99)
    ref = mask[6].astype(np.int64)
    xlen, ylen = 63, 20
    x_side, y_side = int(xlen * RS.uniform(0.1, 2.0, U[6, 1]) / 2), int(ylen * RS.uniform(0.1, 2.0, U[6, 2]) / 2)
    x_loc, y_loc = RS.randint(0, 63, U[6, 3], [0]), RS.randint(10, 30, U[6, 4], [0])
    assert (x_side, x_loc) == (62, 0) and y_loc - y_side >= 0
    ref[y_loc - y_side:y_loc + y_side, x_loc - x_side:x_loc + x_side] = 0
    assert status == 0 and np.array_equal(m, ref) and 0 < ref.sum() < mask[6].sum()


def test_in_place_keypoints_and_misaligned_outputs(A, golden):
    """hcoords' written over hcoords; contiguous outputs at an address that is no multiple of 16 with a width that is a multiple of
    8 take the element path: the same values"""
    rgb, mask, hc, cfg, U = extras(golden)
    dev = torch.device("cuda:0")
    config = A.AugmentConfig(**cfg)
    args = (torch.from_numpy(rgb).to(dev), torch.from_numpy(mask).to(dev))
    packed = A.pack_uniforms(torch.from_numpy(U), config, dev)
    want = A.augment_batch(*args, torch.from_numpy(hc).to(dev), 32, 40, config, packed, 99)
    b = len(rgb)
    flat_i = torch.zeros(b * 3 * 32 * 40 + 4, dtype=torch.float32, device=dev)
    flat_m = torch.zeros(b * 32 * 40 + 16, dtype=torch.uint8, device=dev)
    image, m = flat_i[1:1 + b * 3 * 32 * 40].view(b, 3, 32, 40), flat_m[3:3 + b * 32 * 40].view(b, 32, 40)
    assert image.data_ptr() % 16 == 4 and m.data_ptr() % 16 == 3 and image.is_contiguous() and m.is_contiguous()
    keypoints = torch.from_numpy(hc).to(dev)
    got = A.augment_batch(*args, keypoints, 32, 40, config, packed, 99, out=(image, m, keypoints, torch.empty_like(want[3])))
    torch.cuda.synchronize()
    assert got[2].data_ptr() == keypoints.data_ptr()
    assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(got[1], want[1]) and torch.equal(bits(got[2]), bits(want[2]))
    assert torch.equal(got[3], want[3])
    assert float(flat_i[0]) == 0 and float(flat_i[-1]) == 0 and int(flat_m[:3].sum()) == 0 and int(flat_m[-13:].sum()) == 0   # nothing beyond
    # only the mask misaligned: still the element path for both
    image2 = torch.empty_like(want[0])
    got = A.augment_batch(*args, torch.from_numpy(hc).to(dev), 32, 40, config, packed, 99,
                          out=(image2, m, torch.empty_like(want[2]), torch.empty_like(want[3])))
    torch.cuda.synchronize()
    assert torch.equal(bits(image2), bits(want[0])) and torch.equal(m, want[1])


def test_full_size_index_range(A):
    """(480,640) -> (256,256) and -> (480,640) at b = 4: the sizes of a training batch, more than one block per row group; the last
    two samples have the angle at the two ends of its range (-30 and just below +30 degrees)"""
    rng = np.random.default_rng(11)
    H, W = 480, 640
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    mask = np.stack([((yy - 250) ** 2 + (xx - 300) ** 2 < 70 ** 2), ((yy - 400) ** 2 / 4 + (xx - 560) ** 2 < 50 ** 2)]).astype(np.uint8)
    hc = np.concatenate([rng.uniform(0.0, 640.0, (2, 9, 2)), np.ones((2, 9, 1))], 2)
    U = rng.uniform(0.05, 0.95, (2, 12))
    U[0, [0, 6, 10]] = 0.2, 0.3, 0.2
    U[1, [0, 6, 10]] = 0.7, 0.5, 0.9
    # drawn after everything above, so the first two samples stay what they were
    rgb = np.concatenate([rgb, rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)])
    mask = np.concatenate([mask, np.stack([((yy - 120) ** 2 + (xx - 480) ** 2 < 60 ** 2), ((yy - 330) ** 2 + (xx - 150) ** 2 / 4 < 45 ** 2)]).astype(np.uint8)])
    hc = np.concatenate([hc, np.concatenate([rng.uniform(0.0, 640.0, (2, 9, 2)), np.ones((2, 9, 1))], 2)])
    U = np.concatenate([U, rng.uniform(0.05, 0.95, (2, 12))])
    U[2, [0, 5, 6, 10]] = 0.8, 0.0, 0.4, 0.7
    U[3, [0, 5, 6, 10]] = 0.3, 1.0 - 2.0 ** -53, 0.2, 0.1
    assert RS.trig(U[2, 5], RS.DEFAULTS)[1] == -RS.trig(1.0, RS.DEFAULTS)[1] and abs(RS.trig(U[3, 5], RS.DEFAULTS)[1] - 0.5) < 1e-12
    for size in ((256, 256), (480, 640)):
        got, want = run(A, rgb, mask, hc, size, {}, U, 2024)
        assert want[3].tolist() == [0, 0, 0, 0] and all(p["resized"] and p["rotated"] for p in want[4]) and want[1].sum() > 0
        assert all(want[1][i].sum() > 0 for i in range(4))


def test_graph_capture_replays_and_two_calls_agree(A, golden):
    rgb, mask, hc, cfg, U = extras(golden)
    dev = torch.device("cuda:0")
    config = A.AugmentConfig(**cfg)
    args = (torch.from_numpy(rgb).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(hc).to(dev), 32, 40, config)
    packed = A.pack_uniforms(torch.from_numpy(U), config, dev)
    first = A.augment_batch(*args, packed, 99)
    second = A.augment_batch(*args, packed, 99)
    torch.cuda.synchronize()
    for a, b in zip(first[:3], second[:3]):
        assert torch.equal(bits(a) if a.is_floating_point() else a.cpu(), bits(b) if b.is_floating_point() else b.cpu())
    assert torch.equal(first[3], second[3])
    out = tuple(torch.empty_like(t) for t in first)
    ws = torch.empty(A.augment_workspace_bytes(len(rgb)), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        A.augment_batch(*args, packed, 99, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        A.augment_batch(*args, packed, 99, out=out, workspace=ws)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, out):
        assert torch.equal(bits(a) if a.is_floating_point() else a.cpu(), bits(b) if b.is_floating_point() else b.cpu())


def test_output_feeds_the_head_loss(A, golden):
    """augment_batch -> HeadLoss.from_keypoints, forward and backward, equals the same call on the restatement's output"""
    from pvnet_amd.validation import HeadLoss
    rgb, mask, hc, cfg, U = extras(golden)
    cfg = dict(cfg, use_mask_out=False)
    dev = torch.device("cuda:0")
    got, want = run(A, rgb, mask, hc, (32, 40), cfg, U, 99)
    b, vn = hc.shape[:2]
    gen = torch.Generator().manual_seed(3)
    seg0, vp0 = torch.randn((b, 2, 32, 40), generator=gen), torch.randn((b, 2 * vn, 32, 40), generator=gen)
    results = []
    for m, k in ((got[1], got[2]), (torch.from_numpy(want[1].astype(np.uint8)).to(dev), torch.from_numpy(want[2]).to(dev))):
        seg, vp = seg0.to(dev).requires_grad_(True), vp0.to(dev).requires_grad_(True)
        loss_seg, loss_vertex, precision, recall = HeadLoss().from_keypoints(seg, vp, m, k)
        (loss_seg.sum() + loss_vertex.sum()).backward()
        results.append((loss_seg.detach(), loss_vertex.detach(), precision, recall, seg.grad, vp.grad))
    torch.cuda.synchronize()
    for a, b_ in zip(*results):
        assert torch.equal(bits(a), bits(b_))
    assert float(results[0][1].sum()) > 0 and bool(torch.isfinite(results[0][5]).all())
