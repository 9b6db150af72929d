"""GPU tests of the voting step's trimmed mask kernels and dense-scoring item prologue.

K1 (k1_mask.hip): a full 4096-pixel segment is loaded from one scalar address per wave without a bound test, only an image's last
segment keeps the test per lane; the foreground test reads the low byte and feeds the ballot directly; the thinning histogram takes
its predicates back from the ballot words.  Through the public entry: `tn` and the kept-pixel list (`rec[..., 0:2]`) against the
oracle's foreground() and compact(), for shapes of one double word, exactly one segment, a full plus a partial segment and three
full segments; for patterns that exercise the low byte (256, -1, 1 << 40); for views that reach the pair kernel, the generic
kernel's linear path and its strided path; for every mask type; and one thinned case whose kept list follows the oracle's counter
RNG and whose winners equal the C oracle's.

K4 (k4_exact_body.h): an item's first vote step opens its cell directly.  Exact-mode counts and winners torch.equal to literal
mode at hn = 1024 for items of 1, 2, 7 and 8 pixel tiles, one and several items per key-point; for a near-parallel field at thresh
0.999 whose items are ONE tile, so every flagged cell is a cell of an item's first tile; and for directions 0, 1e-7, 2^62, NaN and
Inf in the first and last row of a tile of an item's first tile, of a later tile and of a second item's first tile."""
import numpy as np
import pytest
import torch

from oracle import cref
from oracle import ransac_voting_oracle as O
from pvnet_amd import synth, voting

pytestmark = pytest.mark.gpu

SEG = 4096   # pixels per K1 workgroup


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def default_selection():
    yield
    voting.set_cull_selection(None)


def random_field(b, h, w, vn, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((b, h, w, vn, 2)).astype(np.float32)).to(dev())


def vote(m, v, hn, **kw):
    b, h, w, vn = v.shape[:4]
    ws = torch.zeros(voting.vote_layout(b, h, w, vn, hn, kw.get("max_num", 30000)).total_bytes, dtype=torch.uint8, device=dev())
    kw.setdefault("inlier_thresh", 0.99)
    kw.setdefault("seed", 11)
    return voting.ransac_voting_layer_v3(m, v, hn, return_debug=True, workspace=ws, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# K1
# ---------------------------------------------------------------------------------------------------------------------------------
def check_kept_list(m, mask_np, keep=None, **kw):
    """tn and the kept pixels of every image against the oracle's foreground() and compact() (keep: the oracle's thinning flags)"""
    b, h, w = mask_np.shape
    v = random_field(b, h, w, 2, 3)
    _, dbg = vote(m, v, 16, min_num=1, **kw)
    tn, tn0 = dbg["tn"].cpu().numpy(), dbg["tn0"].cpu().numpy()
    rec = dbg["rec"].cpu().numpy()
    for bi in range(b):
        fg = O.foreground(mask_np[bi])
        assert int(tn0[bi]) == int(fg.sum()), f"image {bi}: tn0 {int(tn0[bi])} != {int(fg.sum())} foreground pixels"
        if keep is not None:
            fg = fg & keep[bi].reshape(h, w)
        coords, _ = O.compact(fg, np.zeros((h, w, 1, 2), np.float32))
        assert int(tn[bi]) == len(coords), f"image {bi}: tn {int(tn[bi])} != {len(coords)} kept pixels"
        for k in range(rec.shape[1]):
            got = rec[bi, k, :len(coords), 0:2]
            assert np.array_equal(got, coords), f"image {bi}, key-point {k}: kept list differs from the oracle's at rank " \
                                                f"{int(np.flatnonzero((got != coords).any(1))[0])}"
    return dbg


SHAPES = [(2, 64), (64, 64), (65, 64), (64, 66), (96, 128)]
SHAPE_IDS = ["one_double_word", "one_segment", "segment_plus_a_row", "segment_plus_128", "three_segments"]


def pattern(name, h, w, rng):
    m = np.zeros(h * w, np.int64)
    if name == "full":
        m[:] = 1
    elif name == "pixel0":
        m[0] = 1
    elif name == "last":
        m[-1] = 1
    elif name == "checker_even":
        m[0::2] = 1
    elif name == "checker_odd":
        m[1::2] = 1
    elif name == "low_byte":   # 256 and 1 << 40 have a zero low byte: background; -1 and 257 are foreground
        m[:] = rng.choice(np.array([0, 1, 256, -1, 1 << 40, 257, (1 << 40) + 3, -256], np.int64), h * w)
    elif name == "only_256":
        m[:] = 256
    elif name == "only_minus_1":
        m[:] = -1
    elif name == "only_2_40":
        m[:] = 1 << 40
    else:
        assert name == "empty"
    return m.reshape(h, w)


PATTERN_GROUPS = [("empty", "full", "pixel0"), ("last", "checker_even", "checker_odd"), ("only_256", "only_minus_1", "low_byte"),
                  ("only_2_40", "low_byte", "full")]


@pytest.mark.parametrize("names", PATTERN_GROUPS, ids=["+".join(g) for g in PATTERN_GROUPS])
@pytest.mark.parametrize("h,w", SHAPES, ids=SHAPE_IDS)
def test_mask_bits_of_contiguous_int64_masks(h, w, names):
    rng = np.random.default_rng(h * 1000 + w)
    mask = np.stack([pattern(n, h, w, rng) for n in names])
    m = torch.from_numpy(mask).to(dev())
    assert m.is_contiguous() and m.data_ptr() % 16 == 0 and m.dtype == torch.int64   # the pair kernel
    check_kept_list(m, mask)


@pytest.mark.parametrize("h,w", SHAPES, ids=SHAPE_IDS)
def test_mask_views(h, w):
    rng = np.random.default_rng(h + w)
    mask = np.stack([pattern(n, h, w, rng) for n in ("low_byte", "checker_odd", "low_byte")])
    # one image in: still contiguous and 16-byte aligned (the pair kernel at another base)
    big = torch.zeros((4, h, w), dtype=torch.int64, device=dev())
    big[1:] = torch.from_numpy(mask).to(dev())
    big[0] = 1
    view = big[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    check_kept_list(view, mask)
    # one ELEMENT in: contiguous at an address that is 8 mod 16 (the generic kernel, its linear path)
    flat = torch.ones(3 * h * w + 1, dtype=torch.int64, device=dev())
    flat[1:] = torch.from_numpy(mask).to(dev()).reshape(-1)
    odd = flat[1:].view(3, h, w)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    check_kept_list(odd, mask)
    # a column window (the generic kernel, strided)
    wide = torch.ones((3, h, w + 1), dtype=torch.int64, device=dev())
    wide[:, :, 1:] = torch.from_numpy(mask).to(dev())
    win = wide[:, :, 1:]
    assert not win.is_contiguous()
    check_kept_list(win, mask)


@pytest.mark.parametrize("mdt", [np.uint8, np.int16, np.int32, np.float32], ids=["uint8", "int16", "int32", "float32"])
def test_mask_types(mdt):
    h, w = 65, 64
    rng = np.random.default_rng(5)
    if mdt == np.float32:   # .byte() of a float truncates, then wraps: 0.5 -> 0, 256.0 -> 0, -1.0 -> 255, 257.5 -> 1
        vals = np.array([0.0, 0.5, 1.0, 256.0, -1.0, 257.5, -0.25, 511.75], np.float32)
    elif mdt == np.uint8:
        vals = np.array([0, 1, 255, 128, 0, 0], np.uint8)
    else:
        vals = np.array([0, 1, 256, -1, 257, -256, 512, 3], mdt)
    mask = np.stack([rng.choice(vals, (h, w)), np.full((h, w), vals[2], mdt), rng.choice(vals[:2], (h, w))])
    assert mask.dtype == mdt
    check_kept_list(torch.from_numpy(mask).to(dev()), mask)


def test_thinning_follows_the_oracle():
    """about 2 000 foreground pixels, max_num = 100: the histograms of the mask kernel decide which pixels stay"""
    b, h, w, vn, hn, seed, max_num = 3, 96, 128, 9, 64, 13, 100
    mask, planar, _ = synth.make_batch(b, first_index=40, h=h, w=w, vn=vn, radius=25, noise=True, background="normal")
    mask = mask.astype(np.int64)
    tn0 = [int(O.foreground(mask[bi]).sum()) for bi in range(b)]
    assert all(1800 < t < 2200 for t in tn0), tn0
    keep = np.stack([O.subsample_keep(seed, bi, h * w, max_num, tn0[bi]) for bi in range(b)])
    m = torch.from_numpy(mask).to(dev())
    dbg = check_kept_list(m, mask, keep=keep, max_num=max_num, seed=seed)
    assert all(0 < int(t) < 200 for t in dbg["tn"].tolist())
    # the C oracle thins by itself: its winners' inlier counts are counts over ITS kept list
    pt = torch.from_numpy(planar).to(dev())
    vnp = synth.planar_to_vertex_view(planar)
    _, wi, wc = cref.vote_v3(O.foreground(mask), vnp, hn, 0.99, max_num=max_num, seed=seed, return_winners=True)
    _, d2 = vote(m, synth.planar_to_vertex_view(pt), hn, max_num=max_num, seed=seed)
    np.testing.assert_array_equal(d2["win"][:, :, 0].cpu().numpy(), wi)
    np.testing.assert_array_equal(d2["win"][:, :, 1].cpu().numpy(), wc)


# ---------------------------------------------------------------------------------------------------------------------------------
# K4
# ---------------------------------------------------------------------------------------------------------------------------------
HN = 1024
H, W, VN = 48, 64, 9


def mask_with(counts):
    """[b, H, W] int64: image i holds counts[i] foreground pixels, a solid run in raster order from row 8 on"""
    mask = np.zeros((len(counts), H * W), np.int64)
    for i, n in enumerate(counts):
        mask[i, 8 * W + 5:8 * W + 5 + n] = 1
    return mask.reshape(len(counts), H, W)


def towards_points(mask, seed, spread=0.03):
    """float32 [b, H, W, VN, 2]: unit directions towards VN points per image, turned by normal(0, spread) radians"""
    rng = np.random.default_rng(seed)
    b = mask.shape[0]
    ys, xs = np.mgrid[0:H, 0:W]
    f = np.zeros((b, H, W, VN, 2), np.float32)
    for bi in range(b):
        for k in range(VN):
            px, py = rng.uniform(0, W), rng.uniform(0, H)
            ang = np.arctan2(py - ys, px - xs) + rng.normal(0, spread, (H, W))
            f[bi, :, :, k, 0], f[bi, :, :, k, 1] = np.cos(ang), np.sin(ang)
    return f


def item_tiles(tn, npx):
    """pixel tiles of the work items of one key-point (score_exact_body: the record count padded to 8, groups of npx pixels)"""
    tpad = (tn + 7) // 8 * 8
    return [min(npx // 32, (tpad - g * npx + 31) >> 5) for g in range((tn + npx - 1) // npx)]


def exact_equals_literal(mask, field, thresh, concurrent, expect_flagged=None):
    m, v = torch.from_numpy(mask).to(dev()), torch.from_numpy(field).to(dev())
    _, lit = vote(m, v, HN, inlier_thresh=thresh, literal=True)
    lit_counts, lit_win = lit["counts"].clone(), lit["win"].clone()
    tiles = {}
    for sel in ("none", None):   # the dense body scores every key-point; then whatever the library selects
        voting.set_cull_selection(sel)
        _, dbg = vote(m, v, HN, inlier_thresh=thresh, concurrent=concurrent, band_stats=True)
        voting.set_cull_selection(None)
        L = dbg["layout"]
        assert dbg["mode"] == "exact" and dbg["concurrent"] == concurrent
        npx = L.wg_s * L.chunk
        tiles = {int(t): item_tiles(int(t), npx) for t in dbg["tn"].tolist()}
        bad = dbg["counts"] != lit_counts
        assert not bool(bad.any()), f"selection {sel}: {int(bad.sum())} of {bad.numel()} counts differ from literal mode"
        assert torch.equal(dbg["win"], lit_win), f"selection {sel}: winners differ from literal mode"
        if expect_flagged is not None and sel == "none":
            print("band_stats (cells re-evaluated, literal tests):", dbg["band_stats"])
            assert (dbg["band_stats"][0] > 0) == expect_flagged
    return tiles


def items_of_256_pixels(b):
    """b * VN * 2 hypothesis groups >= 128 give the layout 128-pixel chunks: work items of 256 pixels, eight tiles -- the benchmark's"""
    L = voting.vote_layout(b, H, W, VN, HN, 30000)
    assert L.wg_s * L.chunk == 256, (L.wg_s, L.chunk)


@pytest.mark.parametrize("concurrent", [False, True], ids=["alone", "concurrent"])
def test_items_of_1_2_7_and_8_tiles(concurrent):
    """pixel tiles per item = ceil(records in the item's pixel group / 32): 20, 50, 200 and 256 foreground pixels are ONE item per
    key-point and hypothesis slice with 1, 2, 7 and 8 tiles; 276, 512, 562 and 712 are several items per key-point (8 + 1, 8 + 8,
    8 + 8 + 2, 8 + 8 + 7)"""
    counts = [20, 50, 200, 256, 276, 512, 562, 712]
    items_of_256_pixels(len(counts))
    mask = mask_with(counts)
    tiles = exact_equals_literal(mask, towards_points(mask, 1), 0.99, concurrent)
    assert tiles == {20: [1], 50: [2], 200: [7], 256: [8], 276: [8, 1], 512: [8, 8], 562: [8, 8, 2], 712: [8, 8, 7]}, tiles


@pytest.mark.parametrize("counts", [[20, 32] * 4, [300] * 8], ids=["items_of_one_tile", "two_items"])
@pytest.mark.parametrize("concurrent", [False, True], ids=["alone", "concurrent"])
def test_flagged_cells_of_an_items_first_tile(concurrent, counts):
    """a near-parallel field (directions within a few degrees of +x) at thresh 0.999 (2.56 degrees): the hypotheses lie far away
    along x, every pixel sees them under nearly the same angle, and that angle is of the order of the threshold -- tests inside the
    rounding band.  Images of 20 and 32 pixels are items of ONE tile: every flagged cell is a cell of an item's first tile; 300 pixels:
    a first tile followed by seven others, and a second item."""
    items_of_256_pixels(len(counts))
    mask = mask_with(counts)
    rng = np.random.default_rng(8)
    field = np.zeros((len(counts), H, W, VN, 2), np.float32)
    field[..., 0] = 1.0
    field[..., 1] = rng.normal(0, 0.04, field.shape[:-1]).astype(np.float32)
    tiles = exact_equals_literal(mask, field, 0.999, concurrent, expect_flagged=True)
    assert tiles == ({20: [1], 32: [1]} if counts[0] == 20 else {300: [8, 2]}), tiles


HOSTILE = [(0.0, 0.0), (1e-7, -1e-7), (2.0 ** 62, 1.0), (np.nan, 0.5), (np.inf, -np.inf)]
# ranks in the kept list (300 pixels: an item of 8 tiles, an item of 2): first and last row of the first item's first tile, of its
# second tile, of its last tile, and of the second item's first tile
RANKS = [0, 31, 32, 63, 224, 255, 256, 287]


@pytest.mark.parametrize("concurrent", [False, True], ids=["alone", "concurrent"])
def test_hostile_directions_in_first_and_last_rows(concurrent):
    """image i puts hostile value (i + j) % 5 at rank RANKS[j], for every key-point: every value meets every row position"""
    b, n = 8, len(HOSTILE)
    items_of_256_pixels(b)
    mask = mask_with([300] * b)
    field = towards_points(mask, 2)
    flat = field.reshape(b, H * W, VN, 2)
    for i in range(b):
        ranks = np.flatnonzero(mask[i].reshape(-1))
        for j, r in enumerate(RANKS):
            flat[i, ranks[r]] = np.array(HOSTILE[(i + j) % n], np.float32)
    tiles = exact_equals_literal(mask, field, 0.99, concurrent)
    assert tiles == {300: [8, 2]}, tiles
