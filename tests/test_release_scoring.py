"""GPU tests of the RELEASE library's culling-capable path: the merged scoring launch (score_exact_kernel_both_*, k4_score_cull.hip)
that scores every call of a layout with culling buffers -- hn_pad 1 024 (hn 768 .. 1 024), 256-pixel items (b * vn >= 64 at hn
1 024), vn <= 32 -- first its dense items (score_exact_body, k4_exact_body.h), then its disc-culled ones.

Every test here runs knob-free (a PVNET_* knob in the environment would load the development build), on explicitly zeroed
workspaces (the batch gate CF_BATCH_OK otherwise follows whatever a previous call left in recycled memory), and asserts the layout
and the culling marks it claims to have run.  The claim: hypotheses, inlier counts and winners torch.equal to literal mode (the
reference's own arithmetic), key-points within 1e-3 px."""
import os

import numpy as np
import pytest
import torch

from oracle import refkernels
from pvnet_amd import synth, voting

pytestmark = pytest.mark.gpu

# (b, h, w, vn, hn) of the calls below that must get a culling layout from the release library -- tests/test_library_cpu.py pins
# pvnet_vote_layout on them, so a layout change that would turn these tests into plain dense calls fails without a GPU
HEAVY_SHAPE = (8, 240, 320, 9, 1024)
MANY_KP_SHAPES = {32: (2, 240, 320, 32, 1024), 33: (2, 240, 320, 33, 1024), 40: (2, 240, 320, 40, 1024)}
CULLING_SHAPES = (HEAVY_SHAPE, MANY_KP_SHAPES[32])
# the dense body's flagged-cell slots per 256-pixel item (4 waves x 8 hypothesis tiles x 64 lanes) and the first slot that lay
# beyond the merged launch's LDS request before it covered the dense body (36 096 B of 36 864)
CELL_SLOTS, FIRST_SLOT_PAST_OLD_REQUEST = 2048, 1856
RELEASE_BLOCKS, RELEASE_BLOCK = 4, 12   # fuzz cases 30000 .. 30047 (tests/fuzz_cases.py: release_case_params)


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


def zeroed(shape):
    return torch.zeros(voting.vote_layout(*shape, 30000).total_bytes, dtype=torch.uint8, device=dev())


def to_dev(mask, planar):
    return torch.from_numpy(mask).to(dev()), synth.planar_to_vertex_view(torch.from_numpy(planar).to(dev()))


def vote(m, v, hn, shape, literal=False, **kw):
    """one call on a fresh zeroed workspace -> (key-points, counts, winners, hypotheses as bytes, debug dict)"""
    out, d = voting.ransac_voting_layer_v3(m, v, hn, inlier_thresh=0.99, seed=21, literal=literal, return_debug=True,
                                           workspace=zeroed(shape), **kw)
    assert d["mode"] == ("literal" if literal else "exact")
    return out.clone(), d["counts"].clone(), d["win"].clone(), d["hyp"].cpu().numpy().tobytes(), d


def assert_equal_to_literal(ex, lit):
    assert ex[3] == lit[3]                                      # hypotheses: the same draws, the same bytes
    bad = ex[1] != lit[1]
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} counts differ, max |diff| {int((ex[1] - lit[1]).abs().max())}"
    assert torch.equal(ex[2], lit[2])
    assert float((ex[0] - lit[0]).abs().max()) < 1e-3


def assert_counts_equal_the_references_kernel(d, b):
    """the reference's voting_for_hypothesis_kernel itself (oracle/_ref) on the call's compacted records and hypotheses"""
    if not refkernels.available("off"):
        return
    for bi in range(b):
        tn = int(d["tn"][bi])
        rec = d["rec"][bi, :, :tn]
        inl = refkernels.voting_for_hypothesis(rec[:, :, 2:4].permute(1, 0, 2).contiguous(), rec[0, :, 0:2].contiguous(),
                                               d["hyp"][bi].permute(1, 0, 2).contiguous(), 0.99)
        assert torch.equal(d["counts"][bi].T, inl.sum(2, dtype=torch.int32))


def heavy_images(first, n):
    """noisy images (10 % outliers: K3 does not select them for culling) whose directions are scaled to |u| >= 2^61: every record
    is a zero row of the exact kernel (the reference's float32 squares may overflow beyond it), x = 0 against every hypothesis -- each
    (hypothesis, half-wave) cell with a live pixel is flagged and decided by the reference's arithmetic"""
    b, h, w, vn, _ = HEAVY_SHAPE
    mask, planar, _ = synth.make_batch(n, first_index=first, h=h, w=w, vn=vn, radius=30, noise=True, background="normal")
    return mask, (planar * np.float32(2.0 ** 62)).astype(np.float32)


def test_nearly_fully_flagged_dense_items_inside_the_merged_launch():
    """dense items of the merged launch (default selection, nothing culled) whose every cell slot is taken: the flagged cells beyond
    slot 1 856 -- past the launch's old LDS request -- must be counted like the others"""
    b, h, w, vn, hn = HEAVY_SHAPE
    m, v = to_dev(*heavy_images(500, b))
    lit = vote(m, v, hn, HEAVY_SHAPE, literal=True)
    ex = vote(m, v, hn, HEAVY_SHAPE, band_stats=True)
    d = ex[4]
    assert d["layout"].cull == 1 and not bool(d["cull_bits"].any())   # the merged launch (P.cull = 2), dense items only
    tn = d["tn"][:b].cpu().numpy()
    items = vn * int(sum(-(-int(t) // 256) for t in tn))
    assert int(d["total_items"]) == items
    cells = d["band_stats"][0]
    print(f"flagged cells per dense item: {cells / items:.1f} of {CELL_SLOTS} slots")
    assert cells > FIRST_SLOT_PAST_OLD_REQUEST * items, f"{cells / items:.1f} flagged cells per item"
    assert cells <= CELL_SLOTS * items
    assert float((d["win"][:, :, 1] > 0).float().mean()) > 0.5      # the flagged cells decide real inliers
    assert_equal_to_literal(ex, lit)
    assert_counts_equal_the_references_kernel(d, b)


def test_culled_and_fully_flagged_dense_images_in_one_launch():
    """even images clean (K3 culls them: the culling body), odd images the fully flagged field above (the dense body): both bodies in
    one merged launch, the dense one with every cell slot taken"""
    b, h, w, vn, hn = HEAVY_SHAPE
    mask, planar = heavy_images(600, b)
    mc, pc, _ = synth.make_batch(b, first_index=600, h=h, w=w, vn=vn, radius=30, noise=False, background="zeros")
    mask[0::2], planar[0::2] = mc[0::2], pc[0::2]
    m, v = to_dev(mask, planar)
    lit = vote(m, v, hn, HEAVY_SHAPE, literal=True)
    ex = vote(m, v, hn, HEAVY_SHAPE, band_stats=True)
    d = ex[4]
    bits = d["cull_bits"]
    assert d["layout"].cull == 1 and bool(bits[0::2].all()) and not bool(bits[1::2].any())
    steps, full = d["cull_stats"]
    assert 0 < steps < full                                           # the culling body ran, and skipped work
    dense_items = vn * int(sum(-(-int(t) // 256) for t in d["tn"][1:b:2].cpu().numpy()))
    # (band_stats counts the culling body's flagged cells too: this bounds the dense items' share from above only)
    print(f"flagged cells per dense item at most: {d['band_stats'][0] / dense_items:.1f} of {CELL_SLOTS} slots")
    assert d["band_stats"][0] > FIRST_SLOT_PAST_OLD_REQUEST * dense_items
    assert_equal_to_literal(ex, lit)
    assert_counts_equal_the_references_kernel(d, b)


@pytest.mark.parametrize("vn", sorted(MANY_KP_SHAPES))
def test_many_key_points_at_a_culling_layout(vn):
    """32 key-points (all 256 preamble threads of K3's cull_block, marks for 32 key-points, a cull_block grid of vn blocks) and 33 / 40
    (beyond the per-key-point origin: a dense layout) with 256-pixel items at hn 1 024 -- tests/test_exact_mode.py: test_many_key_points
    runs the same key-point counts at a small dense layout"""
    shape = MANY_KP_SHAPES[vn]
    b, h, w, _, hn = shape
    fields = {"clean": synth.make_batch(b, first_index=930, h=h, w=w, vn=vn, radius=30, noise=False, background="zeros")[:2],
              "noisy": synth.make_batch(b, first_index=930, h=h, w=w, vn=vn, radius=30, noise=True, background="normal")[:2]}
    for name, field in fields.items():
        m, v = to_dev(*field)
        lit = vote(m, v, hn, shape, literal=True)
        for sel in ("all", None):
            voting.set_cull_selection(sel)
            try:
                ex = vote(m, v, hn, shape)
            finally:
                voting.set_cull_selection(None)
            d = ex[4]
            bits = d["cull_bits"]
            if vn <= 32:
                assert d["layout"].cull == 1
                if sel == "all" or name == "clean":
                    assert bool(bits.all()), (name, sel)
            else:
                assert d["layout"].cull == 0 and not bool(bits.any())
            assert_equal_to_literal(ex, lit)


@pytest.mark.parametrize("block", range(RELEASE_BLOCKS))
def test_release_fuzz_block(block):
    """knob-free random cases (tests/fuzz_cases.py: run_release_case): the field kind drawn per image, the selection, the workspace's
    history; each block must have reached the merged launch with a mixed batch, a fully culled call and a dense layout"""
    from tests import fuzz_cases as F
    bad, mixed, culled, dense = [], 0, 0, 0
    for case in range(F.RELEASE_FIRST + block * RELEASE_BLOCK, F.RELEASE_FIRST + (block + 1) * RELEASE_BLOCK):
        r = F.run_release_case(case)
        if not r["ok"]:
            bad.append(r)
        if r["cull_layout"]:
            mixed += 0 < r["culled"] < r["keypoints"]
            culled += r["culled"] == r["keypoints"]
        else:
            dense += 1
    assert not bad, bad
    assert mixed >= 1 and culled >= 1 and dense >= 1, (mixed, culled, dense)
