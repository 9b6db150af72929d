"""GPU test of the step-level instruction trim (the scoring bodies' per-item work outside the vote loop, the merged launch without
scratch, K3's key-point blocks behind the batch gate): exact-mode counts torch.equal to literal mode on ONE launch that mixes work
items with flagged cells, work items without any, an image below min_num and an image without foreground -- under the library's
own culling selection and with every key-point culled, for a batch alone (strided items) and for the variant concurrent calls run
(contiguous runs).  tests/test_step_trim_cpu.py looks at the same inputs without a GPU."""
import numpy as np
import pytest
import torch

from pvnet_amd import synth, voting

SHAPE = (8, 240, 320, 9, 1024)          # (b, h, w, vn, hn): a layout with culling buffers (tests/test_library_cpu.py pins it)
MIN_NUM = 20
SEG_PIXELS = 4096                       # pixels per compaction block (K2_WORDS_PER_BLOCK words of 64)
ROLE = ("noisy", "zero_field", "small", "noisy", "empty", "clean", "noisy", "zero_field")


def mixed_batch():
    b, h, w, vn, _ = SHAPE
    mask, planar, _ = synth.make_batch(b, first_index=900, h=h, w=w, vn=vn, radius=30, noise=True, background="normal")
    cmask, cplanar, _ = synth.make_batch(b, first_index=900, h=h, w=w, vn=vn, radius=30, noise=False, background="normal")
    for bi, role in enumerate(ROLE):
        if role == "clean":
            mask[bi], planar[bi] = cmask[bi], cplanar[bi]
        elif role == "zero_field":   # |u| = 0 < 1e-6 on the object: dead rows in exact mode (x = -4: no vote, no flagged cell)
            planar[bi][:, mask[bi] != 0] = 0.0
        elif role == "small":        # fewer than min_num foreground pixels: no work item, zero key-points
            ys, xs = np.nonzero(mask[bi])
            keep = np.zeros_like(mask[bi])
            keep[ys[:MIN_NUM - 7], xs[:MIN_NUM - 7]] = 1
            mask[bi] = keep
        elif role == "empty":
            mask[bi] = 0
    return mask, planar


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _vote(m, v, literal=False, idx=None, **kw):
    hn = SHAPE[4]
    if idx is not None:
        m, v = m[idx], v[idx]
    shape = (m.shape[0],) + SHAPE[1:]
    ws = torch.zeros(voting.vote_layout(*shape, 30000).total_bytes, dtype=torch.uint8, device=_dev())
    out, d = voting.ransac_voting_layer_v3(m, v, hn, inlier_thresh=0.99, min_num=MIN_NUM, seed=77, literal=literal,
                                           return_debug=True, workspace=ws, **kw)
    torch.cuda.synchronize()
    return out.clone(), d["counts"].clone(), d["win"].clone(), d


@pytest.mark.gpu
@pytest.mark.parametrize("selection", [None, "all"])
@pytest.mark.parametrize("concurrent", [False, True])
def test_mixed_launch_counts_equal_literal_mode(selection, concurrent):
    mask, planar = mixed_batch()
    m = torch.from_numpy(mask).to(_dev())
    v = synth.planar_to_vertex_view(torch.from_numpy(planar).to(_dev()))
    voting.set_cull_selection(None)
    lit = _vote(m, v, literal=True)
    try:
        voting.set_cull_selection(selection)
        ex = _vote(m, v, band_stats=True, concurrent=concurrent)
        d = ex[3]
        assert d["mode"] == "exact"
        if selection == "all":
            live = [bi for bi, r in enumerate(ROLE) if r not in ("small", "empty")]
            assert bool(d["cull_bits"][live].all()), "every live key-point goes through the culling body"
        print("band_stats (cells re-evaluated, literal tests):", d["band_stats"], "selection", selection, "concurrent", concurrent)
        assert d["band_stats"][0] > 0, "the launch holds flagged cells"
        # the zero-field images alone: work items, and not one flagged cell -- the mixed launch above holds both kinds
        zf = [bi for bi, r in enumerate(ROLE) if r == "zero_field"]
        z = _vote(m, v, idx=zf, band_stats=True, concurrent=concurrent)
        assert int(z[3]["total_items"]) > 0 and z[3]["band_stats"][0] == 0
        assert int(z[1].abs().sum()) == 0
    finally:
        voting.set_cull_selection(None)
    bad = ex[1] != lit[1]
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} counts differ, max |diff| {int((ex[1] - lit[1]).abs().max())}"
    assert torch.equal(ex[2], lit[2])
    assert float((ex[0] - lit[0]).abs().max()) < 1e-3
    for bi, r in enumerate(ROLE):
        if r in ("small", "empty"):
            assert int(ex[1][bi].abs().sum()) == 0 and float(ex[0][bi].abs().max()) == 0.0
