"""CPU tests of the step-level instruction trim: the merged scoring launch (score_exact_kernel_both_*, k4_score_cull.hip) keeps
nothing in scratch memory, and the inputs of tests/test_step_trim_gpu.py hold what that test claims to exercise (empty
compaction segments, an image below min_num, an image whose records never vote)."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _have_hipcc():
    from pvnet_amd import build as B
    try:
        return os.path.exists(B.hipcc_path())
    except RuntimeError:
        return bool(shutil.which("hipcc"))


@pytest.mark.skipif(not _have_hipcc(), reason="needs hipcc (the kernels are compiled to assembly)")
def test_merged_scoring_kernels_use_no_scratch(tmp_path):
    """every score_exact_kernel_both_* of the release and the development build: .amdhsa_private_segment_fixed_size 0, and the
    build-time checker refuses a merged kernel that spills again"""
    chk = _tool("check_kernel_resources")
    seen = {}
    for _, dev, text in chk.assembly():
        for name, nfv, vmax, scratch in chk.kernels(text):
            if "score_exact_kernel_both_" in name:
                seen[(name, dev)] = scratch
    assert len({n for n, _ in seen}) >= 2, "the release build holds the two untimed merged kernels at least"
    assert all(s == 0 for s in seen.values()), {k: s for k, s in seen.items() if s}
    for pat, want, max_scratch in chk.EXPECTED_ALLOC:
        if "both" in pat:
            assert max_scratch == 0
    body = ("_ZN3pvd12_GLOBAL__N_127score_exact_kernel_both_0_1ENS_10VoteParamsE:\n\tv_add_u32_e32 v127, v0, v1\n\ts_endpgm\n.Lfunc_end0:\n"
            "\t.amdhsa_kernel _ZN3pvd12_GLOBAL__N_127score_exact_kernel_both_0_1ENS_10VoteParamsE\n"
            "\t\t.amdhsa_private_segment_fixed_size %d\n\t\t.amdhsa_next_free_vgpr 136\n\t.end_amdhsa_kernel\n")
    spills, clean = tmp_path / "spills.s", tmp_path / "clean.s"
    spills.write_text(body % 4)
    clean.write_text(body % 0)
    assert chk.main([str(spills)]) == 1 and chk.main([str(clean)]) == 0


def test_mixed_batch_holds_what_the_gpu_test_exercises():
    """the batch of tests/test_step_trim_gpu.py, looked at without a GPU: compaction segments without a foreground pixel next to
    segments with some, one image below min_num, one image whose directions are all zero (its records never vote and flag no cell),
    noisy images that fill several 256-pixel work items each"""
    from tests.test_step_trim_gpu import MIN_NUM, SEG_PIXELS, SHAPE, mixed_batch, ROLE
    b, h, w, vn, hn = SHAPE
    mask, planar = mixed_batch()
    assert mask.shape == (b, h, w) and planar.shape == (b, 2 * vn, h, w)
    fg = mask.reshape(b, -1) != 0
    tn0 = fg.sum(1)
    nseg = -(-h * w // SEG_PIXELS)
    pad = np.zeros((b, nseg * SEG_PIXELS), bool)
    pad[:, :h * w] = fg
    per_seg = pad.reshape(b, nseg, SEG_PIXELS).sum(2)
    for bi in range(b):
        assert (per_seg[bi] == 0).any(), "an empty segment in every image"
        if ROLE[bi] != "empty":
            assert (per_seg[bi] > 0).any()
    small = [bi for bi in range(b) if ROLE[bi] == "small"]
    assert small and all(0 < tn0[bi] < MIN_NUM for bi in small)
    empty = [bi for bi in range(b) if ROLE[bi] == "empty"]
    assert empty and all(tn0[bi] == 0 for bi in empty)
    zero = [bi for bi in range(b) if ROLE[bi] == "zero_field"]
    assert zero and all(tn0[bi] >= 2 * 256 and not planar[bi][:, mask[bi] != 0].any() for bi in zero)
    noisy = [bi for bi in range(b) if ROLE[bi] == "noisy"]
    assert len(noisy) >= 2 and all(tn0[bi] >= 4 * 256 for bi in noisy)
    assert all(np.abs(planar[bi][:, mask[bi] != 0]).max() > 0.5 for bi in noisy)
