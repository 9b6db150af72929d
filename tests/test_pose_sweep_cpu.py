"""The bars of the pose-solve sweep (tests/pose_cases.py: BAR_POSE, BAR_COST), justified on the host library alone -- no GPU.

The device solve is tested against the host library (tests/test_pose_sweep_device.py).  Both run the same algorithm in the same
operation order; the device's sin / cos / atan2 may differ from the host's in the last place.  The LM's stopping rules (relative
decrease < 1e-16, step < 1e-15 |x|) are decided by last-place rounding, so two correct solvers do not end on the same bits.
This module measures that spread on the oracle itself -- the host solver against the host solver on inputs moved by one unit in
the last place -- and asserts that the bars stand well above it (20x for the pose, 50x for the cost: the device differs from the
host in three transcendental functions per evaluation, not in one rounding of the input) and well below what a defect does.

Measured with this module (``pytest -s`` prints every figure), pn in SWEEP_PN, 32 images each, 0.4 px noise:

  self-spread, largest over pn          [R|t] entry   relative cost excess   LM iterations apart
    unweighted                            4.4e-9          2.0e-13               5
    explicit weights                      4.4e-9          1.8e-13               6
    covariances (pn = 9: asserted)        2.4e-9          1.1e-13               5
    covariances (all pn: printed)         3.3e-9          2.3e-13 (pn = 6)      6
  so BAR_POSE = 1e-7 stands 22x above the pose spread and BAR_COST = 1e-11 50x above the cost spread (44x above the covariance
  path's at pn = 6, which is why that path is asserted at one count only).  No image needs more than 23 iterations.
  Evaluator.evaluate_uncertainty against pvnet_pnp_solve with the same weights: at most 3.7e-9 (pn = 10).

  a defect, smallest pose movement over all images and pn   unweighted   explicit weights
    last key-point never read (pn >= 7)                       3.2e-5       1.4e-5     (medians 1.4e-4 .. 4.6e-3)
    last image point = key-point 0's                          3.0e-3       1.2e-3
  so 100 * BAR_POSE = 1e-5 is below every one of them.

  3 px noise, pn = 7, 8, 10, 64 images each, unweighted: one image per pn runs to the 200-iteration limit; there the host differs
  from itself by up to 7.1e-3 (pose) and 1.3e-5 (cost).  The other images need at most 32 iterations and spread by 6.9e-9,
  1.1e-8, 1.2e-8 (iterations up to 6 apart): 3 * BAR_POSE is 26x above.

The iteration counts are printed and not asserted: up to 6 apart host against host, which is why the device sweep puts no slack
on ``status`` beyond the limits.
"""
import functools

import numpy as np
import pytest

from pvnet_amd import pnp as P
from tests import pose_cases as PC

K = P.LINEMOD_K
FORMS = ("unweighted", "weighted", "covariance")
# the covariance path's self-spread is asserted once, at the key-point count the project's Evaluator runs with (8 surface points
# and the centre); the other counts are well-posedness checks that print their figures
COVARIANCE_PN = 9


def solve(form, X, x2, W):
    """the oracle of one form, as the device test uses it: (poses, status, rt)"""
    if form == "covariance":   # W = the covariances; Evaluator.evaluate_uncertainty is the oracle, status from the same weights
        poses = PC.evaluator_solve(X, x2, W, K)
        return poses, PC.host_solve(X, x2, K, PC.covariance_weights(W))[1], PC.poses_to_rt(poses)
    return PC.host_solve(X, x2, K, W if form == "weighted" else None)


def weights_of(form, W, cov):
    return {"unweighted": None, "weighted": W, "covariance": cov}[form]


def last_place(x2, seed):
    """every image coordinate multiplied by 1 +- 2^-52"""
    sign = np.random.default_rng(seed).choice([-1.0, 1.0], size=x2.shape)
    return x2 * (1.0 + sign * 2.0 ** -52)


@functools.lru_cache(maxsize=None)
def base(pn, form):
    X, x2, W, cov = PC.sweep_case(pn)
    Wf = weights_of(form, W, cov)
    poses, status, rt = solve(form, X, x2, Wf)
    Wc = PC.covariance_weights(cov) if form == "covariance" else Wf
    return X, x2, Wf, Wc, poses, status, rt, PC.host_cost(X, x2, Wc, K, rt)


def spread(form, X, x2, Wf, Wc, poses, status, cost, keep=None):
    """host against host on inputs one unit in the last place away: (largest [R|t] difference, largest relative cost excess,
    largest iteration difference) over three sign patterns"""
    keep = np.ones(len(x2), bool) if keep is None else keep
    s_pose = s_cost = 0.0
    s_iter = 0
    for seed in (1, 2, 3):
        p2, st2, rt2 = solve(form, X, last_place(x2, seed), Wf)
        s_pose = max(s_pose, float(np.abs(p2 - poses)[keep].max()))
        c2 = PC.host_cost(X, x2, Wc, K, rt2)   # the other solve's pose on THIS problem
        s_cost = max(s_cost, float(((c2 - cost) / cost)[keep].max()))   # excess, as the device test asserts it
        s_iter = max(s_iter, int(np.abs(st2 - status)[keep].max()))
    return s_pose, s_cost, s_iter


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pn", PC.SWEEP_PN)
def test_sweep_is_well_posed_and_the_oracle_agrees_with_itself_far_below_the_bars(pn, form):
    X, x2, Wf, Wc, poses, status, rt, cost = base(pn, form)
    # well-posed, nothing skipped: every image converges long before the iteration limit
    assert (status >= 0).all()
    assert (status < (PC.LIMIT if form == "unweighted" else 2 * PC.LIMIT)).all(), status
    assert np.isfinite(poses).all() and (cost > 0).all()
    s_pose, s_cost, s_iter = spread(form, X, x2, Wf, Wc, poses, status, cost)
    print(f"pn {pn:2d} {form:10s}: self-spread pose {s_pose:.2e} cost {s_cost:.2e} iterations {s_iter} (most {status.max()})")
    if form != "covariance" or pn == COVARIANCE_PN:
        assert 20 * s_pose <= PC.BAR_POSE
        assert 50 * s_cost <= PC.BAR_COST


@pytest.mark.parametrize("pn", PC.SWEEP_PN)
def test_the_two_host_routes_to_the_covariance_pose_agree(pn):
    """Evaluator.evaluate_uncertainty (two native calls, the pose through Python's Rodrigues formula in between) against
    pvnet_pnp_solve with the same weights (what the device restates): the device test's oracle is the former"""
    X, x2, cov, Wc, poses, _, _, _ = base(pn, "covariance")
    direct = PC.host_solve(X, x2, K, Wc)[0]
    d = float(np.abs(direct - poses).max())
    print(f"pn {pn:2d}: evaluate_uncertainty against pvnet_pnp_solve {d:.2e}")
    assert 20 * d <= PC.BAR_POSE


@pytest.mark.parametrize("form", FORMS[:2])
@pytest.mark.parametrize("pn", PC.SWEEP_PN)
def test_the_bars_tell_a_defect(pn, form):
    """never reading the last key-point, or reading key-point 0's image point for it, moves EVERY image's pose by more than
    100 * BAR_POSE"""
    X, x2, Wf, _, poses, _, _, _ = base(pn, form)
    moved = {}
    if pn >= 7:   # (five points: the linear start refuses)
        dropped, st, _ = PC.host_solve(X[:-1], x2[:, :-1], K, None if Wf is None else Wf[:, :-1])
        assert (st >= 0).all()
        moved["dropped"] = np.abs(dropped - poses).max(axis=(1, 2))
    wrong = x2.copy()
    wrong[:, -1] = x2[:, 0]
    misread, st, _ = PC.host_solve(X, wrong, K, Wf)
    assert (st >= 0).all()
    moved["misread"] = np.abs(misread - poses).max(axis=(1, 2))
    for name, m in moved.items():
        print(f"pn {pn:2d} {form:10s}: last key-point {name}: pose moves by {m.min():.2e} .. {m.max():.2e}, median {np.median(m):.2e}")
        assert (m > 100 * PC.BAR_POSE).all()


@pytest.mark.parametrize("pn", PC.ILL_PN)
def test_three_pixel_noise_few_images_are_ill_posed_and_the_rest_agree(pn):
    """at 3 px some images have no optimum to agree on (the unweighted LM runs to its limit): at most a quarter of them, and the
    others hold 3 * BAR_POSE with the margin of the sweep"""
    X, x2 = PC.ill_posed_case(pn)
    poses, status, rt = PC.host_solve(X, x2, K)
    ill = status >= PC.LIMIT
    assert (status >= 0).all() and ill.sum() <= len(x2) // 4
    good = ~ill
    for seed in (1, 2, 3):   # an image that reaches the limit on a neighbouring input is no image to agree on either
        good &= PC.host_solve(X, last_place(x2, seed), K)[1] < PC.LIMIT
    cost = PC.host_cost(X, x2, None, K, rt)
    s_pose, s_cost, s_iter = spread("unweighted", X, x2, None, None, poses, status, cost, keep=good)
    a_pose, a_cost, _ = spread("unweighted", X, x2, None, None, poses, status, cost, keep=ill) if ill.any() else (0.0, 0.0, 0)
    print(f"pn {pn:2d} 3 px: {int(ill.sum())} of {len(x2)} ill-posed ({int((~good).sum())} with neighbours); well-posed "
          f"self-spread pose {s_pose:.2e} cost {s_cost:.2e} iterations {s_iter} (most {status[good].max()}); ill-posed "
          f"pose {a_pose:.2e} cost {a_cost:.2e}")
    assert 20 * s_pose <= 3 * PC.BAR_POSE
