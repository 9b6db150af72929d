"""What the nearest-neighbour device tests (tests/test_nn_device.py) stand on, checked without a GPU: the oracle against the
reference's loop restated literally, the planner regime of every shape, what the clouds must hold for a wrong kernel to show, the
defects the cases tell, and the refusals of the C entry point that return before any launch."""
import ctypes as C

import numpy as np
import pytest

from oracle import nn_oracle
from pvnet_amd import _abi
from tests import nn_cases as NC


# ------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("family,dim", [(f, d) for f in NC.FAMILIES for d in NC.family_dims(f)])
def test_the_oracle_equals_the_literal_scan(family, dim, exclude_self):
    ref, que = (a.astype(np.float32) for a in NC.clouds(family, 1, 300, 200, dim, seed=7))
    want = NC.scan(ref, que, exclude_self)[0]
    with np.errstate(over="ignore", invalid="ignore"):   # the hostile family overflows and makes NaN on purpose
        got = nn_oracle.find_nearest_point_idx(ref[0], que[0], exclude_self=exclude_self)
    np.testing.assert_array_equal(got, want)
    assert len(np.unique(want)) >= 30
    np.testing.assert_array_equal(NC.scan(ref, que, exclude_self, slice_=NC.TILE)[0], want)   # sliced and merged: the same answer
    if family == "hostile":   # the family does what it is for: some queries have no admissible reference point, most have one
        case = NC.Case(family, dim, "oracle", 1, 300, 200, exclude_self, False)
        ref0_ok = NC._dist(ref, que, 0, False)[0] < NC.FLT_MAX
        ref0_ok[0] &= not exclude_self
        none = (want == 0) & ~ref0_ok
        assert 0.01 <= none.mean() <= 0.25, (case.id, none.mean())


# ------------------------------------------------------------------------------------------------------------ the planner
def test_every_shape_takes_the_path_its_regime_names():
    P = NC.plan
    assert P(1024, 600, 3) == (1, 768, 1, (600,))                    # A: one slice, tiles of 256 + 256 + 88
    assert P(1, 513, 257) == (512, 256, 3, (256, 256, 1))            # B: one-tile slices, the last of one point
    assert P(512, 1100, 5) == (2, 768, 2, (768, 332))                # C: multi-tile slices
    assert P(400, 1000, 7) == (3, 512, 2, (512, 488))                # D: fewer slices than wanted
    for b, pn1, pn2 in NC.REGIME_SHAPES["E"]:                        # E: one-tile slices up to both sides of the tile edges
        p = P(b, pn1, pn2)
        assert p.slice == NC.TILE and p.nslices == -(-pn1 // NC.TILE) and sum(p.sizes) == pn1, (b, pn1, pn2, p)
    assert {P(*s).sizes[-1] for s in NC.REGIME_SHAPES["E"]} == {1, 255, 256}
    for s in NC.REGIME_SHAPES["F"]:                                  # F: one workgroup row, nothing to scan
        assert P(*s)[1:] == (NC.TILE, 1, (0,))
    assert P(171, 1000, 600) == (2, 512, 2, (512, 488))              # X: two slices of two tiles
    assert P(2, 300, 700) == (171, 256, 2, (256, 44))
    assert P(2, 700, 300) == (256, 256, 3, (256, 256, 188))
    # what tests/test_evaluation.py runs never makes a second trip through a slice's tile loop
    for b, pn1, pn2 in [(1, 5000, 7000), (1, 3000, 200), (1, 1, 33), (1, 257, 256), (1, 4097, 9000), (1, 20000, 17), (3, 1500, 1500)]:
        p = P(b, pn1, pn2)
        assert p.slice == NC.TILE and p.nslices == -(-pn1 // NC.TILE), (b, pn1, pn2, p)


# ------------------------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("case", NC.device_cases(), ids=lambda c: c.id)
def test_the_clouds_hold_what_the_device_tests_need(case):
    """Few queries without an admissible reference point, many distinct answers, and on the lattice mostly tied minima.  The counts
    are taken over the whole case, all batch items together.  Thirty answers need thirty queries: the bar on distinct answers holds
    where there are at least 64 reference points per item and 64 queries in the case, and the bar on ties where there are at least
    64 reference points (one point cannot tie with itself)."""
    assert NC.pair_tests(case) <= 1.05e8
    idx = NC.expected(case)
    assert idx.shape == (case.b, case.pn2) and idx.dtype == np.int32
    assert ((idx >= 0) & (idx < max(case.pn1, 1))).all()
    none = NC.nothing_qualifies(case)
    assert none.mean() < 0.25, none.mean()
    if case.pn1 >= 64 and case.b * case.pn2 >= 64:
        assert len(np.unique(idx)) >= 30, len(np.unique(idx))
    if case.family == "lattice" and case.pn1 >= 64:
        assert NC.tied_fraction(case) >= 0.5
    if case.twins:
        ref, que = NC.host_clouds(case)
        m = min(case.pn1, case.pn2)
        own = np.arange(m)[None]
        if case.exclude_self:   # the nearest OTHER point: never the query's own index, and on this lattice still an exact twin
            assert (idx[:, :m] != own).all()
        else:                   # itself, or the first earlier twin: 300 points and more on at most 216 lattice sites have many
            assert (idx[:, :m] <= own).all() and (idx[:, :m] < own).mean() > 0.25
            assert (np.take_along_axis(ref, idx[:, :m, None].astype(np.int64), 1) == que[:, :m]).all()


# ------------------------------------------------------------------------------------------------------------ the defects
def _case(family, dim, regime, shape, exclude_self=False):
    return NC.Case(family, dim, regime, *shape, exclude_self, regime == "X")


# every mutant with the cases that are there to catch it
TELLS = {
    "last_index_wins": [_case("lattice", 3, "B", (1, 513, 257)), _case("lattice", 2, "E", (2, 255, 257))],
    "flushed_subnormals": [_case("tiny", 3, "B", (1, 513, 257)), _case("tiny", 2, "A", (1024, 600, 3))],
    "self_slot_in_every_tile": [_case("lattice", 3, "X", (171, 1000, 600), True), _case("lattice", 2, "X", (2, 700, 300), True)],
    "merge_prefers_larger_index": [_case("lattice", 3, "C", (512, 1100, 5)), _case("lattice", 2, "D", (400, 1000, 7)),
                                   _case("lattice", 3, "B", (1, 513, 257))],
    "first_tile_of_a_slice_only": [_case("cube", 3, "A", (1024, 600, 3)), _case("pixel", 2, "C", (512, 1100, 5)),
                                   _case("lattice", 3, "D", (400, 1000, 7))],
}


@pytest.mark.parametrize("mutant", NC.MUTANTS)
def test_the_cases_tell_a_defect(mutant):
    """each defect a kernel of this layout could have changes the indices of the cases named for it -- so a device test that
    passes on those cases rules the defect out"""
    assert set(TELLS) == set(NC.MUTANTS)
    device_ids = {c.id for c in NC.device_cases()}
    for case in TELLS[mutant]:
        assert case.id in device_ids, case.id
        ref, que = NC.host_clouds(case)
        if case.b > 64:   # the defect shows in any item: a slice of the batch keeps the lockstep scan short
            ref, que = ref[:64], que[:64]
        want = NC.expected(case)[: ref.shape[0]]
        p = NC.plan(case.b, case.pn1, case.pn2)
        sliced = mutant in ("merge_prefers_larger_index", "first_tile_of_a_slice_only")
        got = NC.scan(ref, que, case.exclude_self, mutant, slice_=p.slice if sliced else None)
        wrong = float((got != want).mean())
        print(f"{mutant}: case {case.id}: {100 * wrong:.1f} % of the indices differ")
        assert wrong > 0, f"mutant {mutant} gives the oracle's indices on case {case.id}"
        np.testing.assert_array_equal(NC.scan(ref, que, case.exclude_self, None, slice_=p.slice if sliced else None), want,
                                      err_msg=f"the scan itself on case {case.id}")


# ------------------------------------------------------------------------------------------------------------ the C entry point
def _entry():
    lib = _abi.load_library()
    pts = (C.c_float * 64)()
    out = (C.c_int32 * 64)()
    ws = (C.c_uint64 * 8192)()
    lib.pvnet_nearest_workspace_bytes.restype = C.c_size_t
    lib.pvnet_nearest_point_idx.restype = C.c_int

    def call(b, pn1, pn2, dim, workspace=C.addressof(ws), nbytes=C.sizeof(ws), ref=C.addressof(pts)):
        return lib.pvnet_nearest_point_idx(C.c_void_p(ref), C.c_void_p(C.addressof(pts)), C.c_void_p(C.addressof(out)), b, pn1, pn2,
                                           dim, 0, C.c_void_p(workspace), C.c_size_t(nbytes), None)
    return lib, call, C.addressof(ws)


def test_the_entry_point_refuses_bad_shapes_before_any_launch():
    lib, call, _ = _entry()
    assert call(1, 8, 8, 4) == _abi.E_BADARG            # dim 4
    assert call(1, 8, 8, 1) == _abi.E_BADARG
    assert call(1, 8, 0, 3) == _abi.E_BADARG            # no query
    assert call(1, -1, 8, 3) == _abi.E_BADARG           # a negative reference count
    assert call(0, 8, 8, 3) == _abi.E_BADARG
    assert call(65536, 8, 8, 3) == _abi.E_UNSUPPORTED   # the batch is the grid's z
    assert call(1, 8, 8, 3, ref=0) == _abi.E_BADARG     # a null reference cloud of eight points
    assert lib.pvnet_nearest_workspace_bytes(1, 257) == 2304 and lib.pvnet_nearest_workspace_bytes(1, 0) == 0


def test_the_entry_point_checks_the_workspace_of_a_sliced_search():
    lib, call, ws = _entry()
    b, pn1, pn2 = NC.REGIME_SHAPES["B"][0]
    assert NC.plan(b, pn1, pn2).nslices > 1
    need = lib.pvnet_nearest_workspace_bytes(b, pn2)
    assert need == 2304 and ws % 8 == 0
    assert call(b, pn1, pn2, 3, workspace=ws, nbytes=need - 1) == _abi.E_WORKSPACE   # one byte short
    assert call(b, pn1, pn2, 3, workspace=0, nbytes=need) == _abi.E_WORKSPACE        # none at all
    assert call(b, pn1, pn2, 3, workspace=ws + 1, nbytes=need) == _abi.E_BADARG      # an odd address
    assert call(b, pn1, pn2, 3, workspace=ws + 4, nbytes=need) == _abi.E_BADARG      # 4-byte aligned: the words are 8 bytes
