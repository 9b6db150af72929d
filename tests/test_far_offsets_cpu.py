"""The geometry of tests/far_cases.py, checked with plain integers and no device: for every (call, placement kind, distance) that
tests/test_far_offsets_device.py runs, the thresholds claimed are crossed, no two elements alias, everything lies inside the arena, and
every modelled mistake -- the far term of the address kept in 32 bits as elements or as bytes, sign- or zero-extended (the planted-mistake
style of tests/test_pose_classes_cpu.py) -- sends at least one access to a DIFFERENT address inside a decoy or sentinel window of the
arena.  No library refuses far strides (none returns PVNET_E_UNSUPPORTED for them), so there is no refusal to pin here."""
import pytest
import torch

from tests import far_cases as F

CASES = F.all_cases()
TERMS = ("batch", "planes", "rows")


def plan_of(case):
    call, kind, which, odd = case
    p = F.Plan(kind, which, odd)
    for (name, shape, esize, dims, role) in F.CALLS[call]:
        p.add(name, shape, esize, dims, role)
    return p


def addresses(pl):
    """the byte address of every element, in the logical order"""
    a = torch.full(pl.shape, pl.base, dtype=torch.int64)
    for k, (n, s) in enumerate(zip(pl.shape, pl.strides)):
        view = [1] * len(pl.shape)
        view[k] = n
        a = a + (torch.arange(n, dtype=torch.int64) * (s * pl.esize)).view(view)
    return a


def mistaken_addresses(pl, k, mistake):
    """the same with the term of dimension k under ``mistake``"""
    a = torch.full(pl.shape, pl.base, dtype=torch.int64)
    for j, (n, s) in enumerate(zip(pl.shape, pl.strides)):
        view = [1] * len(pl.shape)
        view[j] = n
        if j == k:
            off = torch.tensor([F.mistaken_bytes(mistake, i * s, pl.esize) for i in range(n)], dtype=torch.int64)
        else:
            off = torch.arange(n, dtype=torch.int64) * (s * pl.esize)
        a = a + off.view(view)
    return a


def expected_bites(esize, top_elems):
    """the mistakes that MUST change an address, from the largest far term alone"""
    top_bytes = top_elems * esize
    want = set()
    if top_elems >= 2 ** 31:
        want.add("i32_elem")
    if top_elems >= 2 ** 32:
        want.add("u32_elem")
    if top_bytes >= 2 ** 31:
        want.add("i32_byte")
    if top_bytes >= 2 ** 32:
        want.add("u32_byte")
    return want


def test_the_constants_are_the_issue_s():
    assert F.ARENA_BYTES == 2 ** 34 + 2 ** 28 and F.MID == 2 ** 33
    assert F.DISTANCES == {1: (2 ** 31, 2 ** 32), 2: (2 ** 31, 2 ** 32), 4: (2 ** 31,), 8: (2 ** 30,)}
    assert F.N_SLOTS * F.SLOT <= 2 ** 28 and F.TWIN_OFF % 16 == 0 and F.SLOT % 4096 == 0
    # the modelled truncations themselves, on known values
    assert F.trunc32(2 ** 31 + 5, True) == -2 ** 31 + 5 and F.trunc32(2 ** 31 + 5, False) == 2 ** 31 + 5
    assert F.trunc32(2 ** 32 + 5, True) == 5 and F.trunc32(2 ** 32 + 5, False) == 5
    assert F.mistaken_bytes("i32_elem", 2 ** 31 + 16, 4) == (-2 ** 31 + 16) * 4 and F.mistaken_bytes("u32_elem", 2 ** 31 + 16, 4) == (2 ** 31 + 16) * 4
    assert F.mistaken_bytes("i32_byte", 2 ** 31 + 16, 4) == 64 and F.mistaken_bytes("u32_byte", 2 ** 30 + 2, 8) == 16
    assert F.mistaken_bytes("i32_byte", 2 ** 30 + 2, 8) == 16 and F.mistaken_bytes("i32_elem", 2 ** 30 + 2, 8) == (2 ** 30 + 2) * 8


def test_every_call_has_its_cases_and_every_kind():
    assert len(CASES) == len(set(CASES))
    for call in F.CALLS:
        kinds = {k for (k, _, _) in F.cases(call)}
        assert kinds == set(F.KINDS), call
        assert any(odd for (_, _, odd) in F.cases(call)), call
        if any(e in (1, 2) for (_, _, e, _, _) in F.CALLS[call]):
            assert {w for (_, w, _) in F.cases(call)} == {0, 1}, call


@pytest.mark.parametrize("case", CASES, ids=F.case_id)
def test_geometry(case):
    call, kind, which, odd = case
    plan = plan_of(case)    # (Plan.add asserts: every window with its guards inside the arena, disjoint from every other of the call)
    assert len(plan.operands) == len(F.CALLS[call]) <= F.N_SLOTS
    every = []
    for (name, role, far, near, lands), spec in zip(plan.operands, F.CALLS[call]):
        esize, k, n = far.esize, far.dim, far.shape[far.dim]
        assert (name, far.shape, esize, role) == (spec[0], spec[1], spec[2], spec[4])
        what = f"{F.case_id(case)} {name}"
        # ---- the base in the middle, the alignment, the twin ----
        assert far.base >= F.MID and far.base % 16 == 0 and near.base % 16 == far.base % 16, what
        assert near.shape == far.shape and all(a == b for j, (a, b) in enumerate(zip(near.strides, far.strides)) if j != k), what
        assert (near.far_stride - far.far_stride) * esize % 16 == 0 and near.far_stride >= far.inner, what
        assert near.far_stride - far.inner < 16, what   # the SMALLEST such stride
        assert near.extent()[1] - near.base < F.TWIN_OFF, what
        # ---- the thresholds claimed ----
        dist = F.DISTANCES[esize][min(which, len(F.DISTANCES[esize]) - 1)]
        delta = F.delta_of(far.shape, k, esize, odd)
        assert delta * esize % 16 == (esize if odd else 0) % 16 and delta > far.inner, what
        top = (n - 1) * far.far_stride
        assert top >= dist + delta, what
        if n == 2:
            assert far.far_stride == dist + delta, what
        else:
            assert far.far_stride % F.ROUND == 0 and far.far_stride == F.round_up(-(-(dist + delta) // (n - 1)), F.ROUND), what
            assert (n - 2) * far.far_stride < dist + delta, what   # only the LAST block lies beyond
        if esize in (1, 2):
            assert top >= (2 ** 31, 2 ** 32)[which], what
        elif esize == 4:
            assert top >= 2 ** 31 and top * 4 >= 2 ** 33, what
        else:
            assert top < 2 ** 31 and top * 8 >= 2 ** 33, what   # (no 8-byte placement of this arena reaches 2^31 elements)
        assert far.crossed()[0] >= top, what
        # ---- no two elements alias, every element inside the arena ----
        for pl in (far, near):
            a = addresses(pl).flatten()
            assert int(a.min()) >= 0 and int(a.max()) + esize <= F.ARENA_BYTES, what
            assert a.unique().numel() == a.numel() and bool((a % esize == 0).all()), what
            if pl is far:
                assert int(a.min()) >= F.MID, what
            every.append(a)
        # ---- the modelled mistakes ----
        true = addresses(far)
        windows = {(s, e) for (_, _, s, e) in lands}
        bites = set()
        for term, dim in zip(TERMS, (F.far_dim(kd, spec[3]) for kd in F.KINDS)):
            for m in F.MISTAKES:
                wrong = mistaken_addresses(far, dim, m)
                assert int(wrong.min()) >= 0 and int(wrong.max()) + esize <= F.ARENA_BYTES, (what, term, m)
                moved = wrong != true
                if dim != k:
                    # the term of a dimension that is not far is small: keeping it in 32 bits changes nothing
                    assert not bool(moved.any()), (what, term, m)
                    continue
                if not bool(moved.any()):
                    continue
                bites.add(m)
                # every moved access lies inside a landing window (a decoy or a sentinel), none on real data
                w = wrong[moved]
                inside = torch.zeros_like(w, dtype=torch.bool)
                for (s, e) in windows:
                    inside |= (w >= s) & (w + esize <= e)
                assert bool(inside.all()), (what, term, m)
        assert bites == expected_bites(esize, top), (what, bites)
        assert bites, what   # at least one modelled mistake is caught on every operand of every placement
        # the landing windows are disjoint from every true window of this operand (Plan checked all operands against all)
        for (s, e) in windows:
            assert all(not F.overlap((s, e), wnd) for wnd in far.windows()) and not F.overlap((s, e), near.extent()), what
    # no two operands of the call share a byte
    a = torch.cat(every)
    assert a.unique().numel() == a.numel(), F.case_id(case)


def test_the_int64_mask_placements_select_both_mask_kernels():
    """launch_mask_bits (pvnet_amd/csrc/k1_mask.hip) takes mask_bits_pair_kernel for an int64 mask whose images are contiguous, whose
    base is 16-byte aligned and whose ms0 and pixel count are even; everything else takes mask_bits_kernel.  The far-batch placement of
    the int64 mask must satisfy the first, its odd placement must not."""
    def pair(pl):
        linear = pl.strides[1] == pl.shape[2] and pl.strides[2] == 1
        return linear and pl.base % 16 == 0 and pl.strides[0] % 2 == 0 and (pl.shape[1] * pl.shape[2]) % 2 == 0
    for odd, want in ((False, True), (True, False)):
        plan = plan_of(("vote_v3-i64-f32-contiguous", "far_batch", 0, odd))
        _, _, far, near, _ = plan.operands[0]
        assert far.esize == 8 and pair(far) == want and pair(near) == want
    _, _, far, near, _ = plan_of(("vote_v3-i64-f32-contiguous", "far_rows", 0, False)).operands[0]
    assert not pair(far) and not pair(near)
