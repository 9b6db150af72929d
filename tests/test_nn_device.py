"""The brute-force nearest-neighbour search (pvnet_nearest_point_idx, nn_search_kernel of pvnet_amd/csrc/pvnet_nn.hip) held to
oracle/nn_oracle.py index for index -- there is no tolerance anywhere in this file -- on every cloud family of tests/nn_cases.py
(uniform cubes, tie-laden lattices, pixel-scale 2-D clouds, subnormal squared distances, non-finite and overflowing coordinates)
at every path of its slice planner: one slice of several tiles, one-tile slices with a ragged end, multi-tile slices, fewer slices
than wanted, both sides of the tile edges, an empty reference cloud, and the self-exclusion in later tiles and other slices.
tests/test_nn_cpu.py holds the oracle to the reference's loop and shows what each case tells; where oracle/_ref/libpvnet_refnn.so
is built, the reference's own device code is the third witness."""
import numpy as np
import pytest
import torch

from oracle import nn_oracle
from pvnet_amd import _abi
from pvnet_amd import evaluation as E
from pvnet_amd._marshal import nbytes as _nbytes, ptr as _ptr, stream as _stream
from tests import nn_cases as NC

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
GUARD = 256


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def up(a):
    return torch.from_numpy(np.array(a)).to(dev())   # a copy: the shared clouds are read-only


def strided(a):
    """the same values as a view that is contiguous in no dimension: every other point of a cloud with a spare column"""
    b, pn, dim = a.shape
    big = torch.full((b, 2 * pn + 1, dim + 1), float("nan"), dtype=torch.float32, device=dev())
    view = big[:, 1::2, :dim]
    view.copy_(up(a))
    assert not view.is_contiguous() or pn == 0
    return view


def entry(ref, que, out, exclude_self=False, workspace=None):
    """pvnet_nearest_point_idx itself, on the current stream: the caller owns the output and the workspace"""
    b, pn1, dim = ref.shape
    rc = _abi.load_library().pvnet_nearest_point_idx(_ptr(ref) if pn1 else None, _ptr(que), _ptr(out), b, pn1, que.shape[1], dim,
                                                     1 if exclude_self else 0, _ptr(workspace),
                                                     0 if workspace is None else _nbytes(workspace), _stream(dev()))
    _abi._check(rc, "pvnet_nearest_point_idx")


def workspace_bytes(b, pn2):
    return int(_abi.load_library().pvnet_nearest_workspace_bytes(b, pn2))


@pytest.mark.parametrize("case", NC.sweep_cases(), ids=lambda c: c.id)
def test_every_family_at_every_planner_regime_equals_the_oracle(case):
    ref, que = NC.host_clouds(case)
    want = NC.expected(case)
    got = E.nearest_point_idx(up(ref), up(que))
    assert got.dtype == torch.int32 and tuple(got.shape) == (case.b, case.pn2)
    got = got.cpu().numpy()
    for i in range(case.b):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"{case.id} item {i}")
    # handed over as views that are not contiguous, and as the float64 draws: the wrapper's conversion gives the host's float32
    np.testing.assert_array_equal(E.nearest_point_idx(strided(ref), strided(que)).cpu().numpy(), want, err_msg=f"{case.id} strided")
    ref64, que64 = NC.raw_clouds(case)
    assert ref64.dtype == np.float64
    np.testing.assert_array_equal(E.nearest_point_idx(up(ref64), up(que64)).cpu().numpy(), want, err_msg=f"{case.id} float64")


@pytest.mark.parametrize("case", NC.x_cases(), ids=lambda c: c.id)
def test_self_exclusion_in_later_tiles_and_other_slices(case):
    """queries that repeat the reference points: with the exclusion the nearest OTHER point (the query's own slot lies in a later
    tile of its slice, or in another slice, or nowhere when pn2 > pn1); without it the query itself or its first earlier twin"""
    ref, que = NC.host_clouds(case)
    want = NC.expected(case)
    got = E.nearest_point_idx(up(ref), up(que), exclude_self=case.exclude_self).cpu().numpy()
    for i in range(case.b):
        np.testing.assert_array_equal(got[i], want[i], err_msg=f"{case.id} item {i}")
    m = min(case.pn1, case.pn2)
    own = np.arange(m)[None]
    if case.exclude_self:
        assert (got[:, :m] != own).all()
    else:
        assert (got[:, :m] <= own).all()
        assert (np.take_along_axis(ref, got[:, :m, None].astype(np.int64), 1) == que[:, :m]).all()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("b,pn1,pn2", NC.REGIME_SHAPES["F"])
def test_an_empty_reference_cloud_answers_index_zero_and_writes_nothing_else(b, pn1, pn2, dim):
    assert pn1 == 0
    _, que = NC.clouds("cube", b, 1, pn2, dim)
    q = up(que.astype(np.float32))
    ref = torch.empty((b, 0, dim), dtype=torch.float32, device=dev())
    got = E.nearest_point_idx(ref, q)
    assert got.dtype == torch.int32 and tuple(got.shape) == (b, pn2) and not got.any()
    one = E.nearest_point_idx(ref[0], q[0])
    assert one.dtype == torch.int32 and tuple(one.shape) == (pn2,) and not one.any()
    # the entry point with a null reference pointer, its output in the middle of a poisoned buffer, its workspace poisoned too
    buf = torch.full((b * pn2 + 2 * GUARD,), POISON, dtype=torch.int32, device=dev())
    ws = torch.full((workspace_bytes(b, pn2) // 4,), POISON, dtype=torch.int32, device=dev())
    entry(ref, q, buf[GUARD: GUARD + b * pn2], workspace=ws)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert not host[GUARD: GUARD + b * pn2].any()
    assert (host[:GUARD] == POISON).all() and (host[GUARD + b * pn2:] == POISON).all()
    assert (ws == POISON).all()   # one slice: the workspace is not used


def test_a_single_slice_needs_no_workspace():
    case = NC.Case("lattice", 3, "A", *NC.REGIME_SHAPES["A"][0], False, False)
    assert NC.plan(case.b, case.pn1, case.pn2).nslices == 1
    ref, que = NC.host_clouds(case)
    out = torch.full((case.b, case.pn2), -1, dtype=torch.int32, device=dev())
    entry(up(ref), up(que), out, workspace=None)
    np.testing.assert_array_equal(out.cpu().numpy(), NC.expected(case))


@pytest.mark.parametrize("family", ["lattice", "hostile"])
def test_garbage_workspace_reuse_and_a_side_stream(family):
    """multi-tile slices merged through the workspace: what the workspace held before, a second call and the stream change nothing"""
    case = NC.Case(family, 3, "C", *NC.REGIME_SHAPES["C"][0], False, False)
    assert NC.plan(case.b, case.pn1, case.pn2).sizes == (768, 332)
    ref, que = (up(a) for a in NC.host_clouds(case))
    want = NC.expected(case)
    need = workspace_bytes(case.b, case.pn2)
    g = torch.Generator(device=dev()).manual_seed(11)
    outs = []
    for ws in (torch.zeros(need, dtype=torch.uint8, device=dev()),
               torch.randint(0, 256, (need,), dtype=torch.uint8, device=dev(), generator=g),
               torch.full((need,), 0xFF, dtype=torch.uint8, device=dev())):
        for _ in range(2):   # the second call finds the first one's words
            out = torch.full((case.b, case.pn2), -1, dtype=torch.int32, device=dev())
            entry(ref, que, out, workspace=ws)
            outs.append(out.cpu().numpy())
    for o in outs:
        assert o.tobytes() == want.tobytes()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = E.nearest_point_idx(ref, que)
    side.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("pn1,pn2,exclude_self", [(600, 300, False), (513, 257, False), (1100, 5, False), (700, 700, True)])
@pytest.mark.parametrize("family,dim", [(f, d) for f in NC.FAMILIES for d in NC.family_dims(f)])
def test_the_references_own_device_code_agrees_on_every_family(family, dim, pn1, pn2, exclude_self):
    """oracle/_ref/libpvnet_refnn.so is the reference's nearest_neighborhood.cu compiled for gfx950, called through its own
    launcher: numpy, the reference kernel and the product give the same indices, the hostile and the subnormal clouds included"""
    from oracle import refkernels
    if not refkernels.nn_available("off"):
        pytest.skip("oracle/_ref/libpvnet_refnn.so not built (needs the reference tree at build time)")
    ref, que = (a.astype(np.float32)[0] for a in NC.clouds(family, 1, pn1, pn2, dim, seed=3))
    if exclude_self:
        que = ref.copy()   # one cloud against itself: the nearest other point
    with np.errstate(over="ignore", invalid="ignore"):
        numpy_idx = nn_oracle.find_nearest_point_idx(ref, que, exclude_self=exclude_self)
    ref_idx = refkernels.find_nearest_point_idx(ref, que, exclude_self=exclude_self)
    got = E.nearest_point_idx(up(ref), up(que), exclude_self=exclude_self).cpu().numpy()
    np.testing.assert_array_equal(got, ref_idx, err_msg="product against the reference kernel")
    np.testing.assert_array_equal(numpy_idx, ref_idx, err_msg="numpy oracle against the reference kernel")
