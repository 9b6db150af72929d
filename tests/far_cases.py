"""Small tensors laid far apart: the geometry and the device arena of tests/test_far_offsets_cpu.py and tests/test_far_offsets_device.py.

Every C ABI of the project takes int64 element strides.  A kernel that worked out ``bi * stride0``, ``c * stride1`` or ``y * stride2`` in 32
bits would pass every test whose operands lie within a few megabytes of their base, so the tests here move ONE stride of every strided
operand beyond 2^31 elements or 2^32 bytes.  No large data is needed: one uninitialised ``uint8`` arena of ``ARENA_BYTES`` is allocated and
a small logical tensor is laid into it as an ``as_strided`` view that touches only its own few kilobytes.

The geometry (``place``, ``Placement``, ``Plan``) is plain integer arithmetic: the CPU test file checks it without a device.  ``Arena``
and ``Session`` are the device part.

Layout of the arena.  Operand j of a call owns slot j: its base is byte ``MID + j * SLOT`` (``MID`` = 2^33, the middle), its near twin lies
``TWIN_OFF`` bytes behind.  Because every base is at byte 2^33 or later, a far offset wrongly truncated to 32 bits -- counted in elements
or in bytes, zero- or sign-extended -- still lands INSIDE the arena (the lowest landing is 2^31 elements of four bytes below the base):
a wrong kernel fails a comparison, it does not fault.  ``Placement.landings`` computes those landing windows; an input gets a decoy
(different seeded data of the same type and scale) there, an output a sentinel pattern that has to survive the call.

Far distance D (elements) by element size: 1 or 2 bytes: 2^31 + delta and 2^32 + delta; 4 bytes: 2^31 + delta (2^33 bytes); 8 bytes:
2^30 + delta -- 2^32 and 2^33 BYTES only: no placement of an 8-byte type in this arena reaches 2^31 elements (that needs 32 GiB).
delta is a multiple of 16 bytes (the vector paths stay eligible; ``odd=True`` adds one element for the element-by-element paths) and
larger than the operand's own extent, so a truncated landing window is disjoint from the real data.

Placement kinds, for a tensor in its STORAGE order (a permuted view is taken of the placed tensor afterwards):
  far_batch   the stride of the batch dimension (size 2) is D, everything else compact: image 1 lies wholly beyond
  far_planes  the stride of the channel dimension is ceil(D / (C - 1)) rounded up to 4096 elements: only the last planes lie beyond
  far_rows    the same over the rows: the general (non-linear image) path
The other dimensions are laid out compactly INSIDE one step of the far stride (their strides are rebuilt), so nothing aliases.  An operand
without the dimension of a kind takes the batch placement.  The near twin of a placement has the same shape, the same base alignment mod
16 bytes and the same strides but for the far one, which is the smallest non-aliasing stride with the same residue mod 16 bytes.
"""
from dataclasses import dataclass
from math import gcd, prod

ARENA_BYTES = 2 ** 34 + 2 ** 28
MID = 2 ** 33                      # every base lies here or later
SLOT = 2 ** 24                     # bytes of the arena an operand's near part owns
N_SLOTS = 16
TWIN_OFF = SLOT // 2               # the near twin lies this far behind its far view's base
GUARD = 4096                       # sentinel bytes on both sides of every window an output writes
SENTINEL = 0xA5
ROUND = 4096                       # far_planes / far_rows strides are multiples of this many elements
KINDS = ("far_batch", "far_planes", "far_rows")
DISTANCES = {1: (2 ** 31, 2 ** 32), 2: (2 ** 31, 2 ** 32), 4: (2 ** 31,), 8: (2 ** 30,)}   # elements, before delta
MISTAKES = ("i32_elem", "u32_elem", "i32_byte", "u32_byte")


def round_up(v, m):
    return -(-v // m) * m


def trunc32(v, signed):
    v &= 0xFFFFFFFF
    return v - 2 ** 32 if signed and v >= 2 ** 31 else v


def mistaken_bytes(mistake, term, esize):
    """the BYTE offset a kernel adds for the element offset ``term`` of one address term when it makes ``mistake``: the term kept in a
    32-bit register as elements (``*_elem``) or after the multiplication by the element size (``*_byte``), sign- or zero-extended"""
    signed = mistake.startswith("i32")
    return trunc32(term, signed) * esize if mistake.endswith("elem") else trunc32(term * esize, signed)


def far_dim(kind, dims):
    """the dimension of an operand that ``kind`` moves: ``dims`` = (batch, planes, rows), None where the operand has none (-> batch)"""
    d = dims[KINDS.index(kind)]
    return dims[0] if d is None else d


@dataclass(frozen=True)
class Placement:
    shape: tuple
    strides: tuple     # elements
    base: int          # byte offset in the arena
    esize: int
    dim: int           # the far dimension
    inner: int         # elements of one compact block (everything but the far dimension)

    @property
    def far_stride(self):
        return self.strides[self.dim]

    def window(self, i, extra=0):
        """bytes [start, end) of block i of the far dimension, ``extra`` bytes added to its start"""
        s = self.base + i * self.far_stride * self.esize + extra
        return s, s + self.inner * self.esize

    def windows(self):
        return [self.window(i) for i in range(self.shape[self.dim])]

    def extent(self):
        return self.base, self.window(self.shape[self.dim] - 1)[1]

    def landings(self):
        """[(mistake, i, start, end)]: where block i of the far dimension is looked for by a kernel that makes ``mistake`` on the far
        term i * stride -- only those that differ from the true window"""
        out = []
        for i in range(self.shape[self.dim]):
            term = i * self.far_stride
            for m in MISTAKES:
                off = mistaken_bytes(m, term, self.esize)
                if off != term * self.esize:
                    s = self.base + off
                    out.append((m, i, s, s + self.inner * self.esize))
        return out

    def crossed(self):
        """the largest element offset and byte offset (from the base) of any element"""
        top = sum((n - 1) * s for n, s in zip(self.shape, self.strides))
        return top, top * self.esize


def _inner_strides(shape, dim):
    """compact strides of ``shape`` with dimension ``dim`` left out (its entry is None)"""
    st, run = [None] * len(shape), 1
    for k in reversed(range(len(shape))):
        if k != dim:
            st[k] = run
            run *= shape[k]
    return st, run


def delta_of(shape, dim, esize, odd=False):
    """delta in elements: a multiple of 16 bytes (one element more with ``odd``) above n blocks and their guards, n = the far dimension's
    size (a plane's landing may lie a fraction of delta behind the base: see place)"""
    inner = prod(shape) // shape[dim]
    d = shape[dim] * round_up(inner * esize + 4 * GUARD, 4096) // esize
    return d + (1 if odd else 0)


def place(shape, esize, dim, slot, which=0, odd=False, align=0):
    """the far placement of an operand: ``dim`` far by ``DISTANCES[esize][which]`` + delta, in slot ``slot``, its base ``align`` bytes
    behind the slot's start"""
    shape = tuple(int(n) for n in shape)
    assert 0 <= slot < N_SLOTS and shape[dim] >= 2 and align % esize == 0
    dist = DISTANCES[esize]
    D = dist[min(which, len(dist) - 1)] + delta_of(shape, dim, esize, odd)
    n = shape[dim]
    S = D if n == 2 else round_up(-(-D // (n - 1)), ROUND)
    st, inner = _inner_strides(shape, dim)
    st[dim] = S
    p = Placement(shape, tuple(st), MID + slot * SLOT + align, esize, dim, inner)
    assert (n - 1) * S >= D and S >= inner
    return p


def twin(p):
    """the near twin: the far stride replaced by the smallest non-aliasing one with the same residue mod 16 bytes, the base TWIN_OFF
    bytes behind (the same alignment mod 16 bytes)"""
    m = 16 // gcd(16, p.esize)
    S = p.inner + (p.far_stride - p.inner) % m
    st = list(p.strides)
    st[p.dim] = S
    t = Placement(p.shape, tuple(st), p.base + TWIN_OFF, p.esize, p.dim, p.inner)
    assert (S * p.esize - p.far_stride * p.esize) % 16 == 0 and (t.base - p.base) % 16 == 0 and S >= p.inner
    return t


def overlap(a, b):
    return a[0] < b[1] and b[0] < a[1]


class Plan:
    """The placements of ONE call: every operand in a slot of its own, every window (data, twin, decoy or sentinel, with the guards)
    registered and checked: inside the arena, disjoint from every other.  Pure integers; ``Session`` executes it on a device."""

    def __init__(self, kind, which=0, odd=False):
        assert kind in KINDS
        self.kind, self.which, self.odd = kind, which, odd
        self.taken = []    # (start, end, what)
        self.operands = []  # (name, role, far, near, landing windows)
        self.landings = {}  # operand -> [(mistake, block, start, end)]: where a truncated far term would look for its blocks

    def _take(self, s, e, what):
        assert 0 <= s - GUARD and e + GUARD <= ARENA_BYTES, f"{what}: bytes {s}..{e} leave the arena"
        for (s2, e2, w2) in self.taken:
            assert not overlap((s - GUARD, e + GUARD), (s2, e2)), f"{what} ({s}..{e}) overlaps {w2} ({s2}..{e2})"
        self.taken.append((s, e, what))

    def add(self, name, shape, esize, dims, role="in", align=0):
        """place operand ``name`` (``role`` "in" or "out"); -> (far, near, landings) with landings = [(mistake, i, start, end)]"""
        slot = len(self.operands)
        far = place(shape, esize, far_dim(self.kind, dims), slot, self.which, self.odd, align)
        near = twin(far)
        assert far.base >= MID and near.extent()[1] + GUARD <= MID + (slot + 1) * SLOT, f"{name}: the twin leaves its slot"
        for i, (s, e) in enumerate(far.windows()):
            self._take(s, e, f"{name} block {i}")
        self._take(*near.extent(), f"{name} twin")
        lands, seen = far.landings(), set()
        for (m, i, s, e) in lands:
            if (s, e) not in seen:       # (two mistakes may land a block on the same window: one decoy serves both)
                seen.add((s, e))
                self._take(s, e, f"{name} block {i} under {m}")
        self.operands.append((name, role, far, near, lands))
        self.landings[name] = lands
        return far, near, lands


# ---- the device part ------------------------------------------------------------------------------------------------------------
class Arena:
    """the one uninitialised uint8 allocation.  A failed allocation is an error with the free-memory figure, never a skip."""

    alive = False   # at most one at a time

    def __init__(self, device):
        import torch
        assert not Arena.alive, "an arena is alive already: free it first"
        self.device = torch.device(device)
        free, total = torch.cuda.mem_get_info(self.device)
        try:
            self.bytes = torch.empty(ARENA_BYTES, dtype=torch.uint8, device=self.device)
        except RuntimeError as e:
            raise RuntimeError(f"the far-offset arena of {ARENA_BYTES} bytes could not be allocated: {free} of {total} bytes were free "
                               f"on {self.device}") from e
        assert self.bytes.data_ptr() % 256 == 0
        Arena.alive = True

    def view(self, p, dtype):
        """the as_strided view of placement ``p``"""
        import torch
        assert p.base % p.esize == 0 and torch.empty((), dtype=dtype).element_size() == p.esize
        lo, hi = p.extent()
        assert 0 <= lo and hi <= ARENA_BYTES
        return torch.as_strided(self.bytes.view(dtype), p.shape, p.strides, p.base // p.esize)

    def free(self):
        import torch
        self.bytes = None
        torch.cuda.empty_cache()
        Arena.alive = False


def shuffled(t, seed):
    """different data of the same type and scale: the values of ``t`` in a seeded order, and where that leaves an element as it was
    (a sparse mask is mostly zeros), the value mirrored inside the tensor's range (min + max - value)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    d = t.flatten()[torch.randperm(t.numel(), generator=g)].view(t.shape)
    return torch.where(d == t, (t.max() + t.min() - t).to(t.dtype), d)


class Session(Plan):
    """A ``Plan`` carried out in an arena: ``input`` lays a host tensor in far and near (and its decoys), ``output`` prepares a far and a
    near output with sentinels, ``check`` compares the outputs bit for bit and looks at every sentinel."""

    def __init__(self, arena, call, kind, which=0, odd=False):
        super().__init__(kind, which, odd)
        self.arena, self.outputs, self.sentinels = arena, [], []
        self.call, self.expect = call, list(CALLS[call])

    def _spec(self, name, shape, esize, role):
        """the next operand of the call's table (what the CPU file checked the geometry of) must be this one -> its dims"""
        assert self.expect, f"{self.call}: the table has no operand left for {name}"
        want = self.expect.pop(0)
        assert want[:3] == (name, tuple(shape), esize) and want[4] == role, f"{self.call}: the table has {want}, the test lays {name} {tuple(shape)}"
        return want[3]

    def _bytes(self, s, e):
        return self.arena.bytes[s:e]

    def input(self, name, t, decoy=None, align=0):
        """``t``: a host tensor in storage order -> (far view, near view) on the device holding its values"""
        import torch
        t = t.contiguous()
        dims = self._spec(name, t.shape, t.element_size(), "in")
        far, near, lands = self.add(name, tuple(t.shape), t.element_size(), dims, "in", align)
        dev_t = t.to(self.arena.device)
        decoy = (shuffled(t, 977 + len(self.operands)) if decoy is None else decoy).to(self.arena.device)
        k = far.dim
        for (_, i, s, e) in lands:   # the decoys first: no landing window overlaps a data window (Plan checked it)
            d = decoy.select(k, i).contiguous()
            assert not torch.equal(d, dev_t.select(k, i)), f"{name}: the decoy of block {i} equals the data"
            self._bytes(s, e).copy_(d.view(-1).view(torch.uint8))
        views = []
        for p in (far, near):
            v = self.arena.view(p, t.dtype)
            v.copy_(dev_t)
            views.append(v)
        for v in views:
            assert torch.equal(v, dev_t), f"{name}: the view does not read back what was laid in"
        return views[0], views[1]

    def output(self, name, shape, dtype, align=0):
        """-> (far view, near view) of an output: sentinels in both, in every landing window and in the guards"""
        import torch
        esize = torch.empty((), dtype=dtype).element_size()
        dims = self._spec(name, shape, esize, "out")
        far, near, lands = self.add(name, tuple(shape), esize, dims, "out", align)
        for (s, e) in far.windows() + [near.extent()]:
            self._bytes(s - GUARD, e + GUARD).fill_(SENTINEL)
            self.sentinels += [(name, s - GUARD, s), (name, e, e + GUARD)]
        for (m, i, s, e) in lands:
            self._bytes(s, e).fill_(SENTINEL)
            self.sentinels.append((f"{name} block {i} under {m}", s, e))
        views = (self.arena.view(far, dtype), self.arena.view(near, dtype))
        self.outputs.append((name, *views))
        return views

    def check(self):
        """every far output bit-equal to its near twin, every sentinel intact"""
        import torch
        assert not self.expect, f"{self.call}: operands of the table were not laid: {self.expect}"
        torch.cuda.synchronize(self.arena.device)
        for (name, far, near) in self.outputs:
            f, n = far.contiguous(), near.contiguous()
            assert torch.equal(f.view(torch.uint8), n.view(torch.uint8)), f"{name}: the far output differs from its near twin"
        for (what, s, e) in self.sentinels:
            assert bool((self._bytes(s, e) == SENTINEL).all()), f"{what}: the sentinel in bytes {s}..{e} was overwritten"


# ---- the calls: what the device tests lay, in the order they lay it (the CPU file checks the geometry of exactly these) -------------
H, W, VN, HN = 40, 56, 9, 64       # the voting layer's smallest shape with more than one 1024-pixel segment (2240 pixels)
BCHW = (0, 1, 2)                   # (batch, planes, rows) of [b,C,h,w]
BHW = (0, None, 1)                 # [b,h,w] and [b,h,w,3]: no channel dimension to move
FIELD_C = (0, 3, 1)                # the contiguous field [b,h,w,vn,2]: the key-point stride is its plane stride
ONE_PLANE = (0, None, 2)           # [b,1,h,w]
PTS = (0, 1, 2)                    # [n,pn,2]: the point stride, then the coordinate stride
PTS_CLASSES = (0, 1, 2)            # [b,nk,pn,2]: the class stride, then the point stride
AH, AW = 37, 53                    # the augmentation's odd source


def _op(name, shape, esize, dims, role="in"):
    return (name, tuple(shape), esize, dims, role)


def _vote(mask_e, field_e, planar, first="mask", first_shape=(2, H, W), first_dims=BHW):
    field = _op("field", (2, 2 * VN, H, W), field_e, BCHW) if planar else _op("field", (2, H, W, VN, 2), field_e, FIELD_C)
    return [_op(first, first_shape, mask_e, first_dims), field]


def _head(pred_e, mask_e, vn=4, nc=3, targets=True, grads=False):
    ops = [_op("seg_pred", (2, nc, H, W), pred_e, BCHW), _op("vertex_pred", (2, 2 * vn, H, W), pred_e, BCHW),
           _op("mask", (2, H, W), mask_e, BHW)]
    if targets:
        ops += [_op("vertex", (2, 2 * vn, H, W), 4, BCHW), _op("vertex_weights", (2, 1, H, W), 4, ONE_PLANE)]
    if grads:
        ops += [_op("grad_seg", (2, nc, H, W), pred_e, BCHW, "out"), _op("grad_vertex", (2, 2 * vn, H, W), pred_e, BCHW, "out")]
    return ops


CALLS = {
    "vote_v3-u8-f32-planar": _vote(1, 4, True),
    "vote_v3-i32-bf16-planar": _vote(4, 2, True),
    "vote_v3-i64-f32-contiguous": _vote(8, 4, False),
    "vote_v3-u8-bf16-contiguous": _vote(1, 2, False),
    "vote_v3_logits-f32": _vote(4, 4, True, "seg_pred", (2, 3, H, W), BCHW),
    "vote_v3_logits-bf16": _vote(2, 2, True, "seg_pred", (2, 3, H, W), BCHW),
    "motion_voting": _vote(1, 4, True),
    "vote_v2-i64": _vote(8, 4, True),
    "vote_v2-u8": _vote(1, 2, True),
    "head_metrics-f32-i64": _head(4, 8),
    "head_metrics-bf16-u8": _head(2, 1),
    "head_grad-f32-i64": _head(4, 8, grads=True),
    "head_grad-bf16-u8": _head(2, 1, grads=True),
    "vertex_targets": [_op("mask", (2, H, W), 8, BHW), _op("vertex", (2, 8, H, W), 4, BCHW, "out"),
                       _op("vertex_weights", (2, 1, H, W), 4, ONE_PLANE, "out")],
    "head_metrics_kp": _head(4, 1, targets=False),
    "head_grad_kp": _head(2, 8, targets=False, grads=True),
    # the augmentation at its 37 x 53 source (w no multiple of 8); the uint8 picture is 1-byte: both distances
    "augment_batch": [_op("rgb", (2, AH, AW, 3), 1, BHW), _op("mask", (2, AH, AW), 4, BHW)],
    "normalize_batch": [_op("rgb", (2, AH, AW, 3), 1, BHW)],
    "jitter_batch": [_op("rgb", (2, AH, AW, 3), 1, BHW), _op("mask", (2, AH, AW), 1, BHW)],
    "augment_jitter_batch": [_op("rgb", (2, AH, AW, 3), 1, BHW), _op("mask", (2, AH, AW), 8, BHW)],
    # the network launches at the narrowest widths of their case tables
    "conv3x3-32-0-32-bf16": [_op("src1", (2, 32, 19, 27), 2, BCHW), _op("residual", (2, 32, 19, 27), 2, BCHW)],
    "conv3x3-64-32-96-f32": [_op("src1", (2, 64, 19, 27), 4, BCHW), _op("src2", (2, 32, 19, 27), 4, BCHW),
                             _op("residual", (2, 96, 19, 27), 4, BCHW)],
    "conv3x3-stride2-f16": [_op("src1", (2, 32, 37, 53), 2, BCHW), _op("residual", (2, 32, 19, 27), 2, BCHW)],
    "fused_stage": [_op("lo", (2, 64, 10, 18), 4, BCHW), _op("skip", (2, 64, 20, 36), 2, BCHW)],
    "fused_stem": [_op("image", (2, 3, 37, 53), 4, BCHW)],
    "fused_stem-bf16": [_op("image", (2, 3, 37, 53), 2, BCHW)],
    "fused_tail": [_op("fm", (2, 32, 20, 28), 2, BCHW), _op("image", (2, 3, 40, 56), 4, BCHW)],
    # the pose solves: the key-points' strides
    "pnp_batch-f32": [_op("points_2d", (2, 9, 2), 4, PTS)],
    "pnp_batch-f64": [_op("points_2d", (2, 9, 2), 8, PTS)],
    "pnp_classes-f32": [_op("points_2d", (2, 3, 9, 2), 4, PTS_CLASSES)],
    "pnp_classes-f64": [_op("points_2d", (2, 3, 9, 2), 8, PTS_CLASSES)],
}


def cases(call):
    """(kind, which, odd) of every placement the device file runs ``call`` under: the three kinds; the second distance where an operand
    of one or two bytes has one; one odd placement of the batch"""
    two = any(e in (1, 2) for (_, _, e, _, _) in CALLS[call])
    out = [(k, w, False) for k in KINDS for w in ((0, 1) if two else (0,))]
    return out + [("far_batch", 0, True)]


def all_cases():
    return [(c, *k) for c in CALLS for k in cases(c)]


def case_id(c):
    call, kind, which, odd = c
    return f"{call}-{kind}-d{which}" + ("-odd" if odd else "")
