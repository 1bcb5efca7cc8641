"""Map / map-reduce front-ends and the device funnel -- mirror of
/root/reference/src/mapreduce.jl:1-117.

Julia's `f!` names become `f_` here (PyTorch's in-place convention).  Every front-end ends in
`_mapreduce_fuse_` -- the reference's single funnel `_mapreduce_fuse!` (src/mapreduce.jl:98) --
which is where this package crosses the C ABI into libstrided_hip.so (`smr_mapreduce`).  All
argument checking happens before the funnel, with the reference's error types
(DimensionMismatch, src/mapreduce.jl:43-46,81); the engine itself never raises for valid input.
"""
from __future__ import annotations

import builtins
import collections
import ctypes as C
import math
import operator
import threading

import numpy as np

from . import _lib as L
from . import expr as E
from .stridedview import DimensionMismatch, StridedView, smr_dtype

_REDOPS = {
    "+": L.SMR_RED_ADD, "add": L.SMR_RED_ADD, "add_sum": L.SMR_RED_ADD, operator.add: L.SMR_RED_ADD,
    "*": L.SMR_RED_MUL, "mul": L.SMR_RED_MUL, "mul_prod": L.SMR_RED_MUL, operator.mul: L.SMR_RED_MUL,
    "min": L.SMR_RED_MIN, min: L.SMR_RED_MIN, "max": L.SMR_RED_MAX, max: L.SMR_RED_MAX,
    "&": L.SMR_RED_AND, "and": L.SMR_RED_AND, operator.and_: L.SMR_RED_AND,
    "|": L.SMR_RED_OR, "or": L.SMR_RED_OR, operator.or_: L.SMR_RED_OR,
}


def _redop_code(op):
    if op is None:
        return L.SMR_RED_NONE
    try:
        if op in _REDOPS:
            return _REDOPS[op]
    except TypeError:
        pass
    name = getattr(op, "__name__", None)
    if name in _REDOPS:
        return _REDOPS[name]
    # _init_reduction!'s last method (src/mapreduce.jl:188-191): unknown reductions are an error
    raise ValueError("unknown reduction; incompatible with the device reduction tree")


def _initop_code(initop):
    """initop -> (smr_initop, beta).  The five forms of test/othertests.jl:76-102 and
    src/linalg.jl:146-160: nothing, identity, zero / x->0, x->x*beta, x->beta, conj."""
    if initop is None:
        return L.SMR_INIT_NONE, 0j
    if isinstance(initop, str):
        table = {"identity": L.SMR_INIT_IDENTITY, "zero": L.SMR_INIT_ZERO, "conj": L.SMR_INIT_CONJ}
        if initop in table:
            return table[initop], 0j
        raise ValueError(f"unknown initop {initop!r}")
    if isinstance(initop, tuple) and len(initop) == 2 and initop[0] in ("scale", "const"):
        return (L.SMR_INIT_SCALE if initop[0] == "scale" else L.SMR_INIT_CONST), complex(initop[1])
    if callable(initop):  # trace x -> ...
        e = E.as_expr(initop(E.Arg(1)))
        if isinstance(e, E.Arg):
            return L.SMR_INIT_IDENTITY, 0j
        if isinstance(e, E.Const):
            return (L.SMR_INIT_ZERO, 0j) if e.value == 0 else (L.SMR_INIT_CONST, e.value)
        if isinstance(e, E.Call) and e.op == "conj" and isinstance(e.args[0], E.Arg):
            return L.SMR_INIT_CONJ, 0j
        if isinstance(e, E.Call) and e.op == "mul" and len(e.args) == 2:
            a, b = e.args
            if isinstance(a, E.Arg) and isinstance(b, E.Const):
                return L.SMR_INIT_SCALE, b.value
            if isinstance(b, E.Arg) and isinstance(a, E.Const):
                return L.SMR_INIT_SCALE, a.value
    raise NotImplementedError("initop outside the device whitelist {identity, zero, x*beta, beta, conj}")


_TORCH_CUR = None


class _StreamStack(threading.local):
    """Per thread (like torch's current stream): the library-owned streams of the enclosing `with S.Stream():` blocks, innermost last."""

    def __init__(self):
        self.stack = []


_STREAM_OVERRIDE = _StreamStack()


def _push_stream(handle: int) -> None:
    _STREAM_OVERRIDE.stack.append(int(handle))


def _pop_stream() -> None:
    _STREAM_OVERRIDE.stack.pop()


def _current_stream() -> int:
    """Raw handle of the stream the front ends launch on: the library-owned stream of an enclosing `with S.Stream():` block, else
    torch's current HIP stream (0 = the null stream when torch / a device is absent)."""
    global _TORCH_CUR
    if _STREAM_OVERRIDE.stack:
        return _STREAM_OVERRIDE.stack[-1]
    if _TORCH_CUR is None:
        try:
            import torch
            _TORCH_CUR = torch.cuda.current_stream if torch.cuda.is_available() else False
        except Exception:
            _TORCH_CUR = False
    if _TORCH_CUR is False:
        return 0
    return int(_TORCH_CUR().cuda_stream)


_FPROG_CACHE: dict = {}


_SCALARS = (int, float, complex, bool, np.generic, type(None))


def _scalar_key(v):
    """(type name, repr) of a captured scalar: `==` would merge 0.0 with -0.0 (and 1 with 1.0 and True), whose programs differ --
    repr tells signed zeros apart, in both parts of a complex too."""
    return (type(v).__name__, repr(v))


def _code_names(code):
    """Global / attribute names read by a code object and by every code object nested in it."""
    names = set(code.co_names)
    for c in code.co_consts:
        if hasattr(c, "co_names"):
            names |= _code_names(c)
    return names


def _closure_key(f):
    """Hashable identity of a plain Python function INCLUDING every value it can read: closure cells, defaults
    and the module globals its code names.  A key is only produced when all of them are immutable scalars (or
    this package's own function table `fn`); a captured callable, object or container can change behind an
    unchanged id() -- `lambda x: g(x) + 1` with a fresh `g` per loop trip, `lambda x: x * cfg.alpha` -- so such
    closures are re-traced on every call (None = do not cache)."""
    code = getattr(f, "__code__", None)
    if code is None or getattr(f, "__self__", None) is not None:
        return None
    cells = ()
    if f.__closure__:
        try:
            cells = tuple(c.cell_contents for c in f.__closure__)
        except ValueError:
            return None
        from . import fn as _fn0
        if not all(isinstance(v, _SCALARS) or v is _fn0 for v in cells):
            return None
        cells = tuple(("module", "fn") if v is _fn0 else _scalar_key(v) for v in cells)
    defaults = f.__defaults__ or ()
    kwdefaults = tuple(sorted((f.__kwdefaults__ or {}).items()))
    if not all(isinstance(v, _SCALARS) for v in defaults) or not all(isinstance(v, _SCALARS) for _, v in kwdefaults):
        return None
    kwdefaults = tuple((k, _scalar_key(v)) for k, v in kwdefaults)
    from . import fn as _fn
    g = f.__globals__
    for n in _code_names(code):
        if n in g and g[n] is not _fn:
            return None  # a module-level scalar, object or function the closure reads: may change between calls
    return (code, cells, tuple(_scalar_key(v) for v in defaults), kwdefaults)


def _serialized(f, M, dts):
    """(code, consts) of f for these operand dtypes.  Tracing a closure and serialising the expression costs
    tens of microseconds of Python -- more than the kernels of a 32^4 problem run -- so the result is kept per
    (closure, captured values, dtypes)."""
    key = None
    if not isinstance(f, E.Expr) and not isinstance(f, str):
        ck = _closure_key(f)
        if ck is not None:
            key = (ck, M, dts)
            try:
                hit = _FPROG_CACHE.get(key)
            except TypeError:  # an unhashable value slipped into the key
                key, hit = None, None
            if hit is not None:
                return hit
    e = E.trace(f, M - 1)
    if E.max_arg(e) > M - 1:
        raise ValueError("f uses more arguments than arrays were given")
    # the library computes the call in the widest float class among ALL operands (csrc/smr_canon.cpp:
    # canonicalise); operations Julia would carry out in Float32 get a ROUND32 when that class is wider
    wide = any(d in (np.dtype(np.float64), np.dtype(np.complex128)) or np.issubdtype(d, np.integer) or d == np.bool_ for d in dts)
    # ... or a strongly typed 64-bit scalar inside f (`A32 .* 0.1`: Julia multiplies in Float64): SMR_OP_WIDEN
    wide = wide or E.needs_wide(e, list(dts[1:]))
    out = E.serialize(e, list(dts[1:]), wide)
    if key is not None:
        if len(_FPROG_CACHE) > 4096:
            _FPROG_CACHE.clear()
        _FPROG_CACHE[key] = out
    return out


def build_problem(f, op, initop, dims, arrays, stream=None):
    """Serialise the funnel's arguments into an `smr_problem` (plus the buffers it points to,
    which the caller must keep alive for the duration of the call)."""
    N, M = len(dims), len(arrays)
    if N == 0:  # 0-dim arrays: one element
        dims = (1,)
        arrays = tuple(StridedView(a.parent, (1,), (1,), a.offset, a.op) for a in arrays)
        N = 1
    if N > L.SMR_MAXN:
        raise L.UnsupportedOnDevice(L.SMR_EUNSUPPORTED, f"rank {N} > {L.SMR_MAXN}")
    if M > L.SMR_MAXM:
        raise L.UnsupportedOnDevice(L.SMR_EUNSUPPORTED, f"{M} operands > {L.SMR_MAXM}")
    dts = [np.dtype(a.dtype) for a in arrays]
    code, consts = _serialized(f, M, tuple(dts))
    p = L.smr_problem()
    p.N, p.M = N, M
    for i, d in enumerate(dims):
        p.dims[i] = int(d)
    for k, a in enumerate(arrays):
        if a.size != tuple(dims):
            raise DimensionMismatch(f"operand {k} has size {a.size}, expected {tuple(dims)}")
        o = p.ops[k]
        o.base = a._base
        o.offset = a.offset
        for i, s in enumerate(a.strides):
            o.strides[i] = int(s)
        o.dtype = smr_dtype(a.dtype)
        o.conj = 1 if a.op == "conj" else 0
    codebuf = (C.c_uint8 * len(code))(*code)
    cflat = []
    for c in consts:
        cflat += [c.real, c.imag]
    constbuf = (C.c_double * max(1, len(cflat)))(*cflat)
    p.fprog = C.cast(codebuf, C.POINTER(C.c_uint8))
    p.fprog_len = len(code) // 2
    p.fconsts = C.cast(constbuf, C.POINTER(C.c_double))
    p.nconsts = len(consts)
    p.redop = _redop_code(op)
    ic, beta = _initop_code(initop)
    p.initop = ic
    p.initarg[0], p.initarg[1] = beta.real, beta.imag
    p.stream = stream if stream is not None else _current_stream()
    return p, (codebuf, constbuf, arrays)


_PROBLEM_CACHE: "collections.OrderedDict" = collections.OrderedDict()  # least recently used first
_SMR_MAPREDUCE = None


def _problem_key(f, op, initop, dims, arrays):
    """Hashable identity of a whole funnel call (function incl. captured values, operators, box, every operand's
    address / layout / type), or None.  Filling the ~700-byte C struct field by field costs ~10 us of Python per
    call -- more than the kernels of a 32^4 problem -- so a repeated call (a loop over fixed arrays) reuses the
    struct it built the first time."""
    if isinstance(f, str):
        fk = f
    elif isinstance(f, E.Expr):
        return None
    else:
        fk = _closure_key(f)
        if fk is None:
            return None
    if not (op is None or isinstance(op, str)):
        return None
    if not (initop is None or isinstance(initop, (str, tuple))):
        return None
    try:
        return (fk, op, initop, tuple(dims), tuple((a._base, a.offset, a.size, a.strides, a.dtype.str, a.op) for a in arrays))
    except AttributeError:
        return None


def _mapreduce_fuse_(f, op, initop, dims, arrays):
    """`_mapreduce_fuse!(f, op, initop, dims, arrays)` (src/mapreduce.jl:98-117): the drop-in
    boundary.  arrays[0] is the destination; all operands already share `dims` (broadcast /
    reduced dims have stride 0); no dim is 0.  Runs asynchronously on the current HIP stream."""
    global _SMR_MAPREDUCE
    for a in arrays:
        if not a.on_device:
            raise RuntimeError(
                "strided_jl_amd computes on MI355X only: every StridedView must wrap a torch tensor on a "
                "HIP device (host views are for the test oracle; there is no CPU fallback)")
    g = _GROUP.cur
    if g is not None:  # inside `with S.group():` -- maps are deferred, anything else runs after what is pending
        if op is None and g.defer(f, dims, arrays):
            return arrays[0]
        if op is not None and g.contract and g.defer(f, dims, arrays, op, initop):  # a contraction: S.group(contract=True)
            return arrays[0]
        if op is not None and g.reduce and g.defer(f, dims, arrays, op, initop, complete=True):  # a complete reduction: S.group(reduce=True)
            return arrays[0]
        if op is not None and g.reduce_part and g.defer(f, dims, arrays, op, initop, part=True):  # any other reduction: S.group(reduce=True, reduce_part=True)
            return arrays[0]
        g.flush()
    if _SMR_MAPREDUCE is None:
        _SMR_MAPREDUCE = L.load().smr_mapreduce
    key = _problem_key(f, op, initop, dims, arrays)
    hit = None
    if key is not None:
        try:
            hit = _PROBLEM_CACHE.get(key)
        except TypeError:
            key = None
    if hit is not None:
        # a private copy per call: ctypes releases the GIL inside smr_mapreduce, so two threads issuing the same keyed call on
        # different streams must not share the struct whose `stream` field they set; the pointers inside (program,
        # constants) stay owned by the cache entry
        p = L.smr_problem()
        C.memmove(C.byref(p), C.byref(hit[0]), C.sizeof(L.smr_problem))
        p.stream = _current_stream()
        try:
            _PROBLEM_CACHE.move_to_end(key)
        except KeyError:  # evicted by another thread in between: `hit` keeps the buffers alive for this call
            pass
    else:
        p, keep = build_problem(f, op, initop, dims, arrays)
        if key is not None:
            # the operand parents are NOT kept alive by the cache entry: the key holds their addresses, and a new
            # array at a recycled address with the same layout and type is the same problem
            _PROBLEM_CACHE[key] = hit = (p, keep[:2])
            while len(_PROBLEM_CACHE) > 1024:  # least recently used first; no wholesale clear in the hot path
                try:
                    _PROBLEM_CACHE.popitem(last=False)
                except KeyError:
                    break
    L.check(_SMR_MAPREDUCE(C.byref(p)))
    return arrays[0]


# ---- grouped launches: `with S.group():` ------------------------------------------------------------------
class _GroupState(threading.local):
    """Per thread: the innermost enclosing `with S.group():` block (None outside one)."""

    def __init__(self):
        self.cur = None


_GROUP = _GroupState()
_GROUP_CACHE: "collections.OrderedDict" = collections.OrderedDict()  # built groups by (member keys, independent, member_scalars -- "contract_scalars" for a contraction bucket under that keyword --, stream, the kind: (forced contraction tile, group_contract_split), "reduce", "reduce_part", or 0 for maps); least recently used first


def _byte_range(a):
    """[lo, hi) in bytes of the bounding range of a view (what the library compares: csrc/smr_group.h operand_span)."""
    lo = hi = a.offset
    for d, st in zip(a.size, a.strides):
        e = (d - 1) * st
        if e < 0:
            lo += e
        else:
            hi += e
    isz = a.dtype.itemsize
    return a._base + lo * isz, a._base + (hi + 1) * isz


def _view_id(a):
    return (a._base, a.offset, a.size, a.strides)


def _member_bytes(arrays):
    """Algorithmic bytes of one call the way the library counts them (every distinct buffer once, csrc/smr_canon.cpp)."""
    foot = {}
    for a in arrays:
        n = 1
        for d, st in zip(a.size, a.strides):
            if st != 0:
                n *= d
        foot[a._base] = max(foot.get(a._base, 0), n * a.dtype.itemsize)
    return builtins.sum(foot.values())  # (this module defines its own `sum`)


def _integer_valued(v) -> bool:
    """Does the integer class take this constant (csrc/smr_canon.cpp: integer-valued within Int64, or an infinite seed)?"""
    v = complex(v)
    if v.imag != 0:
        return False
    r = v.real
    return math.isinf(r) or (r == math.floor(r) and abs(r) <= 9223372036854775808.0) if not math.isnan(r) else False


def _contract_shaped(dims, arrays) -> bool:
    """Host-side mirror of the library's shape rule for a member of a contraction group (csrc/smr_plan_contract.cpp:
    contract_shape, on the canonical problem): exactly three arrays (destination, input 1, input 2); a kept dim (the destination
    varies along it) of extent > 1 along which only input 1 varies and another along which only input 2 varies; both inputs vary
    along the inner reduced dim -- of the dims of extent > 1 the destination does not vary along, the one with the smallest input
    stride, which is the one the kernel walks in chunks; no input on the destination's base; and algorithmic bytes within option
    "group_max_bytes"."""
    if len(arrays) != 3 or len(dims) > L.SMR_MAXN:
        return False
    c, a, b = arrays
    if a._base == c._base or b._base == c._base:
        return False
    only_a = only_b = False
    inner, inner_key = None, None
    for d, n in enumerate(dims):
        if n <= 1:
            continue
        sc, sa, sb = c.strides[d], a.strides[d], b.strides[d]
        if sc != 0:
            only_a = only_a or (sa != 0 and sb == 0)
            only_b = only_b or (sb != 0 and sa == 0)
        else:
            key = min([abs(x) for x in (sa, sb) if x != 0] or [1 << 63])
            if inner is None or key < inner_key:  # (a stable sort: the first of equal strides)
                inner, inner_key = d, key
    if not (only_a and only_b) or inner is None:
        return False
    if a.strides[inner] == 0 or b.strides[inner] == 0:
        return False
    return _member_bytes(arrays) <= L.get_option("group_max_bytes")


def _complete_reduction(dims, arrays) -> bool:
    """Is the call a member of a reduction group: its destination has one element (stride 0 or extent 1 along every dim), and its
    algorithmic bytes are within option "group_max_bytes"?"""
    dest = arrays[0]
    if any(n != 1 and st != 0 for n, st in zip(dims, dest.strides)):
        return False
    return _member_bytes(arrays) <= L.get_option("group_max_bytes")


class _Deferred:
    __slots__ = ("f", "dims", "arrays", "stream", "bucket", "wr", "rd", "key", "op", "initop", "kind")


class group:
    """`with S.group(independent=False, member_scalars=False, contract=False, reduce=False, contract_scalars=False, reduce_part=False) as g:` -- grouped launches.  Inside the block the map front ends (`copy_`, `permutedims_`,
    `map_`, broadcast `copyto_`, `axpby_`, ...) do not launch: eligible calls are deferred and, at the end of the block or at
    `g.flush()`, every bucket of calls with the same (f-program, operand dtypes, operand count, conj flags, repeated inputs, stream) becomes ONE
    kernel launch (L.Group / smr_group_*).  A block never changes results, only launch counts:
      * a call whose byte ranges conflict with a pending call (it writes what one reads or writes, or reads what one writes) first
        flushes everything pending.  With `independent=True` only exact same-view conflicts count -- the caller asserts that
        different views share no element, which is what lets interleaved blocks of one parent array share a launch;
      * reductions (but see `contract`), members above option "group_max_bytes" and host reads (`toarray`, `item`, `Array`) flush what is pending and
        then run as usual;
      * a bucket the library refuses as a group (smr_group_create: SMR_EUNSUPPORTED) runs call by call through the normal path;
        an error a single call would have raised at once is raised at the flush instead.
    `member_scalars=True` (SMR_GROUP_MEMBER_SCALARS): the VALUES of f's captured scalars leave the bucket key, so that
    `axpby_(a_i, X_i, b_i, Y_i)` with a coefficient per block is one launch; every member still computes with its own scalars.
    What the values decide in the library stays in the key: how many constants there are, whether any has an imaginary part and
    whether all are integer-valued (the compute class).  Equal captured values are ONE constant of the f-program (expr.py merges
    them): `a*X + a*Y` is another program than `a*X + b*Y`, and the `linalg` fronts choose another f for alpha = 1 and for
    beta = 0 or 1 -- such calls land in buckets of their own, correctly.
    `contract=True` (contraction groups): reductions of the outer-product shape -- `mul_(C, A, B, alpha, beta)` on matrices, and
    every `_mapreducedim_` shaped like it (`_contract_shaped`) -- are deferred as well and every bucket of them becomes ONE launch
    of the grouped CONTRACT kernel (csrc/smr_k_gcontract.hip).  Their bucket key also holds the reduction's op, the kind of initop
    (zero / none / scale / const / ...: beta = 0, 1 and any other beta are three kinds) and the values of f's captured scalars (alpha)
    -- those always, whatever `member_scalars` says: a contraction group has one f.  beta itself is per member.  Each result is
    bit-identical to the single call's under option "contract" = 2.  Option "group_contract_split" (0 never, 1 the group rule, N >= 2
    slices per member) is read when a bucket is built, like "group_contract_tile": a bucket with split members is TWO launches (the
    members' slices into partials the group owns, then the fold), and a split member is bit-identical to the single call under
    "contract" = 2, "contract_tile" = the group's tile, "contract_split" = its slices.  Without `contract=True` a reduction flushes and runs as usual.
    `contract_scalars=True` (needs `contract=True`; SMR_GROUP_CONTRACT_SCALARS): the VALUES of a contraction's captured scalars leave its
    bucket key, which keeps what `member_scalars` keeps for maps (how many, any imaginary part, all integer-valued): `mul_(C_i, A_i, B_i,
    alpha_i, beta_i)` with a coefficient per block is ONE launch (describe(): f=mul2scale scalars=member), each block bit-identical to
    the single call with its own alpha under "contract" = 2.  alpha = 1 is another f (x * y) and stays in a bucket of its own, alpha = 0
    is a map; maps and complete reductions bucket as without it.
    `reduce=True` (reduction groups): COMPLETE reductions -- `mapreducedim_(f, op, out1, A, B...)` / `_mapreducedim_` with an initop
    into a destination of ONE element, such as element i of a K-vector reshaped to all-ones dims -- within "group_max_bytes" are
    deferred as well, and every bucket of them becomes ONE launch of csrc/smr_k_greduce.hip (L.Group(reduce=True)).  The contraction
    test comes first when `contract=True` is also set.  Their bucket key also holds ("reduce", the op, the kind of initop) and the
    values of f's captured scalars (always: a reduction group has one f); beta is per member.  Each result is bit-identical to the
    single call's under option "reduce_blocks" = 64 where that call runs family REDUCE_ALL (include/strided_hip.h).
    `S.mapreduce(f, op, A)` without `dims` returns a host scalar: like every host read it still flushes, and is never deferred.
    `reduce=True, reduce_part=True` (partial reduction groups): every OTHER reduction with an op into an array destination -- one that
    keeps dims: `mapreducedim_` into a vector of row sums, a matrix-vector product, `sum(A; dims=2)` -- within "group_max_bytes" is
    deferred as well, after the contraction test (under `contract=True`) and the complete-reduction test, which keep their own buckets
    and kinds; every bucket of them becomes ONE launch of csrc/smr_k_greduce_part.hip (L.Group(reduce=True, reduce_part=True)).  The
    bucket key holds ("reduce_part", the op, the kind of initop) and the values of f's captured scalars; beta and the kept dims are per
    member.  Each result is bit-identical to the single call's under option "reduce_part_kind" = 0 where that call reads "form=general
    ... split=1" (include/strided_hip.h).  Destinations that interleave in memory (the columns of one matrix) have intersecting
    bounding ranges: the block then flushes between them unless `independent=True` asserts that no element is shared.  `reduce_part`
    without `reduce` is a ValueError; with `reduce=True` alone no partial reduction is deferred.
    `g.groups` lists the L.Group of every group launch of the block so far; `g.singles` counts calls that took the normal path."""

    MAX_PENDING = 4096

    def __init__(self, independent: bool = False, member_scalars: bool = False, contract: bool = False, reduce: bool = False,
                 contract_scalars: bool = False, reduce_part: bool = False):
        if reduce_part and not reduce:
            raise ValueError("S.group(reduce_part=True) needs reduce=True: the flag turns reduction groups into partial reduction groups")
        self.reduce_part = bool(reduce_part)
        if contract_scalars and not contract:
            raise ValueError("S.group(contract_scalars=True) needs contract=True: the flag is for contraction groups")
        self.contract_scalars = bool(contract_scalars)
        self.independent = bool(independent)
        self.member_scalars = bool(member_scalars)
        self.contract = bool(contract)
        self.reduce = bool(reduce)
        self.pending = []
        self.groups = []
        self.singles = 0
        self._outer = None

    def __enter__(self):
        self._outer = _GROUP.cur
        if self._outer is not None:
            self._outer.flush()
        _GROUP.cur = self
        return self

    def __exit__(self, *exc):
        try:
            self.flush()
        finally:
            _GROUP.cur = self._outer
        return False

    # -- deferring ------------------------------------------------------------------------------------------
    def _conflicts(self, c):
        if self.independent:
            w = _view_id(c.arrays[0])
            for q in self.pending:
                ids = [_view_id(a) for a in q.arrays]
                if w in ids or ids[0] in [_view_id(a) for a in c.arrays[1:]]:
                    return True
            return False
        for q in self.pending:
            for lo, hi in [q.wr] + q.rd:
                if c.wr[0] < hi and lo < c.wr[1]:
                    return True
            for lo, hi in c.rd:
                if lo < q.wr[1] and q.wr[0] < hi:
                    return True
        return False

    def defer(self, f, dims, arrays, op=None, initop=None, complete=False, part=False) -> bool:
        """Takes one map call (destination first), or with `op` one reduction of the contraction shape -- with `complete` one
        complete reduction (a reduction group's member), with `part` any reduction (a partial reduction group's member) instead.  False: the call is not
        eligible (too large, too many operands, a reduction of another shape) -- the caller flushes and runs it through the normal
        path."""
        arrays = tuple(arrays)
        if len(arrays) < 2 or len(arrays) > L.SMR_MAXM or len(dims) > L.SMR_MAXN:
            return False
        if op is not None:
            if part:
                if _member_bytes(arrays) > L.get_option("group_max_bytes"):
                    return False
            elif not (_complete_reduction(dims, arrays) if complete else _contract_shaped(dims, arrays)):
                return False
        elif _member_bytes(arrays) > L.get_option("group_max_bytes"):
            return False
        c = _Deferred()
        c.f, c.dims, c.arrays = f, tuple(int(d) for d in dims), arrays
        c.op, c.initop = op, initop
        c.kind = "map" if op is None else ("reduce_part" if part else ("reduce" if complete else "contract"))
        c.stream = _current_stream()
        dts = tuple(np.dtype(a.dtype) for a in arrays)
        code, consts = _serialized(f, len(arrays), dts)
        # inputs that are one operand to the library (csrc/smr_canon.cpp dedupes identical inputs): calls that differ in this pattern run
        # another kernel signature, and one bucket of them would be refused as a group
        ops = [(a._base, a.offset, a.op, tuple(st for d, st in zip(c.dims, a.strides) if d != 1)) for a in arrays[1:]]
        same = tuple(ops.index(o) for o in ops)
        # what the constants contribute.  A contraction group has one f: their values, whatever member_scalars says.  Under
        # member_scalars a map contributes only what they decide in canonicalise(): count, complex or not, integer class or not
        # (contract_scalars: the same for a contraction, whose group then holds a row of constants per member)
        if (self.member_scalars and op is None) or (self.contract_scalars and op is not None and not complete and not part):
            ck = (len(consts), any(v.imag != 0 for v in consts), all(_integer_valued(v) for v in consts))
        else:
            ck = tuple(consts)
        # a bucket of contractions also has one op and one kind of initop; beta is the member's
        # (so has a bucket of complete reductions)
        tail = () if op is None else (c.kind, _redop_code(op), _initop_code(initop)[0])
        c.bucket = (bytes(code), ck, tuple(d.str for d in dts), len(arrays), tuple(a.op for a in arrays), same, c.stream) + tail
        c.wr = _byte_range(arrays[0])  # (a reduction also reads its destination: a write range conflicts with everything a read does)
        c.rd = [_byte_range(a) for a in arrays[1:]]
        c.key = _problem_key(f, op, initop, c.dims, arrays)
        if self.pending and (len(self.pending) >= self.MAX_PENDING or self._conflicts(c)):
            self.flush()
        self.pending.append(c)
        return True

    # -- launching --------------------------------------------------------------------------------------------
    def flush(self):
        """Launches everything pending: one group per bucket, buckets in order of their first call."""
        calls, self.pending = self.pending, []
        buckets = {}
        for c in calls:
            buckets.setdefault(c.bucket, []).append(c)
        for members in buckets.values():
            self._launch(members, members[0].stream)

    def _launch(self, calls, stream):
        # a bucket of contractions: the library is not passed member_scalars, and plans under the forced tile and the split option
        part = calls[0].kind == "reduce_part"
        reduce = part or calls[0].kind == "reduce"
        if reduce:  # a bucket of complete (partial) reductions: no member_scalars either; nothing an option decides at creation
            scalars, plan_opts = False, calls[0].kind
        elif calls[0].op is not None:
            scalars, plan_opts = False, (L.get_option("group_contract_tile"), L.get_option("group_contract_split"))
        else:
            scalars, plan_opts = self.member_scalars, 0
        # contract_scalars: passed for contraction buckets only, and part of the cached group's key (in the slot of member_scalars)
        cscalars = self.contract_scalars and not reduce and calls[0].op is not None
        key = None
        if all(c.key is not None for c in calls):
            key = (tuple(c.key for c in calls), self.independent, "contract_scalars" if cscalars else scalars, stream, plan_opts)
        grp = None
        if key is not None:
            try:
                grp = _GROUP_CACHE.get(key)
            except TypeError:
                key = None
        if grp is None:
            built = [build_problem(c.f, c.op, c.initop, c.dims, c.arrays, stream=stream) for c in calls]
            try:
                # (like _PROBLEM_CACHE, a cached group does not keep the operand parents alive: its key holds their addresses)
                grp = L.Group([b[0] for b in built], self.independent, keepalive=[b[1][:2] for b in built], member_scalars=scalars,
                              **({"reduce": True, "reduce_part": True} if part else {"reduce": True} if reduce else ({"contract_scalars": True} if cscalars else {})))   # (the other kinds are created exactly as before)
            except L.UnsupportedOnDevice:
                for c in calls:
                    self._single(c)
                return
            if key is not None:
                _GROUP_CACHE[key] = grp
                while len(_GROUP_CACHE) > 256:
                    try:
                        _GROUP_CACHE.popitem(last=False)
                    except KeyError:
                        break
        else:
            try:
                _GROUP_CACHE.move_to_end(key)
            except KeyError:
                pass
        grp.execute(stream)
        self.groups.append(grp)

    def _single(self, c):
        cur, _GROUP.cur = _GROUP.cur, None
        try:
            self.singles += 1
            if c.stream != _current_stream():
                p, keep = build_problem(c.f, c.op, c.initop, c.dims, c.arrays, stream=c.stream)
                L.check(L.load().smr_mapreduce(C.byref(p)))
            else:
                _mapreduce_fuse_(c.f, c.op, c.initop, c.dims, c.arrays)
        finally:
            _GROUP.cur = cur


def flush_group():
    """Launches what the enclosing `with S.group():` block (if any) has pending: called before the host reads device memory."""
    g = _GROUP.cur
    if g is not None:
        g.flush()


def make_plan(f, op, initop, dims, arrays) -> L.Plan:
    """Planned form of the funnel (smr_plan_create): canonicalise + choose the kernel once."""
    p, keep = build_problem(f, op, initop, dims, arrays)
    return L.Plan(p, keep)


# ---- methods based on map! (src/mapreduce.jl:1-14) --------------------------------------------------
def copy_(dst: StridedView, src: StridedView) -> StridedView:
    """`Base.copy!(dst, src)` = map!(identity, dst, src)."""
    return map_(lambda x: x, dst, src)


def conj_(a: StridedView) -> StridedView:
    """`Base.conj!`: no-op for real eltypes (src/mapreduce.jl:5-6)."""
    if not np.issubdtype(a.dtype, np.complexfloating):
        return a
    from . import fn
    return map_(fn.conj, a, a)


def adjoint_(dst: StridedView, src: StridedView) -> StridedView:
    """`LinearAlgebra.adjoint!(dst, src)` = copy!(dst, adjoint(src)) (src/mapreduce.jl:7-10)."""
    return copy_(dst, src.adjoint())


def transpose_(dst: StridedView, src: StridedView) -> StridedView:
    return copy_(dst, src.transpose())


def permutedims_(dst: StridedView, src: StridedView, p) -> StridedView:
    """`Base.permutedims!(dst, src, p)` = copy!(dst, permutedims(src, p)) (src/mapreduce.jl:11-14).
    `p` is 0-based."""
    return copy_(dst, src.permutedims(p))


def copy(a: StridedView) -> StridedView:
    return copy_(a.similar(), a)


def map(f, a1: StridedView, *A: StridedView) -> StridedView:  # noqa: A001
    """`Base.map(f, a1, A...)`: allocates `similar(a1, promote_eltype)` (src/mapreduce.jl:32-36)."""
    e = E.trace(f, 1 + len(A))
    T = E.result_dtype(e, [a1.dtype] + [a.dtype for a in A])
    return map_(e, a1.similar(T), a1, *A)


def map_(f, b: StridedView, a1: StridedView, *A: StridedView) -> StridedView:
    """`Base.map!(f, b, a1, A...)` (src/mapreduce.jl:38-53)."""
    dims = b.size
    if a1.size != dims:
        raise DimensionMismatch()
    for a in A:
        if a.size != dims:
            raise DimensionMismatch()
    if any(d == 0 for d in dims):
        return b  # don't do anything
    _mapreduce_fuse_(f, None, None, dims, (b, a1) + tuple(A))
    return b


# ---- reductions (src/mapreduce.jl:16-30, 55-96) -----------------------------------------------------
def _neutral(op, dtype):
    """_init_reduction! (src/mapreduce.jl:182-187).  For min/max the reference fills with the first
    mapped element; on the device that would cost a device->host read, so the typed
    +inf / -inf is used -- the same result for every non-NaN input."""
    code = _redop_code(op)
    if code == L.SMR_RED_ADD:
        return 0
    if code in (L.SMR_RED_MUL, L.SMR_RED_AND):
        return 1  # one / true (src/mapreduce.jl:185,188)
    if code == L.SMR_RED_OR:
        return 0  # false (:189)
    if np.issubdtype(dtype, np.integer):
        info = np.iinfo(dtype)
        return info.max if code == L.SMR_RED_MIN else info.min
    return np.inf if code == L.SMR_RED_MIN else -np.inf


def _fill_(out: StridedView, value):
    from .broadcast import copyto_
    return copyto_(out, value)


def _reduced_dtype(e, op, A):
    T = E.result_dtype(e, [A.dtype])
    if T == np.bool_ or (np.issubdtype(T, np.integer) and T.itemsize < 8):
        # Base.add_sum / mul_prod widen Bool and small signed ints to Int, small unsigned ints to UInt
        # (src/mapreduce.jl:62-64 via Base.mapreduce_first)
        if _redop_code(op) in (L.SMR_RED_ADD, L.SMR_RED_MUL):
            T = np.dtype(np.uint64) if T.kind == "u" else np.dtype(np.int64)
    if _redop_code(op) in (L.SMR_RED_AND, L.SMR_RED_OR):
        T = np.dtype(np.bool_)
    return T


def _mapreduce(f, op, A: StridedView, init=None):
    """Complete reduction (src/mapreduce.jl:55-72): a 1-element `out` pre-filled with the neutral
    element (or `init`), reshaped to all-ones dims, accumulated into by the engine."""
    e = E.trace(f, 1)
    if len(A) == 0 or any(d == 0 for d in A.size):
        # Base.mapreduce_empty: defined for +, * (zero / one); min/max of an empty collection throw
        code = _redop_code(op)
        if code in (L.SMR_RED_MIN, L.SMR_RED_MAX) and init is None:
            raise ValueError("reducing over an empty collection is not allowed")
        b = _neutral(op, _reduced_dtype(e, op, A))
        return b if init is None else {L.SMR_RED_ADD: b + init, L.SMR_RED_MUL: b * init}.get(code, init)
    T = _reduced_dtype(e, op, A)
    if init is not None:
        T = np.result_type(T, np.asarray(init).dtype) if not isinstance(init, (int, bool)) else T
    out = A.similar(T, (1,))
    _fill_(out, _neutral(op, T) if init is None else init)
    dims = A.size
    _mapreducedim_(e, op, None, dims, (out.sreshape((1,) * len(dims)), A))
    return out.item()


def mapreduce(f, op, A: StridedView, dims=None, init=None):
    """`Base.mapreduce(f, op, A::StridedView; dims=:, init)` (src/mapreduce.jl:16-30).  Without `dims` the result is a host scalar:
    inside `with S.group(reduce=True):` that read flushes what is pending like every host read, so such a call is never grouped with
    others (use `mapreducedim_` into the elements of a device vector for that)."""
    if dims is None:
        return _mapreduce(f, op, A, init)
    if isinstance(dims, int):
        dims = (dims,)
    e = E.trace(f, 1)
    T = _reduced_dtype(e, op, A)
    outsize = tuple(1 if d in dims else n for d, n in enumerate(A.size))
    b = A.similar(T, outsize)  # Base.reducedim_init / reducedim_initarray
    _fill_(b, _neutral(op, T) if init is None else init)
    return mapreducedim_(e, op, b, A)


def mapreducedim_(f, op, b: StridedView, a1: StridedView, *A: StridedView) -> StridedView:
    """`Base.mapreducedim!(f, op, b, a1, A...)` (src/mapreduce.jl:74-84): accumulates INTO b."""
    arrs = (a1,) + tuple(A)
    N = b.ndim
    if any(a.ndim != N for a in arrs):
        raise DimensionMismatch("all arrays must have the same rank")
    dims = tuple(max([b.size[d]] + [a.size[d] for a in arrs]) for d in range(N))
    for x in (b,) + arrs:  # Broadcast.check_broadcast_axes
        for d in range(N):
            if x.size[d] != dims[d] and x.size[d] != 1:
                raise DimensionMismatch("array could not be broadcast to match destination")
    return _mapreducedim_(f, op, None, dims, (b,) + arrs)


def _mapreducedim_(f, op, initop, dims, arrays):
    """`_mapreducedim!` (src/mapreduce.jl:86-96): zero-size rule + promoteshape, then the funnel."""
    from .broadcast import promoteshape
    dims = tuple(int(d) for d in dims)
    if any(d == 0 for d in dims):
        if len(arrays[0]) != 0 and initop is not None:
            code, beta = _initop_code(initop)
            from . import fn
            table = {
                L.SMR_INIT_IDENTITY: lambda x: x, L.SMR_INIT_ZERO: lambda x: x * 0,
                L.SMR_INIT_SCALE: lambda x: x * beta, L.SMR_INIT_CONJ: fn.conj,
            }
            if code == L.SMR_INIT_CONST:
                _fill_(arrays[0], beta if beta.imag else beta.real)
            else:
                map_(table[code], arrays[0], arrays[0])
    else:
        _mapreduce_fuse_(f, op, initop, dims, promoteshape(dims, *arrays))
    return arrays[0]


def sum(A: StridedView, dims=None, f=None):  # noqa: A001
    return mapreduce(f or (lambda x: x), "+", A, dims=dims)


def prod(A: StridedView, dims=None, f=None):
    return mapreduce(f or (lambda x: x), "*", A, dims=dims)


def maximum(A: StridedView, dims=None, f=None):
    return mapreduce(f or (lambda x: x), "max", A, dims=dims)


def minimum(A: StridedView, dims=None, f=None):
    return mapreduce(f or (lambda x: x), "min", A, dims=dims)


# ---- conversion (src/convert.jl:1-17) -----------------------------------------------------------------
def Array(a: StridedView, dtype=None) -> np.ndarray:
    """`Array(a::StridedView)`: allocate dense + copy! (src/convert.jl).  On the device this is
    a strided gather into a contiguous staging buffer followed by ONE device->host copy; the
    result is a column-major NumPy array."""
    if not a.on_device:
        return np.asfortranarray(a.toarray().astype(dtype or a.dtype, copy=False))
    b = a.similar(dtype or a.dtype)
    if len(a) > 0:
        copy_(b, a)
    flush_group()
    host = b.parent.cpu().numpy()
    return host.reshape(a.size, order="F")
