"""Linear-algebra fronts -- mirror of /root/reference/src/linalg.jl.

The scalar / BLAS-1 fronts (src/linalg.jl:2-42) are broadcast callers and land on the natively
compiled functors (scale, axpy, axpby).  Matrix multiplication: the reference routes BLAS
floats to `gemm!` -- a dense contraction, out of scope for this path -- and
everything else to the generic `__mul!` (src/linalg.jl:130-162), which is a 3-operand
map-reduce with `initop`; that form is implemented here for every device element type and runs
as the LDS- and register-tiled CONTRACT kernel family (csrc/smr_k_contract.hip) when the problem is
large enough -- `S.set_option("contract", 0 | 1 | 2)`: never / by size (default) / wherever the
shape qualifies.  Each output is accumulated by one lane over k ascending: for real floats the
result is bit-identical to the sequential loop.
`S.set_option("contract_split", 0 | 1 | N)` (default 0: never) lets the family cut a long reduced
range into slices, one workgroup per (output tile, slice), folded by a second launch in slice
order: 1 = by the planner's rule (few output tiles, long k: `mul_` at (64, 64, 4096) and the like),
N >= 2 = N slices wherever the family plans (tests, measurements).  The order is defined --
dest = op(initop(old), ((P_0 op P_1) op P_2) ...), P_s the sequential accumulation over slice s --
and run-to-run identical, but it is not the unsplit loop's: hence opt-in.
`S.set_option("contract_tile", 0 | 16 | 32 | 64)` forces the tile of single calls (0: the rule).
Many small products (the blocks of a block-sparse contraction) share ONE launch inside
`with S.group(contract=True):` -- calls of `mul_` on matrices with the same alpha and the same kind of
beta (0, 1, or anything else; the value is per call) are deferred and run as a contraction group
(csrc/smr_k_gcontract.hip), each result bit-identical to the single call under "contract" = 2.
`with S.group(contract=True, contract_scalars=True):` also puts calls that differ in alpha into one launch -- a coefficient per
block: the group keeps a row of f's constants per member (SMR_GROUP_CONTRACT_SCALARS, f=mul2scale natively compiled) and every block
is still bit-identical to the single call with its own alpha.  alpha = 1 lowers to another f (x * y) and stays in a bucket of its
own; alpha = 0 is a map.
`S.set_option("group_contract_split", 0 | 1 | N)` (default 0: never) is "contract_split" for those groups: a few blocks with small
open legs and a very long contracted leg (an environment or projection step) get slices of that leg as workgroups of the one
launch, and a second launch folds them in slice order (1 = the group rule, N >= 2 = N slices per member, clamped to its chunks).
A split member is bit-identical to the single call under "contract" = 2, "contract_tile" = the group's tile and
"contract_split" = its slices; the partials belong to the group (one buffer: not on two streams at once).
"""
from __future__ import annotations

from .mapreduce import _mapreducedim_, copy_
from .stridedview import DimensionMismatch, StridedView


def rmul_(dst: StridedView, alpha) -> StridedView:
    """`rmul!(dst, alpha)` = mul!(dst, dst, alpha) (src/linalg.jl:2)."""
    return mul_(dst, dst, alpha)


def lmul_(alpha, dst: StridedView) -> StridedView:
    """`lmul!(alpha, dst)` = mul!(dst, alpha, dst) (src/linalg.jl:3)."""
    return mul_(dst, alpha, dst)


def mul_(dst: StridedView, a, b, alpha=1, beta=0) -> StridedView:
    """`mul!`: scalar forms (src/linalg.jl:5-22) or matrix product C = alpha*A*B + beta*C."""
    if isinstance(a, StridedView) and isinstance(b, StridedView):
        return _matmul_(dst, a, b, alpha, beta)
    if isinstance(b, StridedView):  # mul!(dst, alpha, src)
        alpha_, src = a, b
        if alpha_ == 1:
            return copy_(dst, src)
        return dst.assign(alpha_ * src)
    src, alpha_ = a, b  # mul!(dst, src, alpha)
    if alpha_ == 1:
        return copy_(dst, src)
    return dst.assign(src * alpha_)


def axpy_(a, X: StridedView, Y: StridedView) -> StridedView:
    """`axpy!(a, X, Y)`: Y .= a .* X .+ Y (src/linalg.jl:23-31)."""
    if a == 1:
        return Y.assign(X + Y)
    return Y.assign(a * X + Y)


def axpby_(a, X: StridedView, b, Y: StridedView) -> StridedView:
    """`axpby!(a, X, b, Y)` (src/linalg.jl:32-42)."""
    if b == 1:
        return axpy_(a, X, Y)
    if b == 0:
        return mul_(Y, a, X)
    return Y.assign(a * X + b * Y)


def _matmul_(C: StridedView, A: StridedView, B: StridedView, alpha=1, beta=0) -> StridedView:
    """`__mul!` (src/linalg.jl:130-162): C2=(m,n,1), A2=(m,1,k), B2=(1,n,k) views and one
    `_mapreducedim!(f, +, initop, (m,n,k), (C2, A2, B2))`."""
    if C.ndim != 2 or A.ndim != 2 or B.ndim != 2:
        raise DimensionMismatch("mul_ needs matrices")
    if not (C.size[0] == A.size[0] and C.size[1] == B.size[1] and A.size[1] == B.size[0]):
        raise DimensionMismatch(f"A has size {A.size}, B has size {B.size}, C has size {C.size}")
    m, n = C.size
    k = A.size[1]
    A2 = StridedView(A.parent, (m, 1, k), (A.strides[0], 0, A.strides[1]), A.offset, A.op)
    Bt = B.permutedims((1, 0))
    B2 = StridedView(B.parent, (1, n, k), (0, Bt.strides[0], Bt.strides[1]), B.offset, B.op)
    C2 = StridedView(C.parent, (m, n, 1), (C.strides[0], C.strides[1], 0), C.offset, C.op)
    if alpha == 0 or k == 0:
        return rmul_(C, beta)
    if beta == 0:
        initop = "zero"
    elif beta == 1:
        initop = None
    else:
        initop = ("scale", beta)
    if alpha == 1:
        f = lambda x, y: x * y  # noqa: E731
    else:
        f = lambda x, y: x * y * alpha  # noqa: E731
    _mapreducedim_(f, "+", initop, (m, n, k), (C2, A2, B2))
    return C
