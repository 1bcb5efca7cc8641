"""GPU: grouped launches whose members have scalars of their own (SMR_GROUP_MEMBER_SCALARS, `S.group(member_scalars=True)`,
csrc/smr_k_group.hip: VARC).  Every member is compared bit for bit with the same call issued alone, with the oracle evaluating that
member's own f (bit for bit, or within util.rtol for complex products with a constant and libm functions, as the other group tests
do), and as its destination's whole parent, byte for byte.  Member i's scalars are a function of i: a wrong row of the constant
table shows in the result."""
import numpy as np
import pytest

import group_cases as G
import group_scalar_cases as GS
import strided_jl_amd as S
from group_scalar_cases import CHUNK, FUNCTORS, Run, alpha, beta, member
from test_gpu_seq_group import assert_aql, field
from util import to_device

pytestmark = pytest.mark.gpu
fn = S.fn


def scalars(d):
    return d.rsplit("scalars=", 1)[1] if "scalars=" in d else None


# ---- 1. every natively compiled functor with constants, both bodies ------------------------------------------------------------------
NATIVE = [(dt, fname) for dt in G.FLOATS for fname in ("scale", "sym", "axpy", "axpby", "expr5") if not (G.is_complex(dt) and fname == "expr5")]


@pytest.mark.parametrize("dt,fname", NATIVE, ids=["%s-%s" % (np.dtype(dt).name, f) for dt, f in NATIVE])
def test_native_functors(dt, fname):
    cx = G.is_complex(dt)
    nin, nsc, make, np_make = FUNCTORS[fname]
    rng = np.random.default_rng([101, G.FLOATS.index(dt), sorted(FUNCTORS).index(fname)])
    calls, refs = [], []
    for i, (shp, perm) in enumerate(GS.SPECS):
        ks = (alpha(i, dt), beta(i, dt))[:nsc]
        calls.append((make(*ks), member(rng, shp, perm, dt, nin)))
        refs.append(np_make(*ks) if np_make else None)
    r = Run(calls, refs=refs if np_make else None)
    d = r.group.describe()
    assert scalars(d) == "member" and "jit=0" in d and "f=%s " % fname in d, d
    assert [(x[0], x[2]) for x in r.group.layout()] == list(zip(GS.FORMS, GS.WGS))
    # a complex product (or quotient) with a constant and exp / sin round differently on the host: norm-wise against the oracle
    r.judge(exact=not cx and np_make is None)


# ---- 2. axpby! in place, transposing body ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", G.FLOATS)
def test_axpby_in_place(dt):
    cx = G.is_complex(dt)
    rng = np.random.default_rng([102, G.FLOATS.index(dt)])
    calls = []
    for i, (shp, perm) in enumerate([((33, 31), (1, 0)), ((16, 16), (1, 0)), ((40, 36, 3), (1, 0, 2)), ((64, 48), (1, 0)), ((17, 70, 2), (1, 0, 2))]):
        a, b = alpha(i, dt), beta(i, dt)
        if cx:
            a = np.dtype(dt).type(complex(1 + i / 8, i / 4 - 0.5))
            b = np.dtype(dt).type(complex(2 - i / 16, 0.25 * (i + 1)))
        calls.append((FUNCTORS["axpby"][2](a, b), member(rng, shp, perm, dt, 2, inplace=True, conj=cx)))
    r = Run(calls)
    d = r.group.describe()
    assert scalars(d) == "member" and "f=axpby " in d and "jit=0" in d and "linear=0 " in d, d
    r.judge(exact=not cx)


# ---- 3. the integer class: wrapping arithmetic, saturating conversion of the scalar ---------------------------------------------------
@pytest.mark.parametrize("dt,form,fname", [(np.int32, "xk", "prog"), (np.int64, "xk", "prog"), (np.int64, "kx", "axpy")])
def test_integer_scalars(dt, form, fname):
    """x * k_i + y (an f-program; Int32 operands are converted on load) and k_i * x + y (the native axpy functor of the 64-bit class)."""
    rng = np.random.default_rng([103, np.dtype(dt).itemsize, len(form)])
    ks = [(2 ** 31 + i) * (-1 if i % 2 else 1) for i in range(len(GS.SPECS))] + [2 ** 63]
    specs = GS.SPECS + [((33, 17), (1, 0))]
    calls, truth = [], []
    for k, (shp, perm) in zip(ks, specs):
        arrays = member(rng, shp, perm, dt, 2)
        calls.append(((lambda c: lambda x, y: x * c + y)(k) if form == "xk" else (lambda c: lambda x, y: c * x + y)(k), arrays))
        kk = np.int64(min(k, 2 ** 63 - 1))  # the scalar saturates at 2^63 - 1 on its way into the 64-bit class
        with np.errstate(over="ignore"):
            truth.append((arrays[1].toarray().astype(np.int64) * kk + arrays[2].toarray().astype(np.int64)).astype(dt))
    r = Run(calls)
    d = r.group.describe()
    assert scalars(d) == "member" and "f=%s " % fname in d and {x[0] for x in r.group.layout()} == {0, 1}, d
    r.judge(exact=True, np_truth=truth)


# ---- 4. runtime-compiled f: one compilation serves every set of scalars ------------------------------------------------------------------
JIT_SPECS = [((5, 7), (0, 1)), ((33, 31), (1, 0)), ((CHUNK + 1,), (0,)), ((17, 64), (1, 0)), ((6, 5, 4), (2, 1, 0))]


def poly(k1, k2):
    return lambda p, q: k1 * p + k2 * q * q


def test_runtime_compiled_polynomial():
    rng = np.random.default_rng(104)
    first = Run([(poly(alpha(i), beta(i)), member(rng, shp, perm, np.float64, 2)) for i, (shp, perm) in enumerate(JIT_SPECS)])
    d = first.group.describe()
    assert "jit=1 " in d and "f=prog " in d and scalars(d) == "member", d
    assert first.compiles == 1, "one compilation for the whole group"
    first.judge(exact=True)
    second = Run([(poly(alpha(i + 40), beta(3 * i + 50)), member(rng, shp, perm, np.float64, 2)) for i, (shp, perm) in enumerate(JIT_SPECS)])
    assert second.compiles == 0, "other scalars: the same program text"
    second.judge(exact=True)


def test_runtime_compiled_math_opcode():
    rng = np.random.default_rng(105)

    def powf(e):
        return lambda p, q: p ** e + fn.tanh(q)

    def build(off):
        calls, refs = [], []
        for i, (shp, perm) in enumerate(JIT_SPECS):
            e = 1.25 + (i + off) / 16  # never an integer
            arrays = member(rng, shp, perm, np.float64, 2)
            flat = arrays[1].parent
            np.abs(flat, out=flat)  # a positive base
            flat += 0.5
            calls.append((powf(e), arrays))
            refs.append((lambda e: lambda p, q: np.power(p, e) + np.tanh(q))(e))
        return Run(calls, refs=refs)

    first = build(0)
    d = first.group.describe()
    assert "jit=1 " in d and "f=prog " in d and scalars(d) == "member", d
    assert first.compiles == 1
    first.judge(exact=False)
    second = build(5)
    assert second.compiles == 0
    second.judge(exact=False)


# ---- 5. the interpreter ------------------------------------------------------------------------------------------------------------------
def test_interpreted_polynomial():
    rng = np.random.default_rng(106)
    with GS.option("jit", 0):
        r = Run([(poly(alpha(i), beta(i)), member(rng, shp, perm, np.float64, 2)) for i, (shp, perm) in enumerate(JIT_SPECS)])
        d = r.group.describe()
        assert "jit=0 " in d and "f=prog " in d and scalars(d) == "member", d
        assert r.compiles == 0
        r.judge(exact=True)


# ---- 6. converting groups: Float32 arrays times a Float64 scalar -------------------------------------------------------------------------
@pytest.mark.parametrize("ddt", [np.float32, np.float64])
def test_mixed_float32_arrays_float64_scalar(ddt):
    rng = np.random.default_rng([107, np.dtype(ddt).itemsize])
    calls = [((lambda k: lambda x: x * k)(0.1 + i), member(rng, shp, perm, np.float32, 1, ddt=ddt)) for i, (shp, perm) in enumerate(GS.SPECS)]
    r = Run(calls)
    d = r.group.describe()
    assert "f=prog " in d and scalars(d) == "member", d
    assert {x[0] for x in r.group.layout()} == {0, 1}
    assert all(x.dtype == np.dtype(ddt) for x in r.got)
    r.judge(exact=True)


# ---- 7. member counts: every depth of the member search picks the right row ---------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 257, 2049])
def test_counts(K):
    rng = np.random.default_rng([108, K])
    special = {pos: n % 2 for n, pos in enumerate(sorted({0, K // 2, K - 1}))}
    calls = []
    for i in range(K):
        if i not in special:
            arrays, _ = G.tiny_member(rng)
        elif special[i] == 0:
            arrays, _ = G.linear_member(rng, (CHUNK + 1,), np.float64, 1)
        else:
            arrays, _ = G.plane_member(rng, np.float64, 40, 40)
        calls.append((FUNCTORS["scale"][2](alpha(i)), arrays))
    r = Run(calls)
    d = r.group.describe()
    assert "members=%d " % K in d and "f=scale " in d and scalars(d) == ("member" if K > 1 else "shared"), d
    r.judge(exact=True)


# ---- 8. the flag with equal scalars is the unflagged group ---------------------------------------------------------------------------------
def test_equal_scalars_are_the_shared_group():
    k, h = np.float64(2.5), np.float64(0.5)

    def build(flag):
        rng = np.random.default_rng(109)
        return Run([(FUNCTORS["axpby"][2](k, h), member(rng, shp, perm, np.float64, 2)) for shp, perm in GS.SPECS], member_scalars=flag)

    plain, flagged = build(False), build(True)
    assert scalars(plain.group.describe()) is None and flagged.group.describe() == plain.group.describe() + " scalars=shared"
    flagged.judge(exact=True)
    for i, (x, y) in enumerate(zip(plain.got, flagged.got)):
        assert G.same_bits(x, y), i
        assert G.same_bits(plain.parent(i), flagged.parent(i)), i


# ---- 9. recorded: one packet, cut into block ranges, replayed twice ---------------------------------------------------------------------
def test_recorded_group_replays_like_the_eager_execute():
    rng = np.random.default_rng(110)
    K = 300
    calls = []
    for i in range(K):
        shp, perm = [((5, 7), (1, 0)), ((17, 19), (1, 0)), ((9,), (0,))][i % 3]
        calls.append((FUNCTORS["axpby"][2](alpha(i), beta(i)), member(rng, shp, perm, np.float64, 2)))
    r = Run(calls)
    d = r.group.describe()
    lay = r.group.layout()
    assert scalars(d) == "member" and "f=axpby " in d and all(x[2] == 1 for x in lay) and {x[0] for x in lay} == {0, 1}, d
    r.judge(exact=True)
    eager = r.got
    eager_parents = [r.parent(i) for i in range(K)]

    def reset():
        import torch
        for i, dev in enumerate(r.devs):
            dev[0].parent.copy_(torch.from_numpy(r.before[i]))
        G.sync()

    q = S.Sequence().add_group(r.group)
    for slices, note in ((1, "uncut"), (4, "four block ranges"), (4, "second replay, resident tables reused")):
        q.set("slices", slices)
        reset()
        assert not any(G.same_bits(x, y) for x, y in zip(r.results()[:3], eager[:3])), "the destinations were not reset"
        q.run(1, G.cur_stream())
        q.wait()
        G.sync()
        info = q.info()
        for i, (x, y) in enumerate(zip(r.results(), eager)):
            assert G.same_bits(x, y), "member %d differs from the eager execute (%s): %s" % (i, note, info)
        for i in range(K):
            assert G.same_bits(r.parent(i), eager_parents[i]), "parent of member %d (%s)" % (i, note)
        assert field(info, "items") == "1" and field(info, "groups") == "1", info
        assert_aql(info)
        if field(info, "backend") == "aql":
            assert field(info, "packets") == str(slices) and field(info, "queues") == str(slices), info
            assert field(info, "sliced") == ("1" if slices > 1 else "0"), info


# ---- 10. the front: 40 axpby! calls with a coefficient per block are one launch -----------------------------------------------------------
def test_front_forty_blocks_one_launch():
    rng = np.random.default_rng(111)
    hx, hy = G.hview(rng.standard_normal((35, 48))), G.hview(rng.standard_normal((48, 35)))
    blocks = [(r0, c0) for r0 in range(0, 48, 6) for c0 in range(0, 35, 7)]  # 8 x 5 blocks of 6 x 7 elements in Y, of 7 x 6 in X
    assert len(blocks) == 40
    coef = [(1.125 + i / 8, 2.03125 - i / 16) for i in range(40)]           # never 0 or 1, never equal: one f for all calls
    assert all(a not in (0, 1) and b not in (0, 1) and a != b for a, b in coef)

    def loop(X, Y):
        for (r0, c0), (a, b) in zip(blocks, coef):
            S.axpby_(a, X.sview(slice(c0, c0 + 7), slice(r0, r0 + 6)).permutedims((1, 0)), b, Y.sview(slice(r0, r0 + 6), slice(c0, c0 + 7)))

    def fresh():
        return to_device(hx), to_device(hy)

    X0, Y0 = fresh()
    loop(X0, Y0)
    G.sync()
    want = Y0.parent.cpu().numpy()
    a, b = coef[7]
    r0, c0 = blocks[7]
    assert np.array_equal(Y0.toarray()[r0:r0 + 6, c0:c0 + 7], a * hx.toarray()[c0:c0 + 7, r0:r0 + 6].T + b * hy.toarray()[r0:r0 + 6, c0:c0 + 7])
    for own, launches in ((True, 1), (False, 40)):
        X, Y = fresh()
        G.sync()
        before = S.get_option("launches")
        with S.group(independent=True, member_scalars=own) as g:
            loop(X, Y)
            assert S.get_option("launches") == before
        G.sync()
        assert S.get_option("launches") == before + launches and len(g.groups) == launches and g.singles == 0
        if own:
            assert g.groups[0].count == 40 and scalars(g.groups[0].describe()) == "member" and "f=axpby " in g.groups[0].describe()
        assert G.same_bits(Y.parent.cpu().numpy(), want) and G.same_bits(X.parent.cpu().numpy(), X0.parent.cpu().numpy())
