"""GPU: grouped launches (smr_group_* / `with S.group():`, csrc/smr_k_group.hip) -- many small independent maps in one kernel launch.
Every member is compared with the CPU oracle (tests/oraclelib.py) and, bit for bit, with the same call issued alone."""
import numpy as np
import pytest

import strided_jl_amd as S
from group_cases import CHUNK, ident, rand, run_group, same_bits, sync
from util import host_flat, run_oracle, rtol, to_device

pytestmark = pytest.mark.gpu


SHAPES = [(1,), (5, 7), (31, 33), (32, 32), (33, 31), (64, 1, 3), (3, 65, 2), (2, 3, 4, 5, 2, 3), (4,) * 8, (CHUNK,), (CHUNK + 1,),
          (16, 16), (15, 17), (40, 36, 3), (17, 3, 70)]


def perms_of(n):
    out = [tuple(range(n))]
    if n >= 2:
        out.append(tuple(reversed(range(n))))
    if n >= 3:
        out.append(tuple(range(1, n)) + (0,))
        out.append((n - 1,) + tuple(range(n - 1)))
    return out


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.complex64, np.complex128, np.int32])
def test_mixed_permutedims_members(dt):
    rng = np.random.default_rng(7)
    calls = []
    for shp in SHAPES:
        for p in perms_of(len(shp)):
            src = rand(rng, shp, dt)
            dst = rand(rng, tuple(shp[i] for i in p), dt)
            calls.append((ident, (dst, src.permutedims(p))))
    assert 35 <= len(calls) <= 50
    g, want, got, alone = run_group(calls)
    d = g.describe()
    assert "family=group" in d and "members=%d" % len(calls) in d and "f=%s" % ("bitcopy" if dt is np.int32 else "ident") in d and "jit=0" in d
    forms = [r[0] for r in g.layout()]
    assert 0 in forms and 1 in forms
    for i, (w, x, y) in enumerate(zip(want, got, alone)):
        assert same_bits(x, w), (i, calls[i][1][0].size)
        assert same_bits(x, y), (i, calls[i][1][0].size)


def test_blocks_of_one_parent():
    rng = np.random.default_rng(11)
    dt = np.complex128
    P, Q = rand(rng, (50, 50), dt), rand(rng, (50, 50), dt)
    R, T = rand(rng, (6, 7, 6, 5), dt), rand(rng, (5, 6, 7, 6), dt)
    host, r0 = [], 1
    for k, n in enumerate((6, 34, 9)):  # diagonal blocks, first elements at odd offsets (51 * r0)
        sl = slice(r0, r0 + n)
        src = P.sview(sl, sl)
        if k == 1:
            src = P.sview(slice(r0 + n - 1, r0 - 1, -1), sl)  # a reversed (negative-stride) input view
        if k == 2:
            src = src.conj()
        host.append((ident, (Q.sview(sl, sl), src.permutedims((1, 0)))))
        r0 += n
    for a, b, c in ((slice(1, 3), slice(1, 2), slice(1, 4)), (slice(3, 6), slice(2, 5), slice(4, 7))):  # offsets 301 and 657
        src = R.sview(a, c, a, b)
        dst = T.sview(b, a, c, a)
        host.append((ident, (dst, src.permutedims((3, 2, 1, 0)))))
    cache = {}
    devs = [tuple(to_device(v, cache) for v in arrays) for _, arrays in host]
    sync()
    before = S.get_option("launches")
    with S.group(independent=True) as g:
        for (f, arrays), dev in zip(host, devs):
            S.map_(f, *dev)
        assert S.get_option("launches") == before  # nothing launches inside the block
    sync()
    assert S.get_option("launches") == before + 2 and len(g.groups) == 2 and g.singles == 0  # the conj member is a bucket of its own
    assert sorted(int(x.describe().split("members=")[1].split()[0]) for x in g.groups) == [1, 4]
    for f, arrays in host:
        run_oracle(f, None, None, arrays[0].size, arrays)
    # the whole destination parents: the blocks as the oracle wrote them, every other element untouched
    for parent in (Q, T):
        flat, _ = host_flat(parent)
        dev_parent = cache[flat.ctypes.data].cpu().numpy()
        assert same_bits(dev_parent, flat)


def test_functions():
    rng = np.random.default_rng(13)
    # a*X + b*Y' + z with a broadcast (stride-0) third input
    calls = []
    for m, n in ((5, 7), (33, 31), (64, 48), (1, 9)):
        x, y, z = rand(rng, (m, n), np.float64), rand(rng, (n, m), np.float64), rand(rng, (m, 1), np.float64)
        zb = S.StridedView(z.parent, (m, n), (1, 0), 0)
        calls.append((lambda p, q, r: 2.5 * p + 0.5 * q + r, (x.similar(), x, y.permutedims((1, 0)), zb)))
    g, want, got, alone = run_group(calls)
    assert "jit=1" in g.describe()
    for w, x, y in zip(want, got, alone):
        assert same_bits(x, w) and same_bits(x, y)
    # in place: the destination is its own input
    calls = []
    for shp in ((7,), (33, 5), (CHUNK + 3,)):
        x = rand(rng, shp, np.float32)
        calls.append((lambda v: v * 2, (x, x)))
    x = rand(rng, (40, 40), np.float32)
    calls.append((lambda v: v * 2, (x.sview(slice(1, 40, 2), slice(None)), x.sview(slice(1, 40, 2), slice(None)))))
    g, want, got, alone = run_group(calls)
    for w, x, y in zip(want, got, alone):
        assert same_bits(x, w) and same_bits(x, y)
    # math opcodes: the runtime-compiled path
    calls = []
    for m, n in ((6, 5), (33, 40), (17, 64)):
        x, y = rand(rng, (m, n), np.float64), rand(rng, (n, m), np.float64)
        calls.append((lambda p, q: p ** 2 + S.fn.tanh(q), (x.similar(), x, y.permutedims((1, 0)))))
    g, want, got, alone = run_group(calls, ref=lambda p, q: p * p + np.tanh(q))
    assert "jit=1" in g.describe() and "f=prog" in g.describe()
    for w, x, y in zip(want, got, alone):
        assert same_bits(x, y)
        assert np.allclose(x, w, rtol=rtol(np.float64), atol=0)  # tanh: the device's libm against the host's
    # mixed dtypes: Float32 destination, Float64 input
    calls = []
    for shp, p in (((9,), (0,)), ((33, 31), (1, 0)), ((20, 3, 18), (2, 1, 0)), ((12, 10), (0, 1))):
        src = rand(rng, shp, np.float64)
        calls.append((ident, (rand(rng, tuple(shp[i] for i in p), np.float32), src.permutedims(p))))
    g, want, got, alone = run_group(calls)
    for w, x, y in zip(want, got, alone):
        assert x.dtype == np.float32 and same_bits(x, w) and same_bits(x, y)


def dev_like(rng, shape, dt=np.float64):
    h = rand(rng, shape, dt)
    return h, to_device(h)


def test_front_semantics():
    rng = np.random.default_rng(17)
    ha, A = dev_like(rng, (33, 20))
    _, B = dev_like(rng, (33, 20))
    _, Cc = dev_like(rng, (20, 33))
    a = ha.toarray()
    sync()
    # a map, a reduction over its result, another map
    with S.group() as g:
        S.map_(lambda x: x * 2, B, A)
        s = S.sum(B)
        S.map_(lambda x: x + 1, Cc, B.permutedims((1, 0)))
    sync()
    S.map_(lambda x: x * 2, B, A)
    s_seq = S.sum(B)
    assert s == s_seq and abs(s - (a * 2).sum()) <= 1e-12 * np.abs(a * 2).sum()
    assert np.array_equal(B.toarray(), a * 2) and np.array_equal(Cc.toarray(), (a * 2).T + 1)
    # the third call reads the first call's destination: two group launches
    _, D = dev_like(rng, (33, 20))
    _, E = dev_like(rng, (33, 20))
    sync()
    before = S.get_option("launches")
    with S.group() as g:
        S.copy_(B, A)
        S.copy_(D, A)
        S.copy_(E, B)
    sync()
    assert S.get_option("launches") == before + 2 and [x.count for x in g.groups] == [2, 1]
    assert np.array_equal(E.toarray(), a) and np.array_equal(D.toarray(), a)
    # two different f: two launches
    before = S.get_option("launches")
    with S.group() as g:
        S.map_(lambda x: x * 2, B, A)
        S.map_(lambda x: x * 3, D, A)
        S.map_(lambda x: x * 2, E, A)
    sync()
    assert S.get_option("launches") == before + 2 and sorted(x.count for x in g.groups) == [1, 2]
    assert np.array_equal(B.toarray(), a * 2) and np.array_equal(D.toarray(), a * 3) and np.array_equal(E.toarray(), a * 2)
    # a member above group_max_bytes takes the normal path
    hbig, BIG = dev_like(rng, (64, 64))
    _, BIGD = dev_like(rng, (64, 64))
    old = S.get_option("group_max_bytes")
    S.set_option("group_max_bytes", 2 * 33 * 20 * 8)
    try:
        sync()
        before = S.get_option("launches")
        with S.group() as g:
            S.copy_(B, A)
            S.copy_(D, A)
            S.copy_(BIGD, BIG.permutedims((1, 0)))
            S.copy_(E, A)
        sync()
        assert S.get_option("launches") == before + 3
        assert [x.count for x in g.groups] == [2, 1] and all("members=%d " % x.count in x.describe() for x in g.groups)
    finally:
        S.set_option("group_max_bytes", old)
    assert np.array_equal(BIGD.toarray(), hbig.toarray().T) and np.array_equal(E.toarray(), a)


def test_library_owned_stream():
    rng = np.random.default_rng(19)
    ha, A = dev_like(rng, (40, 24))
    _, B = dev_like(rng, (40, 24))
    _, Cc = dev_like(rng, (24, 40))
    _, D = dev_like(rng, (40, 24))
    _, E = dev_like(rng, (24, 40))
    a = ha.toarray()
    sync()
    st = S.Stream()
    try:
        with st:
            S.map_(lambda x: x * 2, B, A)                         # direct launch writes B
            with S.group() as g:                                  # one group launch (through HIP) reads B
                S.map_(lambda x: x + 1, Cc, B.permutedims((1, 0)))
                S.map_(lambda x: x + 1, D, B)
            S.map_(lambda x: x * 3, E, Cc)                        # direct launch reads the group's output
        assert len(g.groups) == 1 and g.groups[0].count == 2
        assert np.array_equal(B.toarray(), a * 2)
        assert np.array_equal(Cc.toarray(), (a * 2).T + 1) and np.array_equal(D.toarray(), a * 2 + 1)
        assert np.array_equal(E.toarray(), ((a * 2).T + 1) * 3)
    finally:
        st.close()
