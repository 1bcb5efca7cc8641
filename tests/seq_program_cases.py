"""Seeded programs for recorded sequences (tests/test_seq_program_host.py, tests/test_gpu_seq_program.py): lists of 6-12 steps over
windows of four Float64 parents, as pure functions of the seed.  Nothing here imports torch.

A step is one plan (or one group of plans) over windows laid out by window_cases.layout somewhere inside the parents:
  stream       clamped sum / difference of two inputs laid out like the destination              STREAM
  tiled        clamped sum of a transposed and a plain input, 100 x 90                           TILED
  orbit        clamped sum of the four cyclic permutations of one 16^4 region                    ORBIT
  flat         clamped copy with the dims reversed, 3 x 480 x 64                                  FLAT
  generic      clamped difference over stepped, reversed, permuted views, 7 x 9 x 5 x 3           GENERIC
  part         two sums over 8192 elements, partials and a folding launch ("reduce_single" = 0)   REDUCE_PART, two launches
  all          the sum of 32 elements                                                             REDUCE_ALL
  contract     C = A * B' over k = 9                                                              CONTRACT (option "contract" = 2)
  split        the same over k = 64 cut in two slices, recorded TWICE, the second time with the destination rebound to another
               window: the partials belong to the plan, so on a device both recordings are one component
  mapgroup     three small transposing copies as one launch (add_group)
  mulgroup     three small contractions as one launch (add_group)
  big          (every fourth program) a transposing copy over 32^4 whose operands nothing else touches, so its source keeps its first
               values: a component of one single-launch execution, cut into block ranges when slices are asked for (grid 256 >=
               64 * 3).  Its f is the native identity: launches of runtime-compiled kernels are never cut

Values.  Every parent starts with integers of [-4, 4].  Maps clamp their result to [-4, 4] and write parents 0-2 only; reductions and
contractions write parent 3 only, read parents 0-2 only and use initop zero, so every sum has at most 8192 terms of magnitude <= 16 and
is exact in any order, whatever the number of replays.  (The issue's bound of 32 reduced elements is kept where the form allows it: the
two-launch reduction needs 8192 and the split contraction two chunks of 32.)  No step reads what it writes through another view: the
inputs of a step lie in other parents than its destination, or are the destination itself.  No -0.0 arises: sums are added to +0.0.

In the odd programs the steps are dealt to two lanes that use disjoint halves of every parent, so they have several components."""
import collections

import numpy as np

import contract_cases as CC
import strided_jl_amd as S
import window_cases as W
from strided_jl_amd import _lib as L
from strided_jl_amd.broadcast import promoteshape

fn = S.fn
F64 = np.float64
H = 278528                 # elements of one lane of a parent: above the largest window (FLAT: 64 x 480 x (3 + 6))
BIG = 34 * 32 ** 3 + 64    # elements reserved for the operands of the "big" step
PROGRAMS = 8
KINDS = ("stream", "tiled", "orbit", "flat", "generic", "part", "all", "contract", "split", "mapgroup", "mulgroup")
FAMILY = {"stream": "stream", "tiled": "tiled", "orbit": "orbit", "flat": "flat", "generic": "generic", "part": "reduce_part", "all": "reduce_all",
          "contract": "contract", "split": "contract", "big": "tiled"}


def clamp(x):
    return fn.max(fn.min(x, 4), -4)


def npclamp(x):
    return np.clip(x, -4, 4)


# name -> (f for the library, the same in NumPy)
FS = {
    "csum2": (lambda a, b: clamp(a + b), lambda a, b: npclamp(a + b)),
    "cdiff2": (lambda a, b: clamp(a - b), lambda a, b: npclamp(a - b)),
    "csum4": (lambda a, b, c, d: clamp(a + b + c + d), lambda a, b, c, d: npclamp(((a + b) + c) + d)),
    "c1": (lambda a: clamp(a), npclamp),
    "flip": (lambda a: clamp(1 - a), lambda a: npclamp(1 - a)),
    "ident": (lambda a: a, lambda a: a),
    "mul": (lambda a, b: a * b, lambda a, b: a * b),
}

Op = collections.namedtuple("Op", "par size strides offset")


class Step:
    """One recorded execution.  ops[0] is the destination; `twin`: index of the step whose plan this one records again, with the
    destination's base pointer moved by `shift` elements; `members`: the steps of a group."""

    def __init__(self, kind, f, dims, ops, op=None, initop=None, opts=(), members=None, twin=None, shift=0):
        self.kind, self.f, self.dims, self.ops, self.op, self.initop, self.opts = kind, f, tuple(dims), list(ops), op, initop, tuple(opts)
        self.members, self.twin, self.shift = members, twin, shift

    def leaves(self):
        return self.members if self.members else [self]


def index_of(o):
    return W.element_index(o)


def extent(o):
    idx = index_of(o)
    return int(idx.min()), int(idx.max())


def window(par, base, dims, perm, lo, hi, steps=None):
    n, strides, off = W.layout(dims, perm, lo, hi, steps)
    return Op(par, tuple(dims), strides, base + off), n


def expand(o, axes, N):
    size, strides = [1] * N, [0] * N
    for i, d in enumerate(axes):
        size[d], strides[d] = o.size[i], o.strides[i]
    return Op(o.par, tuple(size), tuple(strides), o.offset)


class Builder:
    def __init__(self, seed, floor, lanes):
        self.rng = np.random.default_rng([7, seed])
        self.floor, self.lanes = floor, lanes

    def pick(self, xs):
        return xs[int(self.rng.integers(0, len(xs)))]

    def base(self, n, lane, span=H):
        """Where a window of n elements goes inside a lane: its start, its middle or its end (multiples of 8)."""
        assert n <= span, (n, span)
        lane = lane if self.lanes else int(self.rng.integers(0, 2))
        return self.floor + lane * H + self.pick((0, ((span - n) // 2) & ~7, (span - n) & ~7))

    def pads(self, N):
        return [int(v) for v in self.rng.integers(0, 4, size=N)], [int(v) for v in self.rng.integers(0, 4, size=N)]

    def win(self, par, lane, dims, perm=None, steps=None, pads=True, pad_dims=None, base=None):
        N = len(dims)
        perm = perm or tuple(range(N))
        lo, hi = self.pads(N) if pads else ([0] * N, [0] * N)
        if pad_dims is not None:
            lo = [lo[i] if perm[i] in pad_dims else 0 for i in range(N)]
            hi = [hi[i] if perm[i] in pad_dims else 0 for i in range(N)]
        n = W.layout(dims, perm, lo, hi, steps)[0]
        return window(par, self.base(n, lane) if base is None else base, dims, perm, lo, hi, steps)[0]

    def parents(self, nin, written=(0, 1, 2)):
        """A destination parent and nin input parents, all different from it."""
        d = self.pick(written)
        return d, [self.pick([p for p in range(4) if p != d]) for _ in range(nin)]

    # ---- the kinds ---------------------------------------------------------------------------------------------------------------------
    def stream(self, lane):
        dims = self.pick(((64, 33), (131, 40, 3), (1001, 9)))
        d, (a, b) = self.parents(2)
        return Step("stream", self.pick(("csum2", "cdiff2")), dims, [self.win(d, lane, dims), self.win(a, lane, dims), self.win(b, lane, dims)])

    def tiled(self, lane):
        dims = (100, 90)
        d, (a, b) = self.parents(2)
        return Step("tiled", "csum2", dims, [self.win(d, lane, dims), self.win(a, lane, dims, (1, 0)), self.win(b, lane, dims)])

    def orbit(self, lane):
        dims = (16,) * 4
        d, (a,) = self.parents(1)
        base = self.base(16 ** 4, lane)
        ins = [self.win(a, lane, dims, p, pads=False, base=base) for p in W.CYCLIC]
        return Step("orbit", "csum4", dims, [self.win(d, lane, dims, pad_dims=(3,))] + ins)

    def flat(self, lane):
        dims = (3, 480, 64)
        d, (a,) = self.parents(1)
        return Step("flat", "c1", dims, [self.win(d, lane, dims, pad_dims=(2,)), self.win(a, lane, dims, (2, 1, 0), pad_dims=(2,))])

    def generic(self, lane):
        dims = (7, 9, 5, 3)
        d, (a, b) = self.parents(2)
        ops = []
        for par in (d, a, b):
            perm = tuple(int(p) for p in self.rng.permutation(4))
            steps = [int(self.rng.choice([1, 2, -1, 3])) for _ in range(4)]
            steps[perm.index(0)] = int(self.rng.choice([2, -2, 3]))    # no unit stride anywhere: nothing for another family to vectorise
            ops.append(self.win(par, lane, dims, perm, steps))
        return Step("generic", "cdiff2", dims, ops)

    def part(self, lane):
        dims = (2, 8192)
        a = self.pick((0, 1, 2))
        src = self.win(a, lane, dims, (1, 0), pad_dims=(1,))      # the long dim has unit stride
        dst = expand(self.win(3, lane, (2,), steps=[self.pick((1, 2))]), (0,), 2)
        return Step("part", "ident", dims, [dst, src], "+", "zero", opts=(("reduce_single", 0),))

    def all(self, lane):
        dims = (32,)
        a = self.pick((0, 1, 2))
        dst = Op(3, (1,), (0,), self.base(1, lane))
        return Step("all", "ident", dims, [dst, self.win(a, lane, dims)], "+", "zero")

    def mul(self, lane, dims, kind="contract", opts=(("contract", 2),), base3=None):
        m, n, k = dims
        a, b = self.pick((0, 1, 2)), self.pick((0, 1, 2))
        A = self.win(a, lane, (m, k), self.pick(((0, 1), (1, 0))), steps=[self.pick((1, 1, 2, -1)), 1])
        B = self.win(b, lane, (n, k), self.pick(((0, 1), (1, 0))))
        C = self.win(3, lane, (m, n), self.pick(((0, 1), (1, 0))), base=base3)
        return Step(kind, "mul", dims, [expand(C, (0, 1), 3), expand(A, (0, 2), 3), expand(B, (1, 2), 3)], "+", "zero", opts=opts)

    def contract(self, lane):
        return self.mul(lane, (33, 34, 9))

    def split(self, lane):
        """Returns TWO steps: the plan and its second recording with the destination moved into the other half of the lane."""
        half = H // 2
        first = self.mul(lane, (65, 63, 64), "split", (("contract", 2), ("contract_tile", 16), ("contract_split", 2)),
                         base3=self.floor + (lane if self.lanes else 0) * H + self.pick((0, 8, 64)))
        assert extent(first.ops[0])[1] < self.floor + (lane if self.lanes else 0) * H + half
        second = Step("split", "mul", first.dims, [first.ops[0]._replace(offset=first.ops[0].offset + half)] + first.ops[1:], "+", "zero", first.opts, shift=half)
        return first, second

    def mapgroup(self, lane):
        s, d = self.pick(((0, 1), (1, 2), (2, 0), (1, 0)))
        slot = H // 4
        members = []
        for j, dims in enumerate(((17, 19), (33, 16, 2), (40, 40))):
            perm = (1, 0) + tuple(range(2, len(dims)))
            b = self.floor + (lane if self.lanes else int(self.rng.integers(0, 2))) * H + j * slot
            dst, n1 = window(d, b, dims, tuple(range(len(dims))), *self.pads(len(dims)))
            src, n2 = window(s, b, dims, perm, *self.pads(len(dims)))
            assert max(n1, n2) <= slot
            members.append(Step("member", "ident", dims, [dst, src]))
        return Step("mapgroup", "ident", (), [], members=members)

    def mulgroup(self, lane):
        slot = H // 4
        members = []
        ln = lane if self.lanes else int(self.rng.integers(0, 2))
        for j, dims in enumerate(((17, 19, 8), (33, 16, 5), (16, 16, 32))):
            st = self.mul(lane, dims, "member", (), base3=self.floor + ln * H + j * slot)
            assert extent(st.ops[0])[1] < self.floor + ln * H + (j + 1) * slot
            members.append(st)
        return Step("mulgroup", "mul", (), [], "+", "zero", members=members)

    def big(self):
        dims = (32,) * 4
        src, n1 = window(0, 0, dims, (3, 2, 1, 0), [0, 0, 0, 1], [0, 0, 0, 1])
        dst, n2 = window(2, 0, dims, (0, 1, 2, 3), [0, 0, 0, 0], [0, 0, 0, 2])
        assert max(n1, n2) <= BIG
        return Step("big", "ident", dims, [dst, src])


class Program:
    def __init__(self, name, steps, nelem, data_seed):
        self.name, self.steps, self.nelem = name, steps, nelem
        rng = np.random.default_rng([11, data_seed])
        self.initial = [rng.integers(-4, 5, size=nelem).astype(F64) for _ in range(4)]
        for i, s in enumerate(self.steps):   # the twin of a rebound recording
            if s.shift:
                s.twin = i - 1
            for m in s.leaves():             # every operand inside its parent
                for o in m.ops:
                    lo, hi = extent(o)
                    assert 0 <= lo <= hi < nelem, (name, i, s.kind, lo, hi, nelem)

    def __repr__(self):
        return self.name

    def kinds(self):
        return [s.kind for s in self.steps]


_CACHE = {}


def program(seed):
    if seed in _CACHE:
        return _CACHE[seed]
    big = seed % 4 == 2    # (an even program: few components, so the cut one finds queues to spare)
    b = Builder(seed, BIG if big else 0, lanes=seed % 2 == 1)
    nsteps = 6 + (5 * seed) % 7
    first = sum(6 + (5 * s) % 7 for s in range(seed))     # the kinds go round over the corpus: every kind at least three times
    steps = []
    for j in range(nsteps):
        kind = KINDS[(first + j) % len(KINDS)]
        lane = j % 2
        made = getattr(b, kind)(lane)
        steps.extend(made if isinstance(made, tuple) else [made])
    order = [int(i) for i in b.rng.permutation(len(steps))]
    shuffled = []
    for i in order:                                         # (a rebound recording stays right behind its plan)
        if steps[i].shift:
            continue
        shuffled.append(steps[i])
        if i + 1 < len(steps) and steps[i + 1].shift:
            shuffled.append(steps[i + 1])
    if big:
        shuffled.insert(len(shuffled) // 2, b.big())
    p = Program("program%d" % seed, shuffled, b.floor + 2 * H, seed)
    _CACHE[seed] = p
    return p


def pinned():
    """The smallest chain whose replay barrier bits were unsound (tests/test_seq_schedule_fuzz.py: FIVE) as real plans over four
    buffers of 96^3: (reads, writes) = (1 2, 1), (3, 3), (0 1, 0), (1 3, 2), (3, 0).  Step 3 transposes (the long one); steps 4 and 0
    stream."""
    n = 96
    dims = (n, n, n)
    whole = lambda par, perm=(0, 1, 2): window(par, 0, dims, perm, [0] * 3, [0] * 3)[0]  # noqa: E731
    steps = [Step("stream", "csum2", dims, [whole(1), whole(1), whole(2)]),
             Step("stream", "flip", dims, [whole(3), whole(3)]),
             Step("stream", "cdiff2", dims, [whole(0), whole(0), whole(1)]),
             Step("tiled", "csum2", dims, [whole(2), whole(1, (2, 1, 0)), whole(3)]),
             Step("stream", "flip", dims, [whole(0), whole(3)])]
    return Program("pinned", steps, n ** 3, 99)


# ---- NumPy: the list in order --------------------------------------------------------------------------------------------------------
def apply_numpy(step, parents):
    for s in step.leaves():
        npf = FS[s.f][1]
        ins = [parents[o.par][index_of(o)] for o in s.ops[1:]]
        r = np.broadcast_to(npf(*ins), s.dims)
        dst = s.ops[0]
        if s.op:
            axes = tuple(d for d in range(len(s.dims)) if dst.size[d] == 1 and s.dims[d] > 1)
            r = np.zeros(dst.size) + r.sum(axis=axes, keepdims=True)      # initop zero; +0.0 + (-0.0) = +0.0
        parents[dst.par][index_of(dst)] = r


def run_numpy(prog, reps):
    parents = [a.copy() for a in prog.initial]
    for _ in range(reps):
        for s in prog.steps:
            apply_numpy(s, parents)
    return parents


# ---- plans over given parents (NumPy arrays or device tensors) -------------------------------------------------------------------------
class options:
    def __init__(self, opts):
        self.ctx = [CC.option(k, v) for k, v in opts]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *a):
        for c in reversed(self.ctx):
            c.__exit__(*a)


def views(step, parents):
    vs = tuple(S.StridedView(parents[o.par], o.size, o.strides, o.offset) for o in step.ops)
    return promoteshape(step.dims, *vs) if step.op else vs


class Recorded:
    """The plans and groups of a program over `parents`, and how each step is recorded: items[i] = ("plan", plan, bases or None) or
    ("group", group, None).  pointer(parent) gives a parent's base address; stream: the stream the groups' problems are built for."""

    def __init__(self, prog, parents, pointer, stream=0):
        self.items, self.keep = [], []
        for i, s in enumerate(prog.steps):
            if s.members:
                with options(s.opts):
                    built = [S.build_problem(FS[m.f][0], m.op, m.initop, m.dims, views(m, parents), stream=stream) for m in s.members]
                    self.items.append(("group", L.Group([b[0] for b in built], keepalive=built), None))
            elif s.twin is not None:
                plan = self.items[s.twin][1]
                bases = [pointer(parents[o.par]) + (s.shift * 8 if k == 0 else 0) for k, o in enumerate(s.ops)]
                self.items.append(("plan", plan, bases))
            else:
                with options(s.opts):
                    self.items.append(("plan", S.make_plan(FS[s.f][0], s.op, s.initop, s.dims, views(s, parents)), None))

    def sequence(self):
        q = S.Sequence()
        for kind, x, bases in self.items:
            if kind == "group":
                q.add_group(x)
            else:
                q.add(x, bases=bases)
        return q

    def execute(self, stream):
        for kind, x, bases in self.items:
            if kind == "group":
                x.execute(stream)
            else:
                x.execute(stream, bases=bases)


def footprints(prog, pointer_of_parent):
    """Per step the byte ranges read and written, from the operands alone (no scratch): every operand's lowest to highest element."""
    out = []
    for s in prog.steps:
        rd, wr = [], []
        for m in s.leaves():
            for k, o in enumerate(m.ops):
                lo, hi = extent(o)
                r = (pointer_of_parent(o.par) + 8 * lo, pointer_of_parent(o.par) + 8 * (hi + 1))
                if k == 0:
                    wr.append(r)
                    if m.op and not (s.members and m.initop == "zero"):   # a plan's reduction always counts as reading its destination
                        rd.append(r)
                else:
                    rd.append(r)
        out.append((rd, wr))
    return out
