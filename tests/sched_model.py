"""An independent checker of replay schedules (csrc/smr_sched.cpp: schedule()), for tests/test_seq_schedule_fuzz.py,
tests/test_seq_program_host.py and tools/seq_schedule_search.py.  No torch, no device, no library: plain Python on the synthetic
executions and knobs handed to smr_debug_seq_schedule and on what it returned (the dict made by sched() of tests/test_seq_schedule.py).

The checker works from byte-range conflicts only: two executions conflict when one writes bytes the other reads or writes.  It does not
restate how the scheduler finds its barrier bits (no window is kept): it unrolls three replays of every queue and asks, for every
conflicting pair of packets, whether a barrier bit stands between them.  check() returns a list of (rule, text); RULES names the rules."""

RULES = ("components", "barriers", "acquire", "slices", "completeness", "footprint")

# a packet as sched() returns it per queue: (exec, launch, slice, lo, hi, barrier, acquire)
EXEC, LAUNCH, SLICE, LO, HI, BARRIER, ACQUIRE = range(7)


def _hit(x, y):
    return x[0] < y[1] and y[0] < x[1]


def _any_hit(v, w):
    return any(_hit(x, y) for x in v for y in w)


def conflict(a, b):
    """One writes what the other reads or writes."""
    return _any_hit(a["wr"], b["wr"]) or _any_hit(a["wr"], b["rd"]) or _any_hit(a["rd"], b["wr"])


def conflict_matrix(execs):
    n = len(execs)
    m = [[False] * n for _ in range(n)]
    for i in range(n):
        for j in range(i, n):
            m[i][j] = m[j][i] = conflict(execs[i], execs[j])
    return m


def union_bytes(execs):
    """Bytes touched by any range, counted once: every elementary interval between two neighbouring end points is inside or outside."""
    spans = [s for e in execs for s in list(e["rd"]) + list(e["wr"]) if s[1] > s[0]]
    pts = sorted({p for s in spans for p in s})
    return sum(hi - lo for lo, hi in zip(pts, pts[1:]) if any(s[0] <= lo and hi <= s[1] for s in spans))


def _closure(n, m):
    """Connected components of the conflict graph, numbered in order of first appearance."""
    comp = [-1] * n
    nc = 0
    for i in range(n):
        if comp[i] >= 0:
            continue
        todo = [i]
        comp[i] = nc
        while todo:
            a = todo.pop()
            for b in range(n):
                if m[a][b] and comp[b] < 0:
                    comp[b] = nc
                    todo.append(b)
        nc += 1
    return comp


def check(execs, r, max_queues=4, slices=-1, all_ordered=False, max_total=128 << 20, comp_slices=()):
    """execs: the dicts of test_seq_schedule.ex(); r: what sched() returned for them and these knobs.  Returns [(rule, text), ...]."""
    out = []

    def bad(rule, text, *args):
        assert rule in RULES
        out.append((rule, text % args))

    n = len(execs)
    m = conflict_matrix(execs)
    queues = r["queues"]
    where = [sorted({q for q, pk in queues.items() for p in pk if p[EXEC] == i}) for i in range(n)]   # queue set per execution
    on = {i: {q: [p for p in queues[q] if p[EXEC] == i] for q in where[i]} for i in range(n)}
    members = {}
    for i in range(n):
        members.setdefault(r["comp"][i], []).append(i)

    # 1. components: what conflicts shares a component and a queue set (every ordering is then one inside a queue)
    for i in range(n):
        for j in range(i + 1, n):
            if m[i][j] and r["comp"][i] != r["comp"][j]:
                bad("components", "executions %d and %d conflict and are in components %d and %d", i, j, r["comp"][i], r["comp"][j])
            if m[i][j] and where[i] != where[j]:
                bad("components", "executions %d and %d conflict and are on queues %s and %s", i, j, where[i], where[j])
    if list(r["comp"]) != _closure(n, m):
        bad("components", "components %s, the conflict graph has %s", list(r["comp"]), _closure(n, m))
    if r["ncomp"] != len(set(r["comp"])):
        bad("components", "ncomp %d, the column has %d", r["ncomp"], len(set(r["comp"])))

    # 2. barriers: three replays of every queue; a conflicting pair (a earlier, b later) has a barrier bit somewhere in (a, b]
    for q, pk in sorted(queues.items()):
        three = list(pk) * 3
        upto = [0]   # upto[k]: barrier bits among three[0:k]
        for p in three:
            upto.append(upto[-1] + (1 if p[BARRIER] else 0))
        seen = set()
        for b in range(len(three)):
            for a in range(b):
                if m[three[a][EXEC]][three[b][EXEC]] and upto[b + 1] - upto[a + 1] == 0:
                    key = (a % len(pk), b % len(pk), (b // len(pk)) - (a // len(pk)))
                    if key not in seen:
                        seen.add(key)
                        bad("barriers", "queue %d: packet %d (exec %d) and packet %d (exec %d) %d replays later conflict, no barrier bit between them",
                            q, key[0], three[a][EXEC], key[1], three[b][EXEC], key[2])
        for k, p in enumerate(pk):
            if p[LAUNCH] > 0 and not p[BARRIER]:
                bad("barriers", "queue %d packet %d: launch %d of exec %d without the barrier bit", q, k, p[LAUNCH], p[EXEC])
            if all_ordered and not p[BARRIER]:
                bad("barriers", "queue %d packet %d: all_ordered and no barrier bit", q, k)

    # 3. acquire: later launches read the first one's partials; otherwise whoever reads what the list writes
    raw = [any(_any_hit(execs[j]["wr"], execs[i]["rd"]) for j in range(n)) for i in range(n)]
    for i in range(n):
        if bool(r["acquire"][i]) != raw[i]:
            bad("acquire", "exec %d: acquire column %d, it %s what the list writes", i, r["acquire"][i], "reads" if raw[i] else "does not read")
    for q, pk in sorted(queues.items()):
        for k, p in enumerate(pk):
            if bool(p[ACQUIRE]) != (p[LAUNCH] > 0 or raw[p[EXEC]]):
                bad("acquire", "queue %d packet %d (exec %d launch %d): acquire %d", q, k, p[EXEC], p[LAUNCH], p[ACQUIRE])

    # 4. slices
    want = dict(comp_slices)
    for c, mem in sorted(members.items()):
        first = execs[mem[0]]
        parts = {i: [p for q in where[i] for p in on[i][q] if p[LAUNCH] == 0] for i in mem}   # launch 0, in queue order
        cut = any(len(parts[i]) != 1 or parts[i][0][SLICE] != 0 for i in mem)
        for i in mem:
            e = execs[i]
            if not parts[i]:
                continue   # (completeness reports it)
            if parts[i][0][LO] != 0 or parts[i][-1][HI] != e["grid"]:
                bad("slices", "exec %d: its ranges cover [%d, %d) of [0, %d)", i, parts[i][0][LO], parts[i][-1][HI], e["grid"])
            for x, y in zip(parts[i], parts[i][1:]):
                if x[HI] != y[LO]:
                    bad("slices", "exec %d: slice %d ends at %d, slice %d begins at %d", i, x[SLICE], x[HI], y[SLICE], y[LO])
                if y[LO] % 8:
                    bad("slices", "exec %d: cut at %d, no multiple of 8", i, y[LO])
            for p in parts[i]:
                if p[HI] <= p[LO]:
                    bad("slices", "exec %d: slice %d is empty", i, p[SLICE])
        if not cut:
            continue
        ns = max(len(parts[i]) for i in mem)
        if not (first["nlaunch"] == 1 and first["sliceable"] and first["grid"] >= 64 * ns):
            bad("slices", "component %d is cut in %d: nlaunch %d sliceable %d grid %d", c, ns, first["nlaunch"], first["sliceable"], first["grid"])
        same = mem[0] if first["same_as"] is None else first["same_as"]
        for i in mem[1:]:
            e = execs[i]
            if (i if e["same_as"] is None else e["same_as"]) != same or e["nlaunch"] != 1 or e["grid"] != first["grid"]:
                bad("slices", "component %d is cut and exec %d is no repeat of exec %d", c, i, mem[0])
        asked = want.get(c, max(1, slices))
        if ns != asked and not (slices < 0 and not want and ns == 2):
            bad("slices", "component %d is cut in %d, asked for %d", c, ns, asked)
        q0 = where[mem[0]][0] if where[mem[0]] else 0
        for i in mem:
            for q in where[i]:
                for p in on[i][q]:
                    if q != q0 + p[SLICE]:
                        bad("slices", "exec %d slice %d on queue %d, the component begins on queue %d", i, p[SLICE], q, q0)

    # 5. completeness
    if r["nq"] > max(1, max_queues) or any(q < 0 or q >= r["nq"] for q in queues) or (n and len(queues) != r["nq"]):
        bad("completeness", "nq %d, max_queues %d, queues in use %s", r["nq"], max_queues, sorted(queues))
    for i in range(n):
        got = sorted((p[SLICE], p[LAUNCH]) for q in where[i] for p in on[i][q])
        ns = len({s for s, _ in got}) or 1
        if got != [(s, j) for s in range(ns) for j in range(execs[i]["nlaunch"])]:
            bad("completeness", "exec %d (%d launches): its packets are (slice, launch) %s", i, execs[i]["nlaunch"], got)
        if where[i] and r["queue"][i] != where[i][0]:
            bad("completeness", "exec %d: queue column %d, first packet on queue %d", i, r["queue"][i], where[i][0])
        if where[i] and r["nslices"][i] != ns:
            bad("completeness", "exec %d: nslices column %d, packets have %d", i, r["nslices"][i], ns)
    for q, pk in sorted(queues.items()):
        order = [(p[EXEC], p[LAUNCH]) for p in pk]
        if order != sorted(order) or len(set(order)) != len(order):
            bad("completeness", "queue %d is not in recorded order: %s", q, order)
    if r["nsliced"] != sum(1 for mem in members.values() if len(where[mem[0]]) > 1):
        bad("completeness", "nsliced %d", r["nsliced"])

    # 6. footprint and residency
    fp = union_bytes(execs)
    if r["footprint"] != fp:
        bad("footprint", "footprint %d, the union of all ranges has %d bytes", r["footprint"], fp)
    if bool(r["resident"]) != (r["footprint"] <= max_total):
        bad("footprint", "resident %d with footprint %d and max_total %d", r["resident"], r["footprint"], max_total)
    return out


def rules_broken(violations):
    return sorted({rule for rule, _ in violations}, key=RULES.index)
