// smr_sched.cpp -- which hardware queue every recorded execution goes to, which launches are cut into block ranges, which packets
// carry the barrier bit and which acquire (smr_sched.h).  Arithmetic on byte ranges: no device, no HIP, no options().
#include "smr_sched.h"

#include <algorithm>

namespace smr {

bool overlaps(const Spans& v, const std::pair<uintptr_t, uintptr_t>& x) {
    for (const auto& y : v)
        if (x.first < y.second && y.first < x.second) return true;
    return false;
}
bool overlaps(const Spans& v, const Spans& w) {
    for (const auto& x : w)
        if (overlaps(v, x)) return true;
    return false;
}

// dependency components of a list of executions given their byte ranges (union-find over "one writes what the other reads or writes");
// comp[i] = component of execution i, numbered in order of first appearance; returns their number
int components_of(const std::vector<Spans>& rd, const std::vector<Spans>& wr, std::vector<int>& comp) {
    const size_t ni = rd.size();
    std::vector<int> parent(ni);
    for (size_t i = 0; i < ni; ++i) parent[i] = (int)i;
    auto find = [&](int x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    for (size_t i = 0; i < ni; ++i)
        for (size_t j = i + 1; j < ni; ++j)
            if (overlaps(wr[i], wr[j]) || overlaps(wr[i], rd[j]) || overlaps(rd[i], wr[j])) parent[find((int)j)] = find((int)i);
    std::vector<int> roots;
    comp.assign(ni, 0);
    for (size_t i = 0; i < ni; ++i) {
        const int r = find((int)i);
        size_t c = 0;
        for (; c < roots.size(); ++c)
            if (roots[c] == r) break;
        if (c == roots.size()) roots.push_back(r);
        comp[i] = (int)c;
    }
    return (int)roots.size();
}

// bytes of the union of every range the executions touch (overlapping and nested ranges counted once)
static int64_t union_bytes(const std::vector<SchedExec>& ex) {
    Spans all;
    for (const SchedExec& r : ex) {
        all.insert(all.end(), r.rd.begin(), r.rd.end());
        all.insert(all.end(), r.wr.begin(), r.wr.end());
    }
    std::sort(all.begin(), all.end());
    uintptr_t total = 0, hi = 0;
    for (const auto& x : all) {
        const uintptr_t lo = std::max(x.first, hi);
        if (x.second > lo) total += x.second - lo;
        hi = std::max(hi, x.second);
    }
    return (int64_t)total;
}

// slice s of a launch of `grid` workgroups: [lo, hi), cut at multiples of 8 (workgroup b runs on XCD b mod 8: the planners' tile
// orders rely on it, and a slice that starts at a multiple of 8 keeps every workgroup on the XCD it had in the whole launch)
void slice_range(unsigned grid, int ns, int s2, unsigned& lo, unsigned& hi) {
    const unsigned per = ((grid + ns - 1) / ns + 7u) & ~7u;
    lo = std::min<unsigned>(grid, per * (unsigned)s2);
    hi = std::min<unsigned>(grid, lo + per);
}

namespace {
// what schedule() knows about the dependency components: first execution, bytes touched (every view counted), slices, first queue
struct Comps {
    std::vector<int> first, slices, queue;
    std::vector<int> ranges;  // block ranges of a `fold_after` component on its ONE queue (1: not cut); such a component has slices == 1
    std::vector<size_t> bytes;
};

// returns the number of components that are cut
int choose_slices(const std::vector<SchedExec>& ex, const SchedKnobs& knobs, const std::vector<int>& comp, int maxq, Comps& cs) {
    const size_t ni = ex.size();
    const int ncomp = (int)cs.first.size();
    const std::vector<int>& cfirst = cs.first;
    const std::vector<size_t>& cbytes = cs.bytes;
    std::vector<int>& cslices = cs.slices;
    int nsliced = 0;
    // 3b. slices.  A component that consists of ONE execution with ONE launch whose workgroups are independent (the launcher says so:
    //     RecLaunch::slice_kind) is cut into `slices` contiguous block ranges, each on a queue of its own: slice k of replay r+1 follows
    //     slice k of replay r in its queue, the slices of one replay write disjoint parts of the destination (a workgroup owns its
    //     tiles) and nothing else belongs to the component -- still no cross-queue ordering to express.  This is the device form of
    //     _mapreduce_threaded! (src/mapreduce.jl:195-227: the box is bisected and the halves run as concurrent tasks): while one
    //     slice drains and releases, the next replay's other slice is already running.
    {
        // (a component of SEVERAL executions can be cut when they are all the same execution recorded repeatedly -- same plan, same
        // base pointers: an unrolled replay, slice k of one follows slice k of the previous one like the replays of a single one)
        auto sliceable = [&](int c, int ns) {
            const SchedExec& r = ex[cfirst[c]];
            if (!(ns > 1 && r.nlaunch == 1 && r.sliceable && r.grid >= (unsigned)(64 * ns))) return false;
            for (size_t i = 0; i < ni; ++i)
                if (comp[i] == c && (int)i != cfirst[c])
                    if (ex[i].same_as != r.same_as || ex[i].nlaunch != 1 || ex[i].grid != r.grid) return false;
            return true;
        };
        std::vector<int> want(ncomp, 1);
        for (int c = 0; c < ncomp; ++c) {
            auto it = knobs.comp_slices.find(c);
            const int ns = it != knobs.comp_slices.end() ? it->second : std::max(1, knobs.slices);
            if (sliceable(c, ns)) want[c] = ns;
        }
        // automatic ("slices" = -1, the default): with fewer components than 3 queues, the HEAVIEST single-launch component -- by the
        // bytes its operands span, every view counted: the 4-way sum reads its buffer through four views -- is cut in two when it
        // outweighs the lightest chain by half or more.  Measured on the bench step (profiles/r05_fence_ab.txt): perm | sum/2 | sum/2
        // 5.44 us per step against 5.96 on two queues; cutting the light chain instead, or every chain, or the heavy one in three:
        // 5.77-5.95 (every additional packet is one more release, i.e. one more write-back of all eight L2s).
        if (knobs.slices < 0 && knobs.comp_slices.empty() && ncomp >= 2 && ncomp + 1 <= std::min(maxq, 3)) {
            int heavy = -1;
            size_t lightest = (size_t)-1;
            for (int c = 0; c < ncomp; ++c) {
                lightest = std::min(lightest, cbytes[c]);
                if (sliceable(c, 2) && (heavy < 0 || cbytes[c] > cbytes[heavy])) heavy = c;
            }
            if (heavy >= 0 && cbytes[heavy] * 2 >= lightest * 3) want[heavy] = 2;
            // ... and when every launch of the sequence is self-released (write-through stores, no release fence on its packet) a
            // further packet costs no write-back: every chain that can be cut is cut in two, up to four queues (measured 4.6 us per
            // step on four queues against 5.1 on three and 5.3 on two, profiles/r05_store_mode_ab.txt)
            bool all_self = true;
            for (size_t i = 0; i < ni; ++i) all_self = all_self && ex[i].all_self;
            if (all_self) {
                int total2 = 0;
                std::vector<int> w2(ncomp, 1);
                for (int c = 0; c < ncomp; ++c) {
                    w2[c] = sliceable(c, 2) ? 2 : 1;
                    total2 += w2[c];
                }
                if (total2 <= std::min(maxq, 4)) want = w2;
            }
        }
        int total = 0;
        for (int c = 0; c < ncomp; ++c) total += want[c];
        if (total <= maxq)  // every component keeps at least one queue of its own; otherwise nothing is cut
            for (int c = 0; c < ncomp; ++c)
                if (want[c] > 1) {
                    cslices[c] = want[c];
                    ++nsliced;
                }
        // 3c. a component that is ONE two-launch execution whose second launch folds what the whole first one wrote (`fold_after`:
        //     a split contraction group) is cut only when "slices" asks for it, and on its own queue: the ranges back to back, the
        //     fold behind them with the barrier bit.  It takes no further queue, so it does not count against maxq.
        for (int c = 0; c < ncomp; ++c) {
            auto it = knobs.comp_slices.find(c);
            const int ns = it != knobs.comp_slices.end() ? it->second : std::max(1, knobs.slices);
            const SchedExec& r = ex[cfirst[c]];
            bool ok = ns > 1 && r.fold_after && r.nlaunch == 2 && r.sliceable && r.grid >= (unsigned)(64 * ns);
            for (size_t i = 0; i < ni && ok; ++i)
                if (comp[i] == c && (int)i != cfirst[c]) ok = ex[i].same_as == r.same_as && ex[i].fold_after && ex[i].nlaunch == 2 && ex[i].grid == r.grid;
            if (ok) {
                cs.ranges[c] = ns;
                ++nsliced;
            }
        }
    }
    return nsliced;
}

// returns the number of queues in use
int assign_queues(int maxq, Comps& cs) {
    const int ncomp = (int)cs.first.size();
    const std::vector<size_t>& cbytes = cs.bytes;
    const std::vector<int>& cslices = cs.slices;
    std::vector<int>& cqueue = cs.queue;
    // queues: sliced components own cslices[c] queues each; the others share what is left, longest-processing-time first
    int nextq = 0;
    for (int c = 0; c < ncomp; ++c)
        if (cslices[c] > 1) {
            cqueue[c] = nextq;
            nextq += cslices[c];
        }
    {
        std::vector<int> order;
        for (int c = 0; c < ncomp; ++c)
            if (cslices[c] == 1) order.push_back(c);
        if (!order.empty()) {
            const int nshared = std::max(1, std::min<int>(maxq - nextq, (int)order.size()));
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cbytes[a] > cbytes[b]; });
            std::vector<size_t> load(nshared, 0);
            for (int c : order) {
                int best = 0;
                for (int k = 1; k < nshared; ++k)
                    if (load[k] < load[best]) best = k;
                cqueue[c] = nextq + best;
                load[best] += cbytes[c];
            }
            nextq += nshared;
        }
    }
    return nextq;
}

void order_packets(const std::vector<SchedExec>& ex, const SchedKnobs& knobs, const Comps& cs, Schedule& out) {
    const size_t ni = ex.size();
    const int nq = out.nq;
    const std::vector<int>&comp = out.comp, &cslices = cs.slices, &cqueue = cs.queue;
    // 5. packets + ordering inside each queue: a launch that conflicts with none of the launches since the queue's last ordered one
    //    (its window) goes out without the barrier bit.  A replay follows the previous one in the queue, so the window of a replay's
    //    first launches is the tail of the previous replay UNDER THE BITS CHOSEN.  Two steps:
    //    (a) a starting decision: the bits of the second of two simulated replays.  The first simulated replay opens with a forced
    //        barrier, so its last barrier can stand later than the chosen bits put it, and the window (a) judges the head of the
    //        list against can be smaller than the real one;
    //    (b) the closure: two replays are walked with the bits held fixed and the true window kept (the executions since the last set
    //        bit, over the replay boundary: once the first replay has been walked the window is the one of every later replay).  A free
    //        launch that conflicts with its window gets the bit and the walk starts again, until a whole walk changes nothing.  Every
    //        round sets a bit, so there are at most as many rounds as executions; bits are only added, so a decision of (a) that was
    //        sound stays as it was.
    // which executions read something the sequence writes (their packets acquire; everything else reads only data that is constant
    // for the whole replay and was made visible by the first packet's system-scope acquire)
    out.acquire.assign(ni, 0);
    std::vector<int>& raw = out.acquire;
    for (size_t i = 0; i < ni; ++i)
        for (size_t j = 0; j < ni && !raw[i]; ++j)
            if (overlaps(ex[j].wr, ex[i].rd)) raw[i] = 1;
    auto conflict = [&](size_t a, size_t b) {
        return overlaps(ex[a].rd, ex[b].wr) || overlaps(ex[a].wr, ex[b].wr) || overlaps(ex[a].wr, ex[b].rd);
    };
    out.queues.resize(nq);
    for (int k = 0; k < nq; ++k) {
        std::vector<size_t> mine;  // the executions of this queue, in recorded order
        for (size_t i = 0; i < ni; ++i)
            if (k >= cqueue[comp[i]] && k < cqueue[comp[i]] + cslices[comp[i]]) mine.push_back(i);
        const size_t nm = mine.size();
        std::vector<char> free_(nm, 0);
        {  // (a)
            Spans wrd, wwr;
            for (int pass = 0; pass < 2; ++pass)
                for (size_t p = 0; p < nm; ++p) {
                    const SchedExec& r = ex[mine[p]];
                    bool f = !(wrd.empty() && wwr.empty()) && !knobs.all_ordered;
                    if (f) f = !overlaps(wrd, r.wr) && !overlaps(wwr, r.wr) && !overlaps(wwr, r.rd);
                    if (!f) {
                        wrd.clear();
                        wwr.clear();
                    }
                    wrd.insert(wrd.end(), r.rd.begin(), r.rd.end());
                    wwr.insert(wwr.end(), r.wr.begin(), r.wr.end());
                    free_[p] = f;
                }
        }
        for (bool changed = true; changed;) {  // (b)
            changed = false;
            std::vector<size_t> window;
            for (size_t t = 0; t < 2 * nm && !changed; ++t) {
                const size_t p = t % nm;
                if (free_[p])
                    for (size_t w : window)
                        if (conflict(mine[w], mine[p])) {
                            free_[p] = 0;
                            changed = true;
                            break;
                        }
                if (!free_[p] || ex[mine[p]].nlaunch > 1) window.clear();  // (a later launch of p always carries the bit)
                window.push_back(p);
            }
        }
        for (size_t p = 0; p < nm; ++p) {
            const size_t i = mine[p];
            if (cs.ranges[comp[i]] > 1) {  // a cut `fold_after` execution: its ranges, then the fold, all on this queue
                const int nr = cs.ranges[comp[i]];
                bool first_range = true;
                for (int s3 = 0; s3 < nr; ++s3) {
                    SchedEntry e;
                    e.exec = (int)i;
                    e.launch = 0;
                    e.slice = s3;
                    slice_range(ex[i].grid, nr, s3, e.lo, e.hi);
                    if (e.hi <= e.lo) continue;
                    e.barrier = first_range ? !free_[p] : knobs.all_ordered;
                    e.acquire = raw[i] != 0;
                    first_range = false;
                    out.queues[k].push_back(e);
                }
                SchedEntry e;
                e.exec = (int)i;
                e.launch = 1;
                e.slice = 0;
                e.lo = e.hi = 0;
                e.barrier = e.acquire = true;
                out.queues[k].push_back(e);
                continue;
            }
            const int ns = cslices[comp[i]], s2 = k - cqueue[comp[i]];
            for (int j = 0; j < ex[i].nlaunch; ++j) {
                unsigned lo = 0, hi = j == 0 ? ex[i].grid : 0;
                if (ns > 1) slice_range(ex[i].grid, ns, s2, lo, hi);
                if (j == 0 && hi <= lo) continue;  // an empty slice (tiny grid)
                SchedEntry e;
                e.exec = (int)i;
                e.launch = j;
                e.slice = s2;
                e.lo = lo;
                e.hi = hi;
                e.barrier = j > 0 || !free_[p];  // later launches of one execution (folding passes) depend on the first
                e.acquire = j > 0 || raw[i] != 0;  // ... and read its partials
                out.queues[k].push_back(e);
            }
        }
    }
}
}  // namespace

Schedule schedule(const std::vector<SchedExec>& ex, const SchedKnobs& knobs) {
    Schedule out;
    const size_t ni = ex.size();
    // Self-released launches (write-through stores, no release fence: smr_device.h) pay for the dropped fence with slower stores.
    // That trade wins while everything the sequence touches stays in the caches (the bench step: 5.3 -> 4.6 us) and loses when the
    // stores go to HBM -- 40 launches rotating over 640 MiB of operands: the 4-way sum's 32-byte runs 4.95 -> 5.92 us per launch
    // (profiles/r05_bench_n1.json vs r04).  So: only when the union of all byte ranges of the sequence is at most
    // "self_release_max_total" bytes (default 128 MiB, half the Infinity Cache).
    out.footprint_bytes = union_bytes(ex);
    out.cache_resident = out.footprint_bytes <= knobs.self_release_max_total;
    // 3. dependency components of the recorded list.  Two executions conflict when one writes bytes the other reads or writes
    //    (an execution conflicts with its own next replay through its destination).  Executions of one component stay on ONE
    //    hardware queue, in recorded order -- every ordering the in-order result needs is then an ordering inside a queue, no
    //    cross-queue signal exists, and replay r+1 follows replay r on every queue by construction.  Different components share
    //    nothing that is written: they go to different queues (longest-processing-time first over the bytes they touch) and run
    //    concurrently -- the spawn / wait of src/mapreduce.jl:203-223 at the granularity of whole launches.
    Comps cs;
    {
        std::vector<Spans> rds(ni), wrs(ni);
        std::vector<size_t> bytes(ni, 0);
        for (size_t i = 0; i < ni; ++i) {
            rds[i] = ex[i].rd;
            wrs[i] = ex[i].wr;
            for (const auto& x : ex[i].rd) bytes[i] += x.second - x.first;
            for (const auto& x : ex[i].wr) bytes[i] += x.second - x.first;
        }
        out.ncomp = components_of(rds, wrs, out.comp);
        cs.first.assign(out.ncomp, -1);
        cs.bytes.assign(out.ncomp, 0);
        cs.slices.assign(out.ncomp, 1);
        cs.queue.assign(out.ncomp, 0);
        cs.ranges.assign(out.ncomp, 1);
        for (size_t i = 0; i < ni; ++i) {
            cs.bytes[out.comp[i]] += bytes[i];
            if (cs.first[out.comp[i]] < 0) cs.first[out.comp[i]] = (int)i;
        }
    }
    const int maxq = std::max(1, knobs.max_queues);
    out.nsliced = choose_slices(ex, knobs, out.comp, maxq, cs);
    out.nq = assign_queues(maxq, cs);
    out.queue.resize(ni);
    out.nslices.resize(ni);
    out.same_queue.assign(ni, 0);
    for (size_t i = 0; i < ni; ++i) {
        out.queue[i] = cs.queue[out.comp[i]];
        out.nslices[i] = cs.slices[out.comp[i]];
        if (cs.ranges[out.comp[i]] > 1) {
            out.nslices[i] = cs.ranges[out.comp[i]];
            out.same_queue[i] = 1;
        }
    }
    order_packets(ex, knobs, cs, out);
    return out;
}

}  // namespace smr
