"""The N>1 path on CPU: two ranks over gloo.  The sharding arithmetic (smr_shard) and the
collective step (one all-reduce of the partial destinations, initop applied once) are the
product's; the per-shard compute is delegated to the CPU oracle (test infrastructure) because
there is no GPU here."""
import os
import socket
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        _worker_body(rank, world, port, q)
    except BaseException as e:  # noqa: BLE001 -- report instead of leaving the parent waiting
        import traceback
        q.put((rank, {"error": traceback.format_exc()}))
        raise e


def _worker_body(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import torch.distributed as dist
    import oraclelib
    import strided_jl_amd as S
    from strided_jl_amd import distributed as D
    from strided_jl_amd import fn

    dist.init_process_group("gloo", rank=rank, world_size=world)

    def funnel(f, op, initop, dims, arrays):  # the oracle stands in for the missing GPU
        p, keep = S.build_problem(f, op, initop, dims, arrays, stream=0)
        oraclelib.mapreduce(p, 1)
        return arrays[0]

    sys.modules["strided_jl_amd.mapreduce"]._mapreduce_fuse_ = funnel
    rng = np.random.default_rng(1234)  # same data on every rank (replicated inputs)
    res = {}

    def F(a):
        return S.StridedView(np.asfortranarray(a).copy(order="F"))

    # 1. map: permutedims -- each rank fills its own slab only
    A = rng.standard_normal((6, 5, 8, 7))
    B = F(np.full((7, 8, 5, 6), np.nan))
    D.mapreduce_sharded_(lambda x: x, None, None, B.size, (B, F(A).permutedims((3, 2, 1, 0))))
    dim, slabs = D.shard_slices(B.size, B.strides, world)
    mine = B.toarray()
    lo, hi = slabs[rank]
    sl = [slice(None)] * 4
    sl[dim] = slice(lo, hi)
    ref = A.transpose(3, 2, 1, 0)
    assert np.array_equal(mine[tuple(sl)], ref[tuple(sl)])
    other = np.ones(mine.shape, bool)
    other[tuple(sl)] = False
    assert np.isnan(mine[other]).all()  # nothing outside the slab was written
    res["map"] = True

    # 2. complete reduction: split a reduced dim, all-reduce, initop (x -> 2x) exactly once
    X = rng.standard_normal((40, 30, 8)).astype(np.float64)
    out = F(np.array([10.0]))
    O = S.StridedView(out.parent, X.shape, (0, 0, 0), 0)
    D.mapreduce_sharded_(fn.abs2, "+", (lambda x: 2 * x), X.shape, (O, F(X)))
    res["sum"] = float(out.toarray()[0])
    res["sum_ref"] = float(2 * 10.0 + (X * X).sum())

    # 3. max reduction through the same path
    out = F(np.array([-np.inf]))
    O = S.StridedView(out.parent, X.shape, (0, 0, 0), 0)
    D.mapreduce_sharded_(fn.abs, "max", None, X.shape, (O, F(X)))
    res["max"] = float(out.toarray()[0])
    res["max_ref"] = float(np.abs(X).max())

    # 4. partial reduction whose kept dim is long enough: no collective, each rank owns rows
    Y = rng.standard_normal((64, 50))
    dest = F(np.zeros((64, 1)))
    Dv = S.StridedView(dest.parent, (64, 50), (1, 0), 0)
    D.mapreduce_sharded_(lambda x: x, "+", None, (64, 50), (Dv, F(Y)))
    rows = slice(64 * rank // world, 64 * (rank + 1) // world)
    got = dest.toarray()[:, 0]
    assert np.allclose(got[rows], Y.sum(axis=1)[rows], rtol=1e-12)
    res["partial"] = True

    # 5. partial reduction, kept dims (3, 2): with 2 ranks the slowest kept dim (extent 2) is split,
    #    initop (x -> 3x) is applied to each rank's own column exactly once, no collective
    Z = rng.standard_normal((3, 2, 400))
    dest = F(np.ones((3, 2, 1)))
    Dv = S.StridedView(dest.parent, (3, 2, 400), (1, 3, 0), 0)
    D.mapreduce_sharded_(fn.sin, "+", (lambda x: 3 * x), (3, 2, 400), (Dv, F(Z)))
    got = dest.toarray()[:, :, 0]
    assert np.allclose(got[:, rank], 3.0 + np.sin(Z).sum(axis=2)[:, rank], rtol=1e-12)
    assert np.array_equal(got[:, 1 - rank], np.ones(3))
    # 6. a single kept element per rank is impossible (kept extent 1): the reduced dim is split,
    #    partials are all-reduced, conj initop once -- complex data
    W = rng.standard_normal((1, 600)) + 1j * rng.standard_normal((1, 600))
    dest = F(np.array([[1 + 2j]]))
    Dv = S.StridedView(dest.parent, (1, 600), (1, 0), 0)
    D.mapreduce_sharded_(lambda x: x, "+", "conj", (1, 600), (Dv, F(W)))
    res["part_all"] = [dest.toarray()[0, 0].real, dest.toarray()[0, 0].imag]
    ref = (1 - 2j) + W.sum()
    res["part_all_ref"] = [ref.real, ref.imag]
    dist.barrier()
    dist.destroy_process_group()
    q.put((rank, res))


@pytest.mark.timeout(300)
def test_two_rank_gloo_sharding_and_allreduce():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in procs:
        rank, res = q.get(timeout=240)
        results[rank] = res
    for p in procs:
        p.join(timeout=60)
    for rank in (0, 1):
        r = results[rank]
        assert "error" not in r, r.get("error")
        assert r["map"] and r["partial"]
        assert abs(r["sum"] - r["sum_ref"]) <= 1e-10 * abs(r["sum_ref"])
        assert r["max"] == r["max_ref"]
        assert np.allclose(r["part_all"], r["part_all_ref"], rtol=1e-12)


@pytest.mark.timeout(300)
def test_bench_gpus_flag_launches_that_many_ranks():
    """`python bench.py --gpus N` alone must produce an N-rank job.  --dry stops after the
    rendezvous (gloo, no GPU) and reports what the ranks agreed on."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "7", "--warmup", "1", "--full", "--dry"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout            # rank 0 prints ONE line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["requested_gpus"] == 2 and out["steps"] == 7 and out["warmup"] == 1 and out["full"] is True
    # the shape of the line a 2-rank --full job prints (round 6: the real run asserts the same constants before it prints): the map /
    # permute configs cut into N slabs are there with the reduce path, the README's same-destination step and both roofline witnesses
    # are top-level, and the collective barrier is outside the timed region
    assert {"c1_symmetrise_sharded", "broadcast4_sharded", "c4_mapreduce_abs2_4096x4096x64_f32"} <= set(out["extra_keys"])
    assert {"step_same_destination", "roofline", "ms_per_step_replay", "degraded"} <= set(out["line_keys"]) and "cpu_baseline" not in out["line_keys"]
    assert {"frac", "frac_rocprof_avg", "hbm_cold", "per_kernel"} <= set(out["roofline_keys"])
    assert out["timed_region"].startswith("barrier | per-rank clock")
    # a plain run (no --full) prints the headline alone: the fields its result line is read by, nothing that needs runs of its own
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "1", "--dry"],
                       capture_output=True, text=True, timeout=120, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert plain["full"] is False and plain["steps"] == 7 and plain["warmup"] == 1
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(plain["line_keys"])
    assert not {"step_same_destination", "roofline", "cpu_baseline", "extra"} & set(plain["line_keys"]) and plain["extra_keys"] == []
    sys.path.insert(0, root)
    import bench
    assert "c1_symmetrise_sharded" not in bench.extra_keys(1, "all") and "broadcast4_sharded" in bench.extra_keys(1, "c4,sharded")
    assert bench.extra_keys(8, "c4") == ["c4_mapreduce_abs2_4096x4096x64_f32"]
    src = open(os.path.join(root, "bench.py")).read()
    timed = src[src.index("    t0 = time.perf_counter()\n    if use_seq:"):src.index("    dt = time.perf_counter() - t0")]
    assert "barrier()" not in timed and "torch.cuda.synchronize()" in timed   # no collective between the two clock readings
    # a launcher that started a different number of ranks than --gpus says is an error, not a silent 1-GPU run
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry"], capture_output=True, text=True,
                       timeout=120, env=env2, cwd=root)
    assert r.returncode != 0 and "--gpus 2" in (r.stderr + r.stdout)
