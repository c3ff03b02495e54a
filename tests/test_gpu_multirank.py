"""Two ranks of the frame-sharded HIP path (se_snmf_nat_amd/dist.py ShardedTrainer) on ONE GPU.

The driver's multi-GPU bench runs one process per GPU over RCCL; a single-GPU test box cannot do that,
so this test starts two processes that share device 0 and exchange the statistics buffer over gloo.
Everything but the transport is the product path: HIP plans on frame shards, one sum-all-reduce of the
fp64 statistics per iteration, the deterministic W epilogue on every rank
(src/sparse_nmf.m:186-284 with the frame axis partitioned).  Checked against the fp64 oracle and against
the unsharded HIP run.
"""
import os
import socket

import numpy as np
import pytest

from oracle.sparse_nmf_oracle import sparse_nmf as oracle_nmf, synth_problem

pytestmark = pytest.mark.gpu
REL_WH = 1e-4
REL_COST = 1e-5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, case, q):
    import torch
    import torch.distributed as dist
    from se_snmf_nat_amd.dist import ShardedTrainer, shard_bounds
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    V, W0, H0 = synth_problem(case["F"], case["T"], case["r"])
    t0, t1 = shard_bounds(case["T"], world, rank)
    w_ind = None if "w_ind" not in case else np.array(case["w_ind"], bool)
    h_ind = None if "h_ind" not in case else np.array(case["h_ind"], bool)
    tr = ShardedTrainer(V[:, t0:t1], W0, H0[:, t0:t1], beta=case["beta"], sparsity=case["sparsity"],
                        max_iter=case["max_iter"], conv_eps=case["conv_eps"], cost_check=True,
                        w_update_ind=w_ind, h_update_ind=h_ind, device=0)
    tr.run()
    tr.sync()
    w, h, (div, cost, n_iter) = tr.result()
    q.put((rank, w, h, np.asarray(cost), int(n_iter)))
    dist.barrier()
    dist.destroy_process_group()
    torch.cuda.synchronize()


CASES = [
    dict(F=257, T=2100, r=64, beta=1.0, sparsity=5.0, max_iter=15, conv_eps=0.0),
    dict(F=257, T=1500, r=40, beta=1.0, sparsity=0.5, max_iter=80, conv_eps=2e-3),           # early stop
    dict(F=129, T=700, r=24, beta=2.0, sparsity=0.3, max_iter=10, conv_eps=0.0),
    dict(F=129, T=700, r=24, beta=0.0, sparsity=0.01, max_iter=10, conv_eps=0.0),
    dict(F=257, T=900, r=32, beta=1.0, sparsity=5.0, max_iter=30, conv_eps=1e-3, w_ind=[0] * 32),  # H-only
    dict(F=257, T=900, r=32, beta=1.0, sparsity=5.0, max_iter=30, conv_eps=1e-3, h_ind=[0] * 32),  # W-only
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"F{c['F']}-b{c['beta']}-eps{c['conv_eps']}-"
                         f"{'Honly' if 'w_ind' in c else 'Wonly' if 'h_ind' in c else 'full'}")
def test_two_ranks_one_gpu_match_oracle_and_unsharded(gpu_ctx, case):
    import torch.multiprocessing as mp
    from se_snmf_nat_amd import sparse_nmf
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(rk, world, port, case, q)) for rk in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda x: x[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    V, W0, H0 = synth_problem(case["F"], case["T"], case["r"])
    cf = {1.0: "kl", 2.0: "ed", 0.0: "is"}[case["beta"]]
    p = dict(cf=cf, sparsity=case["sparsity"], max_iter=case["max_iter"], conv_eps=case["conv_eps"], init_w=W0,
             init_h=H0, cost_check=1)
    if "w_ind" in case:
        p["w_update_ind"] = np.array(case["w_ind"], bool)
    if "h_ind" in case:
        p["h_update_ind"] = np.array(case["h_ind"], bool)
    wr, hr, orf = oracle_nmf(V, p)
    w1, h1, o1 = sparse_nmf(V, p, ctx=gpu_ctx)          # unsharded HIP run
    H = np.concatenate([r_[2] for r_ in res], axis=1)
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    assert np.array_equal(res[0][1], res[1][1]), "replicas of W must be bit-identical across ranks"
    for r_ in res:
        assert r_[4] == orf["n_iter"] == o1["n_iter"]
        assert rel(r_[1], wr) < REL_WH
        np.testing.assert_allclose(r_[3][:len(orf["cost"])], orf["cost"], rtol=REL_COST)
    assert rel(H, hr) < REL_WH
    # sharding only reorders fp64 partial sums: the sharded result sits within fp32 rounding of the unsharded one
    assert rel(res[0][1], w1) < 5e-6 and rel(H, h1) < 5e-6


def _rccl_worker(port, q):
    import torch
    import torch.distributed as dist
    from se_snmf_nat_amd.dist import ShardedTrainer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    V, W0, H0 = synth_problem(257, 3000, 64)
    res = []
    for force in (False, True, "native"):
        tr = ShardedTrainer(V.astype(np.float32), W0, H0.astype(np.float32), beta=1.0, sparsity=5.0, max_iter=20, conv_eps=0.0,
                            cost_check=True, device=0)
        if force:
            tr.world = 2  # take the RCCL branch: a sum over the one rank of the group is the identity
        if force == "native":
            # round 6: the collective issued by the library itself (ncclAllReduce from C on the engine's stream: csrc/snmf_tu_rccl.hip,
            # snmf_plan_run_sharded_rccl) on a one-rank communicator of its own
            assert tr.use_native_rccl(force_single=True) and tr.loop.rccl_comm is not None
        tr.run()
        tr.sync()
        w, h, (div, cost, n) = tr.result()
        res.append((w, h, np.asarray(cost)))
    q.put(res)
    dist.destroy_process_group()


def test_rccl_all_reduce_call_path_at_world_size_one(gpu_ctx):
    """The transport the multi-GPU bench uses (RCCL through torch.distributed, issued on the trainer's stream) cannot
    be run with two ranks on a one-GPU box (RCCL refuses a duplicated device), but the call path can: with a
    one-rank group the all-reduce is the identity, so forcing the trainer through it must reproduce the bits of the
    run that skips it."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    (w0, h0, c0), (w1, h1, c1), (w2, h2, c2) = q.get(timeout=900)
    p.join(timeout=120)
    assert p.exitcode == 0
    assert np.array_equal(w0, w1) and np.array_equal(h0, h1) and np.array_equal(c0, c1)
    assert np.array_equal(w0, w2) and np.array_equal(h0, h2) and np.array_equal(c0, c2)  # ... and through the C-side ncclAllReduce


def test_bench_launches_its_own_ranks(tmp_path):
    """`python bench.py --gpus N` with no launcher around it (no WORLD_SIZE) must start the N ranks itself and print
    ONE line with n_gpus = N (it used to solve the whole problem on one GPU and report n_gpus 1).  The
    parent never touches HIP; the two children share this box's one GPU over gloo (SNMF_DIST_BACKEND /
    SNMF_FORCE_DEVICE are the single-GPU dry-run switches of bench.py) -- on an 8-GPU node the same code path runs one
    rank per GPU over RCCL.  --dump-outputs gathers the sampled frames of H from both ranks."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(SNMF_DIST_BACKEND="gloo", SNMF_FORCE_DEVICE="0")
    pr = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
                         "--T", "6400", "--r", "64", "--no-cpu-baseline", "--c5-T", "12800", "--c4-T", "9600", "--full",
                         "--dump-outputs", str(tmp_path)], env=env, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, pr.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["warmup"] == 2 and d["value"] > 0
    assert d["w_replicas_bit_identical"] is True
    assert d["scaling"] == "strong" and "frames/2" in d["config"]["parallelism"]
    assert len(d["roofline"]["kernel_ms_per_rank"]) == 2 and all(k["hstep"] > 0 for k in d["roofline"]["kernel_ms_per_rank"])
    assert d["final_cost"] and d["final_cost"] > 0
    w, h, cost = (np.load(tmp_path / f"{n}.npy") for n in ("w", "h_sample", "cost"))
    assert w.shape == (257, 64) and w.dtype == np.float64 and h.shape == (64, 6400) and h.dtype == np.float32
    assert cost[-1] == d["final_cost"] and np.isfinite(h).all() and (h >= 0).all()
    # the same sharded problem through the one-shot peer-store exchange behind the C ABI, reported beside the RCCL leg
    # (here: two ranks on the one device, hipEvents ordering); a failure of this leg would be an "error" string, not a crash
    one = d["exchange_oneshot"]
    assert "error" not in one, one
    assert one["ms_per_step"] > 0 and one["devices"] == [0, 0] and one["steps"] == 4
    assert abs(one["final_cost"] - d["final_cost"]) <= 1e-6 * d["final_cost"]
    # the extra strong-scaling leg on BASELINE configs[4] (beta = 2, r = 512; here with few frames), beside `value`
    c5 = d["c5_strong"]
    assert "error" not in c5, c5
    assert c5["ms_per_step"] > 0 and c5["steps"] == 10 and c5["final_cost"] > 0 and "r=512" in c5["workload"]
    # ... and the sharded basis-training path of BASELINE configs[3] (run_basis_DNMF.m:36-55: three solves, A_hat resident)
    c4 = d["c4_dnmf"]
    assert "error" not in c4, c4
    assert c4["seconds"] > 0 and c4["value"] > 0 and c4["scaling"] == "strong" and c4["frames_total"] == 9600 and c4["final_cost_solve3"] > 0
    # ... whose line carries the same problem on rank 0's GPU alone: same matrices, same initial values -> the same final cost
    assert "one_gpu_error" not in c4, c4
    assert c4["seconds_one_gpu"] > 0 and c4["strong_scaling_vs_one_gpu"] > 0
    assert abs(c4["final_cost_solve3_one_gpu"] - c4["final_cost_solve3"]) <= 1e-6 * c4["final_cost_solve3"]


def test_bench_extra_legs_cannot_cost_the_headline_line():
    """The N > 1 line's extra legs (C5, the sharded DNMF, the one-shot exchange) run behind a timer: when they do not come back --
    a rank failed inside a loop and its peers sit in a collective -- rank 0 still prints the ONE line with the headline
    measurement, the legs marked as timed out, and every rank exits cleanly."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(SNMF_DIST_BACKEND="gloo", SNMF_FORCE_DEVICE="0", SNMF_BENCH_EXTRA_TIMEOUT="0.001")
    pr = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
                         "--T", "6400", "--r", "64", "--no-cpu-baseline", "--full"], env=env, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, pr.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["steps"] == 4
    assert "timed out" in d["c5_strong"]["error"] and "timed out" in d["c4_dnmf"]["error"]


def test_bench_single_gpu_line_keeps_the_contract():
    """One GPU, launcher-less --full invocation: ONE JSON line with the contract's keys, the roofline object (bound,
    achieved, peak, unit, frac, traffic, measured on the engine's stream with HIP events) and -- with the CPU leg on -- the
    cpu_baseline object.  Small T so that the oracle's sample takes seconds."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    pr = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "5", "--warmup", "2", "--T", "6400", "--r", "64", "--full"],
                        env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, pr.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None and "workload" in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == pytest.approx(157.3)
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"]) and 0 < rf["frac"] < 1 and "traffic" in rf
    assert rf["kernel_ms"]["hstep"] > 0 and rf["kernel_ms"]["wstats"] > 0
    assert rf["kernel"] in ("k_hstep_rp", "k_hstep_rh", "k_hstep", "k_wstats") and rf["kernel"] in d["config"]["geometry"] + " k_wstats"
    assert "separate" in rf["kernel_ms_note"].lower() and "traffic_source" in rf
    # sense, not only keys: the dominant kernel's own time fits inside a step; a quoted traffic figure belongs to the kernel
    # the line names and is at least that kernel's algorithmic bytes
    dom = "hstep" if rf["kernel"].startswith("k_hstep") else "wstats"
    assert rf["kernel_ms"][dom] <= 1.05 * d["ms_per_step"]
    assert rf["algorithmic_bytes_per_launch"] > 0
    if rf["traffic"] is not None:
        assert rf["traffic_source"]["kernel"].startswith(rf["kernel"] + "<")
        assert rf["traffic"] >= rf["algorithmic_bytes_per_launch"] and rf["traffic_ratio"] == pytest.approx(rf["traffic"] / rf["algorithmic_bytes_per_launch"])
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] in ("port", "reference") and cb["sample"]
    # the cold number beside the settled one: a resident 200-iteration (BASELINE configs[1]) and a 100-iteration solve (the
    # reference's default max_iter) from the random start.  At the bench's own size it is never faster than the settled `value`
    # (2 105 against 2 163 it/s: dense random activations draw more power, the clock follows); on THIS test's shape a step is 45 us of
    # launch latency, `value` is timed over 5 steps with one sync and the cold solve over 200, so only the order of magnitude binds
    assert d["from_random_start"] is not None, d["from_random_start_detail"]
    assert 0 < d["from_random_start"] <= 3.0 * d["value"]  # (observed on this shape: 0.9 .. 1.4 x `value`, whose five steps are mostly launch jitter)
    fr = d["from_random_start_detail"]
    assert fr["iters_200"]["iterations_per_s"] == d["from_random_start"] and fr["iters_100"]["iterations_per_s"] > 0


def test_bench_plain_run_is_lean_and_dumps_what_it_computed(tmp_path):
    """A plain run prints the headline line and nothing it does not need (no event pass, no extra legs, no CPU baseline); with
    --dump-outputs it writes what the timed plan holds after its last step -- W, the seeded frame sample of H, the objective of
    every iteration -- and a --full run of the same arguments, whose timed plan starts from the same inputs, writes the same bits."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-dropin"])):
        pr = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "5", "--warmup", "2", "--T", "20000", "--r", "64",
                             "--dump-outputs", str(tmp_path / mode)] + extra, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr[-2000:]
        out = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, pr.stdout
        lines[mode] = json.loads(out[0])
    d = lines["plain"]
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "final_cost"):
        assert k in d, k
    for k in ("roofline", "cost_vs_oracle", "from_random_start", "dropin", "cpu_baseline"):
        assert k not in d, k
    assert "roofline" in lines["full"] and d["steps"] == 5 and d["value"] == pytest.approx(1e3 / d["ms_per_step"])
    got = {m: {n: np.load(tmp_path / m / f"{n}.npy") for n in ("w", "h_sample", "div", "cost")} for m in lines}
    p = got["plain"]
    assert p["w"].shape == (257, 64) and p["w"].dtype == np.float64
    assert p["h_sample"].shape == (64, bench.H_SAMPLE) and p["h_sample"].dtype == np.float32
    assert bench.SETTLE + 5 <= len(p["cost"]) == len(p["div"]) <= bench.SETTLE + 2 + 5 and (p["cost"] > 0).all()
    assert p["cost"][-1] == d["final_cost"]
    assert sum(a.nbytes for a in p.values()) <= 64 << 20
    for n in p:
        np.testing.assert_array_equal(p[n], got["full"][n], err_msg=n)


def _dnmf_worker(rank, world, port, prob, q):
    import torch
    import torch.distributed as dist
    from se_snmf_nat_amd.dist import run_basis_dnmf_sharded, shard_bounds
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    Y, X, D, B, R_x, R_d, p = prob
    T = Y.shape[1]
    t0, t1 = shard_bounds(T, world, rank)
    B_hat, A_loc = run_basis_dnmf_sharded(Y[:, t0:t1], X[:, t0:t1], D[:, t0:t1], B, R_x, R_d, p, device=0, columns=(t0, T))
    q.put((rank, B_hat, A_loc))
    dist.barrier()
    dist.destroy_process_group()
    torch.cuda.synchronize()


def test_sharded_dnmf_loop_world2_equals_the_unsharded_call(gpu_ctx):
    """run_basis_DNMF.m:36-55 with the frames sharded over two ranks (gloo, one GPU) against the unsharded host mirror: every
    rank starts solve 1 from ITS columns of the unsharded call's rand(r, n) (dist.h0_columns), so A_hat -- frames are
    independent given W, nothing but the two cost scalars is exchanged -- comes out BIT FOR BIT the same for any number of
    ranks, early stop included; B_hat's statistics are summed in another order (per rank, then across ranks: fp64), which
    moves W by a few fp32 ulp."""
    import torch.multiprocessing as mp
    from se_snmf_nat_amd import run_basis_dnmf
    rs = np.random.default_rng(8)
    F, T, R_x, R_d = 513, 900, 12, 9
    X = rs.gamma(0.5, 1.0, (F, 6)) @ rs.gamma(0.3, 1.0, (6, T)) + 1e-9
    D = rs.gamma(0.5, 1.0, (F, 5)) @ rs.gamma(0.3, 1.0, (5, T)) + 1e-9
    Y = X + D
    B = rs.random((F, R_x + R_d)) + 0.05
    p = dict(cf="kl", sparsity=5, max_iter=40, conv_eps=1e-3, cost_check=1, random_seed=1)
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dnmf_worker, args=(rk, world, port, (Y, X, D, B, R_x, R_d, p), q)) for rk in range(world)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda x: x[0])
    for pr in procs:
        pr.join(timeout=120)
        assert pr.exitcode == 0
    B1, A1 = run_basis_dnmf(Y, X, D, B, R_x, R_d, p, ctx=gpu_ctx)
    A = np.concatenate([r_[2] for r_ in res], axis=1)
    assert np.array_equal(res[0][1], res[1][1]), "replicas of B_hat must be bit-identical across ranks"
    assert np.array_equal(A, A1)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert rel(res[0][1], B1) < 5e-6


def test_run_sharded_in_the_library_equals_the_step_api(gpu_ctx):
    """snmf_plan_run_sharded (the process-per-GPU loop inside the library, the collective as a callback) against the same loop
    driven call by call over the step API: identical W, H and objective vectors; the callback is called once per iteration on
    the whole statistics buffer (+ once on the two cost scalars for the final objective); an exception raised inside the
    callback comes back as that exception, not as a crash in the C frame.  src/sparse_nmf.m:186-286 per rank."""
    import torch
    from se_snmf_nat_amd import Plan
    F, T, r, iters = 129, 3000, 24, 7
    V, W0, H0 = synth_problem(F, T, r)

    def make():
        pl = Plan(gpu_ctx, F, T, r, beta=1.0, max_iter=iters, conv_eps=0.0, cost_check=True, sparsity=2.0)
        pl.set_v(V); pl.set_w(W0); pl.set_h(H0); pl.init()
        return pl, torch.zeros(pl.stats_len(), dtype=torch.float64, device="cuda:0")

    a, sa = make()
    torch.cuda.synchronize()
    for _ in range(iters):
        a.hstep(); a.wstats(sa.data_ptr()); a.wapply(sa.data_ptr())
    a.objstats(sa.data_ptr()); a.objapply(sa.data_ptr())
    b, sb = make()
    torch.cuda.synchronize()
    calls = []
    ran = b.run_sharded(iters, sb.data_ptr(), lambda ptr, n: calls.append((ptr - sb.data_ptr(), n)))
    assert ran == iters
    assert calls == [(0, b.stats_len())] * iters + [((b.stats_len() - 2) * 8, 2)]
    assert np.array_equal(a.get_w(), b.get_w()) and np.array_equal(a.get_h(), b.get_h())
    assert np.array_equal(a.get_objective()[1], b.get_objective()[1])
    a.close(); b.close()
    c, sc = make()

    def boom(ptr, n):
        raise RuntimeError("collective failed")
    with pytest.raises(RuntimeError, match="collective failed"):
        c.run_sharded(3, sc.data_ptr(), boom)
    c.close()


def test_device_block_cache_does_not_leak_state(monkeypatch):
    """A context hands the device blocks of a destroyed plan to the next plan of the same sizes (SNMF_DEVCACHE_MB): the second
    solve must not see anything of the first -- same results as on a context with the cache off."""
    from se_snmf_nat_amd import Context, sparse_nmf
    V, W0, H0 = synth_problem(129, 2500, 24)
    V2, W2, H2 = synth_problem(129, 2500, 24, seed=7) if "seed" in synth_problem.__code__.co_varnames else (V[:, ::-1].copy(), W0[::-1].copy(), H0[:, ::-1].copy())
    p1 = dict(cf="kl", sparsity=3.0, max_iter=6, conv_eps=0, cost_check=1, init_w=W0, init_h=H0)
    p2 = dict(cf="kl", sparsity=1.0, max_iter=6, conv_eps=0, cost_check=1, init_w=W2, init_h=H2)
    monkeypatch.setenv("SNMF_DEVCACHE_MB", "0")
    c0 = Context(0)
    ref = sparse_nmf(V2, p2, ctx=c0)
    c0.close()
    monkeypatch.delenv("SNMF_DEVCACHE_MB")
    c1 = Context(0)
    sparse_nmf(V, p1, ctx=c1)          # fills the cache with this solve's blocks
    got = sparse_nmf(V2, p2, ctx=c1)   # same sizes: every block is a reused one
    c1.close()
    assert np.array_equal(ref[0], got[0]) and np.array_equal(ref[1], got[1])
    assert np.array_equal(ref[2]["cost"], got[2]["cost"])
