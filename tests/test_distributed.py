"""Multi-GPU path on CPU: world_size-2 `gloo` runs of the sharding + pose-gather logic
(semantic_suma_amd/distributed.py).  There is no GPU here, so the per-rank compute is the CPU oracle
(test infrastructure standing in for the HIP pipeline, which has the same interface and -- by the GPU
parity tests -- the same bits); what is under test is the distribution: LPT sequence assignment,
hypothesis sharding, the single all_gather of poses and the rank-consistent winner selection."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 180, 16


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, mode, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from oracle import pyoracle
    from semantic_suma_amd import synth
    from semantic_suma_amd.distributed import gather_poses, hypothesis_starts, lpt_assign, pick_winner
    from semantic_suma_amd.types import params_with_size
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p = params_with_size(W, H, max_iterations=6)
    try:
        if mode == "sequences":
            lengths = [3, 1, 2]  # scans per sequence
            assign, loads = lpt_assign(lengths, world)
            poses = np.zeros((len(lengths), 4, 4))
            for seq in assign[rank]:
                pipe = pyoracle.OraclePipeline(p)
                for k in range(lengths[seq]):
                    pts, lab, prob, _ = synth.generate_scan(100 * seq + k, n_azimuth=W, height=H)
                    pipe.process_scan(pts, lab, prob, fixed_iterations=6)
                poses[seq] = pipe.pose()
            allp = gather_poses(poses)  # [world, n_seq, 4, 4]; one collective for the whole job
            merged = allp.sum(axis=0)   # every sequence is owned by exactly one rank
            q.put((rank, assign, loads, merged))
        else:
            ora = pyoracle.Oracle(p)
            s0 = synth.generate_scan(0, n_azimuth=W, height=H)
            s1 = synth.generate_scan(1, n_azimuth=W, height=H)
            f0 = ora.preprocess(*s0[:3], 20, ora.frame())
            f1 = ora.preprocess(*s1[:3], 21, ora.frame())
            T0 = np.eye(4)
            T0[0, 3] = 1.0
            starts = hypothesis_starts(T0, 4)
            local = np.zeros((4, 18))
            for k in range(rank, 4, world):  # hypothesis k lives on rank k % world
                T, _, st = ora.minimize(f1, f0, starts[k])
                local[k, :16], local[k, 16], local[k, 17] = T.ravel(), st.error, st.valid
            allr = gather_poses(local).sum(axis=0)
            win = pick_winner([(allr[k, 16], allr[k, 17]) for k in range(4)])
            q.put((rank, win, allr))
    finally:
        dist.destroy_process_group()


class OracleEngine:
    """CPU stand-in with the engine interface of semantic_suma_amd.distributed.HipEngine (test infrastructure)"""

    def __init__(self, params):
        from oracle import pyoracle
        self.params = params
        self.ora = pyoracle.Oracle(params)
        self.current = self.ora.frame()
        self.model = self.ora.frame(model=True)

    def preprocess(self, points, labels, probs, t):
        self.ora.preprocess(points, labels, probs, t, self.current)

    def render(self, pose, ct):
        self.ora.map_render(pose, pose, ct, self.model)

    def minimize(self, starts):
        out, stats = [], []
        for T0 in starts:
            T, _, st = self.ora.minimize(self.current, self.ora.map_frame(1), T0)
            out.append(T)
            stats.append((st.error, st.valid, st.outlier))
        return np.stack(out), stats

    def update(self, pose):
        self.ora.map_update(pose, self.current)

    def map_bytes(self):
        return self.ora.map_surfels().tobytes()


def _hyp_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import hashlib
    import torch.distributed as dist
    from semantic_suma_amd import synth
    from semantic_suma_amd.distributed import run_hypotheses
    from semantic_suma_amd.types import params_with_size
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = params_with_size(W, H, max_iterations=5)
        scans = [synth.generate_scan(k, n_azimuth=W, height=H)[:3] for k in range(4)]
        eng = OracleEngine(p)
        poses, winners = run_hypotheses(eng, scans, 4, rank, world)
        q.put((rank, poses, winners, hashlib.sha256(eng.map_bytes()).hexdigest()))
    finally:
        if world > 1:
            dist.destroy_process_group()


def test_run_hypotheses_world2_equals_world1(oracle_lib):
    """the config-3 runner (semantic_suma_amd.distributed.run_hypotheses): two ranks reach the same winners, poses
    and maps as one process that runs all hypotheses itself"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_hyp_worker, args=(r, 2, port, q)) for r in range(2)]
    procs.append(ctx.Process(target=_hyp_worker, args=(0, 1, _free_port(), q)))
    for pr in procs:
        pr.start()
    out = [q.get(timeout=300) for _ in procs]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    assert len(out) == 3
    ref = out[0]
    for o in out[1:]:
        assert np.array_equal(o[1], ref[1]) and o[2] == ref[2] and o[3] == ref[3]
    assert ref[2][0] == -1 and all(0 <= w < 4 for w in ref[2][1:])
    assert ref[1][-1][0, 3] > 1.0  # it moved along x


def test_run_sequences_threads(oracle_lib):
    """the config-4 runner on one rank that owns three sequences: concurrent pipelines, one per thread"""
    from oracle import pyoracle
    from semantic_suma_amd import synth
    from semantic_suma_amd.distributed import lpt_assign, run_sequences
    from semantic_suma_amd.types import params_with_size
    p = params_with_size(W, H, max_iterations=4)

    class Pipe:
        def __init__(self):
            self.op = pyoracle.OraclePipeline(p)

        def processScan(self, pts, lab, prob, fixed_iterations=0):
            self.op.process_scan(pts, lab, prob, fixed_iterations)

        def getCurrentPose(self):
            return self.op.pose()

    lengths = [3, 2, 2, 1]
    assign, _ = lpt_assign(lengths, 2)

    def scans_of(seq):
        for k in range(lengths[seq]):
            yield synth.generate_scan(100 * seq + k, n_azimuth=W, height=H)[:3]

    a = run_sequences(assign[0] + assign[1], Pipe, scans_of, fixed_iterations=4, threads=True)
    b = run_sequences(assign[0] + assign[1], Pipe, scans_of, fixed_iterations=4, threads=False)
    assert sorted(a) == [0, 1, 2, 3] and all(a[s][0] == lengths[s] for s in a)
    assert all(np.array_equal(a[s][1], b[s][1]) for s in a)


def _run(mode):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, mode, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    out = [q.get(timeout=240) for _ in procs]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    return sorted(out, key=lambda o: o[0])


def _native_gather_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from semantic_suma_amd.distributed import NativeGather, gather_poses
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        class NoCtx:  # a machine without a GPU has no suma_ctx: the bootstrap must say so before anybody needs one
            h = None
        ng = NativeGather(NoCtx(), device=torch.device("cpu"))
        # what bench.py does with the answer: every rank takes the SAME branch
        got = gather_poses(np.full((4, 4), float(rank))) if not ng.ok else None
        q.put((rank, ng.ok, ng.error, None if got is None else got[:, 0, 0].tolist()))
    finally:
        dist.destroy_process_group()


def test_native_gather_bootstrap_fails_together_without_a_gpu():
    """`bench.py --gpus N` gathers its poses through libsuma_hip_dist.so (suma_gather_poses), bootstrapped over the
    launcher's process group (semantic_suma_amd.distributed.NativeGather).  N > 1 ranks on RCCL cannot run here -- but
    the protocol around it can: two gloo ranks on a machine without a GPU.  The library loads, rank 0's RCCL id reaches
    rank 1, ncclCommInitRank fails on both (no device), and BOTH ranks leave the constructor with ok = False and a reason --
    nobody hangs in a collective the other side never enters -- and fall back to the same torch.distributed gather."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_native_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    out = sorted(q.get(timeout=240) for _ in procs)
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    assert [o[0] for o in out] == [0, 1]
    assert all(o[1] is False and o[2] for o in out), out   # both refused, both know why
    assert all(o[3] == [0.0, 1.0] for o in out), out        # and the fallback gather ran on both


def test_lpt_assignment():
    from semantic_suma_amd.distributed import lpt_assign
    kitti = [4541, 1101, 4661, 801, 271, 2761, 1101, 1101, 4071, 1591, 1201]  # odometry 00-10 scan counts
    assign, loads = lpt_assign(kitti, 8)
    assert sorted(i for a in assign for i in a) == list(range(11))
    assert max(loads) == 4661  # makespan bound by the longest sequence
    assert lpt_assign([5], 4)[0] == [[0], [], [], []]


def test_sequence_sharding_gloo_world2(oracle_lib):
    (r0, a0, l0, m0), (r1, a1, l1, m1) = _run("sequences")
    assert a0 == a1 and l0 == l1 and sorted(a0[0] + a0[1]) == [0, 1, 2]
    assert np.array_equal(m0, m1)  # both ranks end with the same gathered trajectory endpoints
    assert all(abs(np.linalg.det(m0[s][:3, :3]) - 1) < 1e-9 for s in range(3))
    assert abs(m0[0][0, 3]) > 0.5  # sequence 0 (3 scans) moved


def test_hypothesis_sharding_gloo_world2(oracle_lib):
    (r0, w0, a0), (r1, w1, a1) = _run("hypotheses")
    assert w0 == w1 and np.array_equal(a0, a1)
    assert (a0[:, 17] > 0).all()  # every hypothesis was evaluated by exactly one rank
    best = min(range(4), key=lambda k: a0[k, 16] / a0[k, 17])
    assert w0 == best


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus N` without a launcher re-executes itself under torch.distributed.run with N ranks
    (round-3 review: --gpus was parsed and ignored); with WORLD_SIZE set, or N = 1, it is a rank and launches nothing"""
    import argparse
    import importlib.util
    spec = importlib.util.spec_from_file_location("suma_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    argv = ["--gpus", "8", "--steps", "20", "--warmup", "5"]
    cmd = bench.relaunch_command(8, argv, port=29511)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nnodes=1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == argv  # the rank processes get this process's own arguments
    calls = []

    def fake_run(c, env):
        calls.append((c, env))
        return 7

    ns = argparse.Namespace(gpus=8)
    assert bench.self_launch_if_needed(ns, argv=argv, environ={"PATH": "/x"}, run=fake_run) == 7
    (c, env), = calls
    assert c[c.index("--nproc-per-node") + 1] == "8" and c[-len(argv):] == argv
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" and "WORLD_SIZE" not in env
    # already a rank (a launcher set WORLD_SIZE), or a single GPU: run in this process
    assert bench.self_launch_if_needed(ns, argv=argv, environ={"WORLD_SIZE": "8"}, run=fake_run) is None
    assert bench.self_launch_if_needed(argparse.Namespace(gpus=1), argv=argv, environ={}, run=fake_run) is None
    assert len(calls) == 1


def test_bench_plain_run_switches_every_other_leg_off():
    """without --full a --mode single run takes no leg besides the headline, whatever the legs' own switches say; with
    --full, and in the other modes (--mode adapter reads --adapter-scans), the switches mean what they say"""
    import argparse
    import importlib.util
    import subprocess
    import sys
    spec = importlib.util.spec_from_file_location("suma_bench_full", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    asked = dict(cpu_scans=20, reference_gl_scans=3, adapter_scans=120, no_kernel_events=False, no_host_vectors=False,
                 no_reference_mode=False, no_loop_closure=False)
    assert set(bench.FULL_ONLY) == set(asked)
    plain = bench.plain_run(argparse.Namespace(full=False, mode="single", steps=20, warmup=5, **asked))
    assert {k: getattr(plain, k) for k in asked} == bench.FULL_ONLY and plain.steps == 20 and plain.warmup == 5
    assert plain.cpu_scans == 0 and plain.adapter_scans == 0 and plain.no_host_vectors and plain.no_kernel_events
    for full, mode in ((True, "single"), (False, "adapter"), (False, "hypotheses")):
        ns = bench.plain_run(argparse.Namespace(full=full, mode=mode, **asked))
        assert {k: getattr(ns, k) for k in asked} == asked
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "--full" in res.stdout


def test_bench_refuses_a_world_size_other_than_gpus():
    """`--gpus 4` under a launcher that started 2 ranks: a scaling point measured on another number of ranks than it
    claims is worthless, so bench.py exits non-zero instead of "using 2" (round-4 review, item 9)."""
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2"], env=env,
                         capture_output=True, timeout=300)
    assert res.returncode != 0
    assert b"--gpus 4 but the launcher started WORLD_SIZE=2" in res.stderr


def test_bench_scan_generation_pool_is_shared_between_the_ranks(monkeypatch):
    """bench.py generates a rank's synthetic scans with a pool of worker processes; N ranks of one node do that at the
    same time, so a rank's pool is what the cgroup grants (not what the box shows) divided by the ranks of the job"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("suma_bench_pool", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)
    # the generator yields the scans in order whatever the pool size (short stretch: generated in-process)
    monkeypatch.setenv("WORLD_SIZE", "8")
    ks = [3, 4, 5]
    out = list(bench.generate_scans(ks, 180, 16))
    assert len(out) == 3 and all(o[0].shape[1] == 4 for o in out)
    from semantic_suma_amd import synth
    assert np.array_equal(out[1][0], synth.generate_scan(4, n_azimuth=180, height=16)[0])
