"""Data-parallel correctness on ONE GPU (pytest -m gpu): the kernels of a rank see only its ray shard, the
all-reduce sums the shards' gradients and 1/world averages them.  Here the two "ranks" are two
half-batches evaluated one after the other in this process -- no extra processes on the card -- and their
summed, halved gradients must equal the gradient of the full batch, for both engines; then the
reduce-callback protocol (asynchronous collectives per parameter range) is driven with a recording callback."""
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True) * 4.0311
    tgt = (torch.rand(n, 3, generator=g) - 0.5) * 1.6
    d = tgt - o
    return o.cuda(), (d / d.norm(dim=-1, keepdim=True)).cuda(), torch.rand(n, 3, generator=g).cuda(), g


def test_vanilla_shard_gradients_sum_to_full_batch_gradient():
    from project_nerf_amd.engine import VanillaNerfEngine
    from project_nerf_amd.parallel import shard_range
    R, S, world = 512, 64, 2
    o, d, target, g = _rays(R, 5)
    u = torch.rand(R, S, generator=g).cuda()
    eng = VanillaNerfEngine(seed=0)
    loss_full = float(eng.compute_gradients(o, d, target, S, u=u))
    full = eng.grads.clone()
    acc, losses = torch.zeros_like(full), []
    for rank in range(world):
        lo, hi = shard_range(R, rank, world)
        losses.append(float(eng.compute_gradients(o[lo:hi].contiguous(), d[lo:hi].contiguous(), target[lo:hi].contiguous(), S,
                                                  u=u[lo:hi].contiguous())))
        acc += eng.grads                                   # what the summing all-reduce leaves in the buffer
    acc /= world                                           # grad_scale = 1/world in the optimiser kernel
    assert abs(np.mean(losses) - loss_full) < 1e-5 * max(1.0, loss_full)
    rel = float((acc - full).norm() / full.norm())
    # not bit-identical: each launch derives its own e5m2 gradient scale from its own largest derivative, and float
    # atomics sum in a different order
    assert rel < 1e-2, rel


def test_instant_shard_gradients_sum_to_full_batch_gradient():
    from project_nerf_amd.engine import InstantNgpEngine
    from project_nerf_amd.parallel import shard_range
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2_instant.yaml.example")))
    R, S, world = 1024, 64, 2
    o, d, target, g = _rays(R, 9)
    u = torch.rand(R, S, generator=g).cuda()
    eng = InstantNgpEngine(cfg, seed=0)
    eng.table.copy_((torch.rand(eng.table.numel(), generator=g) - 0.5).cuda())      # visible densities and colours
    eng.net[2048:2048 + 64] *= 20.0
    from project_nerf_amd import ops
    ops.imlp_pack(eng.net, eng.packed)
    ax = torch.linspace(-1.5, 1.5, 128)
    gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
    eng.binary_grid = ((gx ** 2 + gy ** 2 + gz ** 2) < 1.2 ** 2).cuda()            # part of the samples skipped
    loss_full = float(eng.compute_gradients(o, d, target, S, u=u))
    full_t, full_n = eng.g_table.clone(), eng.g_net.clone()
    acc_t, acc_n, losses = torch.zeros_like(full_t), torch.zeros_like(full_n), []
    seen = []
    for rank in range(world):
        lo, hi = shard_range(R, rank, world)
        # the data-parallel form: gradient ranges handed to the reduce callback as soon as they are complete
        losses.append(float(eng.compute_gradients(o[lo:hi].contiguous(), d[lo:hi].contiguous(), target[lo:hi].contiguous(), S,
                                                  u=u[lo:hi].contiguous(), sync_grads_async=lambda v: seen.append(v.numel()))))
        acc_t += eng.g_table
        acc_n += eng.g_net
    acc_t /= world
    acc_n /= world
    assert abs(np.mean(losses) - loss_full) < 1e-5 * max(1.0, loss_full)
    assert float(full_t.norm()) > 0 and float(full_n.norm()) > 0
    assert float((acc_t - full_t).norm() / full_t.norm()) < 1e-4
    assert float((acc_n - full_n).norm() / full_n.norm()) < 1e-3
    # every rank handed over the tiny-MLP gradients first, then level groups that tile the whole table exactly once
    per_rank = len(seen) // world
    assert seen[0] == eng.g_net.numel() and sum(seen[1:per_rank]) == eng.g_table.numel() and per_rank >= 3


def test_tv_weight_is_independent_of_world_size_in_the_engine():
    """One step of an engine that believes it is 1 of 4 ranks, fed the gradient of 4 identical shards (sum = 4 g),
    must equal one single-rank step with g: in particular the TV term keeps its weight (reference run.py:611-618)."""
    from project_nerf_amd.engine import InstantNgpEngine
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2_instant.yaml.example")))
    cfg["tv_loss_weight"] = 1e-2
    o, d, target, g = _rays(256, 3)
    u = torch.rand(256, 64, generator=g).cuda()
    outs = []
    for world in (1, 4):
        eng = InstantNgpEngine(cfg, seed=0, world_size=world)
        eng.table.copy_((torch.rand(eng.table.numel(), generator=torch.Generator().manual_seed(1)) - 0.5).cuda() * 0.1)
        eng.compute_gradients(o, d, target, 64, u=u)
        eng.g_table *= world
        eng.g_net *= world                                  # the summing all-reduce over identical shards
        eng.apply_gradients()
        outs.append((eng.table.clone(), eng.net.clone()))
    # not bit-equal: the clip norm is an atomic fp32 sum whose order changes from run to run
    assert float((outs[0][0] - outs[1][0]).abs().max()) < 1e-5
    assert float((outs[0][1] - outs[1][1]).abs().max()) < 1e-5


def test_native_rccl_comm_single_rank_world():
    """libnerf_comm.so on the one GPU of the box: a world of one rank through the real RCCL calls (bootstrap
    token, communicator, in-place all-reduce in fp32 and bf16 on a side stream, row-band gather to the root).
    More ranks need more GPUs: RCCL refuses two ranks on one device."""
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd._comm import NativeComm, NerfCommError
    uid = NativeComm.unique_id()
    assert len(uid) == 128
    comm = NativeComm(uid, 0, 1)
    try:
        g = torch.randn(595844, device="cuda")
        want = g.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            comm.allreduce_sum_(g)
            h = torch.randn(4096, device="cuda").to(torch.bfloat16)
            want_h = h.clone()
            comm.allreduce_sum_(h)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(g, want) and torch.equal(h, want_h)
        # the sharded optimiser's exchange on a world of one rank: both collectives are the identity on the rank's slice
        flat = torch.randn(4096, device="cuda")
        keep = flat.clone()
        comm.reduce_scatter_sum_(flat, 4096)
        half = torch.randn(4096, device="cuda").half()
        keep_h = half.clone()
        comm.all_gather_(half, 4096)
        torch.cuda.synchronize()
        assert torch.equal(flat, keep) and torch.equal(half, keep_h)
        band = torch.rand(100, 800, 3, device="cuda")
        img = comm.gather_row_bands(band, 100, dst=0)
        torch.cuda.synchronize()
        assert torch.equal(img, band)
        with pytest.raises(TypeError):
            comm.allreduce_sum_(torch.zeros(4, device="cuda", dtype=torch.float16))
        with pytest.raises(NerfCommError):
            comm.allreduce_sum_(torch.zeros(4))
    finally:
        comm.close()


def test_engine_step_over_the_native_comm_equals_the_plain_step():
    """VanillaNerfEngine.train_step with the gradient ranges handed to libnerf_comm.so (world of one rank: the sum
    is the identity, the stream hand-over and the callback protocol are the real ones) == the step without."""
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import parallel
    from project_nerf_amd._comm import NativeComm
    from project_nerf_amd.engine import VanillaNerfEngine
    comm = NativeComm(NativeComm.unique_id(), 0, 1)
    try:
        o, d, target, _ = _rays(512, 5)
        u = torch.rand(512, 64, generator=torch.Generator().manual_seed(3)).cuda()
        outs = []
        for cb in (None, parallel.native_allreduce_sum_async(comm)):
            eng = VanillaNerfEngine(seed=2)
            eng.compute_gradients(o, d, target, 64, u=u, sync_grads_async=cb)
            outs.append(eng.grads.clone())
            eng.apply_gradients()
        torch.cuda.synchronize()
        # float-atomic order inside wgrad is the only difference
        assert float((outs[0] - outs[1]).norm() / outs[0].norm()) < 1e-5
    finally:
        comm.close()


@pytest.mark.parametrize("workload", ["vanilla", "instant"])
def test_bench_two_rank_control_flow_on_one_device(workload, tmp_path):
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank), rehearsed on
    the one GPU of the box: both ranks on device 0, gloo instead of RCCL.  Covers what no single-process test
    can: every rank takes part in every collective of the run (timed steps, the in-step timing repetitions, the
    replica check, the row-band gather), rank 0 prints ONE JSON line with whole-job throughput."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, NERF_BENCH_SINGLE_DEVICE="1", NERF_DIST_BACKEND="gloo", NERF_BENCH_DP_ITERS="48")
    port = 29650 + (0 if workload == "vanilla" else 1)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--frames", "6",
           "--full", "--no-cpu-baseline", "--render-frames", "1"]
    if workload == "instant":
        cmd += ["--workload", "instant"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["steps"] == 4
    per_rank = 4096 if workload == "vanilla" else 16384
    assert abs(out["value"] - 2 * per_rank / (out["ms_per_step"] * 1e-3)) < 1e-3 * out["value"]     # whole-job rays/s
    assert out["render_fps"] > 0
    if workload == "instant":
        assert out["replica_divergence"] == 0.0
    else:
        assert set(out["kernels_in_step"]) >= {"fwd", "loss", "dgrad", "wgrad", "adam+pack"}
        assert all(v["ms"] > 0 for v in out["kernels_in_step"].values())


def test_instant_rank_without_active_samples_issues_the_same_collectives():
    """A rank whose whole shard misses the occupied cells (n == 0) must enter exactly the collectives its peers
    enter -- same order, same element counts, same wire dtype -- or RCCL hangs / corrupts memory (round-2 advisor
    finding: the empty branch all-reduced the whole table in one call, the others per level group)."""
    from project_nerf_amd.engine import InstantNgpEngine
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2_instant.yaml.example")))
    R, S = 256, 32
    o, d, target, g = _rays(R, 21)
    u = torch.rand(R, S, generator=g).cuda()
    eng = InstantNgpEngine(cfg, seed=0)

    def schedule(grid, wire):
        calls = []
        eng.binary_grid = grid
        loss = eng.compute_gradients(o, d, target, S, u=u, sync_grads_async=lambda v: calls.append((v.numel(), v.dtype)), reduce_dtype=wire)
        assert torch.isfinite(loss)
        return calls
    full = torch.ones(128, 128, 128, dtype=torch.bool, device="cuda")
    for wire in (None, torch.bfloat16):
        busy, idle = schedule(full, wire), schedule(torch.zeros_like(full), wire)
        assert busy == idle and len(busy) == 1 + len(eng.level_groups()), (busy, idle)
        assert sum(nel for nel, _ in busy[1:]) == eng.g_table.numel()
    assert float(eng.g_table.abs().max()) == 0.0 and float(eng.g_net.abs().max()) == 0.0     # the idle rank contributes zeros


def test_vanilla_loss_is_a_copy_not_a_view_of_the_scalar_ring():
    from project_nerf_amd.engine import VanillaNerfEngine
    o, d, target, g = _rays(64, 3)
    eng = VanillaNerfEngine(seed=0)
    first = eng.compute_gradients(o, d, target, 64)
    kept = float(first)
    eng._scalars.zero_()                                   # what happens to the ring every 1024 steps
    eng.compute_gradients(o, d, target, 64)
    assert float(first) == kept and kept > 0.0
