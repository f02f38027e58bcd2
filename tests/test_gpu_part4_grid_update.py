"""nerf_p4_grid_update -- the Part 4 dual-hash field's occupancy-grid refresh as one density-only launch chain (points from the cell
index, ONE deformation gather per time anchor, deformation chain at a scalar t storing x_c alone, canonical gather, sigma-net alone
with the running maximum, threshold and count in its epilogue) -- against today's loop on the same inputs: nerf_grid_lattice ->
part4.forward_chain(train=False) on zero view directions at t = 0, 0.5, 1 -> torch.maximum -> ops.grid_threshold(prev, decay).  The
chain does the same arithmetic on the same values (the blend of three grids with unit weights is one grid's feature), so every
comparison is torch.equal.  Every comparison first checks on the LOOP form that it cannot pass vacuously: the threshold splits the
grid, every anchor is the strict maximum somewhere, the deformation matters, and the history both survives and is overwritten.
Tables of 2^12 / 2^14 entries per hashed level, no grid above 33^3: a few seconds in total."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT

pytestmark = pytest.mark.gpu

BOUND = 1.5
BATCH = 2 ** 18                       # the loop form's batch (GridEngine.lattice_density)
ANCHORS = (0.0, 0.5, 1.0)
N_PARAMS, S1_OFF, S2_ROW0, SCALE = 30145, 16832, 16832 + 64 * 64, 30144      # csrc/p4mlp.hip's flat layout: S1 [64,64], the density row of S2, displacement_scale
CFG = dict(mode="part4", n_levels=16, n_features_per_level=2, log2_hashmap_size=14, base_resolution=16, per_level_scale=1.5,
           scene_bound=BOUND, L_embed_dir=4, L_embed_time=10, hidden_dim=64, time_modulation_dim=64, time_modulation_layers=2,
           deform_n_levels=12, deform_n_features_per_level=2, deform_log2_hashmap_size=12, deform_base_resolution=16,
           deform_per_level_scale=1.5, deform_hidden_dim=64, grid_resolution=17, grid_threshold=0.01, near=2.0, far=6.0)


def formula_table(n, phase=0.0):
    """tests/golden/make_golden.py::instant_test_params, shifted per table as test_gpu_part4.part4_table does"""
    i = torch.arange(n, dtype=torch.float64)
    return (0.5 * torch.sin(0.37 * i + phase + 0.11 * (i % 7))).float()


NET_SEED, TIME_GAIN = 5, 0.1


def seeded_net(seed=None, scale=0.1):
    """seeded normal weights; the density row is amplified (sigma spread over several decades) and the time code's DIRECT columns
    into the sigma-net are scaled by TIME_GAIN, so that which anchor wins a cell is decided by the deformation, cell by cell, and
    not by the time alone for the whole grid (the 2^3 case has only the box's corners to show all three anchors winning)"""
    g = torch.Generator().manual_seed(NET_SEED if seed is None else seed)
    net = torch.randn(N_PARAMS, generator=g) * 0.15
    net[S2_ROW0:S2_ROW0 + 64] *= 8.0
    net[S1_OFF:S1_OFF + 64 * 64].view(64, 64)[:, 32:53] *= TIME_GAIN
    net[SCALE] = scale
    return net.cuda()


class Field:
    """four tables (fp32, and fp16 copies laid out as the engine's: views of ONE flat buffer, which the loop form gathers in one
    launch), packed networks with displacement_scale 0.1 and with 0, the two level tables"""

    def __init__(self):
        from project_nerf_amd import ops, part4
        self.levels_d, self.levels_c = ops.HashLevelTable(12, 12), ops.HashLevelTable(16, 14)
        nd, nc = 2 * self.levels_d.entries, 2 * self.levels_c.entries
        flat = torch.cat([formula_table(nd, 1.0), formula_table(nd, 2.0), formula_table(nd, 3.0), formula_table(nc, 0.0)]).cuda()
        self.flat = {False: flat, True: flat.half()}
        self.cut = [0, nd, 2 * nd, 3 * nd, 3 * nd + nc]
        self.net = seeded_net()
        self.packed = part4.pack(self.net)
        self.net0 = seeded_net(scale=0.0)
        self.packed0 = part4.pack(self.net0)
        self._loop = {}

    def tables(self, half, zero_deform=False):
        flat = self.flat[half]
        if zero_deform:
            flat = flat.clone()
            flat[:self.cut[3]] = 0
        return [flat[self.cut[k]:self.cut[k + 1]].view(-1, 2) for k in range(4)]

    def sigma_of(self, pts, t, tables, moving=True, hash_bound=BOUND):
        """today's field query, density part: DualHashEngine.field on zero view directions at one time, in the loop's batches"""
        from project_nerf_amd import part4
        n = pts.shape[0]
        sig = torch.empty(n, device="cuda")
        zeros = torch.zeros(min(n, BATCH), 3, device="cuda")
        for i in range(0, n, BATCH):
            p = pts[i:i + BATCH].contiguous()
            m = p.shape[0]
            ws = part4.Workspace(m, "cuda", train=False)
            _, s, _, _ = part4.forward_chain(self.packed if moving else self.packed0, self.net if moving else self.net0, tables, self.levels_d,
                                             self.levels_c, hash_bound, p, None, torch.full((m,), float(t), device="cuda"), zeros[:m], ws, False)
            sig[i:i + m] = s
        return sig

    def loop(self, res, half, grid_bound=BOUND, hash_bound=BOUND, zero_deform=False):
        """(sigma at the three anchors, their maximum, the maximum with displacement_scale 0) on the lattice by today's sequence,
        computed once per case and never written to (callers clone)"""
        from project_nerf_amd import ops
        key = (res, half, grid_bound, hash_bound, zero_deform)
        if key not in self._loop:
            pts = ops.grid_lattice(grid_bound, res, "cuda")
            tables = self.tables(half, zero_deform)
            sig = [self.sigma_of(pts, t, tables, True, hash_bound).view(res, res, res) for t in ANCHORS]
            still = [self.sigma_of(pts, t, tables, False, hash_bound).view(res, res, res) for t in ANCHORS]
            fold = lambda s: torch.maximum(torch.maximum(s[0], s[1]), s[2])
            self._loop[key] = (sig, fold(sig), fold(still))
        return self._loop[key]

    def chain(self, res, half, thr, prev, decay, grid_bound=BOUND, hash_bound=BOUND, zero_deform=False, **kw):
        from project_nerf_amd import ops
        return ops.p4_grid_update(self.packed, self.net, self.tables(half, zero_deform), self.levels_d, self.levels_c, hash_bound, res,
                                  grid_bound, thr, prev, decay, **kw)


@pytest.fixture(scope="module")
def field():
    import project_nerf_amd  # noqa: F401
    return Field()


def history(res, thr, seed=17):
    """a random non-negative running density in [0.5, 1.5] x threshold: it straddles the threshold"""
    g = torch.Generator().manual_seed(seed + res)
    return (thr * (0.5 + torch.rand(res, res, res, generator=g))).cuda()


def loop_case(field, res, half, decay, **kw):
    """(threshold, history, (grid, binary, count) of today's fold) with the conditions that keep a comparison from being vacuous
    asserted on the loop form"""
    from project_nerf_amd import ops
    sig, fold, still = field.loop(res, half, **kw)
    thr = float(fold.median())
    for k in range(3):                                                 # every anchor is the strict maximum in at least one cell
        others = torch.maximum(sig[(k + 1) % 3], sig[(k + 2) % 3])
        assert bool((sig[k] > others).any()), f"anchor {ANCHORS[k]} never wins"
    assert not torch.equal(fold, still), "displacement_scale 0 leaves sigma unchanged: the deformation does not matter"
    prev = history(res, thr)
    assert float(prev.min()) > 0.0
    decayed = prev * decay
    kept, overwritten = decayed > fold, fold > decayed
    assert bool(kept.any()) and bool(overwritten.any()), (int(kept.sum()), int(overwritten.sum()))
    grid = prev.clone()
    binary, ratio = ops.grid_threshold(fold.clone(), thr, prev=grid, decay=decay)
    assert 0.0 < ratio < 1.0, ratio
    assert torch.equal(grid[kept], decayed[kept]) and torch.equal(grid[overwritten], fold[overwritten])
    return thr, prev, (grid, binary, int(round(ratio * grid.numel())))


def assert_same_grids(got, want, what):
    grid, binary, count = got
    wgrid, wbinary, wcount = want
    assert grid.shape == wgrid.shape and binary.shape == wbinary.shape and binary.dtype == torch.bool, what
    assert torch.equal(grid, wgrid), f"{what}: {int((grid != wgrid).sum())} of {grid.numel()} values differ, max |diff| {float((grid - wgrid).abs().max()):.3e}"
    assert torch.equal(binary, wbinary), f"{what}: {int((binary != wbinary).sum())} cells flipped"
    assert count.dtype == torch.int64 and int(count) == int(binary.sum()) == wcount, (what, int(count), int(binary.sum()), wcount)


# ------------------------------------------------------------------ 1. bit-equality with today's loop
CASES = [(2, 128), (5, 128), (8, 128), (8, 512), (17, 384), (33, 128), (33, 4096), (33, 2 ** 18)]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("res,slab", CASES)
def test_chain_equals_the_loop_form(field, res, slab, half):
    thr, prev, want = loop_case(field, res, half, 0.95)
    mine = prev.clone()
    got = field.chain(res, half, thr, mine, 0.95, slab_cells=slab)
    assert got[0] is mine                                              # updated in place, as ops.grid_threshold does
    assert_same_grids(got, want, f"res {res} slab {slab}")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_decay_one(field, half):
    thr, prev, want = loop_case(field, 17, half, 1.0)
    got = field.chain(17, half, thr, prev.clone(), 1.0, slab_cells=384)
    assert_same_grids(got, want, "decay 1.0")
    assert not torch.equal(want[0], loop_case(field, 17, half, 0.95)[2][0])        # the other decay is another grid


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_grid_wider_than_the_hash_box(field, half):
    """grid_bound 2.0 > hash_bound 1.5: the outer lattice nodes lie outside the encoders' box and are clamped by them"""
    thr, prev, want = loop_case(field, 17, half, 0.95, grid_bound=2.0, hash_bound=1.5)
    got = field.chain(17, half, thr, prev.clone(), 0.95, grid_bound=2.0, hash_bound=1.5, slab_cells=384)
    assert_same_grids(got, want, "grid_bound 2.0")
    assert not torch.equal(field.loop(17, half, grid_bound=2.0)[1], field.loop(17, half)[1])          # the other bound is another lattice


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_zero_deformation_tables(field, half):
    """all three deformation tables zero: every blended feature is an exact zero, the signed-zero edge of reading one grid where
    the loop adds 0 * f of the other two"""
    thr, prev, want = loop_case(field, 17, half, 0.95, zero_deform=True)
    got = field.chain(17, half, thr, prev.clone(), 0.95, zero_deform=True, slab_cells=384)
    assert_same_grids(got, want, "zero deformation tables")
    assert not torch.equal(field.loop(17, half, zero_deform=True)[1], field.loop(17, half)[1])


def test_mixed_table_types_are_refused(field):
    from project_nerf_amd import ops
    tables = field.tables(False)[:3] + field.tables(True)[3:]
    with pytest.raises(TypeError, match="one dtype"):
        ops.p4_grid_update(field.packed, field.net, tables, field.levels_d, field.levels_c, BOUND, 8, BOUND, 0.01,
                           torch.zeros(8, 8, 8, device="cuda"), 0.95)


# ------------------------------------------------------------------ 2. engine
def make_engines(n=2, **over):
    """engines loaded from ONE module: formula tables, seeded normal networks with a visible density row, displacement_scale 0.1"""
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.part4 import GRIDS, MODULE_SLICES, DualHashEngine
    cfg = {**CFG, **over}
    torch.manual_seed(3)
    model = NeuralField(cfg).cuda()
    net = seeded_net(seed=9)
    with torch.no_grad():
        for k, name in enumerate(GRIDS):
            p = getattr(model, name).encoding.params
            p.copy_(formula_table(p.numel(), float((k + 1) % 4)).cuda())
        sd = dict(model.named_parameters())
        for key, off, cnt in MODULE_SLICES:
            sd[key].copy_(net[off:off + cnt].view(sd[key].shape))
    engines = []
    for _ in range(n):
        eng = DualHashEngine(cfg, device="cuda", seed=1)
        eng.load_from_model(model)
        engines.append(eng)
    return engines


def test_engine_keyword():
    a, b = make_engines()
    assert torch.equal(a.net, b.net) and torch.equal(a.tables, b.tables) and float(a.net[SCALE]) == pytest.approx(0.1)
    assert a.update_grid() == b.update_grid()                          # one loop refresh each: the same state
    thr = float(b.grid.median())
    a.grid_threshold = b.grid_threshold = thr
    g = torch.Generator().manual_seed(2)
    wobble = (0.5 + torch.rand(17, 17, 17, generator=g)).cuda()
    with torch.no_grad():
        a.grid.mul_(wobble)
        b.grid.mul_(wobble)                                            # a history that wins in places and loses in others
    start = b.grid.clone()
    want = b.update_grid(decay=0.95)
    assert 0.0 < want < 1.0
    assert bool((b.grid == start * 0.95).any()) and bool((b.grid > start * 0.95).any())
    before_grid, before_binary = a.grid, a.binary_grid
    got = a.update_grid(decay=0.95, chain=True)
    assert got == want
    assert torch.equal(a.grid, b.grid) and torch.equal(a.binary_grid, b.binary_grid)
    assert a.binary_grid.dtype == torch.bool and a.grid.shape == (17, 17, 17)
    # NEW tensors: the speculative hash backward recognises a refresh by (data_ptr, _version) of binary_grid
    assert a.binary_grid is not before_binary and a.binary_grid.data_ptr() != before_binary.data_ptr()
    assert a.grid is not before_grid and a.grid.data_ptr() != before_grid.data_ptr() and torch.equal(before_grid, start)
    ws, first = a._grid_ws.data_ptr(), a.binary_grid
    assert a.update_grid(decay=0.95, chain=True) == b.update_grid(decay=0.95)
    assert a._grid_ws.data_ptr() == ws                                 # the workspace is kept
    assert a.binary_grid is not first and a.binary_grid.data_ptr() != first.data_ptr()
    assert torch.equal(a.grid, b.grid) and torch.equal(a.binary_grid, b.binary_grid)


def test_part3_engine_keeps_its_loop():
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.part3 import Part3InstantEngine
    from test_gpu_part3_engine import small_cfg
    cfg = small_cfg(grid_resolution=8)
    eng = Part3InstantEngine(cfg, seed=0)
    eng.load_from_model(NeuralField(cfg).cuda())
    with pytest.raises(NotImplementedError, match="chain"):
        eng.update_grid([0.0, 1.0], chain=True)
    assert 0.0 <= eng.update_grid([0.0, 1.0]) <= 1.0                   # without the keyword: the loop, as before


def _sphere(res, radius=1.2):
    ax = torch.linspace(-BOUND, BOUND, res)
    gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ((gx ** 2 + gy ** 2 + gz ** 2) < radius ** 2).cuda()


def _train(chain, steps=40):
    eng, = make_engines(1, grid_resolution=32, learning_rate=1e-2, train_iters=steps, deformation_reg_weight=0.05)
    start = eng.tables.clone()
    eng.update_grid()                                                  # the loop form in BOTH runs: a threshold that splits this field's grid
    eng.grid_threshold = float(eng.grid.median())
    eng.grid.zero_()
    eng.binary_grid = _sphere(32)
    g = torch.Generator().manual_seed(4)
    R, S = 1024, 32
    o = torch.randn(R, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True) * 4.0311
    d = (torch.rand(R, 3, generator=g) - 0.5) * 1.6 - o
    o, d, target = o.cuda(), (d / d.norm(dim=-1, keepdim=True)).cuda(), torch.rand(R, 3, generator=g).cuda()
    t = torch.rand(R, 1, generator=g).cuda()
    ratios = []
    for step in range(1, steps + 1):
        eng.train_step(o, d, target, t, S)
        if step in (16, 32):
            ratios.append(eng.update_grid(decay=0.95, chain=chain))
    return eng.tables.clone(), eng.net.clone(), eng.grid.clone(), eng.binary_grid.clone(), ratios, start


def test_training_through_chain_refreshes_is_bit_equal():
    """40 deterministic steps of 1024 rays x 32 samples, the grid refreshed after steps 16 and 32: the same tables and nets whichever
    form refreshed it (the steps behind a refresh compact against its grid and size the speculative hash backward by it)"""
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import ops
    ops.set_deterministic(True)
    try:
        a, b = _train(True), _train(False)
    finally:
        ops.set_deterministic(False)
    assert all(0.0 < r < 1.0 for r in b[4]) and a[4] == b[4], (a[4], b[4])
    for name, x, y in zip(("tables", "net", "grid", "binary_grid"), a, b):
        assert torch.equal(x, y), name
    assert not torch.equal(b[0], b[5])                                 # it trained


# ------------------------------------------------------------------ 3. graph
def test_graph_capture(field):
    """A capture that completes shows the entry neither allocates nor synchronises; the chain is linear, on one stream (the process
    keeps its default number of hardware queues)"""
    from project_nerf_amd import ops
    res, slab = 17, 384
    thr, prev, want = loop_case(field, res, True, 0.95)
    eager = [t.clone() for t in field.chain(res, True, thr, prev.clone(), 0.95, slab_cells=slab)]
    assert_same_grids(eager, want, "eager")
    ws = torch.empty(ops.p4_grid_update_workspace_bytes(slab), dtype=torch.uint8, device="cuda")
    buf = torch.empty_like(prev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.copy_(prev)                                                # the history is an input: every replay starts from it
        out = field.chain(res, True, thr, buf, 0.95, slab_cells=slab, workspace=ws)
    for replay in range(2):
        out[0].fill_(float("nan"))
        out[1].fill_(False)
        out[2].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]) and torch.equal(out[2], eager[2]), replay
    assert_same_grids(out, want, "graph replay")


# ------------------------------------------------------------------ 4. YAML
def _dynamic_scene(root, size=24):
    from PIL import Image
    from src.dataset import look_at_pose, render_analytic_frame
    focal = 0.5 * size / np.tan(0.5 * 0.6911112070083618)
    for split, count in (("train", 5), ("test", 2)):
        os.makedirs(os.path.join(root, split))
        frames = []
        for k in range(count):
            c2w = torch.tensor(look_at_pose(4.0311 * np.array([np.cos(k + 0.3), np.sin(k + 0.3), 0.5]) / np.sqrt(1.25)), dtype=torch.float32)
            Image.fromarray((render_analytic_frame(c2w, size, focal, 64).numpy() * 255 + 0.5).astype(np.uint8), "RGBA").save(
                os.path.join(root, split, f"r_{k}.png"))
            frames.append({"file_path": f"./{split}/r_{k}", "transform_matrix": c2w.tolist(), "time": k / max(count - 1, 1)})
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, open(os.path.join(root, f"transforms_{split}.json"), "w"))
    return root


def _run_py(tmp_path, **over):
    root = _dynamic_scene(str(tmp_path / "dyn"))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part4.yaml.example")))
    # the run loop refreshes every 32 steps while step < train_iters / 10: 330 iterations is the shortest run that crosses one (step 32)
    cfg.update(train_iters=330, batch_size=256, log_every=110, val_every=330, downscale=1, n_samples=24, render_n_samples=24,
               log2_hashmap_size=12, deform_log2_hashmap_size=10, grid_resolution=24, grid_warmup_iters=8, log_dir=str(tmp_path / "out"),
               grid_update_chain=True, **over)
    cfg_path = tmp_path / "part4.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    return subprocess.run([sys.executable, os.path.join(ROOT, "run.py"), "--config", str(cfg_path), "--data_dir", root, "--render_n", "1"],
                          capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_run_py_refreshes_through_the_chain(tmp_path):
    r = _run_py(tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Skip:" in r.stdout and "Test PSNR" in r.stdout, r.stdout[-2000:]


def test_run_py_refuses_the_key_without_the_engine(tmp_path):
    r = _run_py(tmp_path, engine=False)
    assert r.returncode != 0
    assert "grid_update_chain" in r.stderr and "engine" in r.stderr, r.stderr[-2000:]
