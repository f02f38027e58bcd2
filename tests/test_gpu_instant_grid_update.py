"""nerf_instant_grid_update -- the Instant-NGP occupancy-grid refresh as one density-only launch chain (points from the cell index,
sigma-net alone, threshold + count in the chain's epilogue) -- against today's sequence on the same inputs: nerf_grid_lattice ->
nerf_hash_encode_fwd* (bf16 operand image) -> nerf_imlp_fwd(train = 0) in 2^18-point batches -> nerf_grid_update.  The chain does
the same arithmetic on the same values in the same order, so every comparison with that sequence is torch.equal; only the pin
against the reference's golden carries a tolerance (the one the loop form is already held to).  Table of 2^12 entries per hashed
level, no grid above 65^3: a few seconds in total."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

BOUND = 1.5
BATCH = 2 ** 18                       # the loop form's batch (InstantNgpEngine.update_grid)
CFG = {"mode": "part2_instant", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 16,
       "per_level_scale": 1.5, "scene_bound": BOUND, "hidden_dim": 64, "L_embed_dir": 4, "grid_resolution": 17,
       "near": 2.0, "far": 6.0, "grid_threshold": 0.01}


def formula_table(n):
    """tests/golden/make_golden.py::instant_test_params"""
    i = torch.arange(n, dtype=torch.float64)
    return (0.5 * torch.sin(0.37 * i + 0.11 * (i % 7))).float()


class Field:
    """table (fp32 and its fp16 copy), packed tiny-MLP weights and level table of the fixture"""

    def __init__(self):
        from project_nerf_amd import ops
        from project_nerf_amd.engine import InstantNgpEngine
        self.levels = ops.HashLevelTable(16, 12)
        self.table = formula_table(2 * self.levels.entries).cuda().view(-1, 2)
        self.table_h = self.table.half()
        self.net = InstantNgpEngine._init_net(None, torch.Generator().manual_seed(5)).cuda()
        self.packed = ops.imlp_pack(self.net)
        self._sigma = {}

    def tab(self, half):
        return self.table_h if half else self.table

    def sigma_of(self, pts, half, hash_bound=BOUND):
        """today's field query, density part: hash forward into the decoder's workspace, the whole decoder on zero directions"""
        from project_nerf_amd import _lib, ops
        lib = _lib.load()
        n = pts.shape[0]
        sig = torch.empty(n, device="cuda")
        zeros = torch.zeros(min(n, BATCH), 3, device="cuda")
        for i in range(0, n, BATCH):
            p = pts[i:i + BATCH]
            m = p.shape[0]
            ws = torch.empty(lib.nerf_imlp_workspace_bytes(m), device="cuda", dtype=torch.uint8)
            ops.hash_encode_fwd(p, self.tab(half), self.levels, hash_bound, want_f32=False, out_nat=ws)
            rgb, s = torch.empty(m, 3, device="cuda"), torch.empty(m, device="cuda")
            _lib.check(lib.nerf_imlp_fwd(self.packed.data_ptr(), ws.data_ptr(), zeros.data_ptr(), m, rgb.data_ptr(), s.data_ptr(), 0,
                                         ops._stream()), "nerf_imlp_fwd")
            sig[i:i + m] = s
        return sig

    def loop_sigma(self, res, half, grid_bound=BOUND, hash_bound=BOUND):
        """sigma on the lattice by today's sequence, computed once per case and never written to (callers clone)"""
        from project_nerf_amd import ops
        key = (res, half, grid_bound, hash_bound)
        if key not in self._sigma:
            self._sigma[key] = self.sigma_of(ops.grid_lattice(grid_bound, res, "cuda"), half, hash_bound).view(res, res, res)
        return self._sigma[key]

    def chain(self, source, half, thr, grid_bound=BOUND, hash_bound=BOUND, **kw):
        from project_nerf_amd import ops
        return ops.instant_grid_update(self.packed, self.tab(half), self.levels, hash_bound, source, grid_bound, thr, **kw)


@pytest.fixture(scope="module")
def field():
    import project_nerf_amd  # noqa: F401
    return Field()


def loop_threshold(sigma, thr, prev=None, decay=1.0):
    """today's fold: (grid, binary, count) of ops.grid_threshold on a copy of the loop form's sigma"""
    from project_nerf_amd import ops
    cur = sigma.clone()
    binary, ratio = ops.grid_threshold(cur, thr, prev=prev, decay=decay)
    return (cur if prev is None else prev), binary, int(round(ratio * cur.numel()))


def median_threshold(sigma):
    """the median of the loop form's own sigma, and the proof that it splits the grid: 0 < ratio < 1"""
    thr = float(sigma.median())
    _, binary, count = loop_threshold(sigma, thr)
    assert 0 < count < sigma.numel(), (count, sigma.numel())
    return thr


def assert_same_grids(got, want, what):
    grid, binary, count = got
    wgrid, wbinary, wcount = want
    assert grid.shape == wgrid.shape and binary.shape == wbinary.shape and binary.dtype == torch.bool, what
    assert torch.equal(grid, wgrid), f"{what}: {int((grid != wgrid).sum())} of {grid.numel()} sigma values differ, max |diff| {float((grid - wgrid).abs().max()):.3e}"
    assert torch.equal(binary, wbinary), f"{what}: {int((binary != wbinary).sum())} cells flipped"
    assert count.dtype == torch.int64 and int(count) == int(binary.sum()) == wcount, (what, int(count), int(binary.sum()), wcount)


# ------------------------------------------------------------------ 1. bit-equality with today's sequence
CASES = [(2, 128), (5, 128), (8, 128), (8, 512), (17, 128), (17, 384), (17, 2 ** 18), (33, 4096), (65, 2 ** 18)]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("res,slab", CASES)
def test_lattice_source_equals_the_loop_form(field, res, slab, half):
    sigma = field.loop_sigma(res, half)
    thr = median_threshold(sigma)
    want = loop_threshold(sigma, thr)
    got = field.chain(res, half, thr, slab_cells=slab)
    assert_same_grids(got, want, f"res {res} slab {slab}")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_non_contiguous_table_is_copied_and_kept_until_the_launch(field, half):
    """a strided view of the table: the wrapper's contiguous copy must outlive the grid, workspace and count it allocates after
    making it (nothing else holds the copy), so the result is the contiguous table's"""
    table = field.tab(half)
    wide = torch.zeros(table.shape[0], 4, dtype=table.dtype, device="cuda")
    wide[:, :2] = table
    view = wide[:, :2]
    assert not view.is_contiguous() and torch.equal(view, table)
    from project_nerf_amd import ops
    sigma = field.loop_sigma(33, half)
    thr = median_threshold(sigma)
    want = loop_threshold(sigma, thr)
    got = ops.instant_grid_update(field.packed, view, field.levels, BOUND, 33, BOUND, thr, slab_cells=4096)
    assert_same_grids(got, want, "res 33, strided table")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_grid_wider_than_the_hash_box(field, half):
    """grid_bound 2.0 > hash_bound 1.5: the outer lattice nodes lie outside the encoder's box and are clamped by it"""
    sigma = field.loop_sigma(17, half, grid_bound=2.0, hash_bound=1.5)
    thr = median_threshold(sigma)
    got = field.chain(17, half, thr, grid_bound=2.0, hash_bound=1.5, slab_cells=384)
    assert_same_grids(got, loop_threshold(sigma, thr), "grid_bound 2.0")
    assert not torch.equal(sigma, field.loop_sigma(17, half))          # the other bound is another lattice


# ------------------------------------------------------------------ 2. the fold
@pytest.mark.parametrize("decay", [0.95, 1.0])
def test_running_maximum(field, decay):
    res = 17
    sigma = field.loop_sigma(res, True)
    thr = median_threshold(sigma)
    g = torch.Generator().manual_seed(17)
    prev = (thr * (0.5 + torch.rand(res, res, res, generator=g))).cuda()      # [0.5, 1.5] x threshold: straddles it
    assert 0 < int((prev * decay > thr).sum()) < prev.numel()
    want = loop_threshold(sigma, thr, prev=prev.clone(), decay=decay)
    mine = prev.clone()
    got = field.chain(res, True, thr, prev=mine, decay=decay, slab_cells=384)
    assert got[0] is mine                                              # updated in place, as ops.grid_threshold does
    assert_same_grids(got, want, f"decay {decay}")
    assert not torch.equal(got[0], sigma) and not torch.equal(got[0], prev)   # both operands of the maximum won somewhere


def raw_update(field, half, pts, n, res, grid, binary, count, decay, dynamic, thr, slab=384):
    from project_nerf_amd import _lib, ops
    lib = _lib.load()
    ws = torch.empty(lib.nerf_instant_grid_update_workspace_bytes(slab), dtype=torch.uint8, device="cuda")
    t = field.tab(half)
    _lib.check(lib.nerf_instant_grid_update(field.packed.data_ptr(), None if half else t.data_ptr(), t.data_ptr() if half else None, 16,
                                            *field.levels.host_args(), BOUND, None if pts is None else pts.data_ptr(), n, res, BOUND,
                                            grid.data_ptr(), binary.data_ptr(), decay, dynamic, thr, count.data_ptr(), slab, ws.data_ptr(),
                                            ops._stream()), "nerf_instant_grid_update")


def test_overwrite_form_never_reads_the_grid(field):
    res = 17
    sigma = field.loop_sigma(res, True)
    thr = median_threshold(sigma)
    grid = torch.full((res, res, res), float("nan"), device="cuda")
    binary = torch.empty(res, res, res, dtype=torch.bool, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    raw_update(field, True, None, res ** 3, res, grid, binary, count, 0.95, 0, thr)
    assert bool(torch.isfinite(grid).all())
    assert_same_grids((grid, binary, count), loop_threshold(sigma, thr), "NaN grid buffer, dynamic = 0")


# ------------------------------------------------------------------ 3. point-buffer source
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_point_buffer_source(field, n):
    from project_nerf_amd import ops
    g = torch.Generator().manual_seed(n)
    pts = ((torch.rand(n, 3, generator=g) * 4 - 2)).cuda()              # [-2, 2]^3: some outside the encoder's box
    for half in (False, True):
        sigma = field.sigma_of(pts, half)
        thr = float(sigma.median()) if n > 1 else 0.5 * float(sigma[0])
        got = field.chain(pts, half, thr, slab_cells=128)
        assert got[0].shape == (n,)
        assert_same_grids(got, loop_threshold(sigma, thr), f"{n} points")
        assert int(got[2]) > 0
        # the form the dynamic engines will feed: buffer + running maximum, at the ABI level
        prev = (thr * (0.5 + torch.rand(n, generator=g))).cuda()
        want = loop_threshold(sigma, thr, prev=prev.clone(), decay=0.95)
        grid, binary, count = prev.clone(), torch.empty(n, dtype=torch.bool, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
        raw_update(field, half, pts, n, 0, grid, binary, count, 0.95, 1, thr, slab=128)
        assert_same_grids((grid, binary, count), want, f"{n} points, running maximum")
    none = ops.instant_grid_update(field.packed, field.table, field.levels, BOUND, pts[:0], BOUND, 0.5)
    assert none[0].shape == (0,) and int(none[2]) == 0


# ------------------------------------------------------------------ 4. reference pin
@pytest.mark.parametrize("half_table", [True, False])
def test_engine_chain_refresh_vs_reference_golden(half_table):
    """update_grid(chain=True) around the parameters of golden g13 against the reference's DensityGrid.update (src/renderer.py:35-132),
    within the bounds test_density_grid_update_around_instant_field_vs_reference_golden applies to the loop form"""
    from project_nerf_amd.engine import InstantNgpEngine
    g = golden("g13_instant_glue")
    eng = InstantNgpEngine({**CFG, "grid_resolution": 32, "grid_threshold": 0.05, "half_table": half_table}, device="cuda", seed=0)
    table = formula_table(eng.table.numel())
    np.testing.assert_array_equal(table[::4099].numpy(), g["table_probe"])
    with torch.no_grad():
        eng.table.copy_(table.cuda())
        eng.net.copy_(torch.cat([torch.from_numpy(g["sigma_net"]), torch.from_numpy(g["color_net"])]).cuda())
    eng._pack()
    ratio = eng.update_grid(chain=True)
    ref = g["grid"]
    np.testing.assert_allclose(eng.grid.cpu().numpy(), ref, rtol=0.1, atol=2e-2 * ref.max())
    flips = int((eng.binary_grid.cpu().numpy() != g["binary"]).sum())
    assert flips <= 0.01 * g["binary"].sum(), flips
    assert abs(ratio - float(g["ratio"])) < 0.005


# ------------------------------------------------------------------ 5. engine
def make_engine(seed=1, **over):
    from project_nerf_amd.engine import InstantNgpEngine
    eng = InstantNgpEngine({**CFG, **over}, device="cuda", seed=seed)
    with torch.no_grad():
        eng.table.copy_(formula_table(eng.table.numel()).cuda())
    eng._pack()
    return eng


def test_engine_keyword():
    from project_nerf_amd.instant_shapes import InstantShapeEngine
    a, b = make_engine(), make_engine()
    b.update_grid()
    thr = float(b.grid.median())
    a.grid_threshold = b.grid_threshold = thr
    want = b.update_grid()
    assert 0.0 < want < 1.0
    before = a.binary_grid
    got = a.update_grid(chain=True)
    assert got == want
    assert torch.equal(a.grid, b.grid) and torch.equal(a.binary_grid, b.binary_grid)
    assert a.binary_grid.dtype == torch.bool and a.grid.shape == (17, 17, 17)
    # a NEW binary grid: the speculative hash backward recognises a refresh by (data_ptr, _version)
    assert a.binary_grid is not before and a.binary_grid.data_ptr() != before.data_ptr()
    ws, first = a._grid_ws.data_ptr(), a.binary_grid
    assert a.update_grid(chain=True) == want
    assert a._grid_ws.data_ptr() == ws                                 # the workspace is kept
    assert a.binary_grid is not first and a.binary_grid.data_ptr() != first.data_ptr() and torch.equal(a.binary_grid, first)
    shape_eng = InstantShapeEngine({**CFG, "n_levels": 8, "hidden_dim": 32, "L_embed_dir": 2}, device="cuda")
    with pytest.raises(NotImplementedError, match="chain"):
        shape_eng.update_grid(chain=True)


def _sphere(res, radius=1.2):
    ax = torch.linspace(-BOUND, BOUND, res)
    gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ((gx ** 2 + gy ** 2 + gz ** 2) < radius ** 2).cuda()


def _train(chain, steps=40):
    from project_nerf_amd import ops
    eng = make_engine(seed=0, grid_resolution=32, log2_hashmap_size=14, train_iters=steps, learning_rate=1e-2)
    with torch.no_grad():
        eng.table.mul_(0.5)
        eng.net[2048:2048 + 64] *= 20.0                                # the density row: sigma well above the threshold in places
    ops.imlp_pack(eng.net, eng.packed)
    eng.binary_grid = _sphere(32)
    g = torch.Generator().manual_seed(4)
    R, S = 1024, 32
    o = torch.randn(R, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True) * 4.0311
    d = (torch.rand(R, 3, generator=g) - 0.5) * 1.6 - o
    o, d, target = o.cuda(), (d / d.norm(dim=-1, keepdim=True)).cuda(), torch.rand(R, 3, generator=g).cuda()
    ratios = []
    prepared = eng.prepare_batch(o, d, S)
    for step in range(1, steps + 1):
        nxt = eng.prepare_batch(o, d, S)                               # one batch ahead, as the training loop does
        eng.train_step(o, d, target, S, prepared=prepared)
        prepared = nxt
        if step in (16, 32):
            ratios.append(eng.update_grid(chain=chain))
            prepared = eng.prepare_batch(o, d, S)
    return eng.table.clone(), eng.net.clone(), eng.grid.clone(), eng.binary_grid.clone(), ratios


def test_training_through_chain_refreshes_is_bit_equal():
    """40 deterministic steps of 1024 rays x 32 samples, the grid refreshed after steps 16 and 32: the same table and nets whichever
    form refreshed it (the steps behind a refresh compact against its grid and size the speculative hash backward by it)"""
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import ops
    ops.set_deterministic(True)
    try:
        a, b = _train(True), _train(False)
    finally:
        ops.set_deterministic(False)
    assert all(0.0 < r < 1.0 for r in b[4]) and a[4] == b[4], (a[4], b[4])
    for name, x, y in zip(("table", "net", "grid", "binary_grid"), a, b):
        assert torch.equal(x, y), name
    assert not torch.equal(b[0], 0.5 * formula_table(b[0].numel()).cuda())       # it trained


# ------------------------------------------------------------------ 6. graph
def test_graph_capture(field):
    """A capture that completes shows the entry neither allocates nor synchronises; the chain is linear, on one stream"""
    res, slab = 17, 384
    sigma = field.loop_sigma(res, True)
    thr = median_threshold(sigma)
    eager = [t.clone() for t in field.chain(res, True, thr, slab_cells=slab)]
    ws = torch.empty(64 * slab, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = field.chain(res, True, thr, slab_cells=slab, workspace=ws)
    for replay in range(2):
        out[0].fill_(float("nan"))
        out[1].fill_(False)
        out[2].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]) and torch.equal(out[2], eager[2]), replay
    assert_same_grids(out, loop_threshold(sigma, thr), "graph replay")


# ------------------------------------------------------------------ 7. YAML
def _run_py(tmp_path, **over):
    from src.dataset import write_synthetic_scene
    root = write_synthetic_scene(str(tmp_path / "scene"), n_train=6, n_test=1, size=32)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2_instant.yaml.example")))
    # the run loop refreshes every 32 steps while step < train_iters / 10: 330 iterations is the shortest run that crosses one (step 32)
    cfg.update(train_iters=330, batch_size=256, log_every=110, save_every=0, val_every=330, downscale=1, n_samples=32, render_n_samples=32,
               grid_resolution=32, grid_warmup_iters=16, log2_hashmap_size=14, log_dir=str(tmp_path / "out"), grid_update_chain=True, **over)
    cfg_path = tmp_path / "part2_instant.yaml"
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
