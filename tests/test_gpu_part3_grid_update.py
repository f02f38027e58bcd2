"""nerf_p3_grid_update -- the Part 3 field's occupancy-grid refresh (MLP deformation in front of a hash-grid canonical field) as one
density-only launch chain (points from the cell index, the deformation MLP at a scalar t storing x_c alone, canonical gather,
sigma-net alone with the running maximum, threshold and count in its epilogue) -- against today's loop on the same inputs:
nerf_grid_lattice -> part3.deform_fwd (inference) -> ops.hash_encode_fwd_nat(fp16) -> nerf_p4_canon_fwd(train = 0) on zero view
directions with a torch.full time vector, in 2^18 batches, then ops.grid_threshold(prev, decay) per time, in order.  The chain does
the same arithmetic on the same values in the same order, so every comparison is torch.equal.  Every comparison first checks on the
LOOP form that it cannot pass vacuously: the threshold splits the grid, every time is the strict maximum somewhere, the deformation
matters, and the history both survives and is overwritten.  A canonical table of 2^14 entries per hashed level, no grid above 33^3,
at most four times per case: a few seconds in total."""
import os
import subprocess
import sys

import pytest
import torch
import yaml

from conftest import ROOT
from test_gpu_part3_engine import deform_params, flat_of, small_cfg
from test_gpu_part4_grid_update import _dynamic_scene, _sphere, assert_same_grids, formula_table, history, seeded_net

pytestmark = pytest.mark.gpu

BATCH = 2 ** 18                       # the loop form's batch (GridEngine.lattice_density)
GRID_BOUND, HASH_BOUND = 1.5, 1.0     # Part3InstantEngine's defaults: part of the lattice lies outside the canonical box
W4, B4 = 43904, 44288                 # csrc/p3deform.hip's flat layout: the output layer [3,128] and its bias
L8 = torch.linspace(0, 1, 8).tolist() # entries with no short binary form
TIMES = {1: (L8[3],), 2: (0.0, 1.0), 3: (0.0, L8[2], 1.0), 4: (L8[5], 0.0, 1.0, L8[1]), "sorted": (0.0, L8[1], L8[5], 1.0)}
P = lambda t: None if t is None else t.data_ptr()


class Field:
    """a canonical table (fp32 and its fp16 copy), the packed canonical networks, a packed deformation MLP with displacements of a
    few hundredths and the same MLP with W4 = b4 = 0 (x_c == x)"""

    def __init__(self):
        from project_nerf_amd import ops, part3, part4
        self.levels = ops.HashLevelTable(16, 14)
        table = formula_table(2 * self.levels.entries).cuda()
        self.table = {False: table.view(-1, 2), True: table.half().view(-1, 2)}
        self.packed_c = part4.pack(seeded_net())
        flat = flat_of(deform_params(3)).cuda()
        still = flat.clone()
        still[W4:] = 0
        assert still.numel() == B4 + 3 and float(flat[W4:].abs().max()) > 0.0
        self.packed_d = {True: part3.deform_pack(flat), False: part3.deform_pack(still)}
        self._loop = {}

    def sigma_of(self, pts, t, half, moving, hash_bound):
        """today's field query, density part: Part3InstantEngine.field on zero view directions at one time, in the loop's batches"""
        from project_nerf_amd import _lib, ops, part3, part4
        lib = _lib.load()
        n = pts.shape[0]
        sig = torch.empty(n, device="cuda")
        zeros = torch.zeros(min(n, BATCH), 3, device="cuda")
        for i in range(0, n, BATCH):
            p = pts[i:i + BATCH].contiguous()
            m = p.shape[0]
            tv = torch.full((m,), float(t), device="cuda")
            dx, xc = part3.deform_fwd(self.packed_d[moving], p, tv)
            if not moving:
                assert torch.equal(xc, p) and not bool(dx.any())           # W4 = b4 = 0: x_c == x
            ws = part4.Workspace(m, "cuda", train=False)
            ops.hash_encode_fwd_nat(xc, self.table[half], self.levels, hash_bound, ws.nat(3), fp16=True)
            rgb, s = torch.empty(m, 3, device="cuda"), torch.empty(m, device="cuda")
            _lib.check(lib.nerf_p4_canon_fwd(P(self.packed_c), P(ws.buf), P(tv), P(zeros[:m]), m, P(rgb), P(s), 0, ops._stream()),
                       "nerf_p4_canon_fwd")
            sig[i:i + m] = s
        return sig

    def loop(self, res, half, times, moving=True, grid_bound=GRID_BOUND, hash_bound=HASH_BOUND):
        """sigma on the lattice at every time by today's sequence, computed once per case and never written to (callers clone)"""
        from project_nerf_amd import ops
        key = (res, half, times, moving, grid_bound, hash_bound)
        if key not in self._loop:
            pts = ops.grid_lattice(grid_bound, res, "cuda")
            self._loop[key] = [self.sigma_of(pts, t, half, moving, hash_bound).view(res, res, res) for t in times]
        return self._loop[key]

    def chain(self, res, half, times, thr, prev, decay, moving=True, grid_bound=GRID_BOUND, hash_bound=HASH_BOUND, **kw):
        from project_nerf_amd import ops
        return ops.p3_grid_update(self.packed_d[moving], self.packed_c, self.table[half], self.levels, hash_bound, times, res, grid_bound,
                                  thr, prev, decay, **kw)


@pytest.fixture(scope="module")
def field():
    import project_nerf_amd  # noqa: F401
    return Field()


def fold_of(sig):
    out = sig[0]
    for s in sig[1:]:
        out = torch.maximum(out, s)
    return out


def loop_case(field, res, half, times, decay, moving=True, **kw):
    """(threshold, history, (grid, binary, count) of today's fold, time by time) with the conditions that keep a comparison from
    being vacuous asserted on the loop form"""
    from project_nerf_amd import ops
    sig = field.loop(res, half, times, moving, **kw)
    fold = fold_of(sig)
    other = fold_of(field.loop(res, half, times, not moving, **kw))
    thr = float(fold.median())
    wins = [int((sig[k] > fold_of([s for j, s in enumerate(sig) if j != k])).sum()) if len(sig) > 1 else res ** 3 for k in range(len(sig))]
    print(f"[p3 loop] res {res} fp16 {half} times {len(times)} moving {moving}: strict wins per time {wins}, threshold {thr:.4g}, "
          f"sigma {float(fold.min()):.3g} .. {float(fold.max()):.3g}, {int((fold != other).sum())} cells change with W4 = b4 = 0")
    assert all(w > 0 for w in wins), f"a time never wins: {wins}"       # every time is the strict maximum in at least one cell
    assert not torch.equal(fold, other), "W4 = b4 = 0 leaves sigma unchanged: the deformation does not matter"
    prev = history(res, thr)
    assert float(prev.min()) > 0.0
    decayed = prev * decay
    kept, overwritten = decayed > fold, fold > decayed
    assert bool(kept.any()) and bool(overwritten.any()), (int(kept.sum()), int(overwritten.sum()))
    grid = prev.clone()
    for j, s in enumerate(sig):                                         # the first time folds with the decay, the others with 1
        binary, ratio = ops.grid_threshold(s.clone(), thr, prev=grid, decay=decay if j == 0 else 1.0)
    assert 0.0 < ratio < 1.0, ratio
    assert torch.equal(grid[kept], decayed[kept]) and torch.equal(grid[overwritten], fold[overwritten])
    return thr, prev, (grid, binary, int(round(ratio * grid.numel())))


# ------------------------------------------------------------------ 1. bit-equality with today's loop
# slabs: 128 half a 256-row deformation tile, 256 one tile, 384 seams off the tile edge, 4096 a ragged last slab of 33^3, 2^18 larger
# than any grid here.  The 2^3 lattice is the box's corners: with the canonical box inside the grid they would all be clamped to the
# same eight points at every time, so that case runs with equal bounds.
CASES = [(2, 128, 2, 1.5), (5, 128, 3, 1.0), (5, 256, 1, 1.0), (8, 128, 4, 1.0), (8, 256, 3, 1.0), (17, 384, "sorted", 1.0),
         (17, 256, 1, 1.0), (33, 128, 2, 1.0), (33, 4096, 3, 1.0), (33, 2 ** 18, 4, 1.0)]


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("res,slab,n_times,hash_bound", CASES)
def test_chain_equals_the_loop_form(field, res, slab, n_times, hash_bound, half):
    times = TIMES[n_times]
    thr, prev, want = loop_case(field, res, half, times, 0.95, hash_bound=hash_bound)
    mine = prev.clone()
    got = field.chain(res, half, times, thr, mine, 0.95, hash_bound=hash_bound, slab_cells=slab)
    assert got[0] is mine                                              # updated in place, as ops.grid_threshold does
    assert_same_grids(got, want, f"res {res} slab {slab} times {times}")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_decay_one(field, half):
    """the engine's decay: the reference's sequence of DensityGrid.update(..., decay=1.0) calls"""
    thr, prev, want = loop_case(field, 17, half, TIMES[4], 1.0)
    got = field.chain(17, half, TIMES[4], thr, prev.clone(), 1.0, slab_cells=384)
    assert_same_grids(got, want, "decay 1.0")
    assert not torch.equal(want[0], loop_case(field, 17, half, TIMES[4], 0.95)[2][0])        # the other decay is another grid


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_equal_bounds(field, half):
    """grid_bound == hash_bound 1.5: no lattice node is clamped by the encoder before the deformation moves it"""
    thr, prev, want = loop_case(field, 17, half, TIMES[3], 0.95, hash_bound=1.5)
    got = field.chain(17, half, TIMES[3], thr, prev.clone(), 0.95, hash_bound=1.5, slab_cells=384)
    assert_same_grids(got, want, "hash_bound 1.5")
    assert not torch.equal(fold_of(field.loop(17, half, TIMES[3], hash_bound=1.5)), fold_of(field.loop(17, half, TIMES[3])))


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_zero_output_layer(field, half):
    """W4 = b4 = 0: delta_x is an exact zero and x_c == x (sigma_of asserts it on the loop form)"""
    thr, prev, want = loop_case(field, 17, half, TIMES[2], 0.95, moving=False)
    got = field.chain(17, half, TIMES[2], thr, prev.clone(), 0.95, moving=False, slab_cells=384)
    assert_same_grids(got, want, "W4 = b4 = 0")


def test_default_decay_and_slab(field):
    from project_nerf_amd import ops
    thr, prev, want = loop_case(field, 8, True, TIMES[2], 1.0)
    got = ops.p3_grid_update(field.packed_d[True], field.packed_c, field.table[True], field.levels, HASH_BOUND, TIMES[2], 8, GRID_BOUND, thr,
                             prev.clone())
    assert_same_grids(got, want, "defaults")


def test_ops_argument_checks(field):
    from project_nerf_amd import ops
    call = lambda **kw: ops.p3_grid_update(field.packed_d[True], field.packed_c, kw.pop("table", field.table[True]), field.levels, HASH_BOUND,
                                           kw.pop("times", [0.0, 1.0]), kw.pop("res", 8), GRID_BOUND, 0.01,
                                           kw.pop("prev", torch.zeros(8, 8, 8, device="cuda")), **kw)
    with pytest.raises(ValueError, match="times"):
        call(times=[])
    with pytest.raises(ValueError, match="times"):
        call(times=[0.5] * 257)
    with pytest.raises(ValueError, match="resolution"):
        call(res=1, prev=torch.zeros(1, device="cuda"))
    with pytest.raises(ValueError, match="in place"):
        call(prev=torch.zeros(8, 8, 4, device="cuda"))
    with pytest.raises(ValueError, match="workspace"):
        call(workspace=torch.empty(256, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        call(table=field.table[True].double())


# ------------------------------------------------------------------ 2. engine
ENGINE_TIMES = TIMES["sorted"]


def make_engines(n=2, **over):
    """engines loaded from ONE module: a formula table, seeded normal canonical networks with a visible density row, a deformation
    MLP with displacements of a few hundredths"""
    from project_nerf_amd import part4
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.part3 import Part3InstantEngine
    cfg = small_cfg(**dict(dict(grid_resolution=17), **over))
    torch.manual_seed(3)
    model = NeuralField(cfg).cuda()
    net = seeded_net(seed=9)
    with torch.no_grad():
        p = model.canonical_repr.encoding.params
        p.copy_(formula_table(p.numel()).cuda())
        sd = dict(model.named_parameters())
        for key, off in (("decoder.sigma_net.params", part4.S1), ("decoder.color_net.params", part4.C1)):
            sd[key].copy_(net[off:off + sd[key].numel()].view(sd[key].shape))
        model.deform_net.load_state_dict(deform_params(3).state_dict())
    engines = []
    for _ in range(n):
        eng = Part3InstantEngine(cfg, device="cuda", seed=1)
        eng.load_from_model(model)
        engines.append(eng)
    return engines


def test_engine_method():
    a, b = make_engines()
    assert torch.equal(a.net, b.net) and torch.equal(a.table, b.table)
    assert a.update_grid(ENGINE_TIMES) == b.update_grid(ENGINE_TIMES)  # one loop refresh each: the same state
    thr = float(b.grid.median())
    a.grid_threshold = b.grid_threshold = thr
    g = torch.Generator().manual_seed(2)
    wobble = (0.5 + torch.rand(17, 17, 17, generator=g)).cuda()
    with torch.no_grad():
        a.grid.mul_(wobble)
        b.grid.mul_(wobble)                                            # a history that wins in places and loses in others
    start = b.grid.clone()
    want = b.update_grid(ENGINE_TIMES)
    assert 0.0 < want < 1.0
    assert bool((b.grid == start).any()) and bool((b.grid > start).any())
    before_binary = a.binary_grid
    got = a.update_grid_chain(ENGINE_TIMES)
    assert got == want
    assert torch.equal(a.grid, b.grid) and torch.equal(a.binary_grid, b.binary_grid)
    assert a.binary_grid.dtype == torch.bool and a.binary_grid.shape == (17, 17, 17) and a.grid.shape == (17, 17, 17)
    assert a.binary_grid is not before_binary and a.binary_grid.data_ptr() != before_binary.data_ptr()      # a new tensor, as the loop leaves
    ws, first = a._grid_ws.data_ptr(), a.binary_grid
    assert a._grid_ws.numel() == 19922944
    assert a.update_grid_chain(list(reversed(ENGINE_TIMES))) == b.update_grid(list(reversed(ENGINE_TIMES)))
    assert a._grid_ws.data_ptr() == ws                                 # the workspace is kept
    assert a.binary_grid is not first and a.binary_grid.data_ptr() != first.data_ptr()
    assert torch.equal(a.grid, b.grid) and torch.equal(a.binary_grid, b.binary_grid)
    with pytest.raises(NotImplementedError, match="update_grid_chain"):
        a.update_grid(ENGINE_TIMES, chain=True)                        # the keyword is Part 4's


def _train(chain, steps=40):
    # a rate at which 32 steps move the table visibly but leave the densities on both sides of the threshold taken before them (at
    # 1e-2 the LOOP form's second refresh has every cell active)
    eng, = make_engines(1, grid_resolution=32, learning_rate=1e-3, train_iters=steps)
    start = eng.table.clone()
    eng.update_grid(ENGINE_TIMES)                                      # the loop form in BOTH runs: a threshold that splits this field's grid
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
            ratios.append(eng.update_grid_chain(ENGINE_TIMES) if chain else eng.update_grid(ENGINE_TIMES))
    return eng.table.clone(), eng.net.clone(), eng.grid.clone(), eng.binary_grid.clone(), ratios, start


def test_training_through_chain_refreshes_is_bit_equal():
    """40 deterministic steps of 1024 rays x 32 samples, the grid refreshed after steps 16 and 32: the same table and nets whichever
    form refreshed it (the steps behind a refresh compact against its grid)"""
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
    assert not torch.equal(b[0], b[5])                                 # it trained


# ------------------------------------------------------------------ 3. graph
def test_graph_capture(field):
    """A capture that completes shows the entry neither allocates nor synchronises; the chain is linear, on one stream (the process
    keeps its default number of hardware queues)"""
    from project_nerf_amd import ops
    res, slab, times = 17, 384, TIMES[3]
    thr, prev, want = loop_case(field, res, True, times, 0.95)
    eager = [t.clone() for t in field.chain(res, True, times, thr, prev.clone(), 0.95, slab_cells=slab)]
    assert_same_grids(eager, want, "eager")
    ws = torch.empty(ops.p3_grid_update_workspace_bytes(slab), dtype=torch.uint8, device="cuda")
    buf = torch.empty_like(prev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.copy_(prev)                                                # the history is an input: every replay starts from it
        out = field.chain(res, True, times, thr, buf, 0.95, slab_cells=slab, workspace=ws)
    for replay in range(2):
        out[0].fill_(float("nan"))
        out[1].fill_(False)
        out[2].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]) and torch.equal(out[2], eager[2]), replay
    assert_same_grids(out, want, "graph replay")


# ------------------------------------------------------------------ 4. YAML
def _run_py(tmp_path, **over):
    root = _dynamic_scene(str(tmp_path / "dyn"))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part3_instant.yaml.example")))
    # the run loop refreshes every 16 steps while step < train_iters / 10: 170 iterations is a run in which step 16 is a refresh
    cfg.update(train_iters=170, batch_size=256, log_every=85, val_every=170, downscale=1, n_samples=24, render_n_samples=24,
               log2_hashmap_size=12, grid_resolution=24, grid_warmup_iters=8, log_dir=str(tmp_path / "out"), grid_update_chain=True, **over)
    cfg_path = tmp_path / "part3_instant.yaml"
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
