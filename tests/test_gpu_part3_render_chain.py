"""nerf_p3_render_rays_fwd -- a frame of Part 3 with a hash-grid canonical field as one launch chain whose kernels read the compaction's
active count AND the frame's time from device memory -- against today's loop on the same inputs, built from existing ops: per chunk
ops.sample_compact (a host read of the count) -> part3.deform_fwd with a torch.full time vector -> ops.hash_encode_fwd_nat(fp16) ->
nerf_p4_canon_fwd(train = 0) -> ops.composite_indexed, the background for a chunk without an active sample.  A sample's x_c, hash
features and decoder outputs depend on its own point, direction and the time only, not on its compact slot or the launch shape, so
every comparison is torch.equal.  The fixture first checks on the LOOP that a comparison cannot pass vacuously: every ray with active
samples accumulates something, the deformation matters (W4 = b4 = 0 changes the frame) and the time matters.  A canonical table of 2^12
entries per hashed level and a 16^3 occupancy grid: each test runs in about a second."""
import os
import subprocess
import sys

import pytest
import torch
import yaml

from conftest import ROOT
from test_gpu_instant_render_chain import assert_same, count_word, crossing_rays, inner_rays, seeded_grid
from test_gpu_part3_engine import deform_params, small_cfg
from test_gpu_part3_grid_update import _dynamic_scene

pytestmark = pytest.mark.gpu

RES = 16
GRID_BOUND, HASH_BOUND = 1.5, 1.0     # Part3InstantEngine's defaults: the canonical box lies inside the occupancy grid
L8 = torch.linspace(0, 1, 8).tolist() # entries with no short binary form
W4 = 43904                            # csrc/p3deform.hip's flat layout: the output layer [3,128] and its bias end the vector
P = lambda t: None if t is None else t.data_ptr()


def make_engine(seed=1, **over):
    """an engine at the engine's default bounds whose field varies visibly over the box and over time: table entries in [-1, 1], the
    canonical networks four times their initial draw, a seeded deformation MLP whose output layer has standard deviation 0.05"""
    from project_nerf_amd import part4
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.part3 import Part3InstantEngine
    cfg = small_cfg(**dict(dict(log2_hashmap_size=12, grid_resolution=RES), **over))
    torch.manual_seed(seed)
    model = NeuralField(cfg).cuda()
    with torch.no_grad():
        model.deform_net.load_state_dict(deform_params(seed + 2).state_dict())
    cfg = {k: v for k, v in cfg.items() if k not in ("scene_bound", "grid_bound")}
    eng = Part3InstantEngine(cfg, device="cuda", seed=seed)
    assert (eng.bound, eng.grid_bound) == (HASH_BOUND, GRID_BOUND)
    eng.load_from_model(model)
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        eng.table.copy_((torch.rand(eng.table.numel(), generator=g) * 2 - 1).cuda())
        eng.net[:part4.N_PARAMS].mul_(4.0)
    eng.repack()
    return eng


class Field:
    """what the entry reads, taken from an engine: both packed images (and the deformation image with W4 = b4 = 0), the canonical
    table as fp32 and as its fp16 copy, the level table; a scene (grid, depth range, background) that a test sets"""

    def __init__(self, eng):
        from project_nerf_amd import part3
        self.levels = eng.levels
        self.table = {True: eng.table_h.view(-1, 2).clone(), False: eng.table.view(-1, 2).clone()}
        self.packed_c, self.packed_d = eng.packed_c.clone(), eng.packed_d.clone()
        still = eng.deform_params.clone()
        assert float(still[W4:].abs().max()) > 0.0
        still[W4:] = 0
        self.packed_still = part3.deform_pack(still)
        self.bg = torch.ones(3, device="cuda")

    def loop(self, o, d, S, chunk, grid, t, near=2.0, far=6.0, bg=None, half=True, hash_bound=HASH_BOUND, grid_bound=GRID_BOUND,
             packed_d=None):
        """today's path chunk by chunk, from existing ops (one host read of the active count per chunk, a time vector per chunk)"""
        from project_nerf_amd import _lib, ops, part3, part4
        lib = _lib.load()
        bg = self.bg if bg is None else bg
        outs = []
        for i in range(0, o.shape[0], chunk):
            oc, dc = o[i:i + chunk].contiguous(), d[i:i + chunk].contiguous()
            r = oc.shape[0]
            b = bg[i:i + chunk].contiguous() if bg.dim() == 2 else bg
            z, slots, pts, dirs = ops.sample_compact(oc, dc, near, far, S, grid, grid_bound)
            n = pts.shape[0]
            if n == 0:
                outs.append((b.expand(r, 3).clone(), torch.zeros(r, device="cuda"), torch.zeros(r, device="cuda")))
                continue
            tv = torch.full((n,), float(t), device="cuda")
            _, xc = part3.deform_fwd(self.packed_d if packed_d is None else packed_d, pts, tv)
            ws = part4.Workspace(n, "cuda", train=False)
            ops.hash_encode_fwd_nat(xc, self.table[half], self.levels, hash_bound, ws.nat(3), fp16=True)
            rgb, sigma = torch.empty(n, 3, device="cuda"), torch.empty(n, device="cuda")
            _lib.check(lib.nerf_p4_canon_fwd(P(self.packed_c), P(ws.buf), P(tv), P(dirs), n, P(rgb), P(sigma), 0, ops._stream()),
                       "nerf_p4_canon_fwd")
            outs.append(ops.composite_indexed(rgb, sigma, slots, z, dc, b))
        return tuple(torch.cat([x[k] for x in outs], 0) for k in range(3))

    def chain(self, o, d, S, chunk, grid, t, near=2.0, far=6.0, bg=None, half=True, hash_bound=HASH_BOUND, grid_bound=GRID_BOUND,
              workspace=None):
        from project_nerf_amd import ops
        return ops.p3_render_rays_fwd(self.packed_d, self.packed_c, self.table[half], self.levels, hash_bound, grid, grid_bound, o, d, S,
                                      near, far, torch.tensor([float(t)], device="cuda"), self.bg if bg is None else bg, chunk,
                                      workspace=workspace)


@pytest.fixture(scope="module")
def field():
    import project_nerf_amd  # noqa: F401
    f = Field(make_engine())
    # non-vacuity, on the LOOP, before any chain is compared with it
    o, d = crossing_rays(40, seed=5)
    grid = seeded_grid(11)
    from project_nerf_amd import ops
    slots = ops.sample_compact(o, d, 2.0, 6.0, 64, grid, GRID_BOUND)[1].view(40, 64)
    hit = (slots >= 0).any(dim=1)
    a = f.loop(o, d, 64, 40, grid, 0.25)
    assert int(hit.sum()) > 20 and float(a[2][hit].min()) > 0.0, "a ray with active samples accumulated nothing"
    assert torch.equal(a[2][~hit], torch.zeros_like(a[2][~hit]))
    still = f.loop(o, d, 64, 40, grid, 0.25, packed_d=f.packed_still)
    assert not torch.equal(a[0], still[0]), "W4 = b4 = 0 leaves the frame unchanged: the deformation does not matter"
    later = f.loop(o, d, 64, 40, grid, 0.75)
    assert not torch.equal(a[0], later[0]), "t = 0.25 and t = 0.75 give the same frame: the time does not matter"
    print(f"[p3 loop] {int(hit.sum())} of 40 rays hit; acc {float(a[2][hit].min()):.3g} .. {float(a[2].max()):.3g}; "
          f"{int((a[0] != still[0]).sum())} values change with W4 = b4 = 0, {int((a[0] != later[0]).sum())} between t = 0.25 and 0.75")
    return f


def ones_grid():
    return torch.ones(RES, RES, RES, dtype=torch.bool, device="cuda")


def workspace(chunk, S, fill=None):
    from project_nerf_amd import ops
    ws = torch.empty(ops.p3_render_workspace_bytes(chunk, S), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws


# ------------------------------------------------------------------ 1. counts at the tile edges
# the deformation chain works in 256-row tiles, the gather and the canonical chain in 128-row tiles
@pytest.mark.parametrize("R,S", [(1, 2), (1, 127), (1, 128), (3, 43), (1, 255), (1, 256), (1, 257), (3, 128), (5, 77), (2, 500)])
def test_exact_counts_at_the_tile_edges(field, R, S):
    o, d = inner_rays(R, seed=R * 1000 + S)
    ws = workspace(R, S)
    got = field.chain(o, d, S, R, ones_grid(), L8[3], near=0.1, far=1.0, workspace=ws)
    assert count_word(ws) == R * S
    want = field.loop(o, d, S, R, ones_grid(), L8[3], near=0.1, far=1.0)
    assert float(want[2].min()) > 0.0                    # the field was evaluated: every ray accumulated something
    assert_same(got, want, f"R={R} S={S}")


def test_count_zero_renders_the_background(field):
    o, d = crossing_rays(4, seed=3)
    grid = torch.zeros(RES, RES, RES, dtype=torch.bool, device="cuda")
    ws = workspace(4, 8, fill=0xFF)                      # x_c / rgb / sigma rows hold NaN patterns: nothing may read them
    got = field.chain(o, d, 8, 4, grid, 0.5, workspace=ws)
    assert count_word(ws) == 0
    want = field.loop(o, d, 8, 4, grid, 0.5)
    assert torch.equal(got[0], field.bg.expand(4, 3)) and torch.equal(got[1], torch.zeros(4, device="cuda"))
    assert torch.equal(got[2], torch.zeros(4, device="cuda"))
    assert_same(got, want, "empty grid")


def test_count_one(field):
    """4 rays x 8 samples along +x, 0.343 apart (a cell is 0.1875 wide): the one occupied cell holds exactly one sample of one ray"""
    from project_nerf_amd import ops
    o = torch.tensor([[-1.4, y, 0.05] for y in (-0.9, -0.3, 0.3, 0.9)], device="cuda")
    d = torch.tensor([[1.0, 0.0, 0.0]] * 4, device="cuda")
    near, far, S = 0.2, 2.6, 8
    _, pts, _ = ops.sample_rays(o, d, near, far, S, want_points=True)
    _, idx = ops.active_mask(pts, ones_grid(), GRID_BOUND, want_index=True)
    cell = idx[2 * S + 3].tolist()                       # sample 3 of ray 2
    grid = torch.zeros_like(ones_grid())
    grid[cell[0], cell[1], cell[2]] = True
    slots = ops.sample_compact(o, d, near, far, S, grid, GRID_BOUND)[1]
    assert int((slots >= 0).sum()) == 1 and int(slots[2 * S + 3]) == 0
    ws = workspace(4, S, fill=0xFF)
    got = field.chain(o, d, S, 4, grid, L8[5], near=near, far=far, workspace=ws)
    assert count_word(ws) == 1
    want = field.loop(o, d, S, 4, grid, L8[5], near=near, far=far)
    assert float(want[2][2]) > 0.0 and float(want[2][0]) == 0.0
    assert_same(got, want, "one active sample")


# ------------------------------------------------------------------ 2. compaction passes, chunks, workspace, tables, bounds, times
def test_several_compaction_passes_and_a_partial_grid(field):
    """5120 samples: more than one 4096-sample compaction pass; rays that enter and leave the box; ~30 % of the cells set"""
    o, d = crossing_rays(40, seed=5)
    ws = workspace(40, 128)
    got = field.chain(o, d, 128, 40, seeded_grid(11), 0.25, workspace=ws)
    assert 0 < count_word(ws) < 40 * 128
    assert_same(got, field.loop(o, d, 128, 40, seeded_grid(11), 0.25), "5120 samples")


@pytest.mark.parametrize("chunk", [5, 64])
def test_chunking_and_per_ray_background(field, chunk):
    """13 rays in chunks of 5, 5, 3 (and as one chunk), a background row per ray: the chain slices rays, outputs and bg + r0 * 3"""
    o, d = crossing_rays(13, seed=7)
    bg = (torch.arange(39, dtype=torch.float32).view(13, 3) / 40.0).cuda()
    got = field.chain(o, d, 64, chunk, seeded_grid(12), L8[2], bg=bg)
    want = field.loop(o, d, 64, min(chunk, 13), seeded_grid(12), L8[2], bg=bg)
    assert_same(got, want, f"chunk {chunk}")
    assert len({tuple(r) for r in got[0].tolist()}) == 13           # distinct rows: a wrong bg slice could not go unnoticed


def test_workspace_contents_do_not_matter(field):
    o, d = crossing_rays(40, seed=5)
    o1, d1 = inner_rays(1, seed=9)
    a = field.chain(o, d, 128, 40, seeded_grid(11), 0.25, workspace=workspace(40, 128, fill=0xFF))
    ws = workspace(40, 128, fill=0)
    b = field.chain(o, d, 128, 40, seeded_grid(11), 0.25, workspace=ws)
    assert_same(a, b, "0xFF against zeroed workspace")
    # the 5120-sample call's count, x_c and operand rows are still in ws: a 127-sample call on it must not see them
    got = field.chain(o1, d1, 127, 1, ones_grid(), 0.25, near=0.1, far=1.0, workspace=ws)
    assert count_word(ws) == 127
    assert_same(got, field.loop(o1, d1, 127, 1, ones_grid(), 0.25, near=0.1, far=1.0), "127 samples after 5120 on one workspace")


@pytest.mark.parametrize("half", [True, False], ids=["fp16", "fp32"])
def test_both_table_forms(field, half):
    assert field.table[half].dtype == (torch.float16 if half else torch.float32)
    o, d = crossing_rays(13, seed=13)
    got = field.chain(o, d, 64, 5, seeded_grid(14), L8[6], half=half)
    assert_same(got, field.loop(o, d, 64, 5, seeded_grid(14), L8[6], half=half), "fp16 table" if half else "fp32 table")


@pytest.mark.parametrize("hash_bound,grid_bound", [(1.5, 1.5), (1.0, 1.5), (0.75, 1.25)])
def test_bounds(field, hash_bound, grid_bound):
    """equal bounds, and a canonical box inside the occupancy grid (x_c outside it is clamped by the encoding)"""
    o, d = crossing_rays(13, seed=19)
    kw = dict(hash_bound=hash_bound, grid_bound=grid_bound)
    got = field.chain(o, d, 64, 13, seeded_grid(20), L8[1], **kw)
    assert_same(got, field.loop(o, d, 64, 13, seeded_grid(20), L8[1], **kw), f"bounds {hash_bound} / {grid_bound}")


@pytest.mark.parametrize("t", [0.0, 1.0, L8[3]])
def test_times(field, t):
    o, d = crossing_rays(13, seed=23)
    got = field.chain(o, d, 64, 13, seeded_grid(24), t)
    assert_same(got, field.loop(o, d, 64, 13, seeded_grid(24), t), f"t = {t}")


def test_repeatable(field):
    o, d = crossing_rays(40, seed=15)
    a = field.chain(o, d, 128, 16, seeded_grid(16), L8[4])
    b = field.chain(o, d, 128, 16, seeded_grid(16), L8[4])
    assert_same(a, b, "two calls")


# ------------------------------------------------------------------ 3. graph
def test_graph_capture(field):
    """A capture that completes shows the entry neither allocates nor synchronises; a replay after the table, both packed images, the
    occupancy grid AND the time word were overwritten IN PLACE renders the new field at the new time (the graph holds pointers, not
    values).  The chain is linear, on one stream (the process keeps its default number of hardware queues)."""
    from project_nerf_amd import ops
    other = Field(make_engine(seed=2))
    R, S, chunk = 13, 64, 5
    o, d = crossing_rays(R, seed=17)
    bg = field.bg.clone()
    table, packed_d, packed_c = field.table[True].clone(), field.packed_d.clone(), field.packed_c.clone()
    grid, time = seeded_grid(18).clone(), torch.tensor([0.25], device="cuda")
    ws = workspace(chunk, S)

    def call():
        return ops.p3_render_rays_fwd(packed_d, packed_c, table, field.levels, HASH_BOUND, grid, GRID_BOUND, o, d, S, 2.0, 6.0, time, bg, chunk,
                                      workspace=ws)

    eager = [t.clone() for t in call()]
    assert_same(eager, field.loop(o, d, S, chunk, grid, 0.25), "eager")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, eager, "first replay")
    table.copy_(other.table[True])
    packed_d.copy_(other.packed_d)
    packed_c.copy_(other.packed_c)
    grid.copy_(seeded_grid(19))
    time.fill_(L8[5])
    g.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    fresh = call()
    assert_same(replayed, fresh, "replay on new values")
    assert_same(replayed, other.loop(o, d, S, chunk, grid, L8[5]), "replay against the loop on the new values")
    assert not torch.equal(replayed[0], eager[0])
    # the time word alone: a replay at another time differs from the one before it and equals the loop at that time
    time.fill_(L8[2])
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out[0], replayed[0])
    assert_same(out, other.loop(o, d, S, chunk, grid, L8[2]), "replay at another time")


# ------------------------------------------------------------------ 4. engine
def test_engine_keyword():
    """render_image(chain=True) == render_image(chain=False) on a trained-a-little engine with an occupancy grid of its own"""
    eng = make_engine(seed=3)
    o, d = crossing_rays(256, seed=21)
    gen = torch.Generator().manual_seed(22)
    target, t = torch.rand(256, 3, generator=gen).cuda(), torch.rand(256, 1, generator=gen).cuda()
    for _ in range(3):
        eng.train_step(o, d, target, t, 32)
    times = (0.0, L8[3], 1.0)
    eng.update_grid(times)                               # the field's densities on the lattice, the union over the times ...
    eng.grid_threshold = float(eng.grid.median())        # ... cut at their median: about half of the cells stay occupied
    ratio = eng.update_grid(times)
    assert 0.2 < ratio < 0.8, ratio
    vo, vd = crossing_rays(24 * 24, seed=23)
    vo, vd = vo.view(24, 24, 3), vd.view(24, 24, 3)
    bg = torch.tensor([0.25, 0.5, 0.75], device="cuda")
    for time, kw in ((torch.tensor(L8[3]), {}), (torch.tensor([[L8[6]]]).cuda(), dict(bg=bg))):
        a = eng.render_image(vo, vd, time, 32, chunk=100, chain=True, **kw)
        b = eng.render_image(vo, vd, time, 32, chunk=100, chain=False, **kw)
        assert a.shape == b.shape == (24, 24, 3)
        assert torch.equal(a, b), f"{int((a != b).sum())} values differ"
        assert float((b - eng.bg if not kw else b - bg).abs().max()) > 0.0           # not a frame of background
    assert list(eng._chain_ws) == [(100, 32)]            # the workspace is kept per (chunk, n_samples)
    ws, word = eng._chain_ws[(100, 32)], eng._chain_time
    assert ws.numel() == 100 * 32 * 124 + 256 and float(word) == torch.tensor(L8[6]).item()
    eng.render_image(vo, vd, torch.tensor(0.5), 32, chunk=100, chain=True)
    assert eng._chain_ws[(100, 32)] is ws and eng._chain_time is word and float(word) == 0.5
    eng.render_image(vo, vd, torch.tensor(0.5), 16, chunk=100, chain=True)
    assert set(eng._chain_ws) == {(100, 32), (100, 16)}


def test_the_other_dynamic_engines_refuse_the_keyword():
    from project_nerf_amd.part3_nerf import Part3NerfEngine
    from project_nerf_amd.part4 import DualHashEngine
    from test_gpu_part3_nerf_engine import cfg_of
    from test_gpu_part4_infer_workspace import CFG as PART4
    vo, vd = crossing_rays(16, seed=25)
    for eng in (Part3NerfEngine(cfg_of("standard"), seed=1), DualHashEngine(dict(PART4), device="cuda", seed=1)):
        with pytest.raises(NotImplementedError, match=type(eng).__name__):
            eng.render_image(vo, vd, torch.tensor(0.5), 16, chain=True)
        assert eng.render_image(vo, vd, torch.tensor(0.5), 16, chain=False).shape == (16, 3)      # today's path is untouched


# ------------------------------------------------------------------ 5. YAML
def _run_py(tmp_path, **over):
    root = _dynamic_scene(str(tmp_path / "dyn"))
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part3_instant.yaml.example")))
    cfg.update(train_iters=20, batch_size=256, log_every=10, val_every=20, downscale=1, n_samples=24, render_n_samples=24,
               log2_hashmap_size=12, grid_resolution=24, grid_warmup_iters=8, log_dir=str(tmp_path / "out"), render_chain=True, **over)
    cfg_path = tmp_path / "part3_instant.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    return subprocess.run([sys.executable, os.path.join(ROOT, "run.py"), "--config", str(cfg_path), "--data_dir", root, "--render_n", "1"],
                          capture_output=True, text=True, cwd=ROOT, timeout=600)


def test_run_py_renders_through_the_chain(tmp_path):
    r = _run_py(tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "render_chain" in r.stdout and "nerf_p3_render_rays_fwd" in r.stdout, r.stdout[-2000:]
    assert "[Validation] PSNR" in r.stdout and "Test PSNR" in r.stdout, r.stdout[-2000:]


def test_run_py_refuses_the_key_without_the_engine(tmp_path):
    r = _run_py(tmp_path, engine=False)
    assert r.returncode != 0
    assert "render_chain" in r.stderr and "engine" in r.stderr, r.stderr[-2000:]
