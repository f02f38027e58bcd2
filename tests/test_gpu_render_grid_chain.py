"""nerf_render_rays_grid_fwd -- the vanilla (8x256) field evaluated through an occupancy grid as one launch chain whose decoder
kernel reads the compaction's active count from device memory -- against the host-counted path on the same inputs
(VanillaNerfEngine.render_rays_grid in a Python loop; renderer.render_rays with a density_grid for the module helper) and against
the reference's own masked render (g6_render_masked).  A sample's outputs depend on its own point and direction only (MFMA columns
are independent), not on its compact slot or the launch shape, so every comparison is torch.equal unless stated.  The field is the
g4_decoder golden weights; the occupancy grid is 16^3: each test runs in about a second."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy

BOUND, RES = 1.5, 16


@pytest.fixture(scope="module")
def field():
    """the reference's default NeuralField holding the g4_decoder weights (as tests/test_gpu_surface.py::field builds it)"""
    assert torch.cuda.is_available()
    from src.core import NeuralField
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2.yaml.example")))
    model = NeuralField(cfg).cuda()
    sd = model.state_dict()
    for k, v in golden("g4_decoder").items():
        if k.startswith("w:"):
            assert "decoder." + k[2:] in sd, k
            sd["decoder." + k[2:]] = T(v)
    model.load_state_dict(sd)
    return model


def make_engine(field, **kw):
    from project_nerf_amd.engine import VanillaNerfEngine
    with torch.no_grad():
        return VanillaNerfEngine(params=field.decoder.flat_parameters(), device="cuda", grid_resolution=RES, bound=BOUND, **kw)


@pytest.fixture(scope="module")
def eng(field):
    return make_engine(field)


def ones_grid():
    return torch.ones(RES, RES, RES, dtype=torch.bool, device="cuda")


def seeded_grid(seed, fraction=0.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(RES, RES, RES, generator=g) < fraction).cuda()


def inner_rays(R, seed=0):
    """origins within 0.2 of the centre, unit directions: with near 0.1 / far 1.0 every sample lies inside the box"""
    g = torch.Generator().manual_seed(seed)
    o = ((torch.rand(R, 3, generator=g) - 0.5) * 0.4).cuda()
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).cuda()
    return o.contiguous(), d.contiguous()


def crossing_rays(R, seed=0):
    """origins on the sphere of radius 4 looking at the box: with near 2 / far 6 the first and last samples of a ray lie outside it"""
    g = torch.Generator().manual_seed(seed)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 4.0
    d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, generator=g), dim=-1)
    return o.cuda().contiguous(), d.cuda().contiguous()


class Scene:
    """temporarily points an engine at a grid / depth range / background"""

    def __init__(self, eng, grid, near=2.0, far=6.0, bg=None):
        self.eng, self.new = eng, (grid, near, far, eng.bg if bg is None else bg)

    def __enter__(self):
        e = self.eng
        self.old = (e.binary_grid, e.near, e.far, e.bg)
        e.binary_grid, e.near, e.far, e.bg = self.new
        return e

    def __exit__(self, *exc):
        e = self.eng
        e.binary_grid, e.near, e.far, e.bg = self.old


def loop(eng, o, d, S, chunk):
    """the host-counted path: render_rays_grid chunk by chunk (one host read of the active count per chunk)"""
    bg, outs = eng.bg, []
    try:
        for i in range(0, o.shape[0], chunk):
            if bg.dim() == 2:
                eng.bg = bg[i:i + chunk].contiguous()
            outs.append(eng.render_rays_grid(o[i:i + chunk].contiguous(), d[i:i + chunk].contiguous(), S))
    finally:
        eng.bg = bg
    return tuple(torch.cat([x[k] for x in outs], 0) for k in range(3))


def chain(eng, o, d, S, chunk, workspace=None):
    from project_nerf_amd import ops
    return ops.render_rays_grid_fwd(eng._inference_weights(), eng.binary_grid, eng.bound, o, d, S, eng.near, eng.far, eng.bg, chunk,
                                    workspace=workspace)


def workspace(chunk, S, fill=None):
    from project_nerf_amd import ops
    ws = torch.empty(ops.render_rays_grid_workspace_bytes(chunk, S), dtype=torch.uint8, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    return ws


def count_word(ws):
    return int(ws[:4].view(torch.int32).item())


def assert_same(got, want, what=""):
    for name, a, b in zip(("rgb", "depth", "acc"), got, want):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        assert torch.equal(a, b), f"{what} {name}: {int((a != b).sum())} of {a.numel()} values differ, max |diff| {float((a - b).abs().max()):.3e}"


# counts 2 | 15, 16, 17 (a 16-sample lane group) | 63, 64, 65 (a 64-sample wave) | 255, 256, 257 (a 256-sample tile)
@pytest.mark.parametrize("R,S", [(1, 2), (1, 15), (2, 8), (1, 17), (3, 21), (1, 64), (5, 13), (3, 85), (2, 128), (1, 257)])
def test_exact_counts_at_the_kernel_edges(eng, R, S):
    o, d = inner_rays(R, seed=R * 1000 + S)
    with Scene(eng, ones_grid(), near=0.1, far=1.0):
        ws = workspace(R, S)
        got = chain(eng, o, d, S, R, ws)
        assert count_word(ws) == R * S
        want = loop(eng, o, d, S, R)
    assert float(want[2].min()) > 0.0                    # the field was evaluated: every ray accumulated something
    assert_same(got, want, f"R={R} S={S}")


def test_count_zero_renders_the_background(eng):
    o, d = crossing_rays(4, seed=3)
    with Scene(eng, torch.zeros(RES, RES, RES, dtype=torch.bool, device="cuda")):
        ws = workspace(4, 8, fill=0xFF)                  # rgb / sigma rows hold NaN patterns: nothing may read them
        got = chain(eng, o, d, 8, 4, ws)
        assert count_word(ws) == 0
        want = loop(eng, o, d, 8, 4)
        assert torch.equal(got[0], eng.bg.expand(4, 3)) and torch.equal(got[1], torch.zeros(4, device="cuda"))
        assert torch.equal(got[2], torch.zeros(4, device="cuda"))
    assert_same(got, want, "empty grid")


def test_count_one(eng):
    """4 rays x 8 samples along +x, 0.343 apart (a cell is 0.1875 wide): the one occupied cell holds exactly one sample of one ray"""
    from project_nerf_amd import ops
    o = torch.tensor([[-1.4, y, 0.05] for y in (-0.9, -0.3, 0.3, 0.9)], device="cuda")
    d = torch.tensor([[1.0, 0.0, 0.0]] * 4, device="cuda")
    near, far, S = 0.2, 2.6, 8
    _, pts, _ = ops.sample_rays(o, d, near, far, S, want_points=True)
    _, idx = ops.active_mask(pts, ones_grid(), BOUND, want_index=True)
    cell = idx[2 * S + 3].tolist()                       # sample 3 of ray 2
    grid = torch.zeros(RES, RES, RES, dtype=torch.bool, device="cuda")
    grid[cell[0], cell[1], cell[2]] = True
    slots = ops.sample_compact(o, d, near, far, S, grid, BOUND)[1]
    assert int((slots >= 0).sum()) == 1 and int(slots[2 * S + 3]) == 0
    with Scene(eng, grid, near=near, far=far):
        ws = workspace(4, S, fill=0xFF)
        got = chain(eng, o, d, S, 4, ws)
        assert count_word(ws) == 1
        want = loop(eng, o, d, S, 4)
    assert not bool(torch.isnan(got[0]).any())
    assert float(want[2][0]) == 0.0 and float(want[2][1]) == 0.0 and float(want[2][3]) == 0.0
    assert_same(got, want, "one active sample")


def test_more_tiles_than_workgroups(eng):
    """600 rays x 128 samples = 76,800 samples = 300 tiles of 256, more than the chip's 256 CUs: some workgroup walks two tiles.  The
    same rays against a grid with ONE occupied cell: the launch is still sized for 300 tiles, the count is small and most workgroups
    find no tile (they drain their cold-start DMA and leave)."""
    from project_nerf_amd import ops
    R, S = 600, 128
    o, d = inner_rays(R, seed=41)
    with Scene(eng, ones_grid(), near=0.1, far=1.0):
        ws = workspace(R, S)
        got = chain(eng, o, d, S, R, ws)
        assert count_word(ws) == R * S
        want = loop(eng, o, d, S, R)
        assert_same(got, want, "76,800 active samples")
        assert float(want[2].min()) > 0.0
        _, pts, _ = ops.sample_rays(o, d, 0.1, 1.0, S, want_points=True)
        _, idx = ops.active_mask(pts, ones_grid(), BOUND, want_index=True)
    cell = idx[7 * S + 100].tolist()                     # the cell of sample 100 of ray 7
    grid = torch.zeros(RES, RES, RES, dtype=torch.bool, device="cuda")
    grid[cell[0], cell[1], cell[2]] = True
    with Scene(eng, grid, near=0.1, far=1.0):
        got = chain(eng, o, d, S, R, ws)                 # (the workspace still holds the 76,800 rows of the call above)
        n = count_word(ws)
        print(f"one occupied cell: {n} active samples of {R * S}")
        assert 0 < n < R * S // 16
        want = loop(eng, o, d, S, R)
    assert float(want[2][7]) > 0.0
    assert_same(got, want, "one occupied cell under a 300-tile launch")


def test_several_compaction_passes_and_a_partial_grid(eng):
    """5120 samples: more than one 4096-sample compaction pass; rays that enter and leave the box; ~30 % of the cells set"""
    o, d = crossing_rays(40, seed=5)
    with Scene(eng, seeded_grid(11)):
        ws = workspace(40, 128)
        got = chain(eng, o, d, 128, 40, ws)
        n = count_word(ws)
        assert 0 < n < 40 * 128
        want = loop(eng, o, d, 128, 40)
    assert_same(got, want, "5120 samples")


@pytest.mark.parametrize("chunk", [5, 64])
def test_chunking_and_per_ray_background(eng, chunk):
    """13 rays in chunks of 5, 5, 3 (and as one chunk), a background row per ray: the chain slices rays, outputs and bg + r0 * 3"""
    o, d = crossing_rays(13, seed=7)
    bg = (torch.arange(39, dtype=torch.float32).view(13, 3) / 40.0).cuda()
    with Scene(eng, seeded_grid(12), bg=bg):
        got = chain(eng, o, d, 64, chunk)
        want = loop(eng, o, d, 64, min(chunk, 13))
    assert_same(got, want, f"chunk {chunk}")
    assert len({tuple(r) for r in got[0].tolist()}) == 13           # distinct rows: a wrong bg slice could not go unnoticed


def test_workspace_contents_do_not_matter(eng):
    o, d = crossing_rays(40, seed=5)
    o1, d1 = inner_rays(1, seed=9)
    with Scene(eng, seeded_grid(11)):
        a = chain(eng, o, d, 128, 40, workspace(40, 128, fill=0xFF))
        ws = workspace(40, 128, fill=0)
        b = chain(eng, o, d, 128, 40, ws)
    assert_same(a, b, "0xFF against zeroed workspace")
    # the 5120-sample call's count and rows are still in ws: a 127-sample call on it must not see them
    with Scene(eng, ones_grid(), near=0.1, far=1.0):
        got = chain(eng, o1, d1, 127, 1, ws)
        assert count_word(ws) == 127
        want = loop(eng, o1, d1, 127, 1)
    assert_same(got, want, "127 samples after 5120 on one workspace")


def test_repeatable(eng):
    o, d = crossing_rays(40, seed=15)
    with Scene(eng, seeded_grid(16)):
        a = chain(eng, o, d, 128, 16)
        b = chain(eng, o, d, 128, 16)
    assert_same(a, b, "two calls")


def test_graph_capture(eng):
    """A capture that completes shows the entry neither allocates nor synchronises; a replay after the packed weights and the
    occupancy grid were overwritten IN PLACE renders the new field (the graph holds pointers, not values)."""
    from project_nerf_amd import ops
    other = eng.params.clone()
    other[-3:] += 1.0                                    # rgb_layer.bias: every colour changes
    other_packed = ops.mlp_pack(other)
    R, S, chunk = 13, 64, 5
    o, d = crossing_rays(R, seed=17)
    bg = eng.bg.clone()
    packed, grid = eng._inference_weights().clone(), seeded_grid(18).clone()
    ws = workspace(chunk, S)

    def call():
        return ops.render_rays_grid_fwd(packed, grid, BOUND, o, d, S, 2.0, 6.0, bg, chunk, workspace=ws)

    eager = [t.clone() for t in call()]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, eager, "first replay")
    assert float(eager[2].max()) > 0.0
    packed.copy_(other_packed)
    grid.copy_(seeded_grid(19))
    g.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    fresh = call()
    assert_same(replayed, fresh, "replay on new values")
    assert not torch.equal(replayed[0], eager[0])


def test_compact_rows_equal_point_mode(eng):
    """the chain's compact rgb / sigma rows, read back from the workspace, are nerf_mlp_fwd's in point mode on the same compact points"""
    from project_nerf_amd import ops
    R, S = 40, 128
    n_all = R * S
    up = lambda b: (b + 255) // 256 * 256
    off_pts = 256 + 2 * up(n_all * 4)
    off_dirs = off_pts + up(n_all * 12)
    off_rgb = off_dirs + up(n_all * 12)
    off_sigma = off_rgb + up(n_all * 12)
    o, d = crossing_rays(R, seed=5)
    with Scene(eng, seeded_grid(11)):
        ws = workspace(R, S, fill=0xFF)
        chain(eng, o, d, S, R, ws)
    n = count_word(ws)
    print(f"{n} active samples of {n_all}")
    assert 0 < n < n_all
    rows = lambda off, width: ws[off:off + n * width * 4].view(torch.float32).view(n, width).clone()
    pts, dirs, rgb, sigma = rows(off_pts, 3), rows(off_dirs, 3), rows(off_rgb, 3), rows(off_sigma, 1).view(n)
    want_rgb, want_sigma = ops.mlp_fwd(eng._inference_weights(), pts, dirs, None)
    assert torch.equal(rgb, want_rgb) and torch.equal(sigma, want_sigma)
    assert float(sigma.max()) > 0.0
    # nothing was written behind row n: the fill pattern is still there
    assert bool((ws[off_sigma + n * 4:off_sigma + n_all * 4] == 0xFF).all())
    assert bool((ws[off_rgb + n * 12:off_rgb + n_all * 12] == 0xFF).all())


def test_refuses_another_kernel_family(eng):
    from project_nerf_amd import _lib
    o, d = crossing_rays(4, seed=3)
    _lib.set_option("infer64", 0)
    try:
        with Scene(eng, seeded_grid(11)):
            with pytest.raises(_lib.NerfHipError, match="infer64"):
                chain(eng, o, d, 8, 4)
    finally:
        _lib.set_option("infer64", 1)


def sphere_grid(radius):
    """the 128^3 sphere grid of tests/test_gpu_surface.py::test_render_rays_with_density_grid_vs_reference_golden"""
    from src.renderer import DensityGrid
    grid = DensityGrid(resolution=128, bound=1.5, threshold=0.01).cuda()
    ax = torch.linspace(-1.5, 1.5, 128)
    gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
    grid.binary_grid = ((gx ** 2 + gy ** 2 + gz ** 2) < radius ** 2).cuda()
    return grid


def test_against_the_reference_masked_render(field):
    """pinned to the reference's own masked render of this field (g6_render_masked), at the stated tolerance for the bf16 decoder
    against the reference's fp32 renderer (atol 1e-2), and bit for bit to the module path on the same inputs"""
    from project_nerf_amd import ops
    from src.renderer import render_rays
    gm = golden("g6_render_masked")
    grid = sphere_grid(float(gm["radius"]))
    o, d, bg = T(gm["rays_o"]).cuda(), T(gm["rays_d"]).cuda(), T(gm["bg"]).cuda()
    with torch.no_grad():
        want = render_rays(field, o, d, 2.0, 6.0, 64, False, density_grid=grid, bg_color=bg)
        got = ops.render_rays_grid_fwd(field.decoder.packed_weights(), grid.binary_grid, grid.bound, o, d, 64, 2.0, 6.0, bg, o.shape[0])
    np.testing.assert_allclose(got[0].cpu().numpy(), gm["rgb"], atol=1e-2)
    np.testing.assert_allclose(got[2].cpu().numpy(), gm["acc"], atol=1e-2)
    assert_same(got, want, "module path")


def test_engine_surface(field):
    eng = make_engine(field)
    assert eng.binary_grid is None and eng.grid is None
    vo, vd = crossing_rays(24 * 24, seed=23)
    vo, vd = vo.view(24, 24, 3), vd.view(24, 24, 3)
    with pytest.raises(ValueError, match="grid"):
        eng.render_image(vo, vd, 32, chunk=100, grid=True)
    with pytest.raises(ValueError, match="grid"):
        eng.render_image(vo, vd, 32, chunk=100, grid="loop")
    dense = eng.render_image(vo, vd, 32, chunk=100)      # the default path needs no grid
    eng.update_grid()                                    # the field's densities on the lattice ...
    eng.grid_threshold = float(eng.grid.median())        # ... cut at their median: about half of the cells stay occupied
    ratio = eng.update_grid()
    print(f"update_grid: ratio {ratio:.3f} at the median threshold {eng.grid_threshold:.4g}")
    assert 0.2 < ratio < 0.8
    assert eng.binary_grid.shape == (RES, RES, RES) and eng.binary_grid.dtype == torch.bool
    a = eng.render_image(vo, vd, 32, chunk=100, grid=True)
    b = eng.render_image(vo, vd, 32, chunk=100, grid="loop")
    assert a.shape == b.shape == dense.shape == (24, 24, 3)
    assert torch.equal(a, b), f"{int((a != b).sum())} values differ"
    assert (100, 32) in eng._grid_ws                     # the workspace is kept per (chunk, n_samples)
    ws = eng._grid_ws[(100, 32)]
    eng.render_image(vo, vd, 32, chunk=100, grid=True)
    assert eng._grid_ws[(100, 32)] is ws
    with pytest.raises(ValueError, match="n_fine"):
        eng.render_image(vo, vd, 32, chunk=100, n_fine=16, grid=True)
    assert torch.equal(eng.render_image(vo, vd, 32, chunk=100), dense)          # the default path is untouched by the grid


def test_module_helper(field):
    """renderer.render_rays_nerf_grid_chain == the render_rays(..., density_grid=grid) chunk loop on a NeuralField, when every chunk
    has an active sample; an all-empty grid gives exactly the background (render_rays would query sample 0 of its first ray)"""
    from project_nerf_amd import ops
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.renderer import DensityGrid, render_rays, render_rays_nerf_grid_chain
    grid = DensityGrid(RES, BOUND, 0.01).cuda()
    grid.binary_grid = seeded_grid(32)
    R, S, chunk, near, far = 13, 32, 5, 2.0, 6.0
    o, d = crossing_rays(R, seed=33)
    for i in range(0, R, chunk):                         # every chunk of the loop has an active sample
        slots = ops.sample_compact(o[i:i + chunk].contiguous(), d[i:i + chunk].contiguous(), near, far, S, grid.binary_grid, BOUND)[1]
        assert int((slots.cpu() >= 0).sum()) > 0
    with torch.no_grad():
        parts = [render_rays(field, o[i:i + chunk], d[i:i + chunk], near, far, S, False, density_grid=grid, white_bkgd=True)
                 for i in range(0, R, chunk)]
    want = tuple(torch.cat([p[k] for p in parts], 0) for k in range(3))
    got = render_rays_nerf_grid_chain(field, o, d, near, far, S, grid, True, chunk)
    assert float(want[2].max()) > 0.0
    assert_same(got, want, "module helper")
    with pytest.raises(ValueError, match="density_grid"):
        render_rays_nerf_grid_chain(field, o, d, near, far, S, None, True, chunk)
    grid.binary_grid = torch.zeros(RES, RES, RES, dtype=torch.bool, device="cuda")
    rgb, depth, acc = render_rays_nerf_grid_chain(field, o, d, near, far, S, grid, True, chunk)
    assert torch.equal(rgb, torch.ones(R, 3, device="cuda")) and torch.equal(depth, torch.zeros(R, device="cuda"))
    assert torch.equal(acc, torch.zeros(R, device="cuda"))
    instant = NeuralField({"mode": "part2_instant", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 16,
                           "per_level_scale": 1.5, "scene_bound": BOUND, "hidden_dim": 64, "L_embed_dir": 4}).cuda()
    with pytest.raises(ValueError, match="part2_nerf"):
        render_rays_nerf_grid_chain(instant, o, d, near, far, S, grid, True, chunk)


def test_run_py_cli_with_a_density_grid(tmp_path):
    """run.py part2 with `use_density_grid: true`: the checkpoints hold the grid in the reference's format, evaluation goes through
    the chain and reports a finite PSNR; --eval_only --checkpoint loads the grid instead of rebuilding it"""
    from src.dataset import write_synthetic_scene
    root = write_synthetic_scene(str(tmp_path / "scene"), n_train=6, n_test=1, size=32)
    out = tmp_path / "out"
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2.yaml.example")))
    cfg.update(train_iters=10, batch_size=512, log_every=10, save_every=10, downscale=1, log_dir=str(out), seed=0,
               use_density_grid=True, grid_resolution=32)
    cfg_path = tmp_path / "part2_grid.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "run.py"), "--config", str(cfg_path), "--data_dir", root, "--render_n", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Density grid: rebuilt" in r.stdout
    psnr = float(r.stdout.split("Test PSNR:")[1].split("dB")[0])
    assert np.isfinite(psnr)
    final = out / "checkpoints" / "model_final.pth"
    ckpt = torch.load(final, map_location="cpu")
    assert set(ckpt) == {"model_state_dict", "config", "density_grid"}
    assert set(ckpt["density_grid"]) == {"grid", "binary_grid"}
    assert ckpt["density_grid"]["binary_grid"].shape == (32, 32, 32) and ckpt["density_grid"]["binary_grid"].dtype == torch.bool
    r2 = subprocess.run(cmd + ["--eval_only", "--checkpoint", str(final)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert "Density grid: loaded from the checkpoint" in r2.stdout and "Density grid: rebuilt" not in r2.stdout
    psnr2 = float(r2.stdout.split("Test PSNR:")[1].split("dB")[0])
    assert psnr2 == psnr                                 # the same weights, the same grid, the same chain
