"""The Instant-NGP shape chain (csrc/imlp_shapes.hip, project-nerf_amd/instant_shapes.py) on the GPU.

Reference: the float64 restatement of the chain in tests/test_instant_shapes_layout.py::chain64 with bf16 rounding at the chain's
rounding points, and its float64 autograd.  The bounds are not fixed in advance: the yardstick is what the existing kernels
(nerf_imlp_fwd / nerf_imlp_bwd at 16 levels, 64 hidden units, 4 direction bands) miss the same reference by, on the same points,
directions and cotangents, measured in this module (fixture ``yardstick``); every new-shape bound is 4 x that figure (the margin:
H = 128's doubled sum lengths, the occasional one-ulp bf16 flip of an activation).  Each test prints its figures next to the
bound.  Measured yardstick and largest fraction of a bound used: see DESIGN.md section 4.13.

At (16, 64, 4) the chain runs imlp.hip's k-order step for step: rgb, sigma and d_feat are asserted bit-equal to the existing
kernels'.  The weight gradients are not: the existing kernels sum split-K partial tiles with float atomics, the new ones sum
chunk partials in chunk order; they are held to twice the yardstick (each side is within one yardstick of the reference)."""
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT
from oracle import nerf_oracle as O
from test_instant_shapes_layout import SHAPES, cfg_of, chain64

pytestmark = pytest.mark.gpu

ALL_SHAPES = SHAPES + [(12, 64, 4)]
SWEEP = [1, 31, 32, 33, 127, 128, 129, 257, 1025]
FULL_SWEEP_SHAPES = [(5, 32, 2), (16, 128, 4)]
CASES = [(s, n) for s in ALL_SHAPES for n in (SWEEP if s in FULL_SWEEP_SHAPES else [129, 1025])]
BOUND, LOG2_T, BASE_RES = 1.5, 11, 4
NAMES = ["sigma_net.0", "sigma_net.1", "color_net.0", "color_net.1", "color_net.2", "d_feat"]
P = lambda t: t.data_ptr()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import project_nerf_amd  # noqa: F401
    from project_nerf_amd import ops as _ops
    return _ops


def inputs(shape, n, ops, sigma_scale=None):
    """points, directions, cotangents (non-zero mean) shared by every shape: the first n of one draw; table and weights of the shape"""
    from project_nerf_amd import instant_shapes as S
    L, H, Ld = shape
    g = torch.Generator().manual_seed(1234)
    pts = ((torch.rand(1025, 3, generator=g) - 0.5) * 2 * BOUND * 1.05)[:n].contiguous()
    dirs = torch.nn.functional.normalize(torch.randn(1025, 3, generator=g), dim=-1)[:n].contiguous()
    d_rgb = (torch.randn(1025, 3, generator=g) * 0.5 + 0.3)[:n].contiguous()
    d_sigma = (torch.randn(1025, generator=g) * 0.5 + 0.3)[:n].contiguous()
    levels = ops.HashLevelTable(L, LOG2_T, BASE_RES, 1.5)
    gs = torch.Generator().manual_seed(L * 1000 + H + Ld)
    table = (torch.rand(levels.entries, 2, generator=gs) * 2 - 1) * 0.5
    cfg = cfg_of(L, H, Ld)
    flat = (torch.rand(S.param_count(cfg), generator=gs) * 2 - 1) * 0.4          # pad rows / columns hold values too: never read
    if sigma_scale is not None:
        off = S.slice_table(cfg)[1][1]
        flat[off:off + H] = -flat[off:off + H].abs() * sigma_scale               # row 0 of the sigma head: strongly negative h0
    return dict(cfg=cfg, shape=shape, n=n, levels=levels, pts=pts.cuda(), dirs=dirs.cuda(), d_rgb=d_rgb.cuda(), d_sigma=d_sigma.cuda(),
                table=table.cuda(), flat=flat.cuda())


def run_new(ops, c, train=True, fill=0, backward=True):
    """hash forward into the workspace (pre-filled with `fill` bytes) -> chain forward [-> backward]"""
    lib = ops._lib.load()
    n, shape = c["n"], c["shape"]
    ws = torch.full((lib.nerf_imlp_shape_workspace_bytes(n, *shape),), fill, device="cuda", dtype=torch.uint8)
    packed = torch.empty(lib.nerf_imlp_shape_packed_bytes(*shape), device="cuda", dtype=torch.uint8)
    ops._lib.check(lib.nerf_imlp_shape_pack(P(c["flat"]), *shape, P(packed), ops._stream()), "pack")
    ops.hash_encode_fwd(c["pts"], c["table"], c["levels"], BOUND, want_f32=False, out_nat=ws[lib.nerf_imlp_shape_hash_operand_offset(n, *shape):])
    rgb, sigma = torch.empty(n, 3, device="cuda"), torch.empty(n, device="cuda")
    ops._lib.check(lib.nerf_imlp_shape_fwd(P(packed), P(ws), P(c["dirs"]), n, *shape, P(rgb), P(sigma), 1 if train else 0, ops._stream()), "fwd")
    if not (train and backward):
        return rgb, sigma, None, None
    grads = torch.full_like(c["flat"], float("nan"))
    d_feat = torch.full((n, 2 * shape[0]), float("nan"), device="cuda")
    ops._lib.check(lib.nerf_imlp_shape_bwd(P(packed), P(ws), P(rgb), P(sigma), P(c["d_rgb"]), P(c["d_sigma"]), n, *shape, P(grads), P(d_feat),
                                           ops._stream()), "bwd")
    return rgb, sigma, grads, d_feat


def run_old(ops, c):
    """the existing kernels (imlp.hip) on the same inputs; shape (16, 64, 4) only"""
    lib = ops._lib.load()
    n = c["n"]
    ws = torch.zeros(lib.nerf_imlp_workspace_bytes(n), device="cuda", dtype=torch.uint8)
    packed = ops.imlp_pack(c["flat"])
    ops.hash_encode_fwd(c["pts"], c["table"], c["levels"], BOUND, want_f32=False, out_nat=ws)
    rgb, sigma = torch.empty(n, 3, device="cuda"), torch.empty(n, device="cuda")
    ops._lib.check(lib.nerf_imlp_fwd(P(packed), P(ws), P(c["dirs"]), n, P(rgb), P(sigma), 1, ops._stream()), "imlp fwd")
    grads, d_feat = torch.empty_like(c["flat"]), torch.empty(n, 32, device="cuda")
    ops._lib.check(lib.nerf_imlp_bwd(P(packed), P(ws), P(rgb), P(sigma), P(c["d_rgb"]), P(c["d_sigma"]), n, P(grads), P(d_feat), ops._stream()),
                   "imlp bwd")
    return rgb, sigma, grads, d_feat


_REF = {}


def reference(ops, c, key):
    """matched float64 chain (bf16 at the chain's rounding points) and its autograd; computed once per case"""
    if key in _REF:
        return _REF[key]
    Ld = c["shape"][2]
    x = ops.hash_encode_fwd(c["pts"], c["table"], c["levels"], BOUND)[0].cpu()          # the fp32 features the image holds as bf16
    d = O.fourier_encode(c["dirs"].cpu(), Ld)
    flat = c["flat"].cpu().double().requires_grad_(True)
    x = x.double().requires_grad_(True)
    rgb, sigma = chain64(c["cfg"], flat, x, d, rounded=True)
    ((rgb * c["d_rgb"].cpu().double()).sum() + (sigma * c["d_sigma"].cpu().double()).sum()).backward()
    rgb32, sigma32 = chain64(c["cfg"], c["flat"].cpu().double(), x.detach(), d, rounded=False)
    _REF[key] = dict(rgb=rgb.detach(), sigma=sigma.detach(), g_flat=flat.grad, d_feat=x.grad, rgb32=rgb32, sigma32=sigma32)
    return _REF[key]


def errors(c, ref, rgb, sigma, grads, d_feat):
    from project_nerf_amd import instant_shapes as S
    rel = lambda a, b: float((a.double().cpu() - b).norm() / (b.norm() + 1e-300))
    e = {"rgb_max": float((rgb.double().cpu() - ref["rgb"]).abs().max()), "rgb_rel": rel(rgb, ref["rgb"]), "sigma_rel": rel(sigma, ref["sigma"])}
    for name, off, (o, k), (vr, vc) in S.slice_table(c["cfg"]):
        e[name] = rel(grads[off:off + o * k].view(o, k)[:vr, :vc], ref["g_flat"][off:off + o * k].view(o, k)[:vr, :vc])
    e["d_feat"] = rel(d_feat, ref["d_feat"])
    return e


@pytest.fixture(scope="module")
def yardstick(ops):
    c = inputs((16, 64, 4), 1025, ops)
    y = errors(c, reference(ops, c, ((16, 64, 4), 1025, None)), *run_old(ops, c))
    print("\n[yardstick: nerf_imlp_fwd / nerf_imlp_bwd at (16, 64, 4), n = 1025, against the matched float64 chain] " +
          " ".join(f"{k}={v:.3e}" for k, v in y.items()))
    assert all(0.0 < v < 0.1 for v in y.values()), y
    return y


@pytest.mark.parametrize("shape,n", CASES)
def test_forward_and_gradients_against_the_matched_float64_chain(ops, yardstick, shape, n):
    from project_nerf_amd import instant_shapes as S
    c = inputs(shape, n, ops)
    ref = reference(ops, c, (shape, n, None))
    rgb, sigma, grads, d_feat = run_new(ops, c)
    assert d_feat.shape == (n, 2 * shape[0]) and bool(torch.isfinite(d_feat).all()) and bool(torch.isfinite(grads).all())
    # pad rows and columns of the flat gradient: exactly zero
    for name, off, (o, k), (vr, vc) in S.slice_table(c["cfg"]):
        m = grads[off:off + o * k].view(o, k)
        assert float(m[vr:].abs().sum()) == 0.0 and float(m[:, vc:].abs().sum()) == 0.0, name
    e = errors(c, ref, rgb, sigma, grads, d_feat)
    print(f"\n[{shape} n={n}] " + " ".join(f"{k}={v:.3e} ({v / (4 * yardstick[k]):.2f} of bound)" for k, v in e.items()))
    for k, v in e.items():
        assert v <= 4 * yardstick[k], (shape, n, k, v, 4 * yardstick[k])
    # fp32 oracle (no rounding) at test_gpu_instant.py::test_instant_field_forward's stated bounds
    np.testing.assert_allclose(rgb.cpu().numpy(), ref["rgb32"].numpy(), atol=3e-2)
    np.testing.assert_allclose(sigma.cpu().numpy(), ref["sigma"].numpy(), rtol=2e-2, atol=1e-3)


@pytest.mark.parametrize("shape", [(5, 32, 2), (12, 64, 4)])
def test_poisoned_workspace_changes_nothing(ops, shape):
    """the hash forward leaves columns 2L.. of its operand image unwritten: 0xFF bytes (bf16 NaN) there and everywhere else"""
    c = inputs(shape, 257, ops)
    clean, poisoned = run_new(ops, c, fill=0), run_new(ops, c, fill=0xFF)
    for a, b in zip(clean, poisoned):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


@pytest.mark.parametrize("shape", [(5, 32, 2), (9, 128, 3)])
def test_same_bits_inference_training_and_run_to_run(ops, shape):
    c = inputs(shape, 1025, ops)
    a, b = run_new(ops, c), run_new(ops, c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    rgb, sigma, _, _ = run_new(ops, c, train=False)
    assert torch.equal(rgb, a[0]) and torch.equal(sigma, a[1])


def test_default_shape_against_the_existing_kernels(ops, yardstick):
    c = inputs((16, 64, 4), 1025, ops)
    new, old = run_new(ops, c), run_old(ops, c)
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])          # rgb, sigma: the same k-order, the same bits
    assert torch.equal(new[3], old[3])                                           # d_feat
    from project_nerf_amd import instant_shapes as S
    for name, off, (o, k), _ in S.slice_table(c["cfg"]):
        a, b = new[2][off:off + o * k], old[2][off:off + o * k]
        rel = float((a - b).norm() / b.norm())
        print(f"[default shape, {name}] new against existing weight gradient: rel L2 {rel:.3e} (bound {2 * yardstick[name]:.3e})")
        assert rel <= 2 * yardstick[name], (name, rel)


def test_softplus_gradient_at_strongly_negative_preactivation(ops):
    """test_gpu_instant.py's sigma ~ 0 case at (9, 128, 3): d sigma / d h0 = -expm1(-sigma) must not vanish where sigma is tiny"""
    c = inputs((9, 128, 3), 512, ops, sigma_scale=6.0)
    ref = reference(ops, c, ((9, 128, 3), 512, "negative"))
    assert float(ref["sigma"].min()) < 6e-8 and float(ref["sigma"].median()) < 1e-4
    c["d_sigma"] = (1.0 / ref["sigma"]).float().cuda()                           # every sample weighs ~1
    c["d_rgb"] = torch.zeros_like(c["d_rgb"])
    x = ops.hash_encode_fwd(c["pts"], c["table"], c["levels"], BOUND)[0].cpu().double()
    flat = c["flat"].cpu().double().requires_grad_(True)
    _, sigma = chain64(c["cfg"], flat, x, O.fourier_encode(c["dirs"].cpu(), 3), rounded=True)
    (sigma * c["d_sigma"].cpu().double()).sum().backward()
    _, _, grads, _ = run_new(ops, c)
    from project_nerf_amd import instant_shapes as S
    n_sigma = S.sigma_count(c["cfg"])
    a, b = grads[:n_sigma].cpu().double(), flat.grad[:n_sigma]
    rel = float((a - b).norm() / (b.norm() + 1e-30))
    assert b.norm() > 0 and rel < 0.05, rel


# ------------------------------------------------------------------------------------------------ whole step, optimiser, weights
def rays(R, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g)
    o = (o / o.norm(dim=-1, keepdim=True) * 4.0).cuda()
    d = torch.nn.functional.normalize(-o.cpu() + 0.2 * torch.randn(R, 3, generator=g), dim=-1).cuda().contiguous()
    return o, d, torch.rand(R, 3, generator=g).cuda(), g


def sphere(res, radius=1.0):
    ax = torch.linspace(-BOUND, BOUND, res)
    gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ((gx ** 2 + gy ** 2 + gz ** 2) < radius ** 2).cuda()


def step_cfg(L, H, Ld, **kw):
    return cfg_of(L, H, Ld, log2_hashmap_size=12, base_resolution=4, per_level_scale=1.5, scene_bound=BOUND, grid_resolution=16,
                  near=2.0, far=6.0, white_bkgd=True, **kw)


@pytest.mark.parametrize("shape", [(8, 32, 2), (16, 128, 4)])
def test_whole_step_and_render_against_the_module_path(shape):
    """64 rays x 16 samples through a 16^3 occupancy grid: loss, every gradient and a 24 x 24 render against NeuralField at the
    same shape on the module path (fp32 library GEMMs + autograd); the engine's weights come from the module and go back."""
    from src.core import NeuralField
    from src.renderer import DensityGrid, render_rays
    from project_nerf_amd import instant_shapes as S
    cfg = step_cfg(*shape, half_table=False)
    torch.manual_seed(5)
    model = NeuralField(cfg).cuda()
    assert not model.decoder.fused
    with torch.no_grad():
        model.representation.encoding.params.copy_((torch.rand(model.representation.encoding.params.shape, generator=torch.Generator().manual_seed(6)) - 0.5))
    grid = DensityGrid(16, BOUND, 0.01).cuda()
    grid.binary_grid = sphere(16)
    eng = S.InstantShapeEngine(cfg, seed=0)
    eng.table.copy_(model.representation.encoding.params.detach().reshape(-1))
    eng.set_net(model.decoder.sigma_net.params, model.decoder.color_net.params)
    eng.binary_grid = grid.binary_grid.clone()
    back = S.unflatten(cfg, eng.net)                                           # round trip module -> engine -> module
    assert torch.equal(back["decoder.sigma_net.params"], model.decoder.sigma_net.params.detach())
    assert torch.equal(back["decoder.color_net.params"], model.decoder.color_net.params.detach())
    o, d, target, g = rays(64, 3)
    u = torch.rand(64, 16, generator=g).cuda()
    loss_e = float(eng.compute_gradients(o, d, target, 16, u=u))
    orig = torch.rand
    torch.rand = lambda *a, **k: u.clone()                    # render_rays draws its jitter with torch.rand
    try:
        c, _, _ = render_rays(model, o, d, 2.0, 6.0, 16, True, density_grid=grid, bg_color=torch.ones(3, device="cuda"))
    finally:
        torch.rand = orig
    loss_m = torch.nn.functional.mse_loss(c, target)
    model.zero_grad()
    loss_m.backward()
    print(f"\n[{shape}] loss engine {loss_e:.6f} module {float(loss_m):.6f}")
    assert abs(loss_e - float(loss_m)) < 3e-3
    ns = S.sigma_count(cfg)
    for name, got, want in (("sigma_net", eng.g_net[:ns], model.decoder.sigma_net.params.grad), ("color_net", eng.g_net[ns:], model.decoder.color_net.params.grad),
                            ("table", eng.g_table, model.representation.encoding.params.grad.reshape(-1))):
        rel = float((got - want).norm() / (want.norm() + 1e-20))
        cos = float((got * want).sum() / (got.norm() * want.norm() + 1e-30))
        print(f"[{shape}] {name}: rel L2 {rel:.3e} cos {cos:.5f}")
        assert cos > 0.98 and rel < 0.2, (name, rel, cos)          # bf16 chain vs fp32 autograd: test_gpu_instant.py's stated bounds
    ax = torch.linspace(-0.6, 0.6, 24)
    py, px = torch.meshgrid(ax, ax, indexing="ij")
    io = torch.tensor([0.0, 0.0, 4.0]).expand(24, 24, 3).contiguous().cuda()
    idir = torch.nn.functional.normalize(torch.stack([px, py, -torch.ones_like(px) * 2.0], -1), dim=-1).cuda().contiguous()
    img = eng.render_image(io, idir, 16)
    with torch.no_grad():
        want = render_rays(model, io.reshape(-1, 3), idir.reshape(-1, 3), 2.0, 6.0, 16, False, density_grid=grid)[0]
    assert img.shape == (24, 24, 3)
    np.testing.assert_allclose(img.reshape(-1, 3).cpu().numpy(), want.cpu().numpy(), atol=2e-2)


def test_default_shape_step_and_optimiser_against_the_existing_engine():
    from project_nerf_amd.engine import InstantNgpEngine
    from project_nerf_amd import instant_shapes as S
    cfg = step_cfg(16, 64, 4, speculative_hash_backward=False)
    old, new = InstantNgpEngine(cfg, seed=2), S.InstantShapeEngine(cfg, seed=2)
    assert torch.equal(old.table, new.table)                                    # the same seed: the same table draw
    for e in (old, new):
        e.table.copy_((torch.rand(e.table.numel(), generator=torch.Generator().manual_seed(7)) - 0.5).cuda())
        e.binary_grid = sphere(16)
    new.net.copy_(old.net)
    new._pack()
    o, d, target, g = rays(64, 4)
    u = torch.rand(64, 16, generator=g).cuda()
    l_old, l_new = float(old.compute_gradients(o, d, target, 16, u=u)), float(new.compute_gradients(o, d, target, 16, u=u))
    assert abs(l_old - l_new) <= 1e-6 * max(l_old, 1.0)
    # the chains are bit-equal (test_default_shape_against_the_existing_kernels): the table gradients differ by the counted
    # scatter's float atomics where a bin is cut, at most
    assert float((new.g_table - old.g_table).abs().max()) <= 1e-6 * float(old.g_table.abs().max())
    assert float((new.g_net - old.g_net).norm() / old.g_net.norm()) < 1e-4
    new.g_table.copy_(old.g_table)
    new.g_net.copy_(old.g_net)
    old.apply_gradients()
    new.apply_gradients()
    assert torch.equal(old.table, new.table) and torch.equal(old.net, new.net) and old.step_count == new.step_count == 1
    assert torch.equal(old.table_h, new.table_h)


def test_shape_engine_trains_and_renders(tmp_path):
    """test_gpu_instant.py::test_instant_engine_trains_and_renders's analytic scene and step budget at (8, 32, 2)"""
    from src.dataset import BlenderDataset, write_synthetic_scene
    from project_nerf_amd import instant_shapes as S
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2_instant_small.yaml.example")))
    assert (cfg["n_levels"], cfg["hidden_dim"], cfg["L_embed_dir"]) == (8, 32, 2)
    cfg["train_iters"] = 400
    root = write_synthetic_scene(str(tmp_path / "scene"), n_train=12, n_test=2, size=64)
    ds = BlenderDataset(root, "train", 1, True, 1.0).to("cuda")
    eng = S.InstantShapeEngine(cfg, seed=0)
    torch.manual_seed(0)
    first = None
    for step in range(1, 401):
        o, d, rgba = ds.sample_random_rays(4096, "cuda")
        target = rgba[:, :3] * rgba[:, 3:4] + (1 - rgba[:, 3:4])
        loss = eng.train_step(o, d, target, 64)
        first = first if first is not None else loss.item()
        if step in (128, 256):
            assert 0.0 < eng.update_grid() < 1.0
    assert loss.item() < 0.2 * first, (first, loss.item())


def test_hash_representation_with_four_features_per_level(ops):
    """HashRepresentation(n_features_per_level=4): values and table gradient against the oracle's gather at F = 4 (an
    entry's features adjacent in ``params``), through two passes of the 2-feature kernels."""
    from src.embeddings import HashRepresentation
    torch.manual_seed(3)
    rep = HashRepresentation(n_levels=5, n_features_per_level=4, log2_hashmap_size=LOG2_T, base_resolution=BASE_RES, bound=BOUND).cuda()
    assert rep.out_dim == 20 and rep.encoding.params.numel() == rep.levels.entries * 4
    with torch.no_grad():
        rep.encoding.params.uniform_(-0.5, 0.5)
    g = torch.Generator().manual_seed(8)
    pts = (torch.rand(333, 3, generator=g) - 0.5) * 2 * BOUND * 1.05
    w = torch.randn(333, 20, generator=g)
    feat = rep(pts.cuda())
    (feat * w.cuda()).sum().backward()
    lv = O.hash_grid_levels(5, LOG2_T, BASE_RES, 1.5)
    table = rep.encoding.params.detach().cpu().view(-1, 4).clone().requires_grad_(True)
    ref = O.hash_encode(lv, table, O.hash_normalise(pts, BOUND))
    (ref * w).sum().backward()
    np.testing.assert_allclose(feat.detach().cpu().numpy(), ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(rep.encoding.params.grad.cpu().view(-1, 4).numpy(), table.grad.numpy(), rtol=1e-4, atol=1e-6)
    with pytest.raises(NotImplementedError):
        rep.table()


@pytest.mark.parametrize("case,change,line", [
    ("engine", {}, ">>> Part 2 Instant on the fused HIP shape engine ("),
    ("features4", {"n_features_per_level": 4},
     ">>> Part 2 Instant shape engine not used: n_features_per_level=4 (compiled: 2); training on the module path"),
    ("hidden16", {"hidden_dim": 16},
     ">>> Part 2 Instant shape engine not used: hidden_dim=16 (compiled: 32, 64, 128); training on the module path")])
def test_run_py_cli_small_shape(tmp_path, case, change, line):
    """`run.py` with the small example config and `engine: true`: the compiled shape trains on the shape engine; a shape that is
    not compiled prints the reason and trains on the module path; all evaluate.
    features4: the module path reads 4 features per level through two passes of the 2-feature hash kernels
    (HashRepresentation), so the refusal is the engine's alone; hidden16: the same at a hidden width that is not compiled."""
    import subprocess
    import sys
    from src.dataset import write_synthetic_scene
    root = write_synthetic_scene(str(tmp_path / "scene"), n_train=6, n_test=1, size=32)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2_instant_small.yaml.example")))
    cfg.update(train_iters=40, batch_size=1024, log_every=10, save_every=0, val_every=40, downscale=1, n_samples=48, render_n_samples=48,
               grid_resolution=32, grid_warmup_iters=16, log2_hashmap_size=14, log_dir=str(tmp_path / "out"), engine=True, **change)
    cfg_path = tmp_path / "part2_instant_small.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run.py"), "--config", str(cfg_path), "--data_dir", root, "--render_n", "1"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Test PSNR" in r.stdout
    assert line in r.stdout
