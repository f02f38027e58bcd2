"""Part 3 with the 8x256 canonical field on the fused HIP chains (pytest -m gpu): the canonical chain (csrc/p3canon.hip) and
part3_nerf.Part3NerfEngine against the module path (NeuralField('part3', canonical_type='nerf') + torch autograd, fp32 library
GEMMs), for the standard mode and for direct time conditioning."""
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
MODES = ["standard", "dtc"]


def cfg_of(mode, **kw):
    name = "part3.yaml.example" if mode == "standard" else "part3_dtc.yaml.example"
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg.update(dict(engine=True, use_coord_noise=False))
    cfg.update(kw)
    return cfg


def make_pair(cfg, seed=0):
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.part3_nerf import Part3NerfEngine
    torch.manual_seed(seed)
    model = NeuralField(cfg).cuda()
    with torch.no_grad():          # densities above zero at most points (an initial sigma_layer may cut them all off)
        dec = model.decoder_direct if getattr(model, "direct_time_conditioning", False) else model.decoder
        dec.sigma_layer.bias.fill_(0.5)
    if hasattr(model, "deform_net"):
        with torch.no_grad():      # a displacement of a few hundredths, not the near-zero initial output: d x_c reaches every layer
            model.deform_net.net[6].weight.normal_(0.0, 0.05)
            model.deform_net.net[6].bias.uniform_(-0.01, 0.01)
    eng = Part3NerfEngine(cfg, seed=seed)
    eng.load_from_model(model)
    return model, eng


def rays(R, seed):
    """rays through the scene, a dark target and per-ray times.  The dark target gives the loss gradient one sign per channel,
    as early in training on a real scene.  With per-ray random signs the sum over samples would be a random walk: the few ReLU
    masks the bf16 forward flips against fp32 (a fraction f of the entries) would then move it by sqrt(f) relative, ~5 % per
    layer, which says nothing about the kernels."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True) * 4.0311
    d = (torch.rand(R, 3, generator=g) - 0.5) * 1.2 - o
    d = d / d.norm(dim=-1, keepdim=True)
    return o.cuda(), d.cuda(), (0.1 * torch.rand(R, 3, generator=g)).cuda(), torch.rand(R, 1, generator=g).cuda()


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def blocked_image(ws, off, n_pad, width):
    """[n_pad, width] float64 of a blocked bf16 image in a workspace (mlp_chain.h::stash_block): per 32-sample wave tile and
    32-feature m-tile one 2-KiB block; bf16 element 128 (c >> 2) + 64 hi + 32 h + 8 (c & 3) + j holds sample c, feature
    16 hi + 8 (j >> 2) + 4 h + (j & 3)"""
    raw = ws[off:off + n_pad * width * 2].view(torch.bfloat16).double()
    raw = raw.view(n_pad // 32, width // 32, 8, 2, 2, 4, 2, 4)          # wt, m, c>>2, hi, h, c&3, j>>2, j&3
    return raw.permute(0, 2, 5, 1, 3, 6, 4, 7).reshape(n_pad, width)


def canon_dz(ws, n, layer):
    """dz of pts_layers.<layer> [n, 256] from the canonical workspace (p3canon.hip::layout: bytes per padded sample
    xenc 192 | h 4096 | feat 512 | hv 256 | denc 64 | mask 288 | dsmall 32 | dhv 256 | dfeat 512 | dh 8 x 512)"""
    n_pad = (n + 255) // 256 * 256
    off = n_pad * (192 + 4096 + 512 + 256 + 64 + 288 + 32 + 256 + 512) + layer * n_pad * 512
    return blocked_image(ws, off, n_pad, 256)[:n]


def dx_restated(eng, ws, x):
    """d x through code(x) in float64 from the engine's own bf16 dz0 / dz4 images and bf16 weights: d code = W0[:, :63]^T dz0 +
    W4[:, 256:319]^T dz4, then d [x | sin(2^b pi x) | cos(2^b pi x)] / dx"""
    n, C = x.shape[0], 63 + eng.tdim
    p = eng.canon_params.to(torch.bfloat16).double()
    w0 = p[:256 * C].view(256, C)[:, :63]
    w4_off = 256 * C + 256 + 3 * (256 * 256 + 256)
    w4 = p[w4_off:w4_off + 256 * (256 + C)].view(256, 256 + C)[:, 256:319]
    dcode = canon_dz(ws, n, 0) @ w0 + canon_dz(ws, n, 4) @ w4
    xd = x.double()
    out = dcode[:, :3].clone()
    for b in range(10):
        a = (2.0 ** b) * np.pi
        out += dcode[:, 3 + 6 * b:6 + 6 * b] * a * torch.cos(a * xd) - dcode[:, 6 + 6 * b:9 + 6 * b] * a * torch.sin(a * xd)
    return out


def points(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand(n, 3, generator=g) * 2 - 1) * 1.2).cuda()
    d = torch.randn(n, 3, generator=g)
    d = (d / d.norm(dim=-1, keepdim=True)).cuda()
    return x, d, torch.rand(n, generator=g).cuda()


@pytest.mark.parametrize("mode", MODES)
def test_field_equals_the_module_field(mode):
    """rgb, sigma (and delta_x) at points against NeuralField in eval mode: bf16 operands through ten layers against fp32"""
    model, eng = make_pair(cfg_of(mode))
    x, d, t = points(5000, 1)
    rgb, sigma, dx = eng.field(x, d, t)
    model.eval()
    with torch.no_grad():
        rgb_m, sigma_m, dx_m = model(x, d, t=t.view(-1, 1))
    # measured: rgb 1.9e-4 / 1.5e-4, sigma 1.3e-4 / 7.9e-5 relative, delta_x 5.3e-4 relative (standard / DTC)
    assert float((rgb - rgb_m).abs().max()) < 1e-3
    assert rel(sigma, sigma_m.view(-1)) < 1e-3, rel(sigma, sigma_m.view(-1))
    assert rel(dx, dx_m) < 3e-3 if mode == "standard" else float(dx.abs().max()) == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_canonical_chain_gradients_and_d_x_against_autograd(mode):
    """the canonical chain's backward alone: every weight gradient and (standard mode) d x_c through the Fourier code, against
    autograd through the module decoder and code"""
    from project_nerf_amd import part3_nerf as p3n
    cfg = cfg_of(mode)
    model, eng = make_pair(cfg)
    n = 40000
    x, d, t = points(n, 2)
    g = torch.Generator().manual_seed(3)
    # upstream gradients of one sign per channel and random size (see rays())
    g_rgb = ((0.5 + torch.rand(n, 3, generator=g)) * torch.tensor([1.0, -0.7, 0.4]) * 1e-3).cuda()
    g_sigma = ((0.5 + torch.rand(n, generator=g)) * -1e-3).cuda()
    ws = torch.empty(p3n.canon_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    rgb, sigma = p3n.canon_fwd(eng.packed_c, x, t, d, workspace=ws)
    rgb_i, sigma_i = p3n.canon_fwd(eng.packed_c, x, t, d)
    assert torch.equal(rgb, rgb_i) and torch.equal(sigma, sigma_i)         # training and inference forms agree bit for bit
    grads = torch.full((eng.n_canon,), float("nan"), device="cuda")        # written, not accumulated
    d_x = torch.ones(n, 3, device="cuda")
    p3n.canon_bwd(eng.packed_c, ws, eng.tdim, rgb, sigma, g_rgb, g_sigma, grads, x=x, d_x=d_x)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads).all())
    # autograd through the module's decoder and codes (fp32)
    dec = model.decoder_direct if mode == "dtc" else model.decoder
    enc_x = model.pos_encoder_direct if mode == "dtc" else model.canonical_repr
    xr = x.clone().requires_grad_(True)
    model.zero_grad()
    h = torch.cat([enc_x(xr), model.time_encoder(t.view(-1, 1).contiguous())], -1)
    rgb_m, sigma_m = dec(h, model.dir_representation(d))
    ((rgb_m * g_rgb).sum() + (sigma_m.view(-1) * g_sigma).sum()).backward()
    prefix = "decoder_direct." if mode == "dtc" else "decoder."
    named = dict(model.named_parameters())
    for key, _, off, shape in eng.slice_table():
        if key.startswith(prefix):
            err = rel(grads[off:off + int(np.prod(shape))].view(shape), named[key].grad)
            assert err <= 5e-2, (key, err)
    # d x on matched rounding: the float64 restatement from the engine's own bf16 dz images and weights pins the d-code kernel,
    # its layout and the chain rule (fp32 accumulation and the fp32 argument of the top band's sin: measured 4e-5)
    ref = dx_restated(eng, ws, x)
    err_m = rel(d_x - 1.0, ref)
    # against fp32 autograd, d x is a per-sample quantity: the ReLU masks the bf16 forward flips against fp32 along the chain
    # (a fraction f of the entries) change dz0 / dz4 of those samples outright, nothing averages them out as the sum over samples
    # does for the weight gradients, and the top band multiplies d code by 2^9 pi (measured: 7 %)
    err = rel(d_x - 1.0, xr.grad)
    print(f"[p3 canonical {mode}] d x rel {err:.4f} against fp32 autograd, {err_m:.2e} against the matched restatement")
    assert err_m <= 1e-3, err_m
    assert err <= 1e-1, err


def module_batch(model, cfg, o, d, target, t, S, seed, bg):
    """the module path's loss and gradients (render_rays with times, every sample, MSE + the displacement regulariser, torch
    autograd, fp32 library GEMMs); its jitter is torch.rand(R, S) after torch.manual_seed(seed)"""
    from project_nerf_amd.renderer import render_rays
    model.train()
    model.zero_grad()
    torch.manual_seed(seed)
    pred, _, _, extras = render_rays(model, o, d, 2.0, 6.0, S, True, density_grid=None, times=t, bg_color=bg)
    loss_rgb = torch.nn.functional.mse_loss(pred, target)
    (loss_rgb + torch.mean(extras["mean_delta_x"] ** 2) * float(cfg.get("deformation_reg_weight", 1e-4))).backward()
    return float(loss_rgb.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def module_batch_at_engine_xc(model, cfg, eng, o, d, target, t, S, u, bg):
    """the module path's loss and gradients with the canonical decoder evaluated at the ENGINE's x_c: delta_x takes the value of
    the engine's (fp16-operand) deformation forward while the gradient still flows through the module's own fp32 deformation MLP.
    The canonical code's top band is sin(2^9 pi x_c): the deformation forward's rounding of x_c (~1e-3 of max |delta_x|) moves its
    phase by ~1e-1 rad, so the plain module path evaluates d x_c at other points than the engine does."""
    from project_nerf_amd import ops
    from project_nerf_amd import part3 as p3
    R = o.shape[0]
    z, pts, dirs = ops.sample_rays(o, d, 2.0, 6.0, S, u=u, want_points=True)
    tt = t.expand(R, S).reshape(-1, 1).contiguous()
    with torch.no_grad():
        dx_e, _ = p3.deform_fwd(eng.packed_d, pts, tt.view(-1))
    model.train()
    model.zero_grad()
    dx_m = model.deform_net(model.pos_encoder_for_deform(pts), model.time_encoder(tt))
    dx = dx_e + (dx_m - dx_m.detach())
    rgb, sigma = model.decoder(torch.cat([model.canonical_repr((pts + dx).contiguous()), model.time_encoder(tt)], -1),
                               model.dir_representation(dirs))
    pred, _, _, mean_dx = ops.composite(rgb.view(R, S, 3).contiguous(), sigma.view(R, S).contiguous(), z, d, bg,
                                        dx.view(R, S, 3).contiguous())
    loss_rgb = torch.nn.functional.mse_loss(pred, target)
    (loss_rgb + torch.mean(mean_dx ** 2) * float(cfg.get("deformation_reg_weight", 1e-4))).backward()
    return float(loss_rgb.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def engine_grads(eng):
    return {key: eng.g_net[off:off + int(np.prod(shape))].view(shape).clone() for key, _, off, shape in eng.slice_table()}


@pytest.mark.parametrize("mode", MODES)
def test_engine_batch_equals_module_path(mode):
    """One batch, same weights and depths: the loss within 2e-2 relative, every decoder gradient tensor within 5e-2 relative
    norm of the module path, the deformation MLP's as set out below"""
    cfg = cfg_of(mode)
    model, eng = make_pair(cfg)
    R, S = 1024, 64
    o, d, target, t = rays(R, 1)
    torch.manual_seed(2)
    u = torch.rand(R, S, device="cuda")                    # the draw render_rays makes after the same seed
    loss_e = float(eng.compute_gradients(o, d, target, t, S, u=u))
    torch.cuda.synchronize()
    loss_m, gm = module_batch(model, cfg, o, d, target, t, S, 2, eng.bg)
    print(f"[part3 nerf engine {mode}] loss {loss_e:.6f} vs {loss_m:.6f}")
    assert abs(loss_e - loss_m) <= 2e-2 * loss_m, (loss_e, loss_m)
    ge = engine_grads(eng)
    assert sorted(ge) == sorted(gm)                          # the same trained set (DTC: decoder_direct.* only)
    for key, ref in gm.items():
        if not key.startswith("deform_net."):
            err = rel(ge[key].reshape(ref.shape), ref)
            print(f"[part3 nerf engine {mode}] {key:40s} rel {err:.4f}")
            assert err <= 5e-2, (key, err)
    if mode == "dtc":
        return
    # The deformation MLP sees the loss only through d x_c.  The canonical code's top band is sin(2^9 pi x_c): the deformation
    # forward's fp16 rounding of delta_x (5e-4 relative, see test_field_equals_the_module_field) moves that phase by ~0.1 rad,
    # so the plain module path takes d x_c at other points than the engine (the two fp32 module paths at the two x_c differ
    # by 14-31 % in these tensors).  Compared instead: (1) the engine's deformation backward against fp32 autograd through the
    # module's deformation MLP, fed the d delta_x the engine consumed (regulariser + d x_c, pinned by the test above);
    # (2) the whole step against the module path evaluated at the engine's x_c (bf16 chain vs fp32 in d x_c, as above).
    from project_nerf_amd import ops
    z, pts, dirs = ops.sample_rays(o, d, 2.0, 6.0, S, u=u, want_points=True)
    tt = t.expand(R, S).reshape(-1, 1).contiguous()
    model.zero_grad()
    dx_m = model.deform_net(model.pos_encoder_for_deform(pts), model.time_encoder(tt))
    (dx_m * eng.last_d_dx).sum().backward()
    g_fed = {k: p.grad.detach().clone() for k, p in model.named_parameters() if k.startswith("deform_net.")}
    _, gx = module_batch_at_engine_xc(model, cfg, eng, o, d, target, t, S, u, eng.bg)
    for key, ref in g_fed.items():
        mine = ge[key].reshape(ref.shape)
        err_fed, err_xc = rel(mine, ref), rel(mine, gx[key])
        print(f"[part3 nerf engine {mode}] {key:40s} rel {err_fed:.4f} (same d delta_x), {err_xc:.4f} (module path at the engine's x_c)")
        assert err_fed <= 5e-2, (key, err_fed)
        assert err_xc <= 1.2e-1, (key, err_xc)        # measured 6.5-8.9 %: the d x_c of the bf16 chain against fp32


def test_dtc_leaves_the_unused_parameters_untouched():
    cfg = cfg_of("dtc")
    model, eng = make_pair(cfg)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    o, d, target, t = rays(512, 3)
    losses = [float(eng.train_step(o, d, target, t, 32)) for _ in range(4)]
    eng.copy_to_model(model)
    trained = {k for k, _, _, _ in eng.slice_table()}
    moved = [k for k, p in model.named_parameters() if k in trained and not torch.equal(p, before[k])]
    assert moved and all(np.isfinite(losses))
    for k, p in model.named_parameters():
        if k not in trained:
            assert torch.equal(p, before[k]), k


@pytest.mark.parametrize("mode", MODES)
def test_load_copy_round_trip_and_render(mode):
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.renderer import render_rays
    cfg = cfg_of(mode)
    model, eng = make_pair(cfg)
    torch.manual_seed(7)
    other = NeuralField(cfg).cuda()
    eng.copy_to_model(other)
    trained = {k for k, _, _, _ in eng.slice_table()}
    for k, p in model.named_parameters():
        if k in trained:
            assert torch.equal(p, dict(other.named_parameters())[k]), k
    o, d, _, _ = rays(2048, 4)
    t = torch.tensor([[0.37]], device="cuda")
    img = eng.render_image(o.view(32, 64, 3), d.view(32, 64, 3), t, 64)
    model.eval()
    with torch.no_grad():
        ref = render_rays(model, o, d, 2.0, 6.0, 64, False, density_grid=None, times=t.expand(2048, 1), bg_color=eng.bg)[0]
    err = float((img.view(-1, 3) - ref).abs().max())
    assert err < 2e-2, err


def _frames(n_frames, size):
    from src.dataset import look_at_pose, render_analytic_frame
    focal = 0.5 * size / np.tan(0.5 * 0.6911112070083618)
    poses = torch.stack([torch.tensor(look_at_pose(4.0311 * np.array([np.cos(k), np.sin(k), 0.5]) / np.sqrt(1.25)), dtype=torch.float32)
                         for k in range(n_frames)]).cuda()
    frames = torch.stack([render_analytic_frame(poses[k].cpu(), size, focal, 96) for k in range(n_frames)]).cuda()
    return frames, poses, focal


def _train(cfg, frames, poses, focal, steps, seed=0):
    from project_nerf_amd import ops
    from project_nerf_amd.core import NeuralField
    from project_nerf_amd.part3 import probe_draws
    from project_nerf_amd.part3_nerf import Part3NerfEngine
    torch.manual_seed(seed)
    eng = Part3NerfEngine(cfg, seed=seed)
    model = NeuralField(cfg).cuda()
    with torch.no_grad():          # a density above zero to start from (an initial sigma_layer may cut every sample off)
        (model.decoder_direct if eng.dtc else model.decoder).sigma_layer.bias.fill_(0.5)
    eng.load_from_model(model)
    n_frames, size = frames.shape[0], frames.shape[1]
    times = torch.linspace(0, 1, n_frames).cuda()
    g = torch.Generator("cuda").manual_seed(seed)
    R, S, losses = 1024, 32, []
    for step in range(1, steps + 1):
        idx = torch.randint(0, n_frames * size * size, (R,), device="cuda", generator=g)
        o, d, target, _ = ops.gather_batch(frames, poses, idx, focal, 1.0, bg=eng.bg)
        t = times[idx // (size * size)].view(R, 1)
        probes = None if eng.dtc else probe_draws(cfg, step, "cuda", generator=g)
        losses.append(float(eng.train_step(o, d, target, t, S, probes=probes)))
    return eng, losses


@pytest.mark.parametrize("mode", MODES)
def test_engine_trains_and_is_deterministic(mode):
    frames, poses, focal = _frames(6, 32)
    cfg = cfg_of(mode, learning_rate=1e-3, train_iters=100, grid_warmup_iters=8, use_coord_noise=True, coord_noise_std=1e-3,
                 time_noise_std=1e-2)
    a, la = _train(cfg, frames, poses, focal, 100)
    assert np.mean(la[-10:]) < 0.8 * np.mean(la[:10]), (la[:10], la[-10:])
    assert all(np.isfinite(la)) and bool(torch.isfinite(a.net).all())
    b, lb = _train(cfg, frames, poses, focal, 100)
    assert la == lb and torch.equal(a.net, b.net)


@pytest.mark.parametrize("mode", MODES)
def test_run_py_with_the_engine_trains_and_evaluates(tmp_path, mode):
    from PIL import Image
    from src.dataset import look_at_pose, render_analytic_frame
    root = str(tmp_path / "dyn")
    size = 24
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
    cfg = cfg_of(mode, train_iters=24, batch_size=512, log_every=8, val_every=24, downscale=1, n_samples=32, render_n_samples=32,
                 grid_warmup_iters=8, random_bg_start=16, log_dir=str(tmp_path / "out"))
    cfg_path = tmp_path / "part3.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run.py"), "--config", str(cfg_path), "--data_dir", root, "--render_n", "1"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "not compiled" not in r.stdout
    line = [ln for ln in r.stdout.splitlines() if "Test PSNR" in ln][-1]
    assert np.isfinite(float(line.split("Test PSNR:")[1].split("dB")[0])), line
    ckpt = torch.load(tmp_path / "out" / "dyn" / "best_model.pth", map_location="cpu")
    assert ("decoder_direct.pts_layers.0.weight" if mode == "dtc" else "deform_net.net.0.weight") in ckpt["model_state_dict"]


# ------------------------------------------------------------------ one chain body, two decoders
@pytest.fixture
def compiler_scheduled_family():
    """the vanilla decoder on its compiler-scheduled kernels (library option chain_legacy), restored afterwards"""
    from project_nerf_amd import _lib
    _lib.set_option("chain_legacy", 1)
    yield
    _lib.set_option("chain_legacy", 0)


def embed_vanilla_in_canonical(flat, tdim):
    """the vanilla decoder's parameter vector in the canonical layout for 63 + tdim code columns (p3canon_plan.h::layout): the time
    columns of pts_layers.0 and pts_layers.4 are zero, everything else is copied"""
    C, plain = 63 + tdim, 256 * 256 + 256
    w0 = torch.zeros(256, C)
    w0[:, :63] = flat[:256 * 63].view(256, 63)
    v4 = 256 * 63 + 256 + 3 * plain                        # pts_layers.4.weight [256, 319] in the vanilla vector
    w4 = torch.zeros(256, 256 + C)
    w4[:, :319] = flat[v4:v4 + 256 * 319].view(256, 319)
    return torch.cat([w0.reshape(-1), flat[256 * 63:v4], w4.reshape(-1), flat[v4 + 256 * 319:]])


@pytest.mark.parametrize("n", [1, 300, 70464])
def test_canonical_forward_equals_the_vanilla_forward_bit_for_bit(n, compiler_scheduled_family):
    """mlp_fwd_kernel (vanilla, compiler-scheduled) and p3c::fwd_kernel are two instances of one body (mlp_chain_body.h).  On a
    vanilla parameter vector embedded in the canonical layout they run the same MFMA sequence per m-tile from the same bias, k-step
    0 upward; the canonical chain's two extra k-steps multiply finite time codes by exact zeros, and column 63 has a zero weight
    in both packers: rgb and sigma are equal bit for bit, for any finite t, with and without the training images.
    n = 300: one full tile and a ragged one whose upper waves have no live sample; n = 70464: 276 tiles, more than the CU count,
    so some workgroups take a second pass across the ring's wrap-around."""
    from oracle import nerf_oracle as O
    from project_nerf_amd import ops
    from project_nerf_amd import part3_nerf as p3n
    params = O.nerf_init_params(seed=5)                                   # weights x 2.5: outputs that vary
    flat = torch.cat([(params[k] * 2.5 if k.endswith("weight") else params[k]).reshape(-1) for k, _ in O.nerf_param_shapes()])
    x, d, _ = points(n, 11)
    packed_v = ops.mlp_pack(flat.cuda())
    rgb_v, sigma_v = ops.mlp_fwd(packed_v, x, d, None)
    stash = torch.empty(max(ops.mlp_stash_bytes(n), 256), dtype=torch.uint8, device="cuda")
    rgb_vt, sigma_vt = ops.mlp_fwd(packed_v, x, d, None, stash=stash)
    assert torch.equal(rgb_v, rgb_vt) and torch.equal(sigma_v, sigma_vt)
    assert n == 1 or float(rgb_v.std()) > 0.0                             # not a comparison of constants
    g = torch.Generator().manual_seed(12)
    t = ((torch.rand(n, generator=g) - 0.5) * 40.0).cuda()                # arbitrary finite times
    ws = torch.empty(p3n.canon_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    for tdim in (21, 13):
        canon = embed_vanilla_in_canonical(flat, tdim).cuda()
        packed = p3n.canon_pack(canon, tdim)
        for workspace in (None, ws):
            rgb_c, sigma_c = p3n.canon_fwd(packed, x, t, d, workspace=workspace)
            assert torch.equal(rgb_c, rgb_v) and torch.equal(sigma_c, sigma_v), (tdim, workspace is not None)
