"""Part 2 shape engine (project-nerf_amd/part2.py, csrc/p2chain.hip) on the GPU: forward against the reference's own output (g16,
g4), the fp32 module and the matched float64 restatement; gradients against float64 autograd of the matched restatement, fp32
autograd of the module and g16; a whole step against render_rays + MSE + autograd; Adam, repack, run-to-run bits, dead density,
round trips, render_image, convergence.  Every figure is printed before its assert (pytest -s shows them).

The bounds beside the asserts are 2x the largest value measured on an MI355X over the cases of this file (figures in the
comments).  The matched reference (tests/test_part2_engine_layout.py::decoder64, pinned to g16 on the CPU) has the chain's rounding
points: bf16 codes (from the fp32 ops.fourier_encode output), bf16 weights, every hidden activation rounded after its relu, the
feature vector rounded, float64 sums; its gradients are float64 autograd straight through the roundings.  What is left against it
is fp32 accumulation order, the bf16 gradient images of the backward and rare 1-ulp bf16 flips.

Shapes are (hidden_dim, num_layers, skip_layer, view_dim, L_embed, L_embed_dir); skip_layer == num_layers: no skip.  Sample counts
sit around the wave's 32 samples, the workgroup tile (256; 128 at hidden 256) and the weight-gradient chunk of 1024."""
import os

import numpy as np
import pytest
import torch

from project_nerf_amd import dataset, ops, part2
from project_nerf_amd.core import NeuralField
from project_nerf_amd.renderer import render_image, render_rays
from test_part2_engine_layout import decoder64, golden_case, make_cfg

pytestmark = pytest.mark.gpu
G4 = os.path.join(os.path.dirname(__file__), "golden", "g4_decoder.npz")

# measured on an MI355X, maximum over the cases of this file -> asserted at 2x
FWD_GOLDEN_RGB = 2 * 2.046e-4             # vs the reference's own fp32 output: g16 a 2.0e-4, g16 b and g4 below it
FWD_GOLDEN_SIGMA = 2 * 7.089e-4           # relative to max(1, |sigma|): g16 a
FWD_MODULE_RGB = 2 * 2.037e-4             # vs the fp32 module: (128, 4, 2, 64, 10, 4) n = 1023
FWD_MODULE_SIGMA = 2 * 1.361e-3           # (64, 2, 1, 128, 1, 0) n = 1025
FWD_MATCHED_RGB = 2 * 5.218e-5            # vs the matched float64 chain, no element excluded: (256, 8, 7, 128, 10, 4) n = 1025
FWD_MATCHED_SIGMA = 2 * 1.189e-4          # (128, 4, 2, 64, 10, 4) n = 1023
# per-tensor relative L2 vs float64 autograd of the matched chain, every n of the sweep: worst tensor 0.49 % (pts_layers.0.weight,
# (256, 8, 7, 128, 10, 4) n = 129); per tensor kind 0.08 %-0.49 %.  (With zero-mean cotangents the one-element sigma_layer.bias
# reached 4.8 % at n = 1024 by cancellation: see points().)
GRAD_MATCHED_REL_L2 = 2 * 4.933e-3
# vs fp32 autograd of the module (n >= 255) and g16's stored gradients: relu masks flip where a pre-activation lies within the
# bf16 operand error of zero (0.05-0.15 % of the units per layer, printed): worst 11.1 % (pts_layers.0.weight, (128, 4, 2, 64, 10, 4)
# n = 1025); the heads 0.2-5 %
GRAD_MODULE_REL_L2 = 2 * 0.1111
# whole step vs render_rays + MSE + autograd on the fp32 module, 64 rays x 32, densities away from the relu threshold (step_model()):
# loss 6.2e-7 relative; per tensor 0.02-1.1 % on the colour branch, 1.0-7.1 % on the trunk and the sigma head (relu masks, as above; worst
# pts_layers.0.weight)
STEP_LOSS_REL = 2 * 6.165e-7
STEP_GRAD_REL_L2 = 2 * 7.080e-2
ADAM_MAXABS = 2 * 1.490e-8                # parameters and steps of ~1e-2 in fp32 (ulp 1e-9 .. 6e-8)
IMAGE_MAXABS = 2 * 1.751e-4

SWEEP = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2 * 1024 + 7)
GA, GB, DEFAULT = (64, 3, 1, 64, 4, 2), (128, 4, 4, 128, 10, 0), (256, 8, 4, 128, 10, 4)
CONFIGS = {GA: SWEEP, (128, 4, 2, 64, 10, 4): SWEEP, GB: (257, 1025), (64, 2, 1, 128, 1, 0): (257, 1025),
           (256, 8, 7, 128, 10, 4): (129, 1025), DEFAULT: (257, 1025)}
CASES = [(c, n) for c, ns in CONFIGS.items() for n in ns]


def sigma_err(got, ref):
    """largest |difference| relative to max(1, |reference|): densities span 0 .. tens"""
    return float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())


_MODELS = {}


def model_for(key):
    """one fp32 module per configuration (the goldens' weights for their shapes), shared and never modified"""
    if key not in _MODELS:
        torch.manual_seed(sum(key))
        model = NeuralField(make_cfg(*key))
        if key in (GA, GB):
            model.load_state_dict(golden_case("a" if key == GA else "b")["weights"], strict=False)
        elif key == DEFAULT:
            g = np.load(G4)
            model.load_state_dict({"decoder." + k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}, strict=False)
        else:
            with torch.no_grad():          # densities on both sides of zero
                model.decoder.sigma_layer.bias.fill_(0.02)
        _MODELS[key] = model.cuda().requires_grad_(False)
    return _MODELS[key]


def engine_for(key, **kw):
    eng = part2.Part2Engine(make_cfg(*key), device="cuda", **kw)
    eng.load_from_model(model_for(key))
    return eng


def points(n, seed=0):
    """points, unit directions and fixed cotangents d_rgb [n,3], d_sigma [n].  The cotangents have a non-zero mean: a bias
    gradient is a plain sum over the samples, and with zero-mean cotangents the one-element sum of sigma_layer.bias cancels to
    ~sqrt(n) out of n terms, so that its relative error measures the cancellation (sum |b| / |sum b|) and not the kernel -- seen
    with randn cotangents at (64, 3, 1, 64, 4, 2) n = 1024: 4.8 % on that tensor, every other tensor 0.3-0.6 %."""
    g = torch.Generator().manual_seed(seed + n)
    pts = (torch.rand(n, 3, generator=g) * 2 - 1) * 1.5
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return pts.cuda(), dirs.cuda(), (torch.randn(n, 3, generator=g) + 0.5).cuda(), (torch.randn(n, generator=g) + 1.0).cuda()


def codes(key, pts, dirs):
    L, Ld = key[4], key[5]
    return ops.fourier_encode(pts, L), (ops.fourier_encode(dirs, Ld) if Ld > 0 else dirs)


def module_forward(key, pts, dirs):
    """the fp32 module's layers (NeRFDecoder._layers: library GEMMs) on the HIP Fourier codes"""
    rgb, sigma = model_for(key).decoder._layers(*codes(key, pts, dirs))
    return rgb, sigma[:, 0]


def rays(R, seed=0):
    g = torch.Generator().manual_seed(100 + seed + R)
    o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 4.0
    d = torch.nn.functional.normalize(-o + 0.4 * torch.randn(R, 3, generator=g), dim=-1)       # unit length
    return o.cuda(), d.cuda(), torch.rand(R, 3, generator=g).cuda()


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("tag,key", [("a", GA), ("b", GB)])
def test_forward_matches_the_reference_output_g16(tag, key):
    c = golden_case(tag)
    eng = engine_for(key)
    for train in (False, True):
        rgb, sigma = eng.field(c["pts"].cuda(), c["dirs"].cuda(), train=train)
        e_rgb, e_sig = float((rgb.cpu() - c["rgb"]).abs().max()), sigma_err(sigma.cpu(), c["sigma"])
        print(f"FIG fwd_golden g16 {tag} train={train}: rgb max-abs {e_rgb:.3e} sigma {e_sig:.3e}")
        assert e_rgb <= FWD_GOLDEN_RGB and e_sig <= FWD_GOLDEN_SIGMA


def test_forward_matches_the_reference_output_g4_default_shape():
    g = np.load(G4)
    rgb, sigma = engine_for(DEFAULT).field(torch.from_numpy(g["pts"]).cuda(), torch.from_numpy(g["dirs"]).cuda())
    e_rgb = float((rgb.cpu() - torch.from_numpy(g["rgb"])).abs().max())
    e_sig = sigma_err(sigma.cpu(), torch.from_numpy(g["sigma"])[:, 0])
    print(f"FIG fwd_golden g4: rgb max-abs {e_rgb:.3e} sigma {e_sig:.3e}")
    assert e_rgb <= FWD_GOLDEN_RGB and e_sig <= FWD_GOLDEN_SIGMA


@pytest.mark.parametrize("key,n", CASES)
def test_forward_matches_the_module(key, n):
    pts, dirs, _, _ = points(n)
    rgb, sigma = engine_for(key).field(pts, dirs)
    with torch.no_grad():
        r_rgb, r_sigma = module_forward(key, pts, dirs)
    e_rgb, e_sig = float((rgb - r_rgb).abs().max()), sigma_err(sigma, r_sigma)
    print(f"FIG fwd_module {key} n={n}: rgb max-abs {e_rgb:.3e} sigma {e_sig:.3e}")
    assert rgb.shape == (n, 3) and sigma.shape == (n,) and e_rgb <= FWD_MODULE_RGB and e_sig <= FWD_MODULE_SIGMA


@pytest.mark.parametrize("key,n", [(GA, 2055), ((128, 4, 2, 64, 10, 4), 1025), ((256, 8, 7, 128, 10, 4), 129)])
def test_inference_and_training_forward_and_ray_mode_give_the_same_bits(key, n):
    pts, dirs, _, _ = points(n)
    eng = engine_for(key)
    a, b = eng.field(pts, dirs), eng.field(pts, dirs, train=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for S in (8, 32):
        o, d, _ = rays(max(n // S, 1))
        u = torch.rand(o.shape[0], S, device="cuda")
        z, p, v = ops.sample_rays(o, d, 2.0, 6.0, S, u=u, want_points=True)
        ray, ray_t, pt = eng.field_from_rays(o, d, z), eng.field_from_rays(o, d, z, train=True), eng.field(p, v)
        assert torch.equal(ray[0], pt[0]) and torch.equal(ray[1], pt[1]) and torch.equal(ray[0], ray_t[0]) and torch.equal(ray[1], ray_t[1])


# ---------------------------------------------------------------------------------------------- matched float64 reference
_MATCHED = {}


def matched_case(key, n):
    """one point set per (configuration, n) with the matched forward and the gradients of sum(rgb a) + sum(sigma b): computed once"""
    if (key, n) not in _MATCHED:
        pts, dirs, a, b = points(n, seed=5)
        x_enc, d_enc = (t.cpu() for t in codes(key, pts, dirs))
        W = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model_for(key).named_parameters()}
        with torch.enable_grad():
            rgb, sigma, hs = decoder64(key, W, x_enc, d_enc, rounded=True)
            grads = dict(zip(W, torch.autograd.grad((rgb * a.cpu().double()).sum() + (sigma * b.cpu().double()).sum(), list(W.values()))))
        # fp32 module on the same inputs: its gradients, and how many relu masks differ from the matched ones
        model = model_for(key)
        with torch.enable_grad():
            for p in model.parameters():
                p.requires_grad_(True)
            r_rgb, r_sigma = module_forward(key, pts, dirs)
            g32 = dict(zip(W, torch.autograd.grad((r_rgb * a).sum() + (r_sigma * b).sum(), list(model.parameters()))))
            for p in model.parameters():
                p.requires_grad_(False)
        with torch.no_grad():
            _, _, h32 = decoder64(key, {k: v.detach().float().double() for k, v in W.items()}, x_enc, d_enc, rounded=False)
            flips = [float(((u > 0) != (m > 0)).double().mean()) for u, m in zip(h32, hs)]
        _MATCHED[(key, n)] = dict(pts=pts, dirs=dirs, a=a, b=b, rgb=rgb.detach(), sigma=sigma.detach(), grads=grads, g32=g32, flips=flips)
    return _MATCHED[(key, n)]


@pytest.mark.parametrize("key,n", CASES)
def test_forward_matches_the_matched_float64_chain(key, n):
    c = matched_case(key, n)
    rgb, sigma = engine_for(key).field(c["pts"], c["dirs"])
    e_rgb, e_sig = float((rgb.cpu().double() - c["rgb"]).abs().max()), sigma_err(sigma.cpu().double(), c["sigma"])
    print(f"FIG fwd_matched {key} n={n}: rgb max-abs {e_rgb:.3e} sigma {e_sig:.3e} (no element excluded)")
    assert e_rgb <= FWD_MATCHED_RGB and e_sig <= FWD_MATCHED_SIGMA


def engine_grads(key, c):
    eng = engine_for(key)
    rgb, sigma = eng.field(c["pts"], c["dirs"], train=True)
    eng.backward(rgb, sigma, c["a"].contiguous(), c["b"].contiguous())
    return part2.unflatten(eng.cfg, eng.grads.cpu().double())


@pytest.mark.parametrize("key,n", CASES)
def test_gradients_match_matched_float64_autograd(key, n):
    c = matched_case(key, n)
    got = engine_grads(key, c)
    print(f"matched {key} n={n}: masks differing from the unrounded chain per layer: " + " ".join(f"{f:.2e}" for f in c["flips"]))
    for name, ref in c["grads"].items():
        rel = float((got[name] - ref).norm() / ref.norm().clamp_min(1e-300))
        print(f"FIG grad_matched {key} n={n} {name}: rel-L2 {rel:.3e}")
        assert rel <= GRAD_MATCHED_REL_L2, name


@pytest.mark.parametrize("key,n", CASES)
def test_gradients_match_fp32_autograd_of_the_module(key, n):
    c = matched_case(key, n)
    got = engine_grads(key, c)
    print(f"module {key} n={n}: flipped relu units per layer: " + " ".join(f"{f:.2e}" for f in c["flips"]))
    for name, ref in c["g32"].items():
        rel = float((got[name] - ref.cpu().double()).norm() / ref.norm().clamp_min(1e-30))
        print(f"FIG grad_module {key} n={n} {name}: rel-L2 {rel:.3e}")
        if n >= 255:          # below that the figure is reported only: fp32 masks differ from the engine's, and with a handful of
                              # samples one flip is the whole error; every n is asserted per tensor against the matched reference
            assert rel <= GRAD_MODULE_REL_L2, name


@pytest.mark.parametrize("tag,key", [("a", GA), ("b", GB)])
def test_gradients_match_the_reference_gradients_g16(tag, key):
    c = golden_case(tag)
    eng = engine_for(key)
    rgb, sigma = eng.field(c["pts"].cuda(), c["dirs"].cuda(), train=True)
    eng.backward(rgb, sigma, c["a"].cuda(), c["b"][:, 0].contiguous().cuda())
    got = part2.unflatten(eng.cfg, eng.grads.cpu())
    for name, ref in c["grads"].items():
        rel = float((got[name] - ref).norm() / ref.norm().clamp_min(1e-30))
        print(f"FIG grad_module g16 {tag} {name}: rel-L2 {rel:.3e}")
        assert rel <= GRAD_MODULE_REL_L2, name


# ---------------------------------------------------------------------------------------------- whole step
STEP_KEY = (128, 4, 2, 64, 10, 4)
_STEP_MODEL = []


def step_model():
    """The whole-step case needs densities away from the relu threshold.  The reference gives a ray's last sample the interval
    1e10, so its alpha is 1 if sigma > 0 and 0 if not, and at a random initialisation that sample carries the ray's colour weight
    (measured: 99.9 % of |d rgb|^2 sits on last samples).  With the sigma bias at 0.02, 79 % of the densities are exactly zero and
    ONE ray of the 64 had sigma_last = 3.0e-5 in the bf16 chain and 0 in the fp32 module: its colour moved by 0.51, the loss by
    0.2 % and the colour-branch gradients by 24-33 % -- all of it on that ray, while the same cotangents through the engine's
    backward agreed with the matched float64 chain to 0.4 %.  With the bias at 0.3 no density of either path is zero."""
    if not _STEP_MODEL:
        torch.manual_seed(sum(STEP_KEY))
        model = NeuralField(make_cfg(*STEP_KEY))
        with torch.no_grad():
            model.decoder.sigma_layer.bias.fill_(0.3)
        _STEP_MODEL.append(model.cuda().requires_grad_(False))
    return _STEP_MODEL[0]


def test_loss_and_gradients_of_a_whole_step():
    R, S = 64, 32
    o, d, target = rays(R)
    torch.manual_seed(5)
    u = torch.rand(R, S, device="cuda")
    z = ops.sample_rays(o, d, 2.0, 6.0, S, u=u)
    model = step_model()
    eng = part2.Part2Engine(make_cfg(*STEP_KEY), device="cuda")
    eng.load_from_model(model)
    loss = float(eng.compute_gradients(o, d, target, S, z=z))
    with torch.no_grad():
        s_mod, s_eng = model.field_from_rays(o, d, z)[1].view(R, S), eng.field_from_rays(o, d, z)[1].view(R, S)
    flips = int(((s_mod > 0) != (s_eng > 0)).sum())
    print(f"densities: module min {float(s_mod.min()):.3e}, engine min {float(s_eng.min()):.3e}, relu signs differing on {flips} samples")
    assert float(s_mod.min()) > 0 and float(s_eng.min()) > 0          # the case is conditioned as step_model() says
    with torch.enable_grad():
        for p in model.parameters():
            p.requires_grad_(True)
        torch.manual_seed(5)                 # render_rays draws the same jitter
        pred = render_rays(model, o, d, 2.0, 6.0, S, perturb=True, white_bkgd=True)[0]
        ref_loss = torch.nn.functional.mse_loss(pred, target)
        grads = torch.autograd.grad(ref_loss, list(model.parameters()))
        for p in model.parameters():
            p.requires_grad_(False)
    rel_loss = abs(loss - float(ref_loss)) / float(ref_loss)
    print(f"FIG step_loss: engine {loss:.9f} module {float(ref_loss):.9f} rel {rel_loss:.3e}")
    got = part2.unflatten(eng.cfg, eng.grads)
    rels = {name: float((got[name] - ref).norm() / ref.norm().clamp_min(1e-30)) for (name, _), ref in zip(model.named_parameters(), grads)}
    for name, rel in rels.items():
        print(f"FIG step_grad {name}: rel-L2 {rel:.3e}")
    assert rel_loss <= STEP_LOSS_REL
    for name, rel in rels.items():
        assert rel <= STEP_GRAD_REL_L2, name


def test_apply_gradients_is_adam_and_repacks():
    R, S = 64, 32
    o, d, target = rays(R, seed=1)
    eng = engine_for(STEP_KEY, lr=1e-2)
    before = eng.params.clone()
    eng.train_step(o, d, target, S, u=torch.rand(R, S, device="cuda"))
    p = before.clone().requires_grad_(True)
    p.grad = eng.grads.clone()
    torch.optim.Adam([p], lr=1e-2).step()
    err = float((eng.params - p.detach()).abs().max())
    print(f"FIG adam: max-abs {err:.3e}")
    assert err <= ADAM_MAXABS and eng.step_count == 1 and not torch.equal(eng.params, before)
    twin = part2.Part2Engine(eng.cfg, params=eng.params, device="cuda")           # a fresh pack of the new parameters
    assert torch.equal(twin.packed, eng.packed)


def test_two_runs_give_the_same_bits():
    R, S = 2 * 1024 // 32 + 3, 32             # 2144 samples: three chunks
    o, d, target = rays(R, seed=2)
    us = [torch.rand(R, S, device="cuda") for _ in range(3)]
    runs = []
    for _ in range(2):
        eng = part2.Part2Engine(make_cfg(*STEP_KEY), device="cuda", seed=7)
        losses, grads = [], []
        for u in us:
            losses.append(eng.train_step(o, d, target, S, u=u))
            grads.append(eng.grads.clone())
        runs.append((torch.stack(losses), torch.stack(grads), eng.params.clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert runs[0][1].abs().sum() > 0


def test_loss_slot_across_a_lap_of_the_ring():
    """RING + 1 gradient calls on the same inputs at the smallest compiled shape, 8 rays x 4 samples (one 32-sample wave tile):
    the loss is an ordered sum into a slot that is zero when handed out, so call RING (slot 0 again, after the lap's clear)
    gives the bits of call 0; and what was returned is a copy, so the tensors kept from calls 0 and 1 outlive that clear."""
    R, S = 8, 4
    o, d, target = rays(R, seed=4)
    u = torch.rand(R, S, device="cuda")
    eng = part2.Part2Engine(make_cfg(64, 2, 1, 64, 1, 0), device="cuda", seed=5)
    kept = [eng.compute_gradients(o, d, target, S, u=u) for _ in range(eng.RING + 1)]
    assert float(kept[0]) > 0.0 and torch.equal(kept[0], kept[eng.RING])
    assert torch.equal(kept[1], kept[0])          # slot 1 was cleared by the lap and not yet written again


def test_dead_density_gives_exactly_zero_gradients():
    R, S = 40, 32
    o, d, target = rays(R, seed=3)
    eng = engine_for(GA)
    with torch.no_grad():
        part2.unflatten(eng.cfg, eng.params)["decoder.sigma_layer.bias"].fill_(-10.0)
    eng.repack()
    before = eng.params.clone()
    loss = eng.train_step(o, d, target, S, u=torch.rand(R, S, device="cuda"))
    assert torch.isfinite(loss) and not eng.grads.any() and torch.isfinite(eng.params).all() and torch.equal(eng.params, before)


def test_round_trip_through_the_module():
    eng = part2.Part2Engine(make_cfg(*GA), device="cuda", seed=11)
    model = NeuralField(make_cfg(*GA)).cuda()
    eng.copy_to_model(model)
    flat = eng.params.clone()
    eng.params.zero_()
    eng.load_from_model(model)
    assert torch.equal(eng.params, flat)
    fresh = NeuralField(make_cfg(*GA))
    sd = eng.state_dict("decoder.")
    assert set(sd) == {k for k, _ in fresh.named_parameters()}
    fresh.load_state_dict(sd, strict=False)
    assert torch.equal(part2.flatten(eng.cfg, fresh.state_dict()), flat.cpu())


def test_render_image_matches_the_module():
    side, S = 24, 32
    o, d, _ = rays(side * side, seed=4)
    o, d = o.view(side, side, 3), d.view(side, side, 3)
    img = engine_for(STEP_KEY).render_image(o, d, S, chunk=100)           # ragged last chunk
    with torch.no_grad():
        ref = render_image(model_for(STEP_KEY), o, d, 2.0, 6.0, S, 100, True)
    err = float((img - ref).abs().max())
    print(f"FIG image: max-abs {err:.3e}")
    assert img.shape == (side, side, 3) and err <= IMAGE_MAXABS


# ---------------------------------------------------------------------------------------------- convergence
CONV_KEY, CONV_STEPS = (64, 4, 2, 64, 6, 2), 200


def _scene():
    size, focal = 32, 32 * 1.2
    rng = np.random.default_rng(0)
    os_, ds, cols = [], [], []
    for c2w in dataset.synthetic_poses(4, rng):
        rgba = dataset.render_analytic_frame(c2w, size, focal, n_samples=64)
        j, i = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
        d = torch.stack([(i - size * 0.5) / focal, -(j - size * 0.5) / focal, -torch.ones_like(i)], -1).reshape(-1, 3).float() @ c2w[:3, :3].T
        ds.append(d / d.norm(dim=-1, keepdim=True))
        os_.append(c2w[:3, 3].expand(size * size, 3))
        cols.append((rgba[..., :3] * rgba[..., 3:] + 1 - rgba[..., 3:]).reshape(-1, 3))
    return torch.cat(os_).cuda().contiguous(), torch.cat(ds).cuda().contiguous(), torch.cat(cols).cuda().contiguous()


def _fit(scene, seed, engine):
    o, d, col = scene
    S, B, lr = 32, 1024, 2e-3
    torch.manual_seed(seed)
    model = NeuralField(make_cfg(*CONV_KEY)).cuda()
    g = torch.Generator().manual_seed(99)
    batches = [torch.randint(0, o.shape[0], (B,), generator=g).cuda() for _ in range(CONV_STEPS)]
    if engine:
        eng = part2.Part2Engine(make_cfg(*CONV_KEY), device="cuda", lr=lr)
        eng.load_from_model(model)
        for idx in batches:
            eng.train_step(o[idx], d[idx], col[idx], S)
        pred = eng.render_image(o, d, S)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=lr)
        for idx in batches:
            loss = torch.nn.functional.mse_loss(render_rays(model, o[idx], d[idx], 2.0, 6.0, S, perturb=True, white_bkgd=True)[0], col[idx])
            opt.zero_grad(); loss.backward(); opt.step()
        with torch.no_grad():
            pred = render_image(model, o.view(-1, 32, 3), d.view(-1, 32, 3), 2.0, 6.0, S, 65536, True)
    return -10 * float(torch.log10(torch.nn.functional.mse_loss(pred.reshape(-1, 3), col)))


# measured: module path 16.957 / 18.278 / 19.388 dB at torch seeds 0 / 1 / 2 -> spread 2.430 dB; engine from seed 0's init 16.953 dB
def test_converges_like_the_module_path():
    scene = _scene()
    module = [_fit(scene, seed, False) for seed in (0, 1, 2)]
    psnr = _fit(scene, 0, True)
    spread = max(module) - min(module)
    print(f"FIG psnr: {CONV_STEPS} steps of 1024 rays x 32: engine {psnr:.3f} dB; module path seeds 0,1,2: "
          + " ".join(f"{p:.3f}" for p in module) + f" dB (spread {spread:.3f})")
    assert psnr >= module[0] - spread         # same init as the module path's seed 0
