"""Part 1 fused engine (project-nerf_amd/part1.py, csrc/p1fit.hip) on the GPU: forward against the reference's own output and
the fp32 module, pixel resolution of the raw coordinate columns, loss and gradients against fp32 autograd, the Adam step,
run-to-run bits.  Every figure is printed before its assert (pytest -s shows them).

The bounds beside the asserts are 2x the largest value measured on an MI355X over the cases of this file (figures below).

The sharp references are written here in float64 with the engine's rounding points ("matched"): the raw pair as hi + lo bf16, the
sine / cosine columns from the fp32 ops.fourier_encode output rounded to bf16, weights rounded to bf16, every h rounded to bf16
after its relu, float64 sums; its gradients are float64 autograd, straight through the roundings.  What is left against it is
fp32 accumulation order, the bf16 images of dz / d_pre in the backward and rare 1-ulp bf16 flips.  Against fp32 autograd of the
module the hidden-layer gradients differ by up to 12 % in relative L2: relu masks flip where a pre-activation lies within the
bf16 operand error of zero (a fraction f of flipped units costs about sqrt(f)); the matched test prints that fraction.

Sample counts sit around the wave's 32 samples, the workgroup tile of 256 and the weight-gradient chunk of 1024."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from project_nerf_amd import ops, part1
from project_nerf_amd.core import NeuralField

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g12_part1.npz")
HALF_LEVEL = 1 / 510                      # half an 8-bit level of the saved PNG

# measured on an MI355X, maximum over the cases of this file -> asserted at 2x
FWD_GOLDEN_MAXABS = 2 * 1.318e-4          # predict vs the reference's fp32 rgb, g12 weights: 1.318e-4 = 0.07 of 1/510
FWD_MODULE_MAXABS = 2 * 4.200e-4          # predict vs the fp32 module: 2.8e-5 (256 x 8, L 15) .. 4.2e-4 (64 x 1, L 0); 400-pixel row 1.1e-4
# per-tensor relative L2 vs fp32 autograd of the module, n >= 255: worst tensor per configuration
#   (64,3,15) 0.046-0.117   (128,2,4) 0.039-0.053   (64,1,0) 0.004-0.009   (256,3,10) 0.078-0.082   (256,8,15) 0.092-0.102
#   (128,3,PE off) 0.016-0.066;  output layer alone 0.0009-0.007;  every tensor at n = 1: <= 0.005.  DESIGN 4.8 records 0.04.
GRAD_REL_L2 = 2 * 0.1169
LOSS_REL = 2 * 1.25e-4                    # loss vs the module's: 1.24e-4

SWEEP = (1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2 * 1024 + 7)
CONFIGS = {                               # (H, layers, L, PE): sample counts
    (64, 3, 15, True): SWEEP, (128, 2, 4, True): SWEEP,
    (64, 1, 0, True): (257, 1025), (256, 3, 10, True): (257, 1025), (256, 8, 15, True): (257, 1025), (128, 3, 7, False): (257, 1025),
}
CASES = [(c, n) for c, ns in CONFIGS.items() for n in ns]


def make_cfg(H, layers, L, pe):
    return {"mode": "part1_fourier", "use_positional_encoding": pe, "L_embed": L, "hidden_dim": H, "num_layers": layers, "output_dim": 3}


_MODELS = {}


def model_for(key):
    """one fp32 module per configuration (g12's weights for the golden configuration), shared and never modified"""
    if key not in _MODELS:
        torch.manual_seed(sum(key))
        model = NeuralField(make_cfg(*key))
        if key == (64, 3, 15, True):
            g = np.load(GOLDEN)
            model.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")})
        _MODELS[key] = model.cuda().requires_grad_(False)
    return _MODELS[key]


def engine_for(key, **kw):
    eng = part1.Part1Engine(make_cfg(*key), device="cuda", **kw)
    eng.load_from_model(model_for(key))
    return eng


def batch(n, seed=0, N=None):
    g = torch.Generator().manual_seed(seed + n)
    N = N or n
    return torch.rand(N, 2, generator=g).cuda(), torch.rand(N, 3, generator=g).cuda(), g


def test_forward_matches_the_reference_output():
    g = np.load(GOLDEN)
    eng = engine_for((64, 3, 15, True))
    y = eng.predict(torch.from_numpy(g["coords"]).cuda()).cpu().numpy()
    err = float(np.abs(y - g["rgb"]).max())
    print(f"forward vs reference rgb (g12): max-abs {err:.3e} = {err / HALF_LEVEL:.2f} of 1/510")
    assert err <= FWD_GOLDEN_MAXABS


@pytest.mark.parametrize("key,n", CASES)
def test_forward_matches_the_module(key, n):
    coords, _, _ = batch(n)
    y = engine_for(key).predict(coords)
    with torch.no_grad():
        ref = model_for(key)(coords)
    err = float((y - ref).abs().max())
    print(f"forward vs fp32 module {key} n={n}: max-abs {err:.3e}")
    assert y.shape == (n, 3) and err <= FWD_MODULE_MAXABS


def test_raw_coordinates_keep_pixel_resolution():
    key = (128, 3, 7, False)
    coords = torch.stack([torch.linspace(0, 1, 400), torch.full((400,), 0.37)], -1).cuda()
    y = engine_for(key).predict(coords)
    with torch.no_grad():
        ref = model_for(key)(coords)
    err = float((y - ref).abs().max())
    print(f"400-pixel row, PE off: max-abs vs module {err:.3e}")
    assert err <= FWD_MODULE_MAXABS
    distinct = lambda t: (t[:, None, :] != t[None, :, :]).any(-1)
    both = distinct(ref) & ~distinct(y)
    print(f"pairs distinct in the module but equal in the engine: {int(both.sum())}")
    assert not both.any()


@pytest.mark.parametrize("key,n", CASES)
def test_loss_and_gradients_match_fp32_autograd(key, n):
    N = 3 * n + 5
    coords, target, g = batch(n, seed=1, N=N)
    idx = torch.randint(0, N, (n,), generator=g).cuda() if n > 1 else None          # with repeats
    if idx is None:
        coords, target = coords[:1].contiguous(), target[:1].contiguous()
    eng = engine_for(key)
    loss = float(eng.compute_gradients(coords, target, idx))
    model = model_for(key)
    params = dict(model.named_parameters())
    sel = slice(None) if idx is None else idx
    with torch.enable_grad():
        for p in params.values():
            p.requires_grad_(True)
        ref_loss = torch.nn.functional.mse_loss(model(coords[sel]), target[sel])
        grads = torch.autograd.grad(ref_loss, list(params.values()))
        for p in params.values():
            p.requires_grad_(False)
    print(f"loss {key} n={n}: engine {loss:.6f} module {float(ref_loss):.6f}")
    assert abs(loss - float(ref_loss)) <= LOSS_REL * float(ref_loss)
    got = part1.unflatten(eng.cfg, eng.grads)
    for (name, _), ref in zip(params.items(), grads):
        rel = float((got[name] - ref).norm() / ref.norm().clamp_min(1e-30))
        print(f"  {name}: rel-L2 {rel:.3e}")
        if n >= 255:          # fp32 masks differ from the engine's (module docstring): with a handful of samples one flip is the whole
                              # error; every n is asserted per tensor against the matched reference below
            assert rel <= GRAD_REL_L2, name


@pytest.mark.parametrize("key", [(64, 3, 15, True), (256, 3, 10, True)])
def test_zero_residual_gives_zero_loss_and_gradients(key):
    coords, _, _ = batch(1025, seed=2)
    eng = engine_for(key)
    loss = eng.compute_gradients(coords, eng.predict(coords))
    assert float(loss) == 0.0 and not eng.grads.any()


def test_train_step_is_adam_on_the_engines_gradient():
    key = (128, 2, 4, True)
    coords, target, _ = batch(1025, seed=3)
    eng = engine_for(key, lr=1e-2)
    before, y0 = eng.params.clone(), eng.predict(coords)
    eng.train_step(coords, target)
    p = before.clone().requires_grad_(True)
    p.grad = eng.grads.clone()
    torch.optim.Adam([p], lr=1e-2).step()
    err = float((eng.params - p.detach()).abs().max())
    print(f"one step vs torch.optim.Adam on the same gradient: max-abs {err:.3e}")
    assert err <= 1e-7 and eng.step_count == 1        # measured 1.5e-8; parameters and steps of ~1e-2 in fp32 (ulp 1e-9 .. 6e-8)
    assert not torch.equal(eng.predict(coords), y0)   # the fragment images follow the new weights
    twin = part1.Part1Engine(eng.cfg, params=eng.params, device="cuda")
    assert torch.equal(twin.predict(coords), eng.predict(coords))


def test_two_runs_give_the_same_bits():
    key, n = (128, 2, 4, True), 2 * 1024 + 7
    coords, target, g = batch(n, seed=4)
    idx = [torch.randint(0, n, (n,), generator=g).cuda() for _ in range(5)]
    runs = []
    for _ in range(2):
        eng = part1.Part1Engine(make_cfg(*key), device="cuda", seed=7)
        losses = [float(eng.train_step(coords, target, i)) for i in idx]
        runs.append((eng.params.clone(), losses))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


# ---------------------------------------------------------------------------------------------- matched float64 reference
# measured on an MI355X, maximum over CASES -> asserted at 4x.  No element is excluded (the issue allows up to 1 %).
FWD_MATCHED_MAXABS = 4 * 8.634e-5         # 8.6e-5 at (128,2,4) n = 256; a third of the bound against the reference's output (2.6e-4)
# per-tensor relative L2 against float64 autograd of the matched chain, worst tensor of a case: 0.06 %-0.6 % in 29 of 31 cases,
# 0.89 % at (256,8,15) n = 257, 1.46 % at (64,3,15) n = 257; every n of the sweep is asserted, n = 1, 31, 32, 33 included.  The relu
# masks of the fp32 chain differ from the matched ones in 0.02 %-0.15 % of the units per layer (printed per case): over 3 layers
# about 0.3 % of the units, sqrt -> 5 %, the size of the figures against fp32 autograd above.
GRAD_MATCHED_REL_L2 = 4 * 1.459e-2
LOSS_MATCHED_REL = 4 * 1.26e-6            # 1.26e-6


def _st_bf16(x):
    """bf16 rounding of a float64 tensor, straight-through for autograd"""
    return x + (x.detach().float().bfloat16().double() - x.detach())


def _matched_forward(key, W, coords):
    """(y, [h_1..h_last]) in float64 with the engine's rounding points; coords: fp32 on the GPU"""
    H, layers, L, pe = key
    L = L if pe else 0
    x = coords.cpu()
    hi = x.bfloat16().float()
    h = hi.double() + (x - hi).bfloat16().double()
    if L > 0:
        h = torch.cat([h, ops.fourier_encode(coords, L).cpu()[:, 2:].bfloat16().double()], 1)
    hs = []
    for i in range(layers):
        h = _st_bf16(torch.relu(h @ _st_bf16(W[f"decoder.net.{2 * i}.weight"]).T + W[f"decoder.net.{2 * i}.bias"]))
        hs.append(h)
    return torch.sigmoid(h @ _st_bf16(W[f"decoder.net.{2 * layers}.weight"]).T + W[f"decoder.net.{2 * layers}.bias"]), hs


_MATCHED = {}


def matched_case(key, n):
    """one batch per (configuration, n), drawn with repeats, with the matched forward, loss and gradients: computed once"""
    if (key, n) not in _MATCHED:
        N = 3 * n + 5
        coords, target, g = batch(n, seed=5, N=N)
        idx = torch.randint(0, N, (n,), generator=g).cuda()
        W = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model_for(key).named_parameters()}
        with torch.enable_grad():
            y, hs = _matched_forward(key, W, coords[idx].contiguous())
            loss = ((y - target[idx].cpu().double()) ** 2).mean()
            grads = dict(zip(W, torch.autograd.grad(loss, list(W.values()))))
        # fp32 chain on the same inputs: how many relu masks differ from the matched ones
        with torch.no_grad():
            model = model_for(key)
            h32, flips = model.representation(coords[idx].contiguous()), []
            for i, hm in enumerate(hs):
                lin = model.decoder.net[2 * i]
                h32 = torch.relu(lin(h32))
                flips.append(float(((h32.cpu() > 0) != (hm > 0)).double().mean()))
        _MATCHED[(key, n)] = dict(coords=coords, target=target, idx=idx, y=y.detach(), loss=float(loss), grads=grads, flips=flips)
    return _MATCHED[(key, n)]


@pytest.mark.parametrize("key,n", CASES)
def test_forward_matches_the_matched_float64_chain(key, n):
    c = matched_case(key, n)
    y = engine_for(key).predict(c["coords"][c["idx"]].contiguous()).cpu().double()
    err = float((y - c["y"]).abs().max())
    print(f"forward vs matched float64 {key} n={n}: max-abs {err:.3e} (no element excluded)")
    assert err <= FWD_MATCHED_MAXABS


@pytest.mark.parametrize("key,n", CASES)
def test_gradients_match_matched_float64_autograd(key, n):
    c = matched_case(key, n)
    eng = engine_for(key)
    loss = float(eng.compute_gradients(c["coords"], c["target"], c["idx"]))
    print(f"matched {key} n={n}: loss engine {loss:.7f} matched {c['loss']:.7f}; masks differing from the fp32 chain per layer: "
          + " ".join(f"{f:.2e}" for f in c["flips"]))
    assert abs(loss - c["loss"]) <= LOSS_MATCHED_REL * c["loss"]
    got = part1.unflatten(eng.cfg, eng.grads.cpu().double())
    for name, ref in c["grads"].items():
        rel = float((got[name] - ref).norm() / ref.norm().clamp_min(1e-300))
        print(f"  {name}: rel-L2 vs matched {rel:.3e}")
        assert rel <= GRAD_MATCHED_REL_L2, name


# ---------------------------------------------------------------------------------------------- convergence
# measured: module path 34.601 / 35.396 / 35.149 dB at torch seeds 0 / 1 / 2 -> spread 0.795 dB; engine from seed 0's init 34.579 dB
PSNR_DELTA = 0.795


def _fit(key, seed, engine):
    side = 48
    coords = torch.stack(torch.meshgrid(torch.linspace(0, 1, side), torch.linspace(0, 1, side), indexing="ij"), -1).reshape(-1, 2).cuda()
    img = (0.5 + 0.5 * torch.sin(coords * 12).repeat(1, 2)[:, :3]).contiguous()       # the image of test_gpu_surface.py:197
    torch.manual_seed(seed)
    model = NeuralField(make_cfg(*key)).cuda()
    if engine:
        eng = part1.Part1Engine(make_cfg(*key), device="cuda", lr=1e-3)
        eng.load_from_model(model)
        losses = [eng.train_step(coords, img) for _ in range(300)]
        final = torch.nn.functional.mse_loss(eng.predict(coords), img)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        losses = []
        for _ in range(300):
            loss = torch.nn.functional.mse_loss(model(coords), img)
            opt.zero_grad(); loss.backward(); opt.step()
            losses.append(loss.detach())
        with torch.no_grad():
            final = torch.nn.functional.mse_loss(model(coords), img)
    return float(losses[0]), float(losses[-1]), -10 * float(torch.log10(final))


def test_converges_like_the_module_path():
    key = (64, 2, 6, True)
    module = [_fit(key, seed, False)[2] for seed in (0, 1, 2)]
    first, last, psnr = _fit(key, 0, True)
    print(f"300 full-image steps, 48x48: engine loss {first:.5f} -> {last:.5f}, PSNR {psnr:.3f} dB; module path seeds 0,1,2: "
          + " ".join(f"{p:.3f}" for p in module) + f" dB (spread {max(module) - min(module):.3f})")
    assert last < first
    assert psnr >= module[0] - PSNR_DELTA     # same init as the module path's seed 0


# ---------------------------------------------------------------------------------------------- command line
def _run_cli(tmp_path, hidden):
    Image = pytest.importorskip("PIL.Image")
    import yaml
    rng = np.random.default_rng(0)
    png = tmp_path / "tiny.png"
    Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(png)
    cfg = dict(make_cfg(hidden, 2, 4, True), engine=True, epochs=20, log_every=10, learning_rate=1e-3, batch_size=None, image_size=32,
               log_dir=str(tmp_path / f"out{hidden}"))
    (tmp_path / f"cfg{hidden}.yaml").write_text(yaml.safe_dump(cfg))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "run.py", "--config", str(tmp_path / f"cfg{hidden}.yaml"), "--image", str(png)],
                       cwd=root, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = tmp_path / f"out{hidden}" / "part1" / "tiny"
    assert (out / "final.png").exists() and "Final PSNR" in r.stdout and "Epoch 20/20" in r.stdout
    ckpt = torch.load(out / "model_final.pth", map_location="cpu")
    model = NeuralField(make_cfg(hidden, 2, 4, True))
    assert set(ckpt["model_state_dict"]) == set(model.state_dict())
    model.load_state_dict(ckpt["model_state_dict"])
    return r.stdout, model


def test_cli_trains_on_the_engine(tmp_path):
    out, model = _run_cli(tmp_path, 64)
    assert "fused HIP engine" in out and "engine not used" not in out
    torch.manual_seed(0)
    fresh = NeuralField(make_cfg(64, 2, 4, True))
    assert not torch.equal(model.state_dict()["decoder.net.0.weight"], fresh.state_dict()["decoder.net.0.weight"])


def test_cli_falls_back_for_an_unsupported_shape(tmp_path):
    out, _ = _run_cli(tmp_path, 1024)
    assert "engine not used: hidden_dim=1024 (compiled: 64, 128, 256)" in out and "fused HIP engine" not in out
