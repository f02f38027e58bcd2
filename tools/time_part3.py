"""Step time of Part 3 with a hash-grid canonical field at configs/part3_instant.yaml.example (8192 rays x 128 samples,
occupancy grid at ~12 % active, 2^19-entry canonical table): part3.Part3InstantEngine (fused chains) against the module path
(NeuralField + render_rays + part3_regularisers + torch.optim.AdamW + clip_grad_norm_) on the same batch, probes included.
    python tools/time_part3.py [--steps N] [--engine-only]"""
import argparse, os, sys, time
import torch, yaml
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from src.core import NeuralField
from src.renderer import DensityGrid, render_rays
from project_nerf_amd.dynamic import part3_regularisers
from project_nerf_amd.part3 import Part3InstantEngine, probe_draws

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--engine-only", action="store_true", help="skip the module path (profiler runs of the engine's kernels)")
args = ap.parse_args()
dev = "cuda"
cfg = yaml.safe_load(open(os.path.join(os.path.dirname(__file__), "..", "configs", "part3_instant.yaml.example")))
torch.manual_seed(0)
model = NeuralField(cfg).to(dev)
R, S = cfg["batch_size"], cfg["n_samples"]
o = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1) * 4.03
d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, device=dev), dim=-1)
t = torch.rand(R, 1, device=dev)
target = torch.rand(R, 3, device=dev)
occupied = torch.rand(cfg["grid_resolution"], cfg["grid_resolution"], cfg["grid_resolution"], device=dev) < 0.12


def timed(fn, n):
    for _ in range(3):
        fn(300)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(301 + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


eng = Part3InstantEngine(cfg, device=dev, seed=0)
eng.load_from_model(model)
eng.binary_grid = occupied
ms_eng = timed(lambda step: eng.train_step(o, d, target, t, S, probes=probe_draws(cfg, step, dev)), args.steps)
n_active = int(eng.prepare_batch(o, d, S)[0].get()[2].shape[0])
if args.engine_only:
    print(f"part3 instant, {R} rays x {S} samples, {n_active} active samples: engine {ms_eng:.3f} ms/step")
    sys.exit(0)

grid = DensityGrid(cfg["grid_resolution"], cfg["scene_bound"], cfg["grid_threshold"]).to(dev)
grid.binary_grid = occupied
opt = torch.optim.AdamW(model.parameters(), lr=cfg["learning_rate"], weight_decay=cfg["weight_decay"])


def module_step(step):
    pred, _, _, extras = render_rays(model, o, d, cfg["near"], cfg["far"], S, True, density_grid=grid, times=t, bg_color=eng.bg)
    loss = torch.nn.functional.mse_loss(pred, target) + sum(part3_regularisers(model, cfg, step, extras["mean_delta_x"]).values())
    opt.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    opt.step()


ms_mod = timed(module_step, args.steps)
print(f"part3 instant, {R} rays x {S} samples, {n_active} active samples: engine {ms_eng:.3f} ms/step, module path {ms_mod:.3f} ms/step "
      f"({ms_mod / ms_eng:.2f}x)")
