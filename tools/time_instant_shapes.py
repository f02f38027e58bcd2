"""Step time of Part 2 Instant at non-default hash / tiny-MLP shapes: instant_shapes.InstantShapeEngine (fused HIP chain,
csrc/imlp_shapes.hip) against the module path (NeuralField + DensityGrid + render_rays + mse_loss + autograd + torch.optim.AdamW:
what run.py does without `engine: true`) in one process, same weights, same rays, after one occupancy update on an analytic
scene (a sphere of radius 1 occupied).  4096 and 16384 rays x 128 samples for (n_levels, hidden_dim, L_embed_dir) = (8, 32, 2),
(16, 32, 4), (12, 64, 4), (16, 128, 4); (16, 64, 4) against engine.InstantNgpEngine in its counted form instead of the module
path.  20 warm-up steps, interleaved windows of 30 steps, median of the windows.
    python tools/time_instant_shapes.py [--steps N] [--repeats R] [--engine-only] [--only L,H,Ld,rays]"""
import argparse, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from project_nerf_amd.core import NeuralField
from project_nerf_amd.engine import InstantNgpEngine
from project_nerf_amd.instant_shapes import InstantShapeEngine
from project_nerf_amd.renderer import DensityGrid, render_rays

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only", type=str, default=None, help="one case: L,H,Ld,rays (profiler runs)")
ap.add_argument("--engine-only", action="store_true", help="skip the other path (profiler runs of the engine's kernels)")
args = ap.parse_args()
dev, S, BOUND, RES = "cuda", 128, 1.5, 128
torch.manual_seed(0)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


ax = torch.linspace(-BOUND, BOUND, RES)
gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
occupied = ((gx ** 2 + gy ** 2 + gz ** 2) < 1.0).to(dev)
only = tuple(int(v) for v in args.only.split(",")) if args.only else None
for L, H, Ld in ((8, 32, 2), (16, 32, 4), (12, 64, 4), (16, 128, 4), (16, 64, 4)):
    if only and only[:3] != (L, H, Ld):
        continue
    cfg = {"mode": "part2_instant", "n_levels": L, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
           "per_level_scale": 1.5, "scene_bound": BOUND, "hidden_dim": H, "L_embed_dir": Ld, "grid_resolution": RES,
           "speculative_hash_backward": False}
    eng = InstantShapeEngine(cfg, device=dev)
    eng.binary_grid = occupied.clone()
    default = (L, H, Ld) == (16, 64, 4)
    if default:
        other_name, other = "InstantNgpEngine (counted)", InstantNgpEngine(cfg, device=dev)
        other.table.copy_(eng.table)
        other.net.copy_(eng.net)
        other._pack()
        other.binary_grid = occupied.clone()
    else:
        other_name = "module path"
        model = NeuralField(cfg).to(dev)
        with torch.no_grad():
            model.representation.encoding.params.copy_(eng.table)
            model.decoder.sigma_net.params.copy_(eng.net[:model.decoder.sigma_net.params.numel()])
            model.decoder.color_net.params.copy_(eng.net[model.decoder.sigma_net.params.numel():])
        grid = DensityGrid(RES, BOUND, 0.01).to(dev)
        grid.binary_grid = occupied.clone()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-2, weight_decay=1e-5)
    for R in (4096, 16384):
        if only and only[3] != R:
            continue
        o = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1) * 4.0
        d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, device=dev), dim=-1)
        target = torch.rand(R, 3, device=dev)

        def module_step():
            pred = render_rays(model, o, d, 2.0, 6.0, S, True, white_bkgd=True, density_grid=grid, bg_color=torch.ones(3, device=dev))[0]
            loss = torch.nn.functional.mse_loss(pred, target)
            p = model.representation.encoding.params
            loss = loss + torch.mean(torch.abs(p[1:] - p[:-1])) * 1e-6
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.representation.parameters(), max_norm=1.0)
            torch.nn.utils.clip_grad_norm_(model.decoder.parameters(), max_norm=1.0)
            opt.step()

        engine_step = lambda: eng.train_step(o, d, target, S)
        other_step = (lambda: other.train_step(o, d, target, S)) if default else module_step
        paths = [("engine", engine_step)] + ([] if args.engine_only else [("other", other_step)])
        ms = {name: [] for name, _ in paths}
        for name, fn in paths:
            timed(fn, 20)                                    # warm-up: allocations, code objects, clocks
        for _ in range(args.repeats):
            for name, fn in paths:
                ms[name].append(timed(fn, args.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = f"instant L {L} H {H} L_dir {Ld} rays {R} x {S}: shape engine {med['engine']:.3f} ms/step"
        if "other" in med:
            line += f", {other_name} {med['other']:.3f} ms/step ({med['other'] / med['engine']:.2f}x)"
        print(line + "  [" + " ".join(f"{v:.3f}" for v in ms["engine"]) + "]", flush=True)
