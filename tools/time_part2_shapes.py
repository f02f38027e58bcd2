"""Step time of Part 2 (vanilla NeRF) at non-default decoder shapes: part2.Part2Engine (fused HIP chain) against the module path
(NeuralField + render_rays + mse_loss + autograd + torch.optim.Adam: what run.py does without `engine: true`) in one process, same
weights, same rays.  Batches of 4096 x 64 and 1024 x 64 samples, L_embed 10 / L_embed_dir 4.  Interleaved repeats after a warm-up,
median of the repeats.
    python tools/time_part2_shapes.py [--steps N] [--repeats R] [--engine-only] [--only H,layers,rays]"""
import argparse, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from project_nerf_amd.core import NeuralField
from project_nerf_amd.part2 import Part2Engine
from project_nerf_amd.renderer import render_rays

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only", type=str, default=None, help="one case: H,layers,rays (profiler runs)")
ap.add_argument("--engine-only", action="store_true", help="skip the module path (profiler runs of the engine's kernels)")
args = ap.parse_args()
dev, S = "cuda", 64
torch.manual_seed(0)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


only = tuple(int(v) for v in args.only.split(",")) if args.only else None
for H, layers, skip, V in ((64, 4, 2, 64), (128, 4, 2, 64), (128, 8, 4, 128), (256, 4, 2, 128)):
    if only and only[:2] != (H, layers):
        continue
    cfg = {"mode": "part2_nerf", "use_positional_encoding": True, "L_embed": 10, "use_viewdirs": True, "L_embed_dir": 4,
           "hidden_dim": H, "num_layers": layers, "skip_layer": skip, "view_dim": V}
    model = NeuralField(cfg).to(dev)
    eng = Part2Engine(cfg, device=dev)
    eng.load_from_model(model)
    opt = torch.optim.Adam(model.parameters(), lr=5e-4)
    for R in (4096, 1024):
        if only and only[2] != R:
            continue
        o = torch.nn.functional.normalize(torch.randn(R, 3, device=dev), dim=-1) * 4.0
        d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, device=dev), dim=-1)
        target = torch.rand(R, 3, device=dev)

        def module_step():
            loss = torch.nn.functional.mse_loss(render_rays(model, o, d, 2.0, 6.0, S, True, white_bkgd=True)[0], target)
            opt.zero_grad()
            loss.backward()
            opt.step()

        engine_step = lambda: eng.train_step(o, d, target, S)
        paths = [("engine", engine_step)] + ([] if args.engine_only else [("module", module_step)])
        ms = {name: [] for name, _ in paths}
        for name, fn in paths:
            timed(fn, 20)                                    # warm-up: allocations, code objects, clocks
        for _ in range(args.repeats):
            for name, fn in paths:
                ms[name].append(timed(fn, args.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = f"part2 H {H} layers {layers} skip {skip} view {V} rays {R} x {S}: engine {med['engine']:.3f} ms/step"
        if "module" in med:
            line += f", module path {med['module']:.3f} ms/step ({med['module'] / med['engine']:.2f}x)"
        print(line + "  [" + " ".join(f"{v:.3f}" for v in ms["engine"]) + "]", flush=True)
