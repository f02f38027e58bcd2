"""Frame time of the Instant-NGP evaluation: InstantNgpEngine.render_image's per-chunk loop (one host read of the active count,
fresh pts / dirs / workspace tensors per chunk) against the launch chain (render_image(chain=True): nerf_instant_render_rays_fwd,
counts read on the device, one kept workspace) and against that chain replayed from a torch.cuda.graph capture -- one process,
same engine, same rays.  Analytic scene as tools/time_instant_shapes.py sets it up (the sphere of radius 1 occupied in a 128^3
grid over [-1.5, 1.5]^3), the 800 x 800 view of bench.py at 128 samples per ray, chunk 200000.  5 warm-up frames per leg, five
interleaved windows of 20 frames, a host clock around a final device synchronise; median and min-max of the windows.  Prints one
JSON line.
    python tools/time_instant_render.py [--frames N] [--windows W] [--size PIXELS] [--chunk RAYS]"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from project_nerf_amd import ops
from project_nerf_amd.engine import InstantNgpEngine
from src.dataset import SYNTHETIC_CAMERA_ANGLE, look_at_pose

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--chunk", type=int, default=200000)
args = ap.parse_args()
dev, S, BOUND, RES = "cuda", 128, 1.5, 128
torch.manual_seed(0)

cfg = {"mode": "part2_instant", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
       "per_level_scale": 1.5, "scene_bound": BOUND, "hidden_dim": 64, "L_embed_dir": 4, "grid_resolution": RES}
eng = InstantNgpEngine(cfg, device=dev)
ax = torch.linspace(-BOUND, BOUND, RES)
gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
eng.binary_grid = ((gx ** 2 + gy ** 2 + gz ** 2) < 1.0).to(dev)

H = W = args.size
focal = 0.5 * W / np.tan(0.5 * SYNTHETIC_CAMERA_ANGLE)
c2w = torch.tensor(look_at_pose(4.0311 * np.array([0.6, 0.5, 0.62])), dtype=torch.float32)
j, i = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
d = torch.stack([(i - W * .5) / focal, -(j - H * .5) / focal, -torch.ones_like(i)], -1).reshape(-1, 3).float() @ c2w[:3, :3].T
d = (d / d.norm(dim=-1, keepdim=True)).to(dev).contiguous()
o = c2w[:3, 3].expand_as(d).contiguous().to(dev)

loop = lambda: eng.render_image(o, d, S, chunk=args.chunk)
chain = lambda: eng.render_image(o, d, S, chunk=args.chunk, chain=True)
ref = loop()
same = bool(torch.equal(ref, chain()))

# third leg: the chain captured once and replayed (a linear graph on one stream)
chunk = max(1, min(args.chunk, o.shape[0]))
ws = eng._chain_ws[(chunk, S)]
table = eng._gather_table()
graph = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with torch.cuda.graph(graph):
    captured = ops.instant_render_rays_fwd(eng.packed, table, eng.levels, eng.bound, eng.binary_grid, eng.bound, o, d, S, eng.near, eng.far,
                                           eng.bg, chunk, workspace=ws)[0]
graph.replay()
torch.cuda.synchronize()
same_graph = bool(torch.equal(ref, captured))
active = int((ops.sample_compact(o, d, eng.near, eng.far, S, eng.binary_grid, eng.bound)[1] >= 0).sum())


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


legs = [("loop", loop), ("chain", chain), ("graph", graph.replay)]
ms = {name: [] for name, _ in legs}
for name, fn in legs:
    timed(fn, 5)                                         # warm-up: allocations, code objects, clocks
for _ in range(args.windows):
    for name, fn in legs:
        ms[name].append(timed(fn, args.frames))
out = {"tool": "time_instant_render", "frame": f"{W}x{H} x {S} samples/ray", "chunk": chunk, "active_samples": active,
       "frames_per_window": args.frames, "windows": args.windows, "chain_equals_loop": same, "graph_equals_loop": same_graph,
       "workspace_bytes": ws.numel()}
for name in ms:
    out[name] = {"median_ms": round(statistics.median(ms[name]), 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                 "fps": round(1e3 / statistics.median(ms[name]), 1)}
spread = out["loop"]["max_ms"] - out["loop"]["min_ms"]
out["chain_within_loop_spread"] = bool(out["chain"]["median_ms"] <= out["loop"]["median_ms"] + spread)
print(json.dumps(out), flush=True)
