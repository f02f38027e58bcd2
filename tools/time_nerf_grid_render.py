"""Frame time of the vanilla (8x256) field's evaluation through an occupancy grid, one process, same engine, same rays:
  dense  VanillaNerfEngine.render_image as it is (nerf_render_rays_fwd: every sample of every ray through the decoder) -- the yardstick
  loop   render_image(grid="loop"): per chunk compaction, ONE host read of the active count, point-mode decoder, indexed compositing
  chain  render_image(grid=True): nerf_render_rays_grid_fwd, the count read on the device, one kept workspace
  graph  that chain replayed from a torch.cuda.graph capture
Analytic scene as tools/time_instant_render.py sets it up (the sphere of radius 1 occupied in a 128^3 grid over [-1.5, 1.5]^3), the
800 x 800 view of bench.py at 128 samples per ray, grid legs in chunks of 200000 rays, the dense leg in the engine's default chunk.
5 warm-up frames per leg, five interleaved windows of 20 frames, a host clock around a final device synchronise; median and min-max
of the windows.  Prints one JSON line.
    python tools/time_nerf_grid_render.py [--frames N] [--windows W] [--size PIXELS] [--chunk RAYS] [--dense-chunk RAYS]"""
import argparse, json, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from project_nerf_amd import ops
from project_nerf_amd.engine import VanillaNerfEngine
from src.dataset import SYNTHETIC_CAMERA_ANGLE, look_at_pose

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--chunk", type=int, default=200000)
ap.add_argument("--dense-chunk", type=int, default=65536)
args = ap.parse_args()
dev, S, BOUND, RES = "cuda", 128, 1.5, 128
torch.manual_seed(0)

eng = VanillaNerfEngine(device=dev, seed=0, grid_resolution=RES, bound=BOUND)
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

dense = lambda: eng.render_image(o, d, S, chunk=args.dense_chunk)
loop = lambda: eng.render_image(o, d, S, chunk=args.chunk, grid="loop")
chain = lambda: eng.render_image(o, d, S, chunk=args.chunk, grid=True)
ref = loop()
torch.cuda.synchronize()
same = bool(torch.equal(ref, chain()))

# fourth leg: the chain captured once and replayed (a linear graph on one stream)
chunk = max(1, min(args.chunk, o.shape[0]))
ws = eng._grid_ws[(chunk, S)]
packed = eng._inference_weights()
graph = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with torch.cuda.graph(graph):
    captured = ops.render_rays_grid_fwd(packed, eng.binary_grid, eng.bound, o, d, S, eng.near, eng.far, eng.bg, chunk, workspace=ws)[0]
graph.replay()
torch.cuda.synchronize()
same_graph = bool(torch.equal(ref, captured))
active = 0
for r0 in range(0, o.shape[0], chunk):
    active += int((ops.sample_compact(o[r0:r0 + chunk], d[r0:r0 + chunk], eng.near, eng.far, S, eng.binary_grid, eng.bound)[1] >= 0).sum())
# how far the masked frame is from the dense one: skipped samples contribute nothing instead of the field's value there
dense_diff = float((dense() - ref).abs().max())


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


legs = [("dense", dense), ("loop", loop), ("chain", chain), ("graph", graph.replay)]
ms = {name: [] for name, _ in legs}
for name, fn in legs:
    timed(fn, 5)                                         # warm-up: allocations, code objects, clocks
for _ in range(args.windows):
    for name, fn in legs:
        ms[name].append(timed(fn, args.frames))
total = o.shape[0] * S
out = {"tool": "time_nerf_grid_render", "frame": f"{W}x{H} x {S} samples/ray", "chunk": chunk, "dense_chunk": args.dense_chunk,
       "samples": total, "active_samples": active, "active_fraction": round(active / total, 4),
       "frames_per_window": args.frames, "windows": args.windows, "chain_equals_loop": same, "graph_equals_loop": same_graph,
       "max_abs_diff_dense_vs_grid": dense_diff, "workspace_bytes": ws.numel()}
for name in ms:
    out[name] = {"median_ms": round(statistics.median(ms[name]), 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4),
                 "fps": round(1e3 / statistics.median(ms[name]), 1)}
out["dense_over_chain"] = round(out["dense"]["median_ms"] / out["chain"]["median_ms"], 3)
out["one_over_active_fraction"] = round(total / max(active, 1), 3)
out["loop_over_chain"] = round(out["loop"]["median_ms"] / out["chain"]["median_ms"], 3)
print(json.dumps(out), flush=True)
