"""Frame time of the Part 3 evaluation with a hash-grid canonical field: Part3InstantEngine.render_image's per-chunk loop (one host
read of the active count, a time vector, delta_x, the canonical chain in the training workspace layout and four fresh outputs per
chunk; the deformation chain is p3::fwd_kernel<false>) against the launch chain (render_image(chain=True): nerf_p3_render_rays_fwd,
count and time read on the device, one kept workspace, the scalar-time deformation kernel) and against that chain replayed from a
torch.cuda.graph capture.  Engine at configs/part3_instant.yaml.example with the table, the networks and the deformation MLP of
tools/time_part3_grid_update.py (table 0.5 sin(0.37 i + 0.11 (i mod 7)), seeded normal canonical networks with the density row x 8,
a seeded deformation MLP whose output layer has standard deviation 0.05), the sphere of radius 1 occupied in a 128^3 grid, the
800 x 800 view of bench.py at the config's sample count, the engine's RENDER_CHUNK, time 0.5.  Every leg runs in a FRESH child
process under its own time limit: 5 warm-up frames, five windows of 20 frames, a host clock around a device synchronise; after its
last window the leg compares its output with a loop frame (torch.equal).  The parent never opens the GPU and stops at the first child
that does not exit 0.  Prints one JSON line and writes it to profiles/part3_render_timing.json.
    python tools/time_part3_render.py [--frames N] [--windows W] [--size PIXELS] [--limit SECONDS] [--legs loop,chain,graph]"""
import argparse, json, os, statistics, subprocess, sys, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--limit", type=int, default=240, help="seconds each measuring child may take")
ap.add_argument("--legs", default="loop,chain,graph", help="legs to time (a profiler run of the child takes one: --leg chain)")
ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

if args.leg is None:
    out = {}
    for leg in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--frames", str(args.frames),
               "--windows", str(args.windows), "--size", str(args.size)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            sys.exit(f"the '{leg}' leg ended with status {r.returncode}; the legs behind it were not started")
        res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        out.update(res.pop("scene"))
        out[leg] = res
    if "loop" in out and "chain" in out:
        spread = out["loop"]["max_ms"] - out["loop"]["min_ms"]
        out["chain_within_loop_spread"] = bool(out["chain"]["median_ms"] <= out["loop"]["median_ms"] + spread)
    if "chain" in out and "graph" in out:
        out["graph_not_above_chain_max"] = bool(out["graph"]["median_ms"] <= out["chain"]["max_ms"])
    line = json.dumps(out)
    if args.size == 800 and args.legs == "loop,chain,graph":
        with open(os.path.join(ROOT, "profiles", "part3_render_timing.json"), "w") as f:
            f.write(line + "\n")
    print(line, flush=True)
    sys.exit(0)

import numpy as np
import torch
import yaml
sys.path.insert(0, ROOT)
from project_nerf_amd import ops
from project_nerf_amd import part4 as p4
from project_nerf_amd.part3 import B4, DEFORM0, W1, W2, W3, W4, Part3InstantEngine
from src.dataset import SYNTHETIC_CAMERA_ANGLE, look_at_pose

dev, RES, T = "cuda", 128, 0.5
torch.manual_seed(0)
cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part3_instant.yaml.example")))
cfg["grid_resolution"] = RES
S = int(cfg.get("render_n_samples", cfg.get("n_samples", 64)))
eng = Part3InstantEngine(cfg, device=dev)
gen = torch.Generator().manual_seed(5)
with torch.no_grad():
    i = torch.arange(eng.table.numel(), dtype=torch.float64, device=dev)
    eng.table.copy_((0.5 * torch.sin(0.37 * i + 0.11 * (i % 7))).float())
    del i
    eng.net.zero_()
    eng.net[:p4.N_PARAMS].copy_((torch.randn(p4.N_PARAMS, generator=gen) * 0.15).to(dev))
    eng.net[p4.S2:p4.S2 + 64] *= 8.0
    dw = torch.zeros(B4 + 3)
    for w, fan_in, rows in ((W1, 84, 128), (W2, 128, 128), (W3, 128, 128)):          # torch.nn.Linear's default ranges
        dw[w:w + rows * fan_in + rows] = (torch.rand(rows * fan_in + rows, generator=gen) * 2 - 1) / fan_in ** 0.5
    dw[W4:B4] = torch.randn(B4 - W4, generator=gen) * 0.05
    dw[B4:] = (torch.rand(3, generator=gen) * 2 - 1) * 0.01
    eng.net[DEFORM0:].copy_(dw.to(dev))
eng.repack()
ax = torch.linspace(-eng.grid_bound, eng.grid_bound, RES)
gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
eng.binary_grid = ((gx ** 2 + gy ** 2 + gz ** 2) < 1.0).to(dev)

H = W = args.size
focal = 0.5 * W / np.tan(0.5 * SYNTHETIC_CAMERA_ANGLE)
c2w = torch.tensor(look_at_pose(4.0311 * np.array([0.6, 0.5, 0.62])), dtype=torch.float32)
j, i = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
d = torch.stack([(i - W * .5) / focal, -(j - H * .5) / focal, -torch.ones_like(i)], -1).reshape(-1, 3).float() @ c2w[:3, :3].T
d = (d / d.norm(dim=-1, keepdim=True)).to(dev).contiguous()
o = c2w[:3, 3].expand_as(d).contiguous().to(dev)
t_host = torch.tensor([[T]])
chunk = max(1, min(eng.RENDER_CHUNK, o.shape[0]))

loop = lambda: eng.render_image(o, d, t_host, S)
ref = loop().clone()
active = int((ops.sample_compact(o, d, eng.near, eng.far, S, eng.binary_grid, eng.grid_bound)[1] >= 0).sum())
if args.leg == "loop":
    fn, result = loop, loop
elif args.leg == "chain":
    fn = result = lambda: eng.render_image(o, d, t_host, S, chain=True)
elif args.leg == "graph":
    # the chain captured once and replayed (a linear graph on one stream)
    ws = torch.empty(ops.p3_render_workspace_bytes(chunk, S), dtype=torch.uint8, device=dev)
    time_dev, table = torch.tensor([T], device=dev), eng.table_h.view(-1, 2)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        captured = ops.p3_render_rays_fwd(eng.packed_d, eng.packed_c, table, eng.levels, eng.bound, eng.binary_grid, eng.grid_bound, o, d, S,
                                          eng.near, eng.far, time_dev, eng.bg, chunk, workspace=ws)[0]
    fn, result = graph.replay, lambda: captured
else:
    sys.exit(f"unknown leg {args.leg}")


def timed(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


timed(5)                                                 # warm-up: allocations, code objects, clocks
ms = [timed(args.frames) for _ in range(args.windows)]
fn()
torch.cuda.synchronize()
same = bool(torch.equal(result().view(-1, 3), ref.view(-1, 3)))
scene = {"tool": "time_part3_render", "frame": f"{W}x{H} x {S} samples/ray", "time": T, "chunk": chunk, "chunks": (o.shape[0] + chunk - 1) // chunk,
         "active_samples": active, "frames_per_window": args.frames, "windows": args.windows,
         "workspace_bytes": ops.p3_render_workspace_bytes(chunk, S)}
print(json.dumps({"scene": scene, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                  "fps": round(1e3 / statistics.median(ms), 1), "equals_loop": same}), flush=True)
sys.exit(0 if same else 3)
