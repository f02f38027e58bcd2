"""Frame time of the Part 3 evaluation with the 8x256 canonical field (canonical_type: nerf), standard or under direct time
conditioning: Part3NerfEngine.render_image's per-chunk loop (fresh sampler and field tensors, a time vector, a delta_x nobody reads;
in standard mode the deformation chain is p3::fwd_kernel<false>) against the launch chain (render_image_chain:
nerf_p3_nerf_render_rays_fwd, the time read on the device, one kept workspace, the scalar-time deformation kernel) and against that
chain replayed from a torch.cuda.graph capture.  Engine at configs/part3.yaml.example (--mode standard) or part3_dtc.yaml.example
(--mode dtc) on a seeded NeuralField whose decoder weights are 2.5 times their initial draw with a density bias of 0.5, and in
standard mode a deformation MLP whose output layer has standard deviation 0.05; the 800 x 800 view of bench.py at 128 samples per
ray, the engine's RENDER_CHUNK, time 0.5.  This engine has no occupancy grid: every sample of the frame is evaluated.  Every leg runs
in a FRESH child process under its own time limit: 2 warm-up frames, five windows of frames (a window is sized from the warm-up to
about --window-seconds), a host clock around one device synchronise per window; after its last window the leg compares its output with
a loop frame (torch.equal).  The parent never opens the GPU and stops at the first child that does not exit 0.  Prints one JSON line;
at --size 800 with all three legs it is also stored under the mode's key in profiles/part3_nerf_render_timing.json.
    python tools/time_part3_nerf_render.py [--mode standard|dtc] [--size PIXELS] [--samples S] [--frames N] [--windows W]
                                           [--window-seconds T] [--limit SECONDS] [--legs loop,chain,graph]"""
import argparse, json, os, statistics, subprocess, sys, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="standard", choices=["standard", "dtc"])
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--samples", type=int, default=128)
ap.add_argument("--frames", type=int, default=0, help="frames per window; 0: from the warm-up frame time and --window-seconds")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--window-seconds", type=float, default=8.0)
ap.add_argument("--limit", type=int, default=150, help="seconds each measuring child may take")
ap.add_argument("--legs", default="loop,chain,graph", help="legs to time (a profiler run of the child takes one: --leg chain)")
ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()
STORE = os.path.join(ROOT, "profiles", "part3_nerf_render_timing.json")

if args.leg is None:
    out = {"mode": args.mode}
    for leg in args.legs.split(","):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--mode", args.mode, "--size",
               str(args.size), "--samples", str(args.samples), "--frames", str(args.frames), "--windows", str(args.windows), "--window-seconds",
               str(args.window_seconds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            sys.exit(f"the '{leg}' leg ended with status {r.returncode}; the legs behind it were not started")
        res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        out.update(res.pop("scene"))
        out[leg] = res
    if "loop" in out and "chain" in out:
        spread = out["loop"]["max_ms"] - out["loop"]["min_ms"]
        out["loop_spread_ms"] = round(spread, 4)
        out["chain_gain_ms"] = round(out["loop"]["median_ms"] - out["chain"]["median_ms"], 4)
        # standard: the chain must WIN by more than the loop's own spread; direct time conditioning: it must not LOSE by more than it
        out["criterion"] = "chain median < loop median - loop spread" if args.mode == "standard" else "chain median <= loop median + loop spread"
        out["criterion_met"] = bool(out["chain_gain_ms"] > spread if args.mode == "standard" else out["chain_gain_ms"] >= -spread)
    if "chain" in out and "graph" in out:
        out["graph_minus_chain_ms"] = round(out["graph"]["median_ms"] - out["chain"]["median_ms"], 4)        # reported, not gated
    line = json.dumps(out)
    if args.size == 800 and args.legs == "loop,chain,graph":
        stored = json.load(open(STORE)) if os.path.exists(STORE) else {}
        stored[args.mode] = out
        with open(STORE, "w") as f:
            f.write(json.dumps(stored, indent=1) + "\n")
    print(line, flush=True)
    sys.exit(0)

import numpy as np
import torch
import yaml
sys.path.insert(0, ROOT)
from project_nerf_amd import ops
from project_nerf_amd.core import NeuralField
from project_nerf_amd.part3_nerf import Part3NerfEngine
from src.dataset import SYNTHETIC_CAMERA_ANGLE, look_at_pose

dev, T, S = "cuda", 0.5, args.samples
cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part3.yaml.example" if args.mode == "standard" else "part3_dtc.yaml.example")))
cfg.update(engine=True, use_coord_noise=False)
torch.manual_seed(0)
model = NeuralField(cfg).to(dev)
with torch.no_grad():
    dec = model.decoder_direct if args.mode == "dtc" else model.decoder
    for name, p in dec.named_parameters():
        if name.endswith("weight"):
            p.mul_(2.5)
    dec.sigma_layer.bias.fill_(0.5)
    if args.mode == "standard":
        model.deform_net.net[6].weight.normal_(0.0, 0.05)
        model.deform_net.net[6].bias.uniform_(-0.01, 0.01)
eng = Part3NerfEngine(cfg, device=dev)
eng.load_from_model(model)
del model

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
if args.leg == "loop":
    fn, result = loop, loop
elif args.leg == "chain":
    fn = result = lambda: eng.render_image_chain(o, d, t_host, S)
elif args.leg == "graph":
    # the chain captured once and replayed (a linear graph on one stream)
    ws = torch.empty(ops.p3_nerf_render_workspace_bytes(chunk, S), dtype=torch.uint8, device=dev)
    time_dev = torch.tensor([T], device=dev)
    call = lambda: ops.p3_nerf_render_rays_fwd(eng.packed_d, eng.packed_c, o, d, S, eng.near, eng.far, time_dev, eng.bg, chunk, workspace=ws)[0]
    call()                                               # code objects and launch attributes before the capture
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        captured = call()
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


timed(1)                                                 # warm-up: allocations, code objects
warm = timed(1)                                          # ... and clocks; its time sizes the windows
frames = args.frames or max(2, min(200, int(args.window_seconds * 1e3 / warm)))
ms = [timed(frames) for _ in range(args.windows)]
fn()
torch.cuda.synchronize()
same = bool(torch.equal(result().view(-1, 3), ref.view(-1, 3)))
scene = {"tool": "time_part3_nerf_render", "frame": f"{W}x{H} x {S} samples/ray", "samples": H * W * S, "time": T, "chunk": chunk,
         "chunks": (o.shape[0] + chunk - 1) // chunk, "windows": args.windows, "workspace_bytes": ops.p3_nerf_render_workspace_bytes(chunk, S)}
print(json.dumps({"scene": scene, "frames_per_window": frames, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                  "max_ms": round(max(ms), 4), "fps": round(1e3 / statistics.median(ms), 2), "equals_loop": same}), flush=True)
sys.exit(0 if same else 3)
