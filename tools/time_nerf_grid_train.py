"""Step time of the vanilla (8x256) field's TRAINING through an occupancy grid, one process, one engine, the same resident frames:
  dense  VanillaNerfEngine.train_step as it is, fed by train_batch (every sample of every ray through forward, dgrad, wgrad) -- the yardstick
  two    the grid step fed by train_batch + prepare_batch (two launches), the batch drawn and compacted one step ahead
  fused  the grid step fed by train_batch_compact (one launch), one step ahead
Scene of tools/time_nerf_grid_render.py (default-initialised engine, the sphere of radius 1 occupied in a 128^3 grid over
[-1.5, 1.5]^3), frames as bench.py builds them (uniform-noise 800 x 800 RGBA resident in HBM, cameras on the hemisphere).  Two batch
sizes: 4096 x 64, and the batch at which the ACTIVE samples are about 262144 (4096 / active fraction rays).  5 warm-up steps per
leg, five interleaved windows, a host clock around a final device synchronise; median and min-max of the windows; then the phases
of each leg from HIP events at the engine's `mark` points.  Prints one JSON line and writes it to --out.
    python tools/time_nerf_grid_train.py [--steps N] [--windows W] [--frames F] [--out PATH]"""
import argparse, json, os, statistics, sys, time
import torch
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from bench import hemisphere_poses
from project_nerf_amd.engine import VanillaNerfEngine
from src.dataset import BlenderDataset, SYNTHETIC_CAMERA_ANGLE

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=50, help="steps per window")
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--frames", type=int, default=100)
ap.add_argument("--phase-steps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nerf_grid_train_timing.json"))
args = ap.parse_args()
dev, S, BOUND, RES = "cuda", 64, 1.5, 128
torch.manual_seed(100)

eng = VanillaNerfEngine(device=dev, seed=0, grid_resolution=RES, bound=BOUND)
ax = torch.linspace(-BOUND, BOUND, RES)
gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
eng.binary_grid = ((gx ** 2 + gy ** 2 + gz ** 2) < 1.0).to(dev)
ds = BlenderDataset.from_tensors(torch.rand(args.frames, 800, 800, 4, device=dev), hemisphere_poses(args.frames, 7).to(dev), SYNTHETIC_CAMERA_ANGLE)
counter = [0]


def tick():
    counter[0] += 1
    return counter[0]


class Leg:
    """one way of feeding and running a step; the grid legs keep one batch drawn and compacted ahead"""

    def __init__(self, name, R):
        self.name, self.R, self.ahead, self.active = name, R, [], []

    def draw(self):
        c = tick()
        if self.name == "fused":
            return ds.train_batch_compact(self.R, S, eng.near, eng.far, eng.bg, 100, c, eng.binary_grid, eng.bound)
        o, d, target, z = ds.train_batch(self.R, S, eng.near, eng.far, eng.bg, seed=100, counter=c)
        return (o, d, target, z) if self.name == "dense" else (o, d, target, eng.prepare_batch(o, d, S))

    def step(self, mark=None):
        if self.name == "dense":
            o, d, target, z = self.draw()
            if mark is not None:
                mark("batch")
            return eng.train_step(o, d, target, S, z=z, mark=mark)
        if not self.ahead:
            self.ahead.append(self.draw())
        o, d, target, prepared = self.ahead.pop()
        self.ahead.append(self.draw())
        if mark is not None:
            mark("batch")
        loss = eng.train_step(o, d, target, S, prepared=prepared, mark=mark)
        self.active.append(prepared.get()[2].shape[0])
        return loss


def timed(leg, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        leg.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3 / n
    leg.ahead.clear()            # (a batch left waiting would hold its slot of the count ring while the other legs run)
    return dt


def phases(leg, n):
    acc = {}
    for _ in range(n):
        evs = [("start", torch.cuda.Event(enable_timing=True))]
        evs[0][1].record()

        def mark(name):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append((name, e))
        leg.step(mark)
        torch.cuda.synchronize()
        for (_, e0), (name, e1) in zip(evs[:-1], evs[1:]):
            acc[name] = acc.get(name, 0.0) + e0.elapsed_time(e1)
    leg.ahead.clear()
    return {k: round(v / n, 4) for k, v in acc.items()}


def measure(R):
    legs = [Leg(name, R) for name in ("dense", "two", "fused")]
    ms = {leg.name: [] for leg in legs}
    for leg in legs:
        timed(leg, 5)                                        # warm-up: allocations, code objects, clocks
    for _ in range(args.windows):
        for leg in legs:
            ms[leg.name].append(timed(leg, args.steps))
    out = {"rays": R, "samples": R * S}
    for leg in legs:
        v = ms[leg.name]
        out[leg.name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                         "phases_ms": phases(leg, args.phase_steps)}
        if leg.active:
            out[leg.name]["active_samples_mean"] = round(statistics.mean(leg.active), 1)
    frac = out["fused"]["active_samples_mean"] / (R * S)
    spread = out["dense"]["max_ms"] - out["dense"]["min_ms"]
    out.update(active_fraction=round(frac, 4), one_over_active_fraction=round(1 / frac, 3), dense_window_spread_ms=round(spread, 4),
               dense_over_two=round(out["dense"]["median_ms"] / out["two"]["median_ms"], 3),
               dense_over_fused=round(out["dense"]["median_ms"] / out["fused"]["median_ms"], 3),
               grid_below_dense_by_more_than_its_spread=bool(min(out["two"]["median_ms"], out["fused"]["median_ms"])
                                                             < out["dense"]["median_ms"] - spread),
               fused_within_two_plus_its_spread=bool(out["fused"]["median_ms"]
                                                     <= out["two"]["median_ms"] + out["two"]["max_ms"] - out["two"]["min_ms"]))
    return out


probe = eng.prepare_batch(*ds.train_batch(4096, S, eng.near, eng.far, eng.bg, seed=100, counter=tick())[:2], S)
fraction = probe.get()[2].shape[0] / (4096 * S)
big = int(round(4096 / max(fraction, 1e-3) / 64)) * 64           # active samples ~ 262144
result = {"tool": "time_nerf_grid_train", "scene": f"sphere r=1 in {RES}^3 over [-{BOUND}, {BOUND}]^3, default-initialised field",
          "frames": f"{args.frames} x 800x800 RGBA (uniform noise)", "samples_per_ray": S, "steps_per_window": args.steps,
          "windows": args.windows, "phase_steps": args.phase_steps, "probe_active_fraction": round(fraction, 4),
          "batches": [measure(4096), measure(big)]}
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
