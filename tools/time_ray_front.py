"""Ray front-end timings of ONE source tree, for comparing two builds of csrc/ray_front.h's callers:
    python tools/time_ray_front.py TREE_ROOT OUT.json
run alternately on a checkout of the commit to compare against and on this tree, several times each, in one job
(profiles/ray_front_timing.json holds such a series).  Figures, microseconds per call, each the median of five windows of 200 calls
between device events:
  tools/time_compact.py's four (single pass / ordered at 16384 x 128 and 8192 x 64, in-kernel jitter, sample_compact_async),
  the training front end on tools/time_nerf_grid_train.py's scene at 4096 x 64 and at the batch with ~262144 active samples:
    fused (train_batch_compact) and two calls (train_batch + sample_compact_async),
  bench.py's sample_compact call (16384 x 128, uniforms from a tensor, one host read of the count)."""
import json, os, statistics, sys
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch
import project_nerf_amd  # noqa
from project_nerf_amd import ops, _lib
assert os.path.abspath(_lib.LIB_PATH).startswith(root), (_lib.LIB_PATH, root)
from bench import hemisphere_poses


def event_us(fn, iters=200, windows=5):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)
    return round(statistics.median(out), 3)


res = {}
torch.manual_seed(0)
for R, S, r in ((16384, 128, 128), (8192, 64, 64)):
    o = torch.nn.functional.normalize(torch.randn(R, 3, device="cuda"), dim=-1) * 4.03
    d = torch.nn.functional.normalize(-o + 0.3 * torch.randn(R, 3, device="cuda"), dim=-1)
    ax = torch.linspace(-1.5, 1.5, r)
    gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
    grid = ((gx ** 2 + gy ** 2 + gz ** 2) < 0.75 ** 2).cuda()
    for det in (False, True):
        ops.set_deterministic(det)
        run = lambda: ops.sample_compact_async(o, d, 2.0, 6.0, S, grid, 1.5, jitter=(0, 3))
        res[f"compact_{'ordered' if det else 'single'}_{R}x{S}_us"] = event_us(run)
    ops.set_deterministic(False)
    if R == 16384:
        uu = torch.rand(R, S, device="cuda")
        res["bench_sample_compact_16384x128_us"] = event_us(lambda: ops.sample_compact(o, d, 2.0, 6.0, S, grid, 1.5, u=uu), iters=100)

S, BOUND, RES = 64, 1.5, 128
ax = torch.linspace(-BOUND, BOUND, RES)
gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
grid = ((gx ** 2 + gy ** 2 + gz ** 2) < 1.0).cuda()
images = torch.rand(8, 800, 800, 4, device="cuda")
poses = hemisphere_poses(8, 7).cuda().contiguous()
bg = torch.ones(3, device="cuda")
focal = 1111.1
probe = ops.train_batch_compact(images, poses, focal, 4096, S, 2.0, 6.0, 100, 1, grid, BOUND, bg=bg)[3].get()[2].shape[0]
big = int(round(4096 / max(probe / (4096 * S), 1e-3) / 64)) * 64
res["train_front_big_rays"] = big
ctr = [1]


def fused(R):
    ctr[0] += 1
    return ops.train_batch_compact(images, poses, focal, R, S, 2.0, 6.0, 100, ctr[0], grid, BOUND, bg=bg)


def two(R):
    ctr[0] += 1
    o, d, t, _ = ops.train_batch(images, poses, focal, R, S, 2.0, 6.0, 100, ctr[0] & 0xFFFFFF, bg=bg)
    return ops.sample_compact_async(o, d, 2.0, 6.0, S, grid, BOUND, jitter=(100, ctr[0]))


for R, tag in ((4096, "4096"), (big, "big")):
    res[f"train_front_fused_{tag}x64_us"] = event_us(lambda: fused(R))
    res[f"train_front_two_{tag}x64_us"] = event_us(lambda: two(R))
line = json.dumps(res)
print(line, flush=True)
with open(sys.argv[2], "w") as f:
    f.write(line + "\n")
