"""Hash-grid gather timings of ONE source tree, for comparing two builds of csrc/hash_cell.h's callers:
    python tools/time_hash_gather.py TREE_ROOT OUT.json
run alternately on a checkout of the commit to compare against and on this tree, several times each, in one job
(profiles/hash_gather_timing.json holds such a series).  Figures, microseconds per call, each the median of five windows of 200 calls
between device events.  Points: rays through the box, 128 samples each (the locality of a training batch's active samples).
  operand-image forward, fp16 table, L16 / T2^19, at 200 k and 2^18 points, plain and with the histogram of the binned backward;
  the lattice forward: nerf_instant_grid_update on 64^3 cells as ONE 2^18-cell slab (clear + gather + sigma-net chain);
  the counted forward: nerf_instant_render_rays_fwd, 4096 rays x 64 samples in one chunk (capacity 2^18), a sphere that holds about
    half of the samples (compaction + gather + decoder chain + compositing: the entry is the only way to the kernel);
  three tables of Part 4's deformation shape (L12 / T2^10) at 54 k points, fp16 images, one launch;
  the input gradient (fp16 table, L16 / T2^19) at 54 k and 200 k points: float atomics from row-major and from level-major feature
    gradients, and the ordered form (option "deterministic")."""
import json, os, statistics, sys
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch
import project_nerf_amd  # noqa
from project_nerf_amd import ops, _lib
assert os.path.abspath(_lib.LIB_PATH).startswith(root + os.sep), (_lib.LIB_PATH, root)
lib = _lib.load()


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


def ray_points(n, bound=1.5, samples=128):
    g = torch.Generator().manual_seed(n)
    rays = (n + samples - 1) // samples
    o = torch.nn.functional.normalize(torch.randn(rays, 3, generator=g), dim=-1) * (bound - 0.05)
    d = torch.nn.functional.normalize(-o + 0.5 * torch.randn(rays, 3, generator=g), dim=-1)
    t = torch.linspace(0.0, 2.0 * bound - 0.1, samples)
    return (o[:, None] + d[:, None] * t[None, :, None]).reshape(-1, 3)[:n].clamp(-bound, bound).cuda().contiguous()


res = {}
BOUND = 1.5
torch.manual_seed(0)
L16 = ops.HashLevelTable()
table_h = (torch.rand(L16.entries, 2) * 2e-4 - 1e-4).cuda().half()
for n, tag in ((200000, "200k"), (1 << 18, "262144")):
    pts = ray_points(n)
    image = torch.empty(lib.nerf_imlp_workspace_bytes(n), device="cuda", dtype=torch.uint8)
    res[f"fwd_image_{tag}_us"] = event_us(lambda: ops.hash_encode_fwd(pts, table_h, L16, BOUND, want_f32=False, out_nat=image))
    hist = torch.zeros(ops.hash_encode_bwd_workspace_bytes(n, 16), device="cuda", dtype=torch.uint8)
    res[f"fwd_image_hist_{tag}_us"] = event_us(lambda: _lib.check(lib.nerf_hash_encode_fwd_f16_hist(
        pts.data_ptr(), n, table_h.data_ptr(), 16, *L16.host_args(), BOUND, image.data_ptr(), hist.data_ptr(), hist.numel(), ops._stream()), "hist"))
    del image, hist

# ---- lattice and counted forwards, through their entries
from project_nerf_amd.engine import InstantNgpEngine
net = InstantNgpEngine._init_net(None, torch.Generator().manual_seed(5)).cuda()
packed = ops.imlp_pack(net)
RES = 64
ws = torch.empty(ops.instant_grid_update_workspace_bytes(RES ** 3), device="cuda", dtype=torch.uint8)
prev = torch.zeros(RES, RES, RES, device="cuda")
res["lattice_slab_262144_grid_update_us"] = event_us(
    lambda: ops.instant_grid_update(packed, table_h, L16, BOUND, RES, BOUND, 0.01, prev=prev, slab_cells=RES ** 3, workspace=ws))
R, S, GRES = 4096, 64, 128
g = torch.Generator().manual_seed(7)
o = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 4.0
d = torch.nn.functional.normalize(-o + 0.1 * torch.randn(R, 3, generator=g), dim=-1)
o, d = o.cuda().contiguous(), d.cuda().contiguous()
ax = torch.linspace(-BOUND, BOUND, GRES)
gx, gy, gz = torch.meshgrid(ax, ax, ax, indexing="ij")
grid = ((gx ** 2 + gy ** 2 + gz ** 2) < 1.0).cuda()
rws = torch.empty(ops.instant_render_workspace_bytes(R, S), device="cuda", dtype=torch.uint8)
bg = torch.ones(3, device="cuda")
render = lambda: ops.instant_render_rays_fwd(packed, table_h, L16, BOUND, grid, BOUND, o, d, S, 2.0, 6.0, bg, R, workspace=rws)
render()
torch.cuda.synchronize()
res["counted_live_of_262144"] = int(rws[:4].view(torch.int32).item())
res["counted_capacity_262144_render_us"] = event_us(render)

# ---- three deformation tables in one launch
L12 = ops.HashLevelTable(12, 10)
n = 54000
pts = ray_points(n)
tabs = (torch.rand(3 * L12.entries, 2) * 2e-4 - 1e-4).cuda().half()
words = (n + 127) // 128 * 128 * 32
imgs = torch.empty(3, words, device="cuda", dtype=torch.int16)
three = lambda: ops.hash_encode_fwd_nat_tables(pts, [tabs[k * L12.entries:(k + 1) * L12.entries] for k in range(3)], L12, BOUND,
                                               [imgs[k] for k in range(3)], fp16=True)
assert three()
res["fwd_three_tables_54k_us"] = event_us(three)

# ---- input gradient
for n, tag in ((54000, "54k"), (200000, "200k")):
    pts = ray_points(n)
    d_feat = torch.randn(n, 32, device="cuda")
    lm = d_feat.view(n, 16, 2).permute(1, 0, 2).contiguous()
    res[f"bwd_input_atomic_{tag}_us"] = event_us(lambda: ops.hash_encode_bwd_input(pts, table_h, L16, BOUND, d_feat))
    res[f"bwd_input_atomic_lm_{tag}_us"] = event_us(lambda: ops.hash_encode_bwd_input(pts, table_h, L16, BOUND, None, grad_lm=lm.data_ptr()))
    ops.set_deterministic(True)
    try:
        res[f"bwd_input_ordered_{tag}_us"] = event_us(lambda: ops.hash_encode_bwd_input(pts, table_h, L16, BOUND, d_feat))
    finally:
        ops.set_deterministic(False)
line = json.dumps(res)
print(line, flush=True)
with open(sys.argv[2], "w") as f:
    f.write(line + "\n")
