"""Step-tail timings (TV + squared norm, clip + AdamW, plain Adam) of ONE source tree, for comparing two builds of csrc/adam.hip
(DESIGN 4.26):
    python tools/time_step_tail.py TREE_ROOT OUT.json
run alternately on a checkout of the commit to compare against and on this tree, several times each, in one job
(profiles/step_tail_timing.json holds such a series).  Figures, microseconds per call, each the median of five windows of 200 calls
between device events.  COLD, as tools/time_tv.py: six buffer sets in turn, so that every call reads from HBM as a training step does.
Raw C-ABI calls only, so that the script runs on either tree.
  nerf_tv_normsq_codes with and without a TV weight and nerf_adamw_clip_step_tv with codes and the fp16 copy, at time_tv.py's three
    table sizes (24 M, 12.6 M, 4.5 M elements);
  the generic kernels (both passes) at 12.6 M elements misaligned by one element;
  nerf_clip_adamw_small at 30145 elements, nerf_adam_step at 595844;
  the _piece pair on a quarter of the 24 M table (halo on both sides)."""
import json, os, statistics, sys
root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import torch
import project_nerf_amd  # noqa
from project_nerf_amd import ops, _lib
assert os.path.abspath(_lib.LIB_PATH).startswith(root + os.sep), (_lib.LIB_PATH, root)
lib = _lib.load()
SETS, HYP = 6, (2, 1e-2, 0.9, 0.999, 1e-8, 1e-5)           # step, lr, betas, eps, weight decay
P = lambda t: None if t is None else t.data_ptr()


def event_us(fn, iters=200, windows=5):
    """fn(i): call number i (it picks the buffer set)"""
    for i in range(12):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)
    return round(statistics.median(out), 3)


def buffer_sets(n, mis=0, shadow=True, sets=SETS):
    """(p, g, m, v, fp16 copy, codes) per set; mis: the fp32 views start that many elements late"""
    out = []
    for _ in range(sets):
        p, g = (torch.randn(n + mis, device="cuda") * 0.1)[mis:], (torch.randn(n + mis, device="cuda") * 1e-3)[mis:]
        m, v = torch.zeros(n + mis, device="cuda")[mis:], torch.zeros(n + mis, device="cuda")[mis:]
        assert all(t.data_ptr() % 16 == 4 * (mis % 4) for t in (p, g, m, v))
        out.append((p, g, m, v, torch.empty(n, device="cuda", dtype=torch.float16) if shadow else None,
                    torch.zeros(16 + (n + 3) // 4, dtype=torch.uint8, device="cuda")[16:]))
    return out


res, st, ws, TV_W, GS, MAX_NORM = {}, ops._stream(), ops.normsq_ws("cuda"), 1e-4, 1.0, 1.0


def two_passes(tag, n, mis=0):
    bufs = buffer_sets(n, mis)

    def codes(i, tv_w):
        p, g, _, _, _, c = bufs[i % SETS]
        _lib.check(lib.nerf_tv_normsq_codes(P(p), P(g), n, 1, tv_w, GS, P(ws), 0, P(c), st), "codes")

    def adamw(i):
        p, g, m, v, h, c = bufs[i % SETS]
        _lib.check(lib.nerf_adamw_clip_step_tv(P(p), P(g), P(m), P(v), n, *HYP, P(ws), MAX_NORM, GS, P(c), n, TV_W, n, 0.0, 0, 0, 0.0, P(h), st), "adamw")

    res[f"codes_no_tv_{tag}_us"] = event_us(lambda i: codes(i, 0.0))
    res[f"codes_tv_{tag}_us"] = event_us(lambda i: codes(i, TV_W))          # leaves every set's codes for the second pass
    res[f"adamw_tv_shadow_{tag}_us"] = event_us(adamw)


for n, tag in ((24_000_000, "24M"), (12_600_000, "12.6M"), (4_500_000, "4.5M")):
    two_passes(tag, n)
two_passes("generic_12.6M_mis1", 12_600_000, mis=1)

n = 30145
small = buffer_sets(n, shadow=False)
res["clip_adamw_small_30145_us"] = event_us(lambda i: _lib.check(lib.nerf_clip_adamw_small(
    *(P(t) for t in small[i % SETS][:4]), n, *HYP, MAX_NORM, GS, P(ws), 0, st), "small"))
n = 595844
plain = buffer_sets(n, shadow=False)
res["adam_step_595844_us"] = event_us(lambda i: _lib.check(lib.nerf_adam_step(*(P(t) for t in plain[i % SETS][:4]), n, *HYP, None, st), "adam"))

# ---- a quarter of the 24 M table as one piece with a neighbour on both sides
table, lo = 24_000_000, 6_000_000
n = table // 4
whole = buffer_sets(table)


def piece_codes(i):
    p, g, _, _, _, c = whole[i % SETS]
    _lib.check(lib.nerf_tv_normsq_codes_piece(P(p[lo:]), P(g[lo:]), n, table, 3, TV_W, GS, P(ws), 0, P(c[lo // 4:]), st), "piece codes")


def piece_adamw(i):
    p, g, m, v, h, c = whole[i % SETS]
    _lib.check(lib.nerf_adamw_clip_step_tv_piece(P(p[lo:]), P(g[lo:]), P(m[lo:]), P(v[lo:]), n, *HYP, P(ws), MAX_NORM, GS, P(c[lo // 4:]), TV_W, table, 1,
                                                 P(h[lo:]), st), "piece adamw")


res["piece_codes_quarter_of_24M_us"] = event_us(piece_codes)
res["piece_adamw_quarter_of_24M_us"] = event_us(piece_adamw)
line = json.dumps(res)
print(line, flush=True)
with open(sys.argv[2], "w") as f:
    f.write(line + "\n")
