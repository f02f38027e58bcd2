"""Time of one occupancy-grid refresh of the Part 3 field with a hash-grid canonical field: Part3InstantEngine.update_grid(times)'s
loop (lattice tensor; per time eight 2^18-point batches through field() -- a torch.full time vector, the deformation chain storing
delta_x and x_c, the canonical gather, the whole canonical decoder on zero directions -- then nerf_grid_update and a host read of
the count PER TIME) against the density-only launch chain (update_grid_chain(times): nerf_p3_grid_update, one kept 19.9 MB
workspace, one host read) and against that chain replayed from a torch.cuda.graph capture -- one process, same engine.  Engine at
configs/part3_instant.yaml.example with the canonical table set to 0.5 sin(0.37 i + 0.11 (i mod 7)), seeded normal canonical
networks (density row x 8), a seeded deformation MLP (output layer of standard deviation 0.05: displacements of a few hundredths),
128^3 grid, 16 times linspace(0, 1, 16), threshold = the median of the field's own folded sigma (half of the cells active).  Every
refresh starts from a history that has converged to that sigma (decay 1: the running maximum no longer moves), so each leg does the
same work every time.  5 warm-up refreshes per leg, five interleaved windows of 20 refreshes, a host clock around a final device
synchronise; median and min-max of the windows.  Prints one JSON line and writes it to profiles/part3_grid_update_timing.json.  The
measuring runs in a child process under `timeout`; this process never opens the GPU.
    python tools/time_part3_grid_update.py [--refreshes N] [--windows W] [--res R] [--times T] [--limit SECONDS] [--legs loop,chain,graph]"""
import os, sys

from grid_update_timing import ROOT, report, start

args = start(__file__, "part3_grid_update", 300, lambda ap: ap.add_argument("--times", type=int, default=16))

import torch
import yaml
sys.path.insert(0, ROOT)
from project_nerf_amd import ops
from project_nerf_amd import part4 as p4
from project_nerf_amd.part3 import B4, DEFORM0, W1, W2, W3, W4, B1, Part3InstantEngine

dev = "cuda"
torch.manual_seed(0)
cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part3_instant.yaml.example")))
cfg["grid_resolution"] = args.res
eng = Part3InstantEngine(cfg, device=dev)
gen = torch.Generator().manual_seed(5)
with torch.no_grad():
    i = torch.arange(eng.table.numel(), dtype=torch.float64, device=dev)
    eng.table.copy_((0.5 * torch.sin(0.37 * i + 0.11 * (i % 7))).float())
    del i
    eng.net.zero_()
    eng.net[:p4.N_PARAMS].copy_((torch.randn(p4.N_PARAMS, generator=gen) * 0.15).to(dev))
    eng.net[p4.S2:p4.S2 + 64] *= 8.0
    d = torch.zeros(B4 + 3)
    for w, fan_in, rows in ((W1, 84, 128), (W2, 128, 128), (W3, 128, 128)):          # torch.nn.Linear's default ranges
        d[w:w + rows * fan_in + rows] = (torch.rand(rows * fan_in + rows, generator=gen) * 2 - 1) / fan_in ** 0.5
    d[W4:B4] = torch.randn(B4 - W4, generator=gen) * 0.05
    d[B4:] = (torch.rand(3, generator=gen) * 2 - 1) * 0.01
    eng.net[DEFORM0:].copy_(d.to(dev))
assert B1 == W1 + 128 * 84
eng.repack()
TIMES = torch.linspace(0, 1, args.times).tolist()
eng.update_grid(TIMES)
eng.grid_threshold = float(eng.grid.median())

loop = lambda: eng.update_grid(TIMES)
chain = lambda: eng.update_grid_chain(TIMES)
start = eng.grid.clone()                                  # the converged history: max(start, sigma at every time) = start
ratio = loop()
ref = (eng.grid.clone(), eng.binary_grid.clone())
eng.grid.copy_(start)
ratio_chain = chain()
same = bool(torch.equal(ref[0], eng.grid) and torch.equal(ref[1], eng.binary_grid) and ratio == ratio_chain and torch.equal(ref[0], start))

# third leg: the chain captured once and replayed (a linear graph on one stream, no host read)
table = eng.table_h.view(-1, 2)
hist = start.clone()
graph = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with torch.cuda.graph(graph):
    captured = ops.p3_grid_update(eng.packed_d, eng.packed_c, table, eng.levels, eng.bound, TIMES, args.res, eng.grid_bound,
                                  eng.grid_threshold, hist, 1.0, slab_cells=eng._GRID_SLAB, workspace=eng._grid_ws)
graph.replay()
torch.cuda.synchronize()
same_graph = bool(torch.equal(ref[0], captured[0]) and torch.equal(ref[1], captured[1]) and int(captured[2]) == int(ref[1].sum()))

cells = args.res ** 3
slabs = (cells + eng._GRID_SLAB - 1) // eng._GRID_SLAB
out = {"tool": "time_part3_grid_update", "grid": f"{args.res}^3", "cells": cells, "slab_cells": eng._GRID_SLAB, "slabs": slabs,
       "times": args.times, "enqueues_per_chain_refresh": 3 * args.times * slabs + 1, "decay": 1.0, "active_ratio": round(ratio, 4),
       "table": str(table.dtype).replace("torch.", ""), "refreshes_per_window": args.refreshes, "windows": args.windows,
       "chain_equals_loop": same, "graph_equals_loop": same_graph, "workspace_bytes": eng._grid_ws.numel()}
report(args, out, loop, chain, graph.replay)
