"""Time of one occupancy-grid refresh of the Part 4 dual-hash field: DualHashEngine.update_grid()'s loop (lattice tensor, three time
anchors x eight 2^18-point batches through the whole forward_chain -- all three deformation gathers, the deformation chain, the
canonical gather, the whole canonical decoder on zero directions -- torch.maximum per batch, nerf_grid_update) against the
density-only launch chain (update_grid(chain=True): nerf_p4_grid_update, one kept 36.7 MB workspace) and against that chain replayed
from a torch.cuda.graph capture -- one process, same engine.  Engine at configs/part4.yaml.example with the four tables set to
0.5 sin(0.37 i + k + 0.11 (i mod 7)), seeded normal networks (density row x 8, displacement_scale 0.1), 128^3 grid, threshold = the
median of the field's own folded sigma (half of the cells active).  Every refresh starts from a history that has converged to that
sigma, so each leg does the same work every time.  The loop and chain legs include their one host read of the count; the graph replay
has none.  5 warm-up refreshes per leg, five interleaved windows of 20 refreshes, a host clock around a final device synchronise;
median and min-max of the windows.  Prints one JSON line and writes it to profiles/part4_grid_update_timing.json.  The measuring runs
in a child process under `timeout`; this process never opens the GPU.
    python tools/time_part4_grid_update.py [--refreshes N] [--windows W] [--res R] [--limit SECONDS] [--legs loop,chain,graph]"""
import os, sys

from grid_update_timing import ROOT, report, start

args = start(__file__, "part4_grid_update", 300)

import torch
import yaml
sys.path.insert(0, ROOT)
from project_nerf_amd import ops
from project_nerf_amd.part4 import DualHashEngine, S2, SCALE

dev = "cuda"
torch.manual_seed(0)
cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part4.yaml.example")))
cfg["grid_resolution"] = args.res
eng = DualHashEngine(cfg, device=dev)
with torch.no_grad():
    for k in range(4):
        i = torch.arange(eng.table(k).numel(), dtype=torch.float64, device=dev)
        eng.table(k).copy_((0.5 * torch.sin(0.37 * i + float((k + 1) % 4) + 0.11 * (i % 7))).float())
        del i
    eng.net.copy_((torch.randn(eng.net.numel(), generator=torch.Generator().manual_seed(5)) * 0.15).to(dev))
    eng.net[S2:S2 + 64] *= 8.0
    eng.net[SCALE] = 0.1
eng.repack()
eng.update_grid(decay=1.0)
eng.grid_threshold = float(eng.grid.median())
DECAY = float(cfg.get("grid_decay", 0.95))

loop = lambda: eng.update_grid(decay=DECAY)
chain = lambda: eng.update_grid(decay=DECAY, chain=True)
start = eng.grid.clone()                                  # the converged history: max(start * decay, sigma) = sigma = start
ratio = loop()
ref = (eng.grid.clone(), eng.binary_grid.clone())
eng.grid = start.clone()
ratio_chain = chain()
same = bool(torch.equal(ref[0], eng.grid) and torch.equal(ref[1], eng.binary_grid) and ratio == ratio_chain and torch.equal(ref[0], start))

# third leg: the chain captured once and replayed (a linear graph on one stream, no host read)
tables = eng._tables_for_forward()
hist = start.clone()
graph = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with torch.cuda.graph(graph):
    captured = ops.p4_grid_update(eng.packed, eng.net, tables, eng.levels_d, eng.levels_c, eng.bound, args.res, eng.grid_bound,
                                  eng.grid_threshold, hist, DECAY, slab_cells=eng._GRID_SLAB, workspace=eng._grid_ws)
graph.replay()
torch.cuda.synchronize()
same_graph = bool(torch.equal(ref[0], captured[0]) and torch.equal(ref[1], captured[1]) and int(captured[2]) == int(ref[1].sum()))

cells = args.res ** 3
out = {"tool": "time_part4_grid_update", "grid": f"{args.res}^3", "cells": cells, "slab_cells": eng._GRID_SLAB,
       "slabs": (cells + eng._GRID_SLAB - 1) // eng._GRID_SLAB, "anchors": 3, "decay": DECAY, "active_ratio": round(ratio, 4),
       "tables": str(tables[0].dtype).replace("torch.", ""), "refreshes_per_window": args.refreshes, "windows": args.windows,
       "chain_equals_loop": same, "graph_equals_loop": same_graph, "workspace_bytes": eng._grid_ws.numel(),
       "loop_workspace_bytes_per_batch": ops._lib.load().nerf_p4_infer_workspace_bytes(min(cells, 2 ** 18))}
report(args, out, loop, chain, graph.replay)
