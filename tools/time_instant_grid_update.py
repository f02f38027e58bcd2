"""Time of one occupancy-grid refresh of the Instant-NGP field: InstantNgpEngine.update_grid()'s loop (lattice tensor, eight
2^18-point batches through the whole decoder with a fresh workspace each, nerf_grid_update) against the density-only launch chain
(update_grid(chain=True): nerf_instant_grid_update, one kept 16 MB operand image) and against that chain replayed from a
torch.cuda.graph capture -- one process, same engine.  Engine default-initialised at configs/part2_instant.yaml.example with the
table set to 0.5 sin(0.37 i + 0.11 (i mod 7)), 128^3 grid, threshold = the median of the field's own sigma (half of the cells
active).  The loop and chain legs include their one host read of the count; the graph replay has none.  5 warm-up refreshes per leg,
five interleaved windows of 20 refreshes, a host clock around a final device synchronise; median and min-max of the windows.
Prints one JSON line and writes it to profiles/instant_grid_update_timing.json.  The measuring runs in a child process under
`timeout`; this process never opens the GPU.
    python tools/time_instant_grid_update.py [--refreshes N] [--windows W] [--res R] [--limit SECONDS] [--legs loop,chain,graph]"""
import os, sys

from grid_update_timing import ROOT, report, start

args = start(__file__, "instant_grid_update", 240)

import torch
import yaml
sys.path.insert(0, ROOT)
from project_nerf_amd import ops
from project_nerf_amd.engine import InstantNgpEngine

dev = "cuda"
torch.manual_seed(0)
cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "part2_instant.yaml.example")))
cfg["grid_resolution"] = args.res
eng = InstantNgpEngine(cfg, device=dev)
with torch.no_grad():
    i = torch.arange(eng.table.numel(), dtype=torch.float64, device=dev)
    eng.table.copy_((0.5 * torch.sin(0.37 * i + 0.11 * (i % 7))).float())
    del i
eng.update_grid()
eng.grid_threshold = float(eng.grid.median())

loop = lambda: eng.update_grid()
chain = lambda: eng.update_grid(chain=True)
ratio = loop()
ref = (eng.grid.clone(), eng.binary_grid.clone())
ratio_chain = chain()
same = bool(torch.equal(ref[0], eng.grid) and torch.equal(ref[1], eng.binary_grid) and ratio == ratio_chain)

# third leg: the chain captured once and replayed (a linear graph on one stream, no host read)
table = eng._gather_table()
graph = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with torch.cuda.graph(graph):
    captured = ops.instant_grid_update(eng.packed, table, eng.levels, eng.bound, args.res, eng.bound, eng.grid_threshold,
                                       slab_cells=eng._GRID_SLAB, workspace=eng._grid_ws)
graph.replay()
torch.cuda.synchronize()
same_graph = bool(torch.equal(ref[0], captured[0]) and torch.equal(ref[1], captured[1]) and int(captured[2]) == int(ref[1].sum()))

cells = args.res ** 3
out = {"tool": "time_instant_grid_update", "grid": f"{args.res}^3", "cells": cells, "slab_cells": eng._GRID_SLAB,
       "slabs": (cells + eng._GRID_SLAB - 1) // eng._GRID_SLAB, "active_ratio": round(ratio, 4), "table": str(table.dtype).replace("torch.", ""),
       "refreshes_per_window": args.refreshes, "windows": args.windows, "chain_equals_loop": same, "graph_equals_loop": same_graph,
       "workspace_bytes": eng._grid_ws.numel(), "loop_workspace_bytes_per_batch": ops._lib.load().nerf_imlp_workspace_bytes(min(cells, 2 ** 18))}
report(args, out, loop, chain, graph.replay)
