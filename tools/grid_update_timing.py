"""What tools/time_instant_grid_update.py, time_part4_grid_update.py and time_part3_grid_update.py share: the command line, the parent
that starts the measuring child under `timeout` and never opens the GPU, and the measurement itself -- 5 warm-up refreshes per leg,
interleaved windows, a host clock around a final device synchronise, median and min-max of the windows, the two verdicts.  Each tool
keeps its engine set-up, its three legs and its own JSON fields."""
import argparse, json, os, statistics, subprocess, sys, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def start(script, name, limit, add_arguments=None):
    """The parsed command line -- in the measuring child.  In the parent: run ``script`` again as the child under `timeout`, write its
    last JSON line to profiles/<name>_timing.json, print it and exit."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--refreshes", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--res", type=int, default=128)
    if add_arguments is not None:
        add_arguments(ap)
    ap.add_argument("--limit", type=int, default=limit, help="seconds the measuring child may take")
    ap.add_argument("--legs", default="loop,chain,graph", help="legs to time (a profiler run of the child takes one: --child --legs chain)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return args
    r = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(script), "--child"] + sys.argv[1:],
                       capture_output=True, text=True)
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        sys.exit(f"the measuring process ended with status {r.returncode}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    json.loads(line)
    with open(os.path.join(ROOT, "profiles", f"{name}_timing.json"), "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
    sys.exit(0)


def timed(fn, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def report(args, out, loop, chain, replay):
    """Time the legs named in ``args.legs``, add their figures and the two verdicts to ``out`` (the tool's own fields) and print it
    as one JSON line."""
    legs = [(name, fn) for name, fn in (("loop", loop), ("chain", chain), ("graph", replay)) if name in args.legs.split(",")]
    ms = {name: [] for name, _ in legs}
    for name, fn in legs:
        timed(fn, 5)                                         # warm-up: allocations, code objects, clocks
    for _ in range(args.windows):
        for name, fn in legs:
            ms[name].append(timed(fn, args.refreshes))
    for name in ms:
        out[name] = {"median_ms": round(statistics.median(ms[name]), 4), "min_ms": round(min(ms[name]), 4), "max_ms": round(max(ms[name]), 4)}
    if "loop" in ms and "chain" in ms:
        out["chain_median_below_loop_min"] = bool(out["chain"]["median_ms"] < out["loop"]["min_ms"])
    if "chain" in ms and "graph" in ms:
        out["graph_not_above_chain_max"] = bool(out["graph"]["median_ms"] <= out["chain"]["max_ms"])
    print(json.dumps(out), flush=True)
