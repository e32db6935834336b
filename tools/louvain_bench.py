"""tools/louvain_bench.py -- GPU: Louvain communities (lzx_louvain; Engine.louvain_raw) on BASELINE's C2 and C3 graphs
(bench.WORKLOADS, imported) and on the stochastic block model of tools/communities_bench.py (64 blocks of 4 096), in one process:

  - louvain_raw(): the counted levels, the nodes, entries, colours, sweeps and moves of each, the milliseconds per sweep of the
    whole call next to lzx_bench_spmv of the same handle, color_ms, sweep_ms and aggregate_ms, the communities, the largest one
    and Q;
  - label_propagation_raw() of the same handle beside it: its communities and Q.

Every GPU step runs under a time limit of its own: a watchdog ends the process (exit status 124) when a step overruns it, and an
exception in a step ends the tool there, so nothing further is started on the device after a failure.

    python tools/louvain_bench.py [--workloads c2,c3,sbm] [--out FILE] [--step-limit SECONDS] [--max-sweeps N] [--max-levels N]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from communities_bench import generate, limit, ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3,sbm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds for each GPU step (the graph's generation: three times this)")
    ap.add_argument("--max-sweeps", type=int, default=100)
    ap.add_argument("--max-levels", type=int, default=32)
    args = ap.parse_args()
    pkg = ge.load_pkg()
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    for name in args.workloads.split(","):
        with limit(3 * args.step_limit, f"{name}: the graph"):
            eng = pkg.Engine(0)
            t0 = time.perf_counter()
            generate(eng, name)
            handover_s = time.perf_counter() - t0
            gi = eng.info()
        print(f"{name}: n={gi['n']:,} nnz={gi['nnz']:,} (graph {handover_s:.1f} s)", flush=True)
        with limit(args.step_limit, f"{name}: lzx_bench_spmv"):
            eng.bench_spmv(5)
            spmv_avg, spmv_min = eng.bench_spmv(20)
        with limit(3 * args.step_limit, f"{name}: lzx_louvain"):
            _, _, levels, info = eng.louvain_raw(max_sweeps=args.max_sweeps, max_levels=args.max_levels, want_labels=False, want_level_labels=False)
        for l, rec in enumerate(levels):
            emit(workload=name, case="level", level=l, **{key: (value if key == "path_rows" else int(value)) for key, value in rec.items()})
        sweeps = max(int(info["sweeps"]), 1)
        emit(workload=name, case="louvain", n=gi["n"], nnz=gi["nnz"], levels=int(info["levels"]), nodes_per_level=[int(rec["nodes"]) for rec in levels],
             sweeps=int(info["sweeps"]), moves=int(info["moves"]), sweep_ms=round(info["sweep_ms"], 3), ms_per_sweep=round(info["sweep_ms"] / sweeps, 3),
             spmv_ms=round(spmv_min, 4), sweep_vs_spmv=round(info["sweep_ms"] / sweeps / spmv_min, 1), color_ms=round(info["color_ms"], 3),
             aggregate_ms=round(info["aggregate_ms"], 3), call_ms=round(info["loop_ms"], 3), communities=int(info["n_communities"]),
             largest_size=int(info["largest_size"]), modularity=info["modularity"])
        with limit(2 * args.step_limit, f"{name}: the propagation"):
            try:
                lpa = eng.label_propagation_raw(max_sweeps=args.max_sweeps, want_labels=False)[1]
            except pkg.LzxError as e:
                if "(-6)" not in str(e):
                    raise
                print(f"{name}: {e}", flush=True)
                lpa = None
        if lpa is not None:
            emit(workload=name, case="label_propagation", communities=int(lpa["n_communities"]), largest_size=int(lpa["largest_size"]),
                 modularity=lpa["modularity"], sweeps=int(lpa["sweeps"]), call_ms=round(lpa["loop_ms"], 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
