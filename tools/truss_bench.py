"""tools/truss_bench.py -- GPU: edge support and truss numbers (lzx_truss; Engine.truss_raw) on BASELINE's C2 and C3 graphs
(bench.WORKLOADS, imported), in one process:

  - truss_raw(): support_ms (orientation, edge ids and the support count) and peel_ms (the peeling loop, the host's reads per
    round included), each by one device event pair, best of three after a warm-up, with rounds, levels, the largest truss
    number and the main truss's edges, next to lzx_bench_spmv of the same handle; the whole call with all four vectors
    crossing PCIe and with the counts only.

Every GPU step runs under a time limit of its own: a watchdog ends the process (exit status 124) when a step overruns it, and an
exception in a step ends the tool there, so nothing further is started on the device after a failure.

    python tools/truss_bench.py [--workloads c2,c3] [--out FILE] [--step-limit SECONDS]
"""
import argparse
import contextlib
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from bench import WORKLOADS  # noqa: E402


@contextlib.contextmanager
def limit(seconds, what):
    """one GPU step: past `seconds` the process ends at once with status 124 (a step that hangs never reaches the next)"""
    def overrun():
        print(f"truss_bench: {what} ran longer than {seconds} s -- ending here", file=sys.stderr, flush=True)
        os._exit(124)
    watchdog = threading.Timer(seconds, overrun)
    watchdog.daemon = True
    watchdog.start()
    try:
        yield
    finally:
        watchdog.cancel()


def generate(eng, name):
    _, kind, scale, n, draws, gseed, _ = WORKLOADS[name]
    if kind == "rmat":
        eng.gen_rmat(scale, n, draws, gseed)
    else:
        eng.gen_er(n, draws, gseed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds for each GPU step (the graph's generation: three times this)")
    args = ap.parse_args()
    pkg = ge.load_pkg()
    rows = []
    ints = ("edges", "triangles", "main_truss_edges", "max_support", "max_truss", "levels", "rounds")

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
        with limit(args.step_limit, f"{name}: the warm-up call"):
            warm = eng.truss_raw(False, False, False, False)[4]
        print(f"{name}: warm-up support_ms={warm['support_ms']:.3f} peel_ms={warm['peel_ms']:.3f} rounds={warm['rounds']}", flush=True)
        with limit(args.step_limit, f"{name}: three calls with all four vectors"):
            full = [eng.truss_raw()[4] for _ in range(3)]
        with limit(args.step_limit, f"{name}: three calls, counts only"):
            counts = [eng.truss_raw(False, False, False, False)[4] for _ in range(3)]
        assert all(i[key] == warm[key] for i in full + counts for key in ints)
        best = min(full + counts, key=lambda i: i["peel_ms"])
        support_ms = min(i["support_ms"] for i in full + counts)
        emit(workload=name, case="truss", n=gi["n"], nnz=gi["nnz"], support_ms=round(support_ms, 4), peel_ms=round(best["peel_ms"], 4),
             **{key: int(warm[key]) for key in ints}, spmv_ms=round(spmv_min, 4), spmv_avg_ms=round(spmv_avg, 4),
             support_vs_spmv=round(support_ms / spmv_min, 2), peel_vs_spmv=round(best["peel_ms"] / spmv_min, 2),
             peel_us_per_round=round(1e3 * best["peel_ms"] / max(int(best["rounds"]), 1), 2),
             call_ms_with_vectors=round(min(i["loop_ms"] for i in full), 3), call_ms_counts_only=round(min(i["loop_ms"] for i in counts), 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
