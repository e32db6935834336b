"""tools/sweep_bench.py -- GPU: sweep cuts (lzx_sweep_cut; Engine.sweep_cut_raw / spectral_bisection) on BASELINE's C2 and C3
graphs (bench.WORKLOADS, imported), in one process:

  - sweep_cut_raw() of ns = 1, 4 and 16 random score vectors, nothing but the best prefixes crossing back: sort_ms (uploads,
    keys, radix sorts and positions of the ns columns), sweep_ms (the one pass over the edges) and scan_ms (2 ns inclusive sums
    and the reduction) by the call's device events, the median of three calls after a warm-up;
  - beside the edge sweep, on the same handle: lzx_bench_spmv, and the batched path's SpMM of the same width.  lzx_spmm_f64
    itself crosses PCIe with ns n values each way, so its launches are timed by the device events of a basis-free Lanczos run
    of ns probes (stats spmv_ms_min), as tools/paths_bench.py does.  Per entry the sweep gathers 4 B bytes where the SpMM
    gathers 8 B;
  - the whole spectral_bisection() of the giant component (largest_component(): built on the device), with lambda_2, the
    restarts, the size and the conductance of the cut.

Every GPU step runs under a time limit of its own: a watchdog ends the process (exit status 124) when a step overruns it, and an
exception in a step ends the tool there, so nothing further is started on the device after a failure.

    python tools/sweep_bench.py [--workloads c2,c3] [--out FILE] [--step-limit SECONDS] [--tol TOL] [--m M] [--max-restarts R]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from communities_bench import generate, limit  # noqa: E402

WIDTHS = (1, 4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds for each GPU step (the graph's generation and the bisection: three times this)")
    ap.add_argument("--tol", type=float, default=1e-6, help="eigsh's tolerance in spectral_bisection")
    ap.add_argument("--m", type=int, default=48, help="eigsh's basis size in spectral_bisection")
    ap.add_argument("--max-restarts", type=int, default=600)
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
        n = gi["n"]
        print(f"{name}: n={n:,} nnz={gi['nnz']:,} (graph {handover_s:.1f} s)", flush=True)
        with limit(args.step_limit, f"{name}: lzx_bench_spmv"):
            eng.bench_spmv(5)
            spmv_min = eng.bench_spmv(20)[1]
        rng = np.random.default_rng(17)
        for ns in WIDTHS:
            S = rng.standard_normal((ns, n))
            with limit(args.step_limit, f"{name}: the sweep of {ns} columns, warm-up and three calls, and the SpMM of that width"):
                warm = eng.sweep_cut_raw(S, want_order=False)
                calls = [eng.sweep_cut_raw(S, want_order=False) for _ in range(3)]
                spmm = statistics.median(eng.lanczos_probes(7, 0, ns, 5)[3]["spmv_ms_min"] for _ in range(3))
            assert all(c[3] == warm[3] for c in calls)
            med = lambda key: statistics.median(c[4][key] for c in calls)
            best = warm[3][0]
            emit(workload=name, case="sweep_cut", n=n, nnz=gi["nnz"], ns=ns, width=int(warm[4]["width"]), entries=int(warm[4]["entries"]),
                 sort_ms=round(med("sort_ms"), 3), sort_ms_per_column=round(med("sort_ms") / ns, 3), sweep_ms=round(med("sweep_ms"), 3),
                 scan_ms=round(med("scan_ms"), 3), call_ms=round(med("loop_ms"), 3), spmv_ms=round(spmv_min, 4), spmm_ms=round(spmm, 4),
                 sweep_vs_spmv=round(med("sweep_ms") / spmv_min, 2), sweep_vs_spmm=round(med("sweep_ms") / spmm, 2),
                 best_k=int(best["k"]), best_value=best["value"])
        with limit(3 * args.step_limit, f"{name}: the giant component and its spectral bisection"):
            t0 = time.perf_counter()
            sub, old = eng.largest_component()
            giant_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            try:
                members, value, lambda2, info = sub.spectral_bisection(tol=args.tol, m=args.m, max_restarts=args.max_restarts)
            except pkg.LzxError as e:   # eigsh ran out of restarts: reported, not hidden
                if "(-6)" not in str(e):
                    raise
                emit(workload=name, case="spectral_bisection", giant_n=int(sub.n), tol=args.tol, error=str(e), seconds=round(time.perf_counter() - t0, 3))
                sub.close()
                eng.close()
                continue
            bisect_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            check = sub.conductance(members)
            set_s = time.perf_counter() - t0
        assert check == value
        emit(workload=name, case="spectral_bisection", giant_n=int(sub.n), giant_nnz=int(sub.info()["nnz"]), giant_s=round(giant_s, 3), tol=args.tol, m=args.m,
             lambda2=lambda2, restarts=int(info["restarts"]), matvecs=int(info["matvecs"]), eigsh_ms=round(info["loop_ms"], 1),
             bisection_s=round(bisect_s, 3), members=int(len(members)), cut=int(info["sweep"]["cut"]), den=int(info["sweep"]["den"]),
             conductance=value, conductance_call_s=round(set_s, 3))
        sub.close()
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
