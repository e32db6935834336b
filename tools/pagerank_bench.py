"""tools/pagerank_bench.py -- GPU: PageRank by multi-shift CG in the degree inner product (lzx_pagerank_f64, Engine.pagerank) on
BASELINE's C2 and C3 graphs (bench.WORKLOADS, imported), in one process:

  - iterations to tol 1e-10 at damping 0.85, uniform teleport vector, and the call's wall time;
  - iterations of every damping of the grid 0.5, 0.6, 0.7, 0.8, 0.85, 0.9, 0.95, 0.99 in one call;
  - nd = 1, 4, 8, 16 dampings, every one kept live (tol 1e-300, a fixed number of iterations): per-iteration device time of the
    SpMV and of the two vector kernels, next to Engine.solve_shifted with the same number of shifts on the same graph (the
    two alternate --reps times; the median run of each is reported, with the largest max / min over the repeats);
  - that ratio next to the one the byte model predicts.

Byte model per iteration and row of n_loc_pad (DESIGN.md sections 13 and 15): the shifted solver's vector kernels move
8 (9 + 4 (ns - 1)) B; PageRank's read one 4-byte degree more in each of the two kernels: + 8 B.  The SpMV is the same launch in
both, so the predicted ratio of a whole iteration is (spmv + vec * (bytes + 8 rows) / bytes) / (spmv + vec) with the solver's
measured spmv and vec times.

    python tools/pagerank_bench.py [--workloads c2,c3] [--iters 40] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from bench import WORKLOADS  # noqa: E402

GRID = [0.5, 0.6, 0.7, 0.8, 0.85, 0.9, 0.95, 0.99]


def solver_vec_bytes(rows, ns):
    return 8.0 * rows * (9 + 4 * (ns - 1))


def total(info):
    """device event time of a run's SpMVs and vector kernels"""
    return info["spmv_ms"] + info["vec_ms"]


def partial_info(pkg, call):
    """info of a call that is meant to run out of maxiter with everything live"""
    try:
        call()
        raise RuntimeError("tol 1e-300 was met")
    except pkg.LzxError as e:
        return e.partial[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = ge.load_pkg()
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    for name in args.workloads.split(","):
        desc, kind, scale, n, draws, gseed, _ = WORKLOADS[name]
        eng = pkg.Engine(0)
        t0 = time.perf_counter()
        if kind == "rmat":
            eng.gen_rmat(scale, n, draws, gseed)
        else:
            eng.gen_er(n, draws, gseed)
        gi = eng.info()
        rows_pad = -(-gi["rows_local"] // 64) * 64
        print(f"{name}: n={n:,} nnz={gi['nnz']:,} (graph {time.perf_counter() - t0:.1f} s)", flush=True)
        eng.pagerank([0.85], tol=1e-10)                                   # warm-up (builds the degree array)
        t0 = time.perf_counter()
        _, info = eng.pagerank([0.85], tol=1e-10)
        emit(workload=name, case="pagerank 0.85, tol 1e-10", iterations=int(info["iters"][0]), launched=info["launched"],
             wall_ms=round((time.perf_counter() - t0) * 1e3, 2), resid=float(info["resid"][0]))
        t0 = time.perf_counter()
        _, info = eng.pagerank(GRID, tol=1e-10)
        emit(workload=name, case="pagerank grid, tol 1e-10", dampings=GRID, iters=[int(i) for i in info["iters"]],
             wall_ms=round((time.perf_counter() - t0) * 1e3, 2), max_resid=float(info["resid"].max()))
        lam = float(eng.eigsh(nev=1, which="LA", tol=1e-10, want_vectors=False)[0][0])
        ones = np.ones(n)
        for ns in (1, 4, 8, 16):
            dampings = 0.99 - 0.01 * np.arange(ns)
            shifts = lam * (1.01 + 0.01 * np.arange(ns))
            partial_info(pkg, lambda: eng.pagerank(dampings, tol=1e-300, maxiter=8))                        # warm-up
            partial_info(pkg, lambda: eng.solve_shifted(ones, shifts, tol=1e-300, maxiter=8))
            prs, svs = [], []
            for _ in range(args.reps):                                    # alternating, the median run of each is reported
                prs.append(partial_info(pkg, lambda: eng.pagerank(dampings, tol=1e-300, maxiter=args.iters)))
                svs.append(partial_info(pkg, lambda: eng.solve_shifted(ones, shifts, tol=1e-300, maxiter=args.iters)))
            pr, sv = sorted(prs, key=total)[len(prs) // 2], sorted(svs, key=total)[len(svs) // 2]
            it_p, it_s = pr["launched"], sv["launched"]
            per_p, per_s = total(pr) / it_p, total(sv) / it_s
            spread = max(max(map(total, prs)) / min(map(total, prs)), max(map(total, svs)) / min(map(total, svs)))
            vb = solver_vec_bytes(rows_pad, ns)
            byte_ratio = (vb + 8.0 * rows_pad) / vb
            predicted = (sv["spmv_ms"] + sv["vec_ms"] * byte_ratio) / (sv["spmv_ms"] + sv["vec_ms"])
            emit(workload=name, case=f"nd = ns = {ns}", iterations=it_p,
                 pagerank_ms_per_iter=round(per_p, 4), pagerank_spmv_ms=round(pr["spmv_ms"] / it_p, 4), pagerank_vec_ms=round(pr["vec_ms"] / it_p, 4),
                 pagerank_loop_ms=round(pr["loop_ms"], 3), solver_loop_ms=round(sv["loop_ms"], 3),
                 solver_ms_per_iter=round(per_s, 4), solver_spmv_ms=round(sv["spmv_ms"] / it_s, 4), solver_vec_ms=round(sv["vec_ms"] / it_s, 4),
                 spread_max_over_min=round(spread, 3), ratio=round(per_p / per_s, 3), ratio_predicted=round(predicted, 3),
                 vec_ratio=round((pr["vec_ms"] / it_p) / (sv["vec_ms"] / it_s), 3), vec_ratio_predicted=round(byte_ratio, 3),
                 pagerank_vec_tbs=round((vb + 8.0 * rows_pad) / (pr["vec_ms"] / it_p * 1e-3) / 1e12, 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
