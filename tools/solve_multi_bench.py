"""tools/solve_multi_bench.py -- GPU: many right-hand sides by a batch of independent CG solves (lzx_solve_multi_f64,
Engine.solve_multi) on BASELINE's C2 and C3 graphs (bench.WORKLOADS, imported), in one process:

  - nb = 1, 2, 4, 8, 16 right-hand sides, every column kept live (tol 1e-300, a fixed number of iterations): per-iteration device
    event time of the SpMM and of the two vector kernels;
  - next to it nb x the per-iteration time of Engine.solve_shifted with one shift on the same graph, i.e. what nb separate
    solves cost today (the two alternate --reps times; the median run of each is reported, with the largest max / min over
    the repeats);
  - the byte model of DESIGN.md section 16 and the rates it implies.

Byte model per iteration: the SpMM reads col_idx once and the row pointers of the work list, gathers and writes 8 bytes per row
and column, 4 nnz + 8 (n + 1) + 16 nb n; the two vector kernels move 48 + 24 = 72 bytes per row and padded column, 72 B n.

    python tools/solve_multi_bench.py [--workloads c2,c3] [--iters 40] [--reps 3] [--out FILE]
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


def total(info):
    """device event time of a run's SpMMs / SpMVs and vector kernels"""
    return info["spmv_ms"] + info["vec_ms"]


def partial_info(pkg, call):
    """info of a call that is meant to run out of maxiter with everything live"""
    try:
        call()
        raise RuntimeError("tol 1e-300 was met")
    except pkg.LzxError as e:
        return e.partial[1]


def pad_width(nb):
    return 2 if nb <= 2 else 4 if nb <= 4 else 8 if nb <= 8 else 16


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
        nnz = eng.info()["nnz"]
        print(f"{name}: n={n:,} nnz={nnz:,} (graph {time.perf_counter() - t0:.1f} s)", flush=True)
        lam = float(eng.eigsh(nev=1, which="LA", tol=1e-10, want_vectors=False)[0][0])
        rng = np.random.default_rng(1)
        b1 = rng.standard_normal(n)
        partial_info(pkg, lambda: eng.solve_shifted(b1, 1.05 * lam, tol=1e-300, maxiter=8))       # warm-up
        for nb in (1, 2, 4, 8, 16):
            Bm = rng.standard_normal((nb, n))
            shifts = lam * (1.05 + 0.01 * np.arange(nb))
            partial_info(pkg, lambda: eng.solve_multi(Bm, shifts, tol=1e-300, maxiter=8))        # warm-up
            ms, ss = [], []
            for _ in range(args.reps):                                    # alternating, the median run of each is reported
                ms.append(partial_info(pkg, lambda: eng.solve_multi(Bm, shifts, tol=1e-300, maxiter=args.iters)))
                ss.append(partial_info(pkg, lambda: eng.solve_shifted(b1, 1.05 * lam, tol=1e-300, maxiter=args.iters)))
            mi, si = sorted(ms, key=total)[len(ms) // 2], sorted(ss, key=total)[len(ss) // 2]
            it_m, it_s = mi["launched"], si["launched"]
            per_m, per_s = total(mi) / it_m, total(si) / it_s
            spread = max(max(map(total, ms)) / min(map(total, ms)), max(map(total, ss)) / min(map(total, ss)))
            B = pad_width(nb)
            spmm_bytes = 4.0 * nnz + 8.0 * (n + 1) + 16.0 * nb * n
            vec_bytes = 72.0 * B * n
            emit(workload=name, case=f"nb = {nb} (B = {B})", iterations=it_m,
                 multi_ms_per_iter=round(per_m, 4), multi_spmm_ms=round(mi["spmv_ms"] / it_m, 4), multi_vec_ms=round(mi["vec_ms"] / it_m, 4),
                 multi_loop_ms=round(mi["loop_ms"], 3), single_loop_ms=round(si["loop_ms"], 3),
                 single_ms_per_iter=round(per_s, 4), nb_singles_ms_per_iter=round(nb * per_s, 4),
                 speedup_over_nb_singles=round(nb * per_s / per_m, 3), spread_max_over_min=round(spread, 3),
                 spmm_model_mb=round(spmm_bytes / 1e6, 1), spmm_tbs=round(spmm_bytes / (mi["spmv_ms"] / it_m * 1e-3) / 1e12, 3),
                 vec_model_mb=round(vec_bytes / 1e6, 1), vec_tbs=round(vec_bytes / (mi["vec_ms"] / it_m * 1e-3) / 1e12, 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
