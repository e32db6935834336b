"""tools/solve_bench.py -- GPU: shifted systems by multi-shift CG (lzx_solve_shifted_f64, Engine.solve_shifted / katz) on BASELINE's
C2 and C3 graphs (bench.WORKLOADS, imported), in one process:

  - the lazy Lanczos loop's iteration rate (lzx_lanczos_f64, k = 50) next to a seed-only CG iteration on the same graph;
  - ns = 1, 4, 8, 16 shifts, every one kept live (tol 1e-300, a fixed number of iterations): per-iteration device time of the
    SpMV and of the two vector kernels, and the vector kernels' bytes over their time against the byte model;
  - Katz for four alpha in {0.5, 0.7, 0.85, 0.95} / lambda_max, tol 1e-10: one multi-shift call against four single-shift calls;
  - on C2 only, the route a user has without it: scipy cg over Engine.spmv (S x = x / alpha - A x), alpha = 0.85 / lambda_max.

Byte model of the vector kernels per iteration, per row of n_loc_pad: k_cg_update<false> reads p, w, r, x_0
and writes r, x_0 (48 B); k_cg_direction<false> reads r, p and writes p (24 B), and reads and writes x_s, p_s of every live shift
other than the seed (32 B each): 8 (9 + 4 (ns - 1)) B per row.

    python tools/solve_bench.py [--workloads c2,c3] [--iters 40] [--out FILE] [--no-scipy]
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


def vec_bytes(rows, ns):
    return 8.0 * rows * (9 + 4 * (ns - 1))


def fixed_iterations(eng, lam, ns, iters):
    """ns shifts lambda (1.01 + 0.01 i), none of which meets tol 1e-300 in a few dozen iterations: exactly `iters` iterations
    with every shift live"""
    pkg = ge.load_pkg()
    shifts = lam * (1.01 + 0.01 * np.arange(ns))
    try:
        eng.solve_shifted(np.ones(eng.n), shifts, tol=1e-300, maxiter=iters)
        raise RuntimeError("a shift met tol 1e-300")
    except pkg.LzxError as e:
        _, info = e.partial
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scipy", action="store_true")
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
        lam = float(eng.eigsh(nev=1, which="LA", tol=1e-10, want_vectors=False)[0][0])
        ones = np.ones(n)
        k = 50
        eng.lanczos(ones, k, want_q=False)                                # warm-up
        st = eng.lanczos(ones, k, want_q=False)[4]
        lz_ms = st["loop_ms"] / k
        emit(workload=name, case="lanczos k=50", ms_per_iter=round(lz_ms, 4), iters_per_s=round(1e3 / lz_ms, 1),
             spmv_ms_per_iter=round(st["spmv_ms"] / k, 4), lambda_max=lam)
        fixed_iterations(eng, lam, 1, 20)                                 # warm-up
        base = None
        for ns in (1, 4, 8, 16):
            info = fixed_iterations(eng, lam, ns, args.iters)
            it = info["launched"]
            per = (info["spmv_ms"] + info["vec_ms"]) / it
            vb = vec_bytes(rows_pad, ns)
            row = dict(workload=name, case=f"cg ns={ns}", iterations=it, ms_per_iter=round(per, 4),
                       wall_ms_per_iter=round(info["loop_ms"] / it, 4), iters_per_s=round(1e3 / per, 1),
                       spmv_ms_per_iter=round(info["spmv_ms"] / it, 4), vec_ms_per_iter=round(info["vec_ms"] / it, 4),
                       vec_mb_model=round(vb / 1e6, 1), vec_tbs=round(vb / (info["vec_ms"] / it * 1e-3) / 1e12, 3),
                       vec_frac_8tbs=round(vb / (info["vec_ms"] / it * 1e-3) / 8e12, 3))
            if ns == 1:
                base = per
                row["vs_lanczos"] = round(per / lz_ms, 3)
            else:
                row["vs_ns1"] = round(per / base, 3)
            emit(**row)
        alphas = np.array([0.5, 0.7, 0.85, 0.95]) / lam
        eng.katz(list(alphas))                                            # warm-up
        t0 = time.perf_counter()
        X = eng.katz(list(alphas))
        one = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        Xs = [eng.katz(a) for a in alphas]
        four = (time.perf_counter() - t0) * 1e3
        _, info = eng.solve_shifted(ones, 1.0 / alphas)
        emit(workload=name, case="katz 4 alpha", one_call_ms=round(one, 2), four_calls_ms=round(four, 2), iterations=info["iterations"],
             iters=[int(i) for i in info["iters"]], max_resid=float(info["resid"].max()),
             max_diff_vs_single=float(max(np.abs(X[i] - Xs[i]).max() for i in range(4))))
        if name == "c2" and not args.no_scipy:
            from scipy.sparse.linalg import LinearOperator, cg
            a = 0.85 / lam
            calls = [0]

            def mv(x):
                calls[0] += 1
                x = np.ascontiguousarray(x.ravel())
                return x / a - eng.spmv(x)
            op = LinearOperator((n, n), matvec=mv, dtype=np.float64)
            t0 = time.perf_counter()
            x, rc = cg(op, ones, rtol=1e-10, maxiter=1000)
            wall = (time.perf_counter() - t0) * 1e3
            xd, info = eng.solve_shifted(ones, 1.0 / a)
            t0 = time.perf_counter()
            eng.solve_shifted(ones, 1.0 / a)
            dev = (time.perf_counter() - t0) * 1e3
            emit(workload=name, case="scipy cg + Engine.spmv, alpha=0.85/lambda", wall_ms=round(wall, 2), matvecs=calls[0], rc=int(rc),
                 device_ms=round(dev, 2), device_iters=int(info["iters"][0]),
                 rel_diff=float(np.linalg.norm(x - xd) / np.linalg.norm(xd)))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
