"""Iterations per second under both operators (option "operator"): adjacency and the Laplacian L = D - A, on BASELINE C2
and C3 at k = 50 with the single-vector loop (the form one GPU takes by default: the lazy loop in blocked mode), and on C2
with the batched path at b = 16 (vector-iterations per second).

    python tools/operator_bench.py [--workloads c2,c3] [--k 50] [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from bench import WORKLOADS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    pkg = ge.load_pkg()
    for w in args.workloads.split(","):
        _, kind, scale, n, draws, seed, _ = WORKLOADS[w]
        eng = pkg.Engine(0)
        if kind == "rmat":
            eng.gen_rmat(scale, n, draws, seed)
        else:
            eng.gen_er(n, draws, seed)
        x0 = np.random.default_rng(1).standard_normal(n)
        row = {"workload": w, "n": n, "k": args.k}
        for name, op in (("adjacency", 0), ("laplacian", 1)):
            eng.set_option("operator", op)
            eng.lanczos(x0, args.k, want_q=False)   # warm-up (and the degree array under L)
            best = None
            for _ in range(args.reps):
                st = eng.lanczos(x0, args.k, want_q=False)[4]
                best = st["loop_ms"] if best is None else min(best, st["loop_ms"])
            row[f"{name}_ms_per_iter"] = best / args.k
            row[f"{name}_iter_per_s"] = 1e3 * args.k / best
        row["laplacian_over_adjacency"] = row["laplacian_ms_per_iter"] / row["adjacency_ms_per_iter"]
        if w == "c2":
            X = np.random.default_rng(2).standard_normal((16, n))
            for name, op in (("adjacency", 0), ("laplacian", 1)):
                eng.set_option("operator", op)
                eng.lanczos_multi(X, args.k)
                best = min(eng.lanczos_multi(X, args.k)[5]["loop_ms"] for _ in range(args.reps))
                row[f"batched16_{name}_vec_iter_per_s"] = 16e3 * args.k / best
            eng.multi_release()
        print(json.dumps(row), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
