"""tools/triangles_bench.py -- GPU: triangle counts and clustering (lzx_triangles; Engine.triangles_raw / transitivity) on
BASELINE's C2 and C3 graphs (bench.WORKLOADS, imported), in one process:

  - triangles_raw(): orient_ms (degrees, out-counts, scan and fill of the oriented copy) and count_ms (the counting launches)
    by device events, best of five after a warm-up, T, the transitivity, the average clustering, the entries and the longest
    list of the oriented copy, next to lzx_bench_spmv of the same handle; the whole call with both vectors crossing PCIe and
    with the counts only;
  - on C2 only, the route a user has without it: get_graph_csr() over PCIe and scipy's (A @ A).multiply(A) on the host
    (networkx is out of reach at this size).  --no-scipy leaves it out: A @ A of a 1 M-vertex R-MAT graph needs tens of GB.

    python tools/triangles_bench.py [--workloads c2,c3] [--out FILE] [--no-scipy]
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
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_pkg()
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    for name in args.workloads.split(","):
        eng = pkg.Engine(0)
        t0 = time.perf_counter()
        generate(eng, name)
        handover_s = time.perf_counter() - t0
        gi = eng.info()
        print(f"{name}: n={gi['n']:,} nnz={gi['nnz']:,} (graph {handover_s:.1f} s)", flush=True)
        eng.bench_spmv(5)
        spmv_avg, spmv_min = eng.bench_spmv(20)
        eng.triangles_raw(want_triangles=False, want_clustering=False)        # warm-up
        best = None
        for _ in range(5):
            tri, clus, info = eng.triangles_raw()
            if best is None or info["orient_ms"] + info["count_ms"] < best["orient_ms"] + best["count_ms"]:
                best = info
        counts = min((eng.triangles_raw(want_triangles=False, want_clustering=False)[2] for _ in range(5)), key=lambda i: i["loop_ms"])
        T, wedges = int(best["triangles"]), int(best["wedges"])
        emit(workload=name, case="triangles", triangles=T, wedges=wedges, transitivity=0.0 if T == 0 else (6 * T) / (2 * wedges),
             avg_clustering=best["avg_clustering"], max_triangles=int(best["max_triangles"]), oriented_entries=int(best["oriented_entries"]),
             oriented_max_degree=int(best["oriented_max_degree"]), orient_ms=round(best["orient_ms"], 4), count_ms=round(best["count_ms"], 4),
             spmv_ms=round(spmv_min, 4), spmv_avg_ms=round(spmv_avg, 4), count_vs_spmv=round(best["count_ms"] / spmv_min, 2),
             call_ms_with_vectors=round(best["loop_ms"], 3), call_ms_counts_only=round(counts["loop_ms"], 3))
        if name == "c2" and not args.no_scipy:
            import scipy.sparse as sp
            t0 = time.perf_counter()
            rp, ci = eng.get_graph_csr()
            fetch = (time.perf_counter() - t0) * 1e3
            A = sp.csr_matrix((np.ones(len(ci), dtype=np.int64), ci.astype(np.int64), rp.astype(np.int64)), shape=(gi["n"], gi["n"]))
            A.setdiag(0)
            A.eliminate_zeros()
            t_host = np.asarray((A @ A).multiply(A).sum(axis=1)).ravel() // 2
            wall = (time.perf_counter() - t0) * 1e3
            emit(workload=name, case="get_graph_csr + scipy (A @ A).multiply(A)", wall_ms=round(wall, 2), of_which_fetch_ms=round(fetch, 2),
                 equal=bool(np.array_equal(t_host.astype(np.uint64), tri)), device_call_ms=round(best["loop_ms"], 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
