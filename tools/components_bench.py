"""tools/components_bench.py -- GPU: connected components and the largest component's subgraph (lzx_components,
lzx_set_graph_induced; Engine.components / largest_component) on BASELINE's C2 and C3 graphs (bench.WORKLOADS, imported), in one
process:

  - components(): rounds, the device time of one edge sweep (sweep_ms / rounds) against the byte model and next to
    lzx_bench_spmv of the same graph with propagation_blocking off -- the same gather pattern, 8-byte values instead of 4-byte
    labels -- and next to the handle's own (blocked) SpMV; the whole call with and without the labels crossing PCIe;
  - largest_component(): the whole call, the hand-over of the subgraph included, next to handing the same subgraph over as a
    CSR from host memory;
  - on C2 only, the route a user has without it: get_graph_csr() over PCIe and scipy's connected_components on the host.

Byte model of one sweep: 4 nnz (col_idx) + 8 (n + 1) (row_ptr) + 4 nnz (one gathered label per entry)
+ 12 per row with an edge (its parent, grandparent and parent's parent).

    python tools/components_bench.py [--workloads c2,c3] [--out FILE] [--no-scipy]
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


def sweep_bytes(gi):
    return 8.0 * gi["nnz"] + 8.0 * (gi["n"] + 1) + 12.0 * gi["active_vertices"]


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
        plain = pkg.Engine(0, propagation_blocking=0)
        generate(plain, name)
        plain.bench_spmv(5)
        plain_avg, plain_min = plain.bench_spmv(20)
        plain.close()
        eng = pkg.Engine(0)
        t0 = time.perf_counter()
        generate(eng, name)
        handover_s = time.perf_counter() - t0
        gi = eng.info()
        print(f"{name}: n={gi['n']:,} nnz={gi['nnz']:,} (graph {handover_s:.1f} s)", flush=True)
        eng.bench_spmv(5)
        own_avg, own_min = eng.bench_spmv(20)
        eng.components()                                                   # warm-up
        best = None
        for _ in range(5):
            labels, info = eng.components()
            if best is None or info["sweep_ms"] < best["sweep_ms"]:
                best = info
        counts = min((eng.components(want_labels=False)[1] for _ in range(5)), key=lambda i: i["loop_ms"])
        per = best["sweep_ms"] / best["rounds"]
        model = sweep_bytes(gi)
        emit(workload=name, case="components", n_components=best["n_components"], largest_size=best["largest_size"],
             largest_label=best["largest_label"], rounds=best["rounds"], sweep_ms=round(best["sweep_ms"], 4),
             sweep_ms_per_round=round(per, 4), sweep_mb_model=round(model / 1e6, 1), sweep_tbs_model=round(model / (per * 1e-3) / 1e12, 3),
             spmv_plain_ms=round(plain_min, 4), spmv_plain_avg_ms=round(plain_avg, 4), sweep_vs_spmv_plain=round(per / plain_min, 3),
             spmv_own_ms=round(own_min, 4), call_ms_with_labels=round(best["loop_ms"], 3), call_ms_counts_only=round(counts["loop_ms"], 3))
        t0 = time.perf_counter()
        sub, old = eng.largest_component()
        whole = (time.perf_counter() - t0) * 1e3
        keep = labels == best["largest_label"]
        t0 = time.perf_counter()
        sub2, _ = eng.induced(keep)
        induce = (time.perf_counter() - t0) * 1e3
        rp, ci = sub.get_graph_csr()
        ref = pkg.Engine(0)
        t0 = time.perf_counter()
        ref.set_graph_csr(rp, ci)
        csr = (time.perf_counter() - t0) * 1e3
        emit(workload=name, case="largest_component", n=sub.n, nnz=sub.info()["nnz"], whole_call_ms=round(whole, 2),
             induced_ms=round(induce, 2), set_graph_csr_of_it_ms=round(csr, 2), generator_handover_ms=round(handover_s * 1e3, 2))
        for e in (sub, sub2, ref):
            e.close()
        if name == "c2" and not args.no_scipy:
            import scipy.sparse as sp
            import scipy.sparse.csgraph as csg
            t0 = time.perf_counter()
            rp, ci = eng.get_graph_csr()
            fetch = (time.perf_counter() - t0) * 1e3
            A = sp.csr_matrix((np.ones(len(ci), dtype=np.int8), ci.astype(np.int32), rp.astype(np.int64)), shape=(gi["n"], gi["n"]))
            nc, _ = csg.connected_components(A, directed=False)
            wall = (time.perf_counter() - t0) * 1e3
            emit(workload=name, case="get_graph_csr + scipy connected_components", wall_ms=round(wall, 2), of_which_fetch_ms=round(fetch, 2),
                 n_components=int(nc), device_call_ms=round(best["loop_ms"], 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
