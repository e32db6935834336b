"""tools/paths_bench.py -- GPU: batched BFS and betweenness (lzx_bfs_multi, lzx_betweenness_f64; Engine.bfs / betweenness_raw)
on BASELINE's C2 and C3 graphs (bench.WORKLOADS, imported), in one process:

  - one batch of 16 sources (drawn by default_rng(1) among the vertices that reach more than themselves): levels, sweeps, and
    the device-event time per forward sweep (a bfs call: sweep_ms / sweeps) and per backward sweep (the betweenness call's
    sweep time and sweeps beyond the bfs call's);
  - beside those, the batched path's SpMM of the same width on the same graph: lzx_spmm_f64 itself crosses PCIe with 16 n
    values each way, so its launches (k_multi_spmm, then the split rows and alpha partials) are timed by the device events of
    a basis-free 16-probe Lanczos run (stats spmv_ms_min).  The three measurements alternate; medians of three;
  - the whole betweenness call for the 16 sources, and 16 times that as the estimate for k = 256 samples;
  - on C2 only, the route a user has without it: get_graph_csr() over PCIe and networkx's Brandes pass for one source.

    python tools/paths_bench.py [--workloads c2,c3] [--out FILE] [--no-networkx]
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
    ap.add_argument("--no-networkx", action="store_true")
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
        gi = eng.info()
        print(f"{name}: n={gi['n']:,} nnz={gi['nnz']:,} (graph {time.perf_counter() - t0:.1f} s)", flush=True)
        cand = np.random.default_rng(1).choice(gi["n"], size=64, replace=False)
        reach = eng.bfs(cand, dist=False)[1]["reached"]
        src = cand[reach > 1][:16]
        assert len(src) == 16
        eng.betweenness_raw(src)                                            # warm-up (and the work list)
        spmm, fwd, bwd, total, levels, sweeps = [], [], [], [], 0, 0
        for _ in range(3):
            spmm.append(eng.lanczos_probes(7, 0, 16, 5)[3]["spmv_ms_min"])
            f = eng.bfs(src, dist=False)[1]
            _, b = eng.betweenness_raw(src)
            fwd.append(f["sweep_ms"] / f["sweeps"])
            bwd.append((b["sweep_ms"] - f["sweep_ms"]) / max(b["sweeps"] - f["sweeps"], 1))
            total.append(b["loop_ms"])
            levels, sweeps = b["max_level"], b["sweeps"]
        eng.multi_release()
        med = lambda v: float(np.median(v))   # noqa: E731
        emit(workload=name, case="16 sources", n=gi["n"], nnz=gi["nnz"], levels=levels, sweeps=sweeps, forward_sweeps=sweeps - levels,
             backward_sweeps=levels, forward_ms_per_sweep=round(med(fwd), 4), backward_ms_per_sweep=round(med(bwd), 4),
             spmm16_ms=round(med(spmm), 4), forward_vs_spmm=round(med(fwd) / med(spmm), 3), betweenness_16_sources_ms=round(med(total), 3),
             estimate_k256_ms=round(16 * med(total), 1), reached_min=int(reach[reach > 1][:16].min()), reached_max=int(reach.max()))
        if name == "c2" and not args.no_networkx:
            import networkx as nx
            import scipy.sparse as sp
            t0 = time.perf_counter()
            rp, ci = eng.get_graph_csr()
            fetch = time.perf_counter() - t0
            A = sp.csr_matrix((np.ones(len(ci), dtype=np.int8), ci.astype(np.int32), rp.astype(np.int64)), shape=(gi["n"], gi["n"]))
            G = nx.from_scipy_sparse_array(A)
            build = time.perf_counter() - t0
            t0 = time.perf_counter()
            nx.betweenness_centrality_subset(G, [int(src[0])], list(G), normalized=False)
            one = time.perf_counter() - t0
            emit(workload=name, case="get_graph_csr + networkx, one source", fetch_s=round(fetch, 2), graph_build_s=round(build, 1),
                 brandes_one_source_s=round(one, 1), device_16_sources_ms=round(med(total), 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
