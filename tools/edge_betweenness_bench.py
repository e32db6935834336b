"""tools/edge_betweenness_bench.py -- GPU: the edge pass of lzx_brandes_f64 (Engine.brandes_raw) on BASELINE's C2 and C3 graphs
(bench.WORKLOADS, imported), in one process, one batch of 16 sources (drawn as tools/paths_bench.py draws them):

  - edge_ms of the batch: the device-event time of the one edge pass, and what it moves per stored entry against DESIGN.md
    section 24's model of at most 4 + 4 B + 16 B + 16 = 340 bytes at B = 16;
  - beside it the device-event time per forward sweep (a bfs call: sweep_ms / sweeps) and the batched path's SpMM of width 16
    (the device events of a basis-free 16-probe Lanczos run, stats spmv_ms_min).  The three alternate; medians of three;
  - the whole call with ebc (bc and ebc, and ebc alone) and without it (lzx_betweenness_f64), host clock.

    python tools/edge_betweenness_bench.py [--workloads c2,c3] [--out profiles/edge_betweenness_bench.txt]
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

MODEL_BYTES = 4 + 4 * 16 + 16 * 16 + 16


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
        eng.brandes_raw(src)                                                # warm-up (and the work list)
        spmm, fwd, edge, both, alone, plain, levels, lanes = [], [], [], [], [], [], 0, 0
        for _ in range(3):
            spmm.append(eng.lanczos_probes(7, 0, 16, 5)[3]["spmv_ms_min"])
            f = eng.bfs(src, dist=False)[1]
            fwd.append(f["sweep_ms"] / f["sweeps"])
            b = eng.brandes_raw(src)[2]
            lanes = eng.shape("graph_lanes_rows")
            edge.append(b["edge_ms"] / b["batches"])
            both.append(b["loop_ms"])
            alone.append(eng.brandes_raw(src, want_bc=False)[2]["loop_ms"])
            plain.append(eng.betweenness_raw(src)[1]["loop_ms"])
            levels = b["max_level"]
        eng.multi_release()
        med = lambda v: float(np.median(v))   # noqa: E731
        emit(workload=name, case="16 sources", n=gi["n"], nnz=gi["nnz"], levels=levels, lanes_per_row=lanes,
             edge_ms_per_batch=round(med(edge), 4), forward_ms_per_sweep=round(med(fwd), 4), spmm16_ms=round(med(spmm), 4),
             edge_vs_forward=round(med(edge) / med(fwd), 3), edge_vs_spmm=round(med(edge) / med(spmm), 3),
             model_bytes_per_entry=MODEL_BYTES, model_gb_per_s=round(MODEL_BYTES * gi["nnz"] / (med(edge) * 1e6), 1),
             call_bc_and_ebc_ms=round(med(both), 3), call_ebc_alone_ms=round(med(alone), 3), call_betweenness_ms=round(med(plain), 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
