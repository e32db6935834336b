"""tools/multi_bench.py -- GPU: the batched, independent Lanczos path (lzx_lanczos_multi_f64) against the single-vector loop
(lzx_lanczos_f64) on BASELINE's C2 and C3 graphs (bench.WORKLOADS, imported), in one process.  For b in {1, 2, 4, 8, 16} at
k = 50: loop ms, vector-iterations/s (b * k / loop s), SpMM ms (the SpMM + split-row / alpha-partial launches per iteration),
the algorithmic bytes of one SpMM (4 nnz + 8 (n + 1) + 16 b n) and their fraction of 8 TB/s, and the single-vector loop's
iterations/s on the same graph.  Every figure is from one timed decomposition after a warm-up one of the same shape.
One JSON line per workload at the end (--out: also written to that file)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from bench import HBM_PEAK_GBS, WORKLOADS  # noqa: E402


def run(pkg, name, k, widths, seed):
    desc, kind, scale, n, draws, gseed, _ = WORKLOADS[name]
    eng = pkg.Engine(0)
    if kind == "rmat":
        eng.gen_rmat(scale, n, draws, gseed)
    else:
        eng.gen_er(n, draws, gseed)
    gi = eng.info()
    ones = np.ones(n)
    eng.lanczos(ones, k, want_q=False)                        # warm-up
    _, _, _, _, st1 = eng.lanczos(ones, k, want_q=False)
    single = k / (st1["loop_ms"] * 1e-3)
    print(f"{name}: n={n:,} nnz={gi['nnz']:,}  single-vector loop {st1['loop_ms']:.2f} ms for k={k}: {single:,.1f} iter/s", flush=True)
    X = np.random.default_rng(seed).random((max(widths), n))
    rows = []
    for b in widths:
        eng.lanczos_multi(X[:b], k)                           # warm-up (the first call builds the work list)
        _, _, ku, _, _, st = eng.lanczos_multi(X[:b], k)
        loop_s = st["loop_ms"] * 1e-3
        spmm_ms = st["spmv_ms"] / k
        frac = st["spmv_bytes"] / (spmm_ms * 1e-3) / (HBM_PEAK_GBS * 1e9)
        r = dict(b=b, loop_ms=round(st["loop_ms"], 3), vec_iter_per_s=round(b * k / loop_s, 1), spmm_ms=round(spmm_ms, 4),
                 spmm_ms_min=round(st["spmv_ms_min"], 4), vec_kernels_ms=round(st["vec_ms"] / k, 4), spmm_bytes=st["spmv_bytes"],
                 spmm_frac_8tbs=round(frac, 4), vs_single=round(b * k / loop_s / single, 3), k_used_min=int(ku.min()))
        rows.append(r)
        print(f"  b={b:2d}  loop {r['loop_ms']:9.2f} ms  {r['vec_iter_per_s']:11,.1f} vector-iter/s ({r['vs_single']:.2f}x single)  "
              f"SpMM {spmm_ms:.3f} ms (min {r['spmm_ms_min']:.3f})  vector kernels {r['vec_kernels_ms']:.3f} ms/iter  "
              f"{st['spmv_bytes'] / 1e9:.3f} GB per SpMM = {frac:.3f} of 8 TB/s", flush=True)
    eng.close()
    return dict(workload=name, desc=desc, n=n, nnz=gi["nnz"], k=k, single_iter_per_s=round(single, 1),
                single_loop_ms=round(st1["loop_ms"], 3), batched=rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--widths", default="1,2,4,8,16")
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = ge.load_pkg()
    widths = [int(w) for w in args.widths.split(",")]
    res = [run(pkg, w, args.k, widths, args.seed) for w in args.workloads.split(",")]
    for r in res:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
