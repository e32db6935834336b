"""tools/trace_bench.py -- GPU: stochastic Lanczos quadrature (lzx_lanczos_probes_f64, lzx_probe_diag_f64, Engine.trace_expm) on
BASELINE's C2 and C3 graphs (bench.WORKLOADS, imported), and C5 with --workloads c5, at b = 16 and k = 50, in one process:

  - probe-iterations/s (b * k / loop s, the library's host clock around the k iterations) of lanczos_probes basis-free, of
    lanczos_probes with the basis kept, and of lanczos_multi with the same probes uploaded as X (basis kept);
  - the batch-state bytes of each mode from the shapes: kept = (k + 2) n B 8 (basis, two work vectors), basis-free
    = 4 n B 8 (three ring slots, one work vector), work list and partials not counted;
  - probe_diag ms per batch (host clock around the call: T upload, the kernel, the n-vector copy back) and the bytes the
    kernel reads (the basis once, k n B 8);
  - trace_expm end to end (host clock, Lanczos + host quadrature) for 64 probes.

Every timed figure is the best of --reps after a warm-up of the same shape.  One JSON line per workload at the end.

    python tools/trace_bench.py [--workloads c2,c3] [--k 50] [--reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from bench import HBM_PEAK_GBS, WORKLOADS  # noqa: E402

B = 16


def best(fn, reps):
    fn()                                                   # warm-up
    out = None
    for _ in range(reps):
        r = fn()
        out = r if out is None or r < out else out
    return out


def run(pkg, name, k, reps, seed):
    desc, kind, scale, n, draws, gseed, _ = WORKLOADS[name]
    eng = pkg.Engine(0)
    t0 = time.perf_counter()
    if kind == "rmat":
        eng.gen_rmat(scale, n, draws, gseed)
    else:
        eng.gen_er(n, draws, gseed)
    gi = eng.info()
    print(f"{name}: n={n:,} nnz={gi['nnz']:,} (graph {time.perf_counter() - t0:.1f} s)", flush=True)
    row = dict(workload=name, desc=desc, n=n, nnz=gi["nnz"], b=B, k=k,
               state_bytes_basis_free=4 * n * B * 8, state_bytes_kept=(k + 2) * n * B * 8)
    row["probe_iter_per_s_basis_free"] = round(B * k / best(lambda: eng.lanczos_probes(seed, 0, B, k)[3]["loop_ms"] * 1e-3, reps), 1)
    try:
        row["probe_iter_per_s_kept"] = round(B * k / best(lambda: eng.lanczos_probes(seed, 0, B, k, keep_basis=True)[3]["loop_ms"] * 1e-3,
                                                          reps), 1)
        X = eng.probes(seed, 0, B)
        row["vec_iter_per_s_multi_explicit_x"] = round(B * k / best(lambda: eng.lanczos_multi(X, k)[5]["loop_ms"] * 1e-3, reps), 1)
        del X
        a, b, ku, _ = eng.lanczos_probes(seed, 0, B, k, keep_basis=True)
        T = pkg.slq_diag_coefficients(a, b, ku, n, 1.0 if eng.operator == 0 else -1.0, float(a.max() + 2 * b.max()))

        def diag():
            t = time.perf_counter()
            eng.probe_diag(T)
            return time.perf_counter() - t
        ms = best(diag, reps) * 1e3
        row["probe_diag_ms"] = round(ms, 3)
        row["probe_diag_read_bytes"] = k * n * B * 8
        row["probe_diag_frac_8tbs"] = round(k * n * B * 8 / (ms * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
    except pkg.LzxError as e:                            # C5: the kept basis (640 GB) does not fit
        row["kept"] = str(e)
    eng.multi_release()

    def trace():
        t = time.perf_counter()
        eng.trace_expm(1.0, n_probes=64, k=k, seed=seed)
        return time.perf_counter() - t
    row["trace_expm_64_probes_s"] = round(best(trace, max(1, reps - 1)), 4)
    lt, rel, _ = eng.trace_expm(1.0, n_probes=64, k=k, seed=seed)
    row["log_estrada"] = float(lt)
    row["rel_stderr"] = float(rel)
    for key, v in row.items():
        if key not in ("desc", "workload"):
            print(f"  {key:34s} {v}", flush=True)
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = ge.load_pkg()
    res = [run(pkg, w, args.k, args.reps, args.seed) for w in args.workloads.split(",")]
    for r in res:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            for r in res:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
