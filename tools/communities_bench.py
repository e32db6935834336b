"""tools/communities_bench.py -- GPU: greedy colouring, label-propagation communities and modularity (lzx_color,
lzx_label_propagation, lzx_modularity; Engine.color_raw / label_propagation_raw / modularity_raw) on BASELINE's C2 and C3 graphs
(bench.WORKLOADS, imported) and on a stochastic block model made with numpy and handed over as edges, in one process:

  - color_raw(): colours, rounds and color_ms (the colouring by one device event pair, the host's reads per round included),
    hashed ties, best of three after a warm-up, next to lzx_bench_spmv of the same handle;
  - label_propagation_raw(): sweeps, sweep_ms and the milliseconds per sweep against the plain SpMV, the launches per sweep (the
    colours times the paths that have rows are not reported by the library: the colours are), communities, the largest one and Q;
  - modularity_raw() of the returned labels: the whole call, labels up and the sums down.

Every GPU step runs under a time limit of its own: a watchdog ends the process (exit status 124) when a step overruns it, and an
exception in a step ends the tool there, so nothing further is started on the device after a failure.

    python tools/communities_bench.py [--workloads c2,c3,sbm] [--out FILE] [--step-limit SECONDS] [--max-sweeps N]
"""
import argparse
import contextlib
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from bench import WORKLOADS  # noqa: E402

SBM = dict(blocks=64, size=4096, deg_in=24.0, deg_out=2.0, seed=5)   # 262 144 vertices, about 3.4 M edges


@contextlib.contextmanager
def limit(seconds, what):
    """one GPU step: past `seconds` the process ends at once with status 124 (a step that hangs never reaches the next)"""
    def overrun():
        print(f"communities_bench: {what} ran longer than {seconds} s -- ending here", file=sys.stderr, flush=True)
        os._exit(124)
    watchdog = threading.Timer(seconds, overrun)
    watchdog.daemon = True
    watchdog.start()
    try:
        yield
    finally:
        watchdog.cancel()


def sbm_edges(blocks, size, deg_in, deg_out, seed):
    """a stochastic block model by edge draws: blocks * size * deg_in / 2 pairs inside a block, blocks * size * deg_out / 2 anywhere"""
    rng = np.random.default_rng(seed)
    n = blocks * size
    m_in, m_out = int(n * deg_in / 2), int(n * deg_out / 2)
    block = rng.integers(0, blocks, m_in)
    src = np.concatenate([block * size + rng.integers(0, size, m_in), rng.integers(0, n, m_out)])
    dst = np.concatenate([block * size + rng.integers(0, size, m_in), rng.integers(0, n, m_out)])
    keep = src != dst
    return n, src[keep].astype(np.int64), dst[keep].astype(np.int64)


def generate(eng, name):
    if name == "sbm":
        n, src, dst = sbm_edges(**SBM)
        eng.set_graph_edges(n, src, dst)
        return
    _, kind, scale, n, draws, gseed, _ = WORKLOADS[name]
    if kind == "rmat":
        eng.gen_rmat(scale, n, draws, gseed)
    else:
        eng.gen_er(n, draws, gseed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3,sbm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds for each GPU step (the graph's generation: three times this)")
    ap.add_argument("--max-sweeps", type=int, default=100)
    args = ap.parse_args()
    pkg = ge.load_pkg()
    rows = []

    def emit(**row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    for name in args.workloads.split(","):
        with limit(3 * args.step_limit, f"{name}: the graph"):
            eng = pkg.Engine(0)
            t0 = time.perf_counter()
            generate(eng, name)
            handover_s = time.perf_counter() - t0
            gi = eng.info()
        print(f"{name}: n={gi['n']:,} nnz={gi['nnz']:,} (graph {handover_s:.1f} s)", flush=True)
        with limit(args.step_limit, f"{name}: lzx_bench_spmv"):
            eng.bench_spmv(5)
            spmv_avg, spmv_min = eng.bench_spmv(20)
        with limit(args.step_limit, f"{name}: the colouring, warm-up and three calls"):
            warm = eng.color_raw(want_colors=False)[1]
            color = min((eng.color_raw(want_colors=False)[1] for _ in range(3)), key=lambda i: i["color_ms"])
        assert all(color[key] == warm[key] for key in ("colors", "rounds", "largest_class"))
        emit(workload=name, case="color", n=gi["n"], nnz=gi["nnz"], colors=int(color["colors"]), rounds=int(color["rounds"]),
             largest_class=int(color["largest_class"]), color_ms=round(color["color_ms"], 3), call_ms=round(color["loop_ms"], 3),
             color_us_per_round=round(1e3 * color["color_ms"] / max(int(color["rounds"]), 1), 2), spmv_ms=round(spmv_min, 4),
             color_vs_spmv=round(color["color_ms"] / spmv_min, 1))
        with limit(2 * args.step_limit, f"{name}: the propagation"):
            try:
                labels, lpa = eng.label_propagation_raw(max_sweeps=args.max_sweeps)
                converged = True
            except pkg.LzxError as e:
                if "(-6)" not in str(e):
                    raise
                print(f"{name}: {e}", flush=True)
                labels, lpa, converged = None, None, False
        if lpa is not None:
            ms_per_sweep = lpa["sweep_ms"] / max(int(lpa["sweeps"]), 1)
            emit(workload=name, case="label_propagation", n=gi["n"], nnz=gi["nnz"], converged=converged, sweeps=int(lpa["sweeps"]),
                 updates=int(lpa["updates"]), colors=int(lpa["colors"]), sweep_ms=round(lpa["sweep_ms"], 3), ms_per_sweep=round(ms_per_sweep, 3),
                 spmv_ms=round(spmv_min, 4), sweep_vs_spmv=round(ms_per_sweep / spmv_min, 1),
                 us_per_class=round(1e3 * ms_per_sweep / max(int(lpa["colors"]), 1), 2), color_ms=round(lpa["color_ms"], 3),
                 communities=int(lpa["n_communities"]), largest_size=int(lpa["largest_size"]), modularity=lpa["modularity"],
                 call_ms=round(lpa["loop_ms"], 3))
            with limit(args.step_limit, f"{name}: the modularity of the labels"):
                q, mod = eng.modularity_raw(labels)
            assert q == lpa["modularity"] and mod["communities"] == lpa["n_communities"]
            emit(workload=name, case="modularity", communities=int(mod["communities"]), inner_entries=int(mod["inner_entries"]),
                 entries=int(mod["entries"]), q=q, call_ms=round(mod["loop_ms"], 3))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
