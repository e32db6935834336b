"""tools/similarity_bench.py -- GPU: the similarity of two vertices (lzx_similarity; Engine.similarity_raw) on BASELINE's C2 and C3
graphs (bench.WORKLOADS, imported), in one process.  Three cases per graph, all five measures asked for:

  - random   2^20 seeded random pairs
  - hubs     2^16 pairs drawn among the 1024 vertices of largest degree: the worst case, both rows long
  - edges    edges mode: every stored entry, each undirected edge intersected once

For each case: prep_ms (degrees, tables, the pair list of edges mode) and count_ms (classification, walks, the closing launch),
each by one device event pair, best of three after a warm-up; pairs per second and entries walked per second over count_ms; the
pairs on each path; next to lzx_bench_spmv of the same handle and, for edges mode, to support_ms of lzx_truss on the same graph.

Every GPU step runs under a time limit of its own: a watchdog ends the process (exit status 124) when a step overruns it, and an
exception in a step ends the tool there, so nothing further is started on the device after a failure.

    python tools/similarity_bench.py [--workloads c2,c3] [--cases random,hubs,edges] [--out FILE] [--step-limit SECONDS]
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


@contextlib.contextmanager
def limit(seconds, what):
    """one GPU step: past `seconds` the process ends at once with status 124 (a step that hangs never reaches the next)"""
    def overrun():
        print(f"similarity_bench: {what} ran longer than {seconds} s -- ending here", file=sys.stderr, flush=True)
        os._exit(124)
    watchdog = threading.Timer(seconds, overrun)
    watchdog.daemon = True
    watchdog.start()
    try:
        yield
    finally:
        watchdog.cancel()


def generate(eng, name):
    _, kind, scale, n, draws, gseed, _ = WORKLOADS[name]
    if kind == "rmat":
        eng.gen_rmat(scale, n, draws, gseed)
    else:
        eng.gen_er(n, draws, gseed)


def distinct_pairs(rng, pool, count):
    """`count` pairs u != v drawn from the vertex ids in `pool`"""
    i = rng.integers(0, len(pool), count)
    j = (i + rng.integers(1, len(pool), count)) % len(pool)
    return np.stack([pool[i], pool[j]], axis=1).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--cases", default="random,hubs,edges")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-limit", type=float, default=120.0, help="seconds for each GPU step (the graph's generation: three times this)")
    args = ap.parse_args()
    pkg = ge.load_pkg()
    rows = []
    ints = ("pairs", "walked", "short_pairs", "long_pairs", "sliced_pairs", "max_common", "lanes")

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
        rng = np.random.default_rng(2024)
        cases = {}
        if "random" in args.cases:
            cases["random"] = distinct_pairs(rng, np.arange(gi["n"], dtype=np.int64), 1 << 20)
        if "hubs" in args.cases:
            with limit(args.step_limit, f"{name}: the graph's CSR for the degrees"):
                rp, _ = eng.get_graph_csr()
            top = np.argsort(-np.diff(rp.astype(np.int64)), kind="stable")[:1024]
            cases["hubs"] = distinct_pairs(rng, top, 1 << 16)
            del rp
        if "edges" in args.cases:
            cases["edges"] = None
        for case, pairs in cases.items():
            with limit(args.step_limit, f"{name}/{case}: the warm-up call"):
                warm = eng.similarity_raw(pairs, want_common=False, want_degrees=False)[4]
            print(f"{name}/{case}: warm-up prep_ms={warm['prep_ms']:.3f} count_ms={warm['count_ms']:.3f} walked={warm['walked']:,}", flush=True)
            with limit(args.step_limit, f"{name}/{case}: three calls"):
                runs = [eng.similarity_raw(pairs, want_common=False, want_degrees=False)[4] for _ in range(3)]
            assert all(i[key] == warm[key] for i in runs for key in ints)
            best = min(runs, key=lambda i: i["count_ms"])
            intersected = sum(int(best[k]) for k in ("short_pairs", "long_pairs", "sliced_pairs"))
            extra = {}
            if case == "edges":
                with limit(args.step_limit, f"{name}/{case}: lzx_truss for its support_ms"):
                    extra["truss_support_ms"] = round(eng.truss_raw(False, False, False, False)[4]["support_ms"], 4)
            emit(workload=name, case=case, n=gi["n"], nnz=gi["nnz"], prep_ms=round(min(i["prep_ms"] for i in runs), 4), count_ms=round(best["count_ms"], 4),
                 **{key: int(warm[key]) for key in ints}, pairs_per_s=round(1e3 * intersected / best["count_ms"], 1),
                 walked_per_s=round(1e3 * int(best["walked"]) / best["count_ms"], 1), spmv_ms=round(spmv_min, 4), spmv_avg_ms=round(spmv_avg, 4),
                 count_vs_spmv=round(best["count_ms"] / spmv_min, 2), call_ms=round(min(i["loop_ms"] for i in runs), 3), **extra)
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
