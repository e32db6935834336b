"""tools/eig_bench.py -- GPU: extreme eigenpairs by thick-restart Lanczos (lzx_eigsh_f64, Engine.eigsh) on BASELINE's C2 and C3
graphs (bench.WORKLOADS, imported), in one process:

  - under A: nev = 1 (spectral radius and centrality vector) and nev = 10, "LA", tol 1e-10;
  - under L: the largest 4;
  - on C2 only, the route a user has without it: scipy eigsh over Engine.spmv as a LinearOperator, same tol (--no-scipy skips it).

Per case: wall time (host clock around the call), matvecs, restarts, the spmv / orth / host split of lzx_eig_info, and the
bytes and TB/s of the orthogonalisation.  Bytes: every Lanczos step j of a cycle reads the J = nw + j + 1 basis columns four
times (CGS2: two projections, two updates) and reads / writes w about 2 J / 8 + 6 times; a restart reads m and writes p
columns.  The model counts 8 n (4 J + 2 J / 8 + 6) per step and 8 n (m + p) per restart; the rate is that over orth_ms.

    python tools/eig_bench.py [--workloads c2,c3] [--out FILE] [--no-scipy]
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


def orth_bytes(n, info, nev):
    """the byte model above, summed over the run's steps (cycle structure rebuilt from m, nev and the counts)"""
    m = info["m"]
    p = nev + (m - nev) // 2
    total, steps_left, j0 = 0.0, info["matvecs"], 0
    while steps_left > 0:
        for j in range(j0, m):
            if steps_left == 0:
                break
            J = j + 1
            total += 8.0 * n * (4 * J + 2 * J / 8 + 6)
            steps_left -= 1
        j0 = p
    total += info["restarts"] * 8.0 * n * (m + p)
    return total


def case(eng, n, what, **kw):
    t0 = time.perf_counter()
    try:
        w, _, info = eng.eigsh(want_vectors=False, **kw)
        ok = True
    except ge.load_pkg().LzxError as e:
        w, _, info = e.partial
        ok = False
    wall = (time.perf_counter() - t0) * 1e3
    ob = orth_bytes(n, info, kw["nev"])
    row = dict(case=what, ok=ok, wall_ms=round(wall, 2), matvecs=info["matvecs"], restarts=info["restarts"], m=info["m"],
               converged=info["converged"], spmv_ms=round(info["spmv_ms"], 2), orth_ms=round(info["orth_ms"], 2),
               host_ms=round(info["host_ms"], 2), orth_gb=round(ob / 1e9, 2),
               orth_tbs=round(ob / (info["orth_ms"] * 1e-3) / 1e12, 3) if info["orth_ms"] > 0 else None,
               top=[float(x) for x in (w[::-1][:3] if kw.get("which", "LA") == "LA" else w[:3])],
               max_resid=float(np.max(info["resid"])))
    print(json.dumps(row), flush=True)
    return row


def scipy_route(eng, n, tol):
    from scipy.sparse.linalg import LinearOperator, eigsh
    calls = [0]

    def mv(x):
        calls[0] += 1
        return eng.spmv(np.ascontiguousarray(x.ravel()))
    op = LinearOperator((n, n), matvec=mv, dtype=np.float64)
    t0 = time.perf_counter()
    w = eigsh(op, k=10, which="LA", tol=tol, return_eigenvectors=False)
    row = dict(case="scipy eigsh + Engine.spmv, A, nev=10", wall_ms=round((time.perf_counter() - t0) * 1e3, 2), matvecs=calls[0],
               top=[float(x) for x in np.sort(w)[::-1][:3]])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c2,c3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    pkg = ge.load_pkg()
    rows = []
    for name in args.workloads.split(","):
        desc, kind, scale, n, draws, gseed, _ = WORKLOADS[name]
        eng = pkg.Engine(0)
        t0 = time.perf_counter()
        if kind == "rmat":
            eng.gen_rmat(scale, n, draws, gseed)
        else:
            eng.gen_er(n, draws, gseed)
        print(f"{name}: n={n:,} nnz={eng.info()['nnz']:,} (graph {time.perf_counter() - t0:.1f} s)", flush=True)
        eng.eigsh(nev=1, which="LA", tol=1e-6, want_vectors=False)           # warm-up (code objects, allocations)
        for nev in (1, 10):
            rows.append(dict(workload=name, **case(eng, n, f"A, LA, nev={nev}", nev=nev, which="LA", tol=1e-10)))
        eng.set_option("operator", 1)
        rows.append(dict(workload=name, **case(eng, n, "L, LA, nev=4", nev=4, which="LA", tol=1e-10)))
        eng.set_option("operator", 0)
        if name == "c2" and not args.no_scipy:
            rows.append(dict(workload=name, **scipy_route(eng, n, 1e-10)))
        eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
