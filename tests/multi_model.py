"""Host model of the batched path's work list -- lzx_multi_build_tables of csrc/lzx_multi.hip -- and of the SpMM that walks it
(k_multi_spmm and k_multi_alpha of csrc/lzx_multi_shared.h), in numpy.  No GPU and no import of the package: the tests hand it a
CSR and the chunk L, and compare what it counts with what the library reports (tests/test_gpu_multi_tables.py) or with int64
arithmetic (tests/test_multi_model_host.py).

What is restated:
  segments     a row of at most L entries is one segment whose total is the row's output; a longer row is ceil(len / L) chunks of
               L entries, the last one shorter, each with a slot of chunk totals; the slots of a row are contiguous, rows ascending.
  order        all segments stably sorted by length, longest first (a counting sort over the rows in ascending order, a row's
               chunks in chunk order), then padded to a multiple of 32 with entries of length 0 that have no output.
  run_split    per 32-row run q (and one behind the last): the index of the first split row at or behind row 32 q.
  partials     n_seg = ceil(n / 2048) row segments; the vector kernels launch min(max(n_seg, 1), 4 x compute units) workgroups.
  spmm         every segment summed with ONE accumulator in entry order; an unsplit row's total stored to its row, a chunk's to its
               slot; then per split row the slots added in chunk order from 0.0; under L every row's v = fma(d, x, -v).  Rows of
               length 0 are segments too (they store 0.0); nothing but the list writes an output.
exact_start() makes the integer start vectors whose first Lanczos coefficients are exact in any summation order.
"""
import math
from fractions import Fraction

import numpy as np

CHUNK = 2048          # LZX_MULTI_CHUNK: the default L
RUN = 32              # LZX_MULTI_RUN
SEG = 2048            # LZX_MULTI_SEG
PAD_TO = 32           # the list is padded to a multiple of this
NO_OUTPUT = -1        # dst of a padding entry (LZX_MULTI_PAD)
CU_COUNT = 256        # MI355X


def pad_width(b):
    """lzx_multi_pad_width"""
    return 2 if b <= 2 else 4 if b <= 4 else 8 if b <= 8 else 16


class Model:
    pass


def build(rp, ci, L=CHUNK):
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    n = len(rp) - 1
    m = Model()
    m.n, m.L, m.rp, m.ci = n, int(L), rp, ci
    deg = rp[1:] - rp[:-1]
    m.deg = deg
    split = deg > L
    m.split_row = np.flatnonzero(split)
    nch = (deg[split] + L - 1) // L
    m.split_first = np.concatenate([[0], np.cumsum(nch)]).astype(np.int64)
    m.n_split, m.n_parts = len(m.split_row), int(m.split_first[-1])
    # segments in the builder's second pass: rows ascending, a split row's chunks in chunk order
    per_row = np.where(split, (deg + L - 1) // L, 1)
    row_of = np.repeat(np.arange(n), per_row)
    first = np.concatenate([[0], np.cumsum(per_row)])[:-1]
    k = np.arange(len(row_of)) - first[row_of]                    # chunk number within the row
    beg = rp[row_of] + k * L
    length = np.minimum(L, deg[row_of] - k * L)
    slot = np.full(n, -1, dtype=np.int64)
    slot[m.split_row] = m.split_first[:-1]
    is_part = split[row_of]
    dst = np.where(is_part, slot[row_of] + k, row_of)
    order = np.argsort(-length, kind="stable")                    # longest first, ties in the order above
    m.segs = len(row_of)
    m.n_wl = (m.segs + PAD_TO - 1) // PAD_TO * PAD_TO
    pad = m.n_wl - m.segs
    m.wl_beg = np.concatenate([beg[order], np.zeros(pad, dtype=np.int64)])
    m.wl_len = np.concatenate([length[order], np.zeros(pad, dtype=np.int64)])
    m.wl_dst = np.concatenate([dst[order], np.full(pad, NO_OUTPUT, dtype=np.int64)])
    m.wl_part = np.concatenate([is_part[order], np.zeros(pad, dtype=bool)])
    runs = (n + RUN - 1) // RUN
    m.runs = runs
    m.run_split = np.searchsorted(m.split_row, np.arange(runs + 1) * RUN, side="left")
    m.n_seg = (n + SEG - 1) // SEG
    return m


def vector_grid(m, cus=CU_COUNT):
    return min(max(m.n_seg, 1), 4 * cus)


def shapes(m, cus=CU_COUNT):
    """what lzx_test_get_shape reports once the tables exist"""
    return dict(multi_chunk=m.L, multi_work_items=m.n_wl, multi_split_rows=m.n_split, multi_chunk_slots=m.n_parts,
                multi_row_segments=m.n_seg, multi_vector_grid=vector_grid(m, cus))


def fma(a, b, c):
    """fma(a, b, c) elementwise with ONE rounding: where a * b is exact in fp64 (every use with integer data) the plain
    expression, elsewhere through exact rationals"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    p = a * b
    out = p + c
    inexact = np.flatnonzero((a.astype(np.longdouble) * b.astype(np.longdouble) != p.astype(np.longdouble)).ravel())
    if len(inexact):
        out = out.copy()
        flat = out.reshape(-1)
        af, bf, cf = a.reshape(-1), b.reshape(-1), c.reshape(-1)
        for i in inexact.tolist():
            flat[i] = float(Fraction(float(af[i])) * Fraction(float(bf[i])) + Fraction(float(cf[i])))   # float(Fraction): rounded once
    return out


def spmm(m, X, laplacian=False, stale=None):
    """Y (n, b) from X (n, b), the list walked as the device walks it.  stale: the value every output holds before the walk (a
    row that no list entry writes keeps it -- there is no such row when the list is right)."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        return spmm(m, X[:, None], laplacian, stale)[:, 0]
    b = X.shape[1]
    acc = np.zeros((m.n_wl, b))
    # k_multi_spmm: one accumulator per (segment, column), entries added in ascending order.  The list is longest first, so the
    # segments that still have an entry i are a prefix of it.
    neg = -m.wl_len
    for i in range(int(m.wl_len[0]) if m.n_wl else 0):
        live = int(np.searchsorted(neg, -i, side="left"))           # entries with len > i
        acc[:live] += X[m.ci[m.wl_beg[:live] + i]]
    Y = np.full((m.n, b), np.nan if stale is None else stale)
    part = np.full((max(m.n_parts, 1), b), np.nan)
    out = m.wl_dst != NO_OUTPUT
    rows = out & ~m.wl_part
    Y[m.wl_dst[rows]] = acc[rows]
    chunks = out & m.wl_part
    part[m.wl_dst[chunks]] = acc[chunks]
    # k_multi_alpha: per split row the slots added in chunk order
    for ks, r in enumerate(m.split_row.tolist()):
        v = np.zeros(b)
        for p in range(int(m.split_first[ks]), int(m.split_first[ks + 1])):
            v = v + part[p]
        Y[r] = v
    if laplacian:
        Y = fma(m.deg.astype(np.float64)[:, None], X, -Y)
    return Y


def exact_start(n, rng):
    """(x, m): x integer-valued with every entry in +-{1, 2, 3} and sum x_i^2 = 4^m for the smallest m that allows it: a ones, b
    twos and c threes with a + b + c = n and a + 4 b + 9 c = 4^m, i.e. 3 b + 8 c = 4^m - n with c in {0, 1, 2}.  Then ||x|| = 2^m
    exactly and q_0 = x / 2^m is exact.  None where no m works (n = 2: the sums 2, 5, 8, 10, 13, 18 hold no power of 4)."""
    m = 0
    while 4 ** m <= 9 * n:
        rest = 4 ** m - n
        for c in (0, 1, 2):
            if rest - 8 * c >= 0 and (rest - 8 * c) % 3 == 0 and (rest - 8 * c) // 3 + c <= n:
                b = (rest - 8 * c) // 3
                mag = np.concatenate([np.full(n - b - c, 1.0), np.full(b, 2.0), np.full(c, 3.0)])
                x = rng.permutation(mag) * rng.choice([-1.0, 1.0], size=n)
                return x, m
        m += 1
    return None


def first_coefficients(rp, ci, x, m, laplacian=False):
    """In Python integers, for q_0 = x / 2^m: (p, S) with alpha_0 = p / 4^m (p = x' M x) and beta_0 = sqrt(S) / 2^(3m)
    (S = sum u_int^2, u_int = 4^m (M x) - p x); and `fits`: every value the device forms on the way to ||u||^2 is an integer
    below 2^53 over a power of two (S < 2^53 and the products behind it), so that every partial sum is exact in any order."""
    rp, ci = np.asarray(rp, dtype=np.int64), np.asarray(ci, dtype=np.int64)
    xi = np.asarray(x).astype(np.int64)
    n = len(xi)
    Mx = np.add.reduceat(np.concatenate([xi[ci], [0]]), np.minimum(rp[:-1], len(ci))) if n else np.zeros(0, dtype=np.int64)
    Mx = np.where(rp[1:] > rp[:-1], Mx, 0)
    if laplacian:
        Mx = (rp[1:] - rp[:-1]) * xi - Mx
    p = int((xi * Mx).sum())                       # |p| <= 9 nnz: int64 holds it
    umax = 4 ** m * int(np.abs(Mx).max(initial=0)) + 3 * abs(p)
    assert umax < 2 ** 40 and n < 2 ** 22                      # int64 holds u, and the three sums of the split squares below
    u = (4 ** m) * Mx - p * xi
    hi, lo = u >> 20, u & ((1 << 20) - 1)                      # u = hi 2^20 + lo, 0 <= lo < 2^20, |hi| < 2^20
    S = (int((hi * hi).sum()) << 40) + (int((hi * lo).sum()) << 21) + int((lo * lo).sum())
    big = max(umax, int(np.abs(xi * Mx).sum()))
    return p, S, (S < 2 ** 53 and big < 2 ** 53)


def beta_exact(S, m):
    """sqrt(S) / 2^(3m) rounded once (S < 2^53: S / 2^(6m) is an fp64 value and math.sqrt rounds correctly)"""
    assert S < 2 ** 53
    return math.sqrt(S / 2.0 ** (6 * m))
