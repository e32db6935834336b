"""The graphs of tests/test_gpu_graph_lanes.py, built in numpy: the row lengths, vertex counts and oriented-list lengths at which
the graph routines' kernel templates over G lanes per row (csrc/lzx_graph_call.h: lzx_lanes_per_row, lzx_with_lanes, lzx_row_grid)
change what they do.  tests/test_lanes_graphs_host.py asserts the table below without a GPU.

(a) ladder(residue, reverse).  One hub per length T of HUB_LENGTHS:
        {G - 1, G, G + 1, 2 G - 1, 2 G, 2 G + 1, 64 G - 1, 64 G, 64 G + 1 : G = 4, 8, 16, 32} and {127, 128, 129}
    -- 30 hubs, T from 3 to 2049.  The hub of T is joined to the leaves 0 .. T - 1 and to nothing else, so the leaf sets are
    nested and two hubs have min(T, T') common neighbours.  The 2049 leaves form paths of 8 (leaf i -- leaf i + 1 unless 8 | i + 1),
    which keeps the rounds of the peeling restatements small (one ring of all leaves needs 2026 rounds of the core restatement).
    Beside them and apart from each other: a path of 70 vertices, which lzx_components merges over several rounds; a K_40, whose
    core number 39 and truss number 40 are above everything else's, so that it alone is the last window of lzx_core_numbers and
    lzx_truss -- the window that is never peeled -- and every hub is a row of a window that is; and isolated vertices (rows of
    length 0) up to the first n that is `residue` modulo 64: 0, 1 and 63, which is n mod (256 / G) = 0, 1 and 256 / G - 1 for
    every G.  Order: the hubs by descending T (the row of 2049 entries is row 0), the leaves, the path, the clique, the
    isolated vertices.  reverse: vertex v becomes n - 1 - v, and the row of 2049 entries the last row, in a last workgroup that
    is not full unless residue = 0.
(b) complete(m), m = 200 and 70: with ties broken by id the oriented lists of K_m have every length 0 .. m - 1;
    C(m - 1, 2) triangles per vertex, clustering 1.  two_cliques() = K_70 and K_200 apart: K_70 is one window of lzx_truss
    that is peeled, its edges' rows have 69 entries.
    twin_hubs(): two hubs joined to the same 2049 leaves and a third joined to the first 2048 of them -- the one pair of vertices
    whose shorter row has 64 * 32 + 1 entries, which the ladder, with one row of 2049 entries, cannot hold (lzx_similarity's split at
    32 lanes).
    split_gadgets(): the ladder's hubs outlive their leaves, so what a peeling kernel does with a hub's row changes nothing -- every
    neighbour is gone by then, or goes in the same round.  Here a long row is peeled while neighbours that depend on it remain.
    One gadget per T of SPLIT_LENGTHS (64 G and 64 G + 1): cliques A = K_10 and B = K_12 that share the vertex w; u in A and v in B
    are joined, and each has pendant leaves of its own up to T entries in its row.  lzx_truss: the edge (u, v) has support 1 (the
    triangle u v w) and the shorter of its rows T entries; it is peeled in round 2, and only its two decrements bring (u, w) and
    (v, w) down to their cliques' supports in time for rounds 3 and 4.  lzx_core_numbers: u, at 2 after its leaves and its mates
    in A have gone, is peeled in a round of its own, and only its decrements bring v and w down to B's 11.  A K_14 apart is the
    last window of both.  Without the decrements the layers of those edges and vertices, and the rounds, come out one higher.
(c) circulant(n, k, isolated): C_n(1 .. k), degree 2 k, for the rule itself; `isolated` vertices behind it without an edge."""
import functools
import itertools

import numpy as np
import scipy.sparse as sp

WIDTHS = (4, 8, 16, 32)
HUB_LENGTHS = tuple(sorted({G * f + d for G in WIDTHS for f in (1, 2, 64) for d in (-1, 0, 1)} | {127, 128, 129}, reverse=True))
LEAVES = max(HUB_LENGTHS)
LEAF_PATH = 8
SIDE_PATH = 70
CLIQUE = 40
RESIDUES = (0, 1, 63)
SPLIT_LENGTHS = tuple(64 * G + d for G in WIDTHS for d in (0, 1))
# (residue of n modulo 64, reversed): the four ladders of the GPU tests
LADDERS = ((0, False), (1, False), (63, False), (63, True))
# 2 k of the circulants and the lanes per row the rule picks for each (max_g = 32)
CIRCULANT_DEGREES = (6, 8, 14, 16, 30, 32, 62, 64)
CIRCULANT_LANES = (4, 8, 8, 16, 16, 32, 32, 32)


def adjacency(n, u, v):
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    A = sp.csr_matrix(sp.coo_matrix((np.ones(2 * len(u)), (np.concatenate([u, v]), np.concatenate([v, u]))), shape=(n, n)))
    A.data[:] = 1.0
    A.sort_indices()
    return A


def rule(A, max_g=32):
    """lzx_lanes_per_row: 4 .. max_g lanes, about half the mean length of the rows that have an entry"""
    lengths = np.diff(sp.csr_matrix(A).indptr)
    mean = int(lengths.sum()) // max(int((lengths > 0).sum()), 1)
    G = 4
    while G < max_g and 2 * G <= mean:
        G *= 2
    return G


def ladder_layout(residue=0):
    """where the parts of the unreversed ladder lie: a dict of (first, one past the last) vertex, and n"""
    at, out = 0, {}
    for name, count in (("hubs", len(HUB_LENGTHS)), ("leaves", LEAVES), ("path", SIDE_PATH), ("clique", CLIQUE)):
        out[name] = (at, at + count)
        at += count
    n = at + (residue - at) % 64
    out["isolated"] = (at, n)
    out["n"] = n
    return out


@functools.lru_cache(maxsize=None)
def ladder(residue=0, reverse=False):
    lay = ladder_layout(residue)
    n, leaf0, path0, clique0 = lay["n"], lay["leaves"][0], lay["path"][0], lay["clique"][0]
    u = [np.repeat(np.arange(len(HUB_LENGTHS)), HUB_LENGTHS)]
    v = [np.concatenate([leaf0 + np.arange(T) for T in HUB_LENGTHS])]
    i = np.arange(LEAVES - 1)
    i = i[(i + 1) % LEAF_PATH != 0]
    u.append(leaf0 + i)
    v.append(leaf0 + i + 1)
    u.append(path0 + np.arange(SIDE_PATH - 1))
    v.append(path0 + np.arange(1, SIDE_PATH))
    pairs = np.array(list(itertools.combinations(range(CLIQUE), 2)), dtype=np.int64)
    u.append(clique0 + pairs[:, 0])
    v.append(clique0 + pairs[:, 1])
    u, v = np.concatenate(u), np.concatenate(v)
    if reverse:
        u, v = n - 1 - u, n - 1 - v
    return adjacency(n, u, v)


def ladder_ids(residue=0, reverse=False):
    """(hub of every length of HUB_LENGTHS, leaf 0 .. LEAVES - 1) as vertex ids of ladder(residue, reverse)"""
    lay = ladder_layout(residue)
    hubs, leaves = np.arange(*lay["hubs"]), np.arange(*lay["leaves"])
    return (lay["n"] - 1 - hubs, lay["n"] - 1 - leaves) if reverse else (hubs, leaves)


def ladder_pairs(residue=0, reverse=False, seed=29):
    """the pairs of the similarity tests: all 435 hub-hub pairs (min(T, T') common neighbours), then 200 hub-leaf and 200
    leaf-leaf pairs from a seeded draw"""
    hubs, leaves = ladder_ids(residue, reverse)
    rng = np.random.default_rng(seed)
    hh = np.array(list(itertools.combinations(hubs.tolist(), 2)), dtype=np.int64)
    hl = np.stack([rng.choice(hubs, 200), rng.choice(leaves, 200)], axis=1)
    a = rng.integers(0, LEAVES, 200)
    b = (a + rng.integers(1, LEAVES, 200)) % LEAVES
    b[:100] = np.minimum(a[:100] + rng.integers(1, 3, 100), LEAVES - 1)      # half of them one or two places apart: common hubs and a path
    b[b == a] -= 1
    return np.concatenate([hh, hl, np.stack([leaves[a], leaves[b]], axis=1)]).astype(np.int64)


def ladder_name(residue, reverse):
    return f"ladder_n%64={residue}" + ("_reversed" if reverse else "")


@functools.lru_cache(maxsize=None)
def complete(m):
    pairs = np.array(list(itertools.combinations(range(m), 2)), dtype=np.int64)
    return adjacency(m, pairs[:, 0], pairs[:, 1])


@functools.lru_cache(maxsize=None)
def two_cliques(a=70, b=200):
    A = sp.csr_matrix(sp.block_diag([complete(a), complete(b)]))
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def twin_hubs():
    """vertices 0 and 1: hubs of the leaves 3 .. 2051; vertex 2: hub of the leaves 3 .. 2050"""
    u = np.concatenate([np.zeros(LEAVES, dtype=np.int64), np.ones(LEAVES, dtype=np.int64), np.full(LEAVES - 1, 2)])
    v = np.concatenate([3 + np.arange(LEAVES), 3 + np.arange(LEAVES), 3 + np.arange(LEAVES - 1)])
    return adjacency(3 + LEAVES, u, v)


def split_gadget_ids():
    """{T: (u, v, w)} of split_gadgets()"""
    out, at = {}, 0
    for T in SPLIT_LENGTHS:
        out[T] = (at, at + 10, at + 9)          # A = at .. at + 9 (u first, w last), B = at + 9 .. at + 20 (w first, v second)
        at += 21 + (T - 10) + (T - 12)
    return out


@functools.lru_cache(maxsize=None)
def split_gadgets():
    u, v, at = [], [], 0
    for T in SPLIT_LENGTHS:
        A, B = list(range(at, at + 10)), list(range(at + 9, at + 21))
        pairs = list(itertools.combinations(A, 2)) + list(itertools.combinations(B, 2)) + [(A[0], B[1])]
        leaf = at + 21
        pairs += [(A[0], leaf + i) for i in range(T - 10)]            # u: 9 mates, v and T - 10 leaves
        leaf += T - 10
        pairs += [(B[1], leaf + i) for i in range(T - 12)]            # v: 11 mates, u and T - 12 leaves
        at = leaf + T - 12
        u += [a for a, _ in pairs]
        v += [b for _, b in pairs]
    pairs = list(itertools.combinations(range(at, at + 14), 2))
    u += [a for a, _ in pairs]
    v += [b for _, b in pairs]
    return adjacency(at + 14, u, v)


@functools.lru_cache(maxsize=None)
def circulant(n, k, isolated=0):
    i = np.repeat(np.arange(n), k)
    j = (i + np.tile(np.arange(1, k + 1), n)) % n
    return adjacency(n + isolated, i, j)


def coverage(A):
    """what a graph puts in front of a launch over G lanes per row, for every G of WIDTHS: the facts the coverage tables assert"""
    lengths = np.diff(sp.csr_matrix(A).indptr)
    n = len(lengths)
    present = set(lengths.tolist())
    out = dict(n=n, nnz=int(lengths.sum()), lengths=present, longest=int(lengths.max()), first_is_longest=bool(lengths[0] == lengths.max()),
               last_is_longest=bool(lengths[-1] == lengths.max()))
    for G in WIDTHS:
        rows = 256 // G
        out[G] = dict(row_lengths={0, 1, G - 1, G, G + 1, 2 * G - 1, 2 * G + 1} <= present, split={64 * G, 64 * G + 1} <= present, fill=n % rows)
    return out
