"""CPU: csrc/lzx_prepare_plan.h, the decisions of the graph hand-over (lzx_graph_prepare of csrc/lzx_graph.hip), run on the host
and compared with the numpy models that restate them.  tests/prepare_plan_check.cc is a program of its own: it is compiled here with
the host compiler and -fsanitize=address,undefined and run as a child process (nothing of it is loaded into this interpreter); it
reads the cases this test writes into a text file and prints every planned quantity.

Compared with: sell_model.staging (blocked mode and the staged slots), sell_model.exchange (xs, xs0), sell_model.build (the split
rows, the items and their lengths, the slices and slice_w, the classes and perm, grid and fin_grid), partition_model.slice_len /
exchange_len / chunk0_len.  sell_model.build takes a graph: model_tables() hands it one whose local rows have exactly the wanted
degl -- every entry in column 0, whose vertex has degree rank 0 and is staged in blocked mode -- so synthetic degl of 2 Mi rows go
through the model like a graph's.

What the models do not hold is restated here from the comments of the header: the unset-option defaults (blocked from 512 Ki
vertices and 8 Mi entries per rank; 16 Ki staged slots in blocked mode, 18 Ki on one rank from 4 Mi vertices, 8 Ki in plain mode;
at most n and 20 000, even), the 1 % rule (blocked, hub_entries unset, entries in the staged columns x 100 < nnz, n > 2048: 1 Ki
slots), the two zero slots of blocked mode, the padding code, and which of steps 1a and 1b run."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import partition_model as pm
import sell_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "msc-hpc-final-project_amd", "csrc")
LISTS = ("h_long_ptr", "h_item_first", "h_item_beg", "h_item_len", "h_slice_off", "h_slice_w", "perm", "h_slice_w0")
OPTIONS = ("pb_opt", "hub_opt", "overlap_opt", "xfp32_opt", "pb_cb_opt", "sparse_opt", "tie_sort_opt", "long_row_opt", "item_opt", "narrow_opt",
           "spmv_wgs_opt")
KI, MI = 1 << 10, 1 << 20
MASK = (1 << 64) - 1


def round_up(a, m):
    return (a + m - 1) // m * m


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def case(name, degl=(), **inp):
    c = dict(world=1, rank=0, cu_count=256, comm_kind=1, nnz=1000, n_active=inp["n"], max_degree=7, hub_share=0, xc1=100, vectors=1)
    c.update({k: -1 for k in OPTIONS})
    c.update(inp)
    assert len(degl) <= ((c["n"] - c["rank"] + c["world"] - 1) // c["world"] if c["rank"] < c["n"] else 0), name
    return name, c, np.asarray(degl, dtype=np.int64)


def sampled_cases():
    """worlds 1, 2, 3 and 8; n below, at and above one slice and two larger; the staged slots 0, odd, above n, above n_active and
    above 20 000 as asked for; n_active 0, 1, slots + 1; the shapes drawn per case"""
    rng = np.random.default_rng(11)
    out = []
    for world in (1, 2, 3, 8):
        for n in (40, 64, 65, 1000, 3000):
            for hub_opt in (0, 7, 200, n + 5, 25000):
                h = min(hub_opt, n, 20000) & ~1
                for n_active in sorted({0, 1, min(h + 1, n), n // 2, n}):
                    for pb_opt in (int(rng.integers(2)),) if n_active in (0, n // 2) else (0, 1):
                        rank = int(rng.integers(world))
                        rows = (n - rank + world - 1) // world if rank < n else 0
                        d = np.sort(rng.geometric(0.02, rows))[::-1] * int(rng.choice([1, 1, 8]))
                        if rng.random() < 0.5:
                            d = rng.integers(0, d + 1)       # blocked mode's counts are not monotone
                        pick = lambda *v: int(rng.choice(v))   # noqa: E731
                        out.append(case(f"w{world}_n{n}_h{hub_opt}_pb{pb_opt}_a{n_active}", d, n=n, world=world, rank=rank, hub_opt=hub_opt,
                                        pb_opt=pb_opt, n_active=n_active, nnz=int(d.sum()) * world + 1, comm_kind=pick(1, 2, 3),
                                        tie_sort_opt=pick(-1, 0, 2), sparse_opt=pick(-1, 0), overlap_opt=pick(-1, -1, 0, 1),
                                        xfp32_opt=pick(-1, -1, -1, 1), long_row_opt=pick(-1, -1, 4), item_opt=pick(-1, -1, 4),
                                        narrow_opt=pick(-1, 0, 1), spmv_wgs_opt=pick(-1, 1, 2), xc1=int(rng.integers(0, 500))))
    return out


def boundary_cases():
    out = []
    blocked = dict(pb_opt=1, hub_opt=200)
    # a row at long_thr and at long_thr + 1: plain 128, blocked 256, forced 4
    for pb_opt, long_row, thr in ((0, -1, 128), (1, -1, 256), (1, 4, 4)):
        for top in (thr, thr + 1):
            out.append(case(f"thr_pb{pb_opt}_lr{long_row}_top{top}", [top] + [3] * 100, n=640, pb_opt=pb_opt, hub_opt=200, long_row_opt=long_row))
    # the last real row over the threshold (blocked: degl is not monotone): the rounding reaches the padded rows, no slice is left
    out.append(case("split_rows_reach_the_padding", [1] * 99 + [300], n=100, pb_opt=1, hub_opt=20))
    # item caps 4, 2048 and 8192 with degl at the cap, cap + 1 and 0 among the split rows
    for item_opt, long_row, cap, last in ((4, 4, 4, 9), (-1, -1, 2048, 300), (8192, -1, 8192, 300)):
        out.append(case(f"item_cap_{cap}", [cap, cap + 1, 0, last], n=256, item_opt=item_opt, long_row_opt=long_row, **blocked))
    # slices of width 0, 4, 8 and 12, narrow_slices 0, 1 and unset, on each side of 8 CUs 16 slices (one CU: 128); spmv_wgs 1, 2, unset
    for slices in (127, 128):
        widths = np.repeat(np.asarray([0, 3, 8, 11])[np.arange(slices) % 4], 64)
        for narrow, wgs in ((-1, -1), (0, 1), (1, 2)):
            out.append(case(f"classes_s{slices}_narrow{narrow}_wgs{wgs}", widths, n=64 * slices, cu_count=1, narrow_opt=narrow, spmv_wgs_opt=wgs, **blocked))
    # units just below and at CUs 512 (four CUs), blocked and plain
    for units in (4 * 512 - 1, 4 * 512):
        for pb_opt in (0, 1):
            out.append(case(f"units_{units}_pb{pb_opt}", n=64 * units, cu_count=4, pb_opt=pb_opt, hub_opt=200))
    # rows_live at 2 Mi - 64 and at 2 Mi: the blocked threshold goes from 256 to 1024
    for n_active in (2 * MI - 64, 2 * MI):
        out.append(case(f"rows_live_{n_active}", [1025, 300, 257, 5], n=2 * MI, n_active=n_active, vectors=0, **blocked))
    # the band choice: 7 ranks whose x layout is exactly 16 MiB (7 x 299 584 + 64 doubles), and one slice more each; the band forced
    for xs, band in ((299584, -1), (299584 + 64, -1), (299584 + 64, 16384)):
        out.append(case(f"band_xs{xs}_cb{band}", n=7 * xs, world=7, rank=3, pb_cb_opt=band, vectors=0, **blocked))
    # the 1 % rule on each side of staged x 100 = nnz, n at 2048 and 2049
    for n in (2048, 2049):
        for share in (999, 1000):
            out.append(case(f"one_per_cent_n{n}_share{share}", n=n, pb_opt=1, nnz=100000, hub_share=share))
    # the unset-option defaults at their thresholds: blocked from 512 Ki vertices and 8 Mi entries per rank ...
    for n, nnz, world in ((512 * KI - 1, 8 * MI, 1), (512 * KI, 8 * MI - 1, 1), (512 * KI, 8 * MI, 1), (512 * KI, 16 * MI - 1, 2), (512 * KI, 16 * MI, 2)):
        for share in (nnz // 2, 0) if (n, nnz, world) == (512 * KI, 8 * MI, 1) else (nnz // 2,):
            out.append(case(f"default_pb_n{n}_nnz{nnz}_w{world}_share{share}", n=n, nnz=nnz, world=world, hub_share=share, vectors=0))
    # ... and the staged slots: 16 Ki blocked, 18 Ki on one rank from 4 Mi vertices, 8 Ki plain; the cap of 20 000
    for n, world, pb_opt in ((4 * MI - 1, 1, 1), (4 * MI, 1, 1), (4 * MI, 2, 1), (4 * MI, 1, 0), (4 * MI, 1, -1)):
        out.append(case(f"default_hub_n{n}_w{world}_pb{pb_opt}", n=n, world=world, pb_opt=pb_opt, nnz=64 * MI, hub_share=32 * MI, vectors=0))
    out.append(case("hub_above_20000", n=30000, pb_opt=1, hub_opt=25000))
    return out


def limit_cases():
    return [case("limit_n", n=1 << 31), case("limit_layout", n=(1 << 31) - 1, world=1 << 26)]


# ---- what the models and the header's comments say -----------------------------------------------------------------------------------
def model_tables(c, degl, pb, hub_real):
    """sell_model.build on a graph whose local rows of this rank have exactly degl"""
    n, world, rank = c["n"], c["world"], c["rank"]
    ids = np.arange(rank, n, world)
    deg = np.zeros(n, dtype=np.int64)
    deg[ids[:len(degl)]] = degl
    rp = np.concatenate([[0], np.cumsum(deg)])
    opt = lambda k: c[k] if c[k] >= 0 else None   # noqa: E731
    return sm.build(rp, np.zeros(rp[-1], dtype=np.int64), ids, np.arange(n), max(hub_real, 1), pb, c["n_active"], world=world, rank=rank,
                    long_row=opt("long_row_opt"), item_len=opt("item_opt"), narrow_slices=opt("narrow_opt"), spmv_wgs=opt("spmv_wgs_opt"),
                    cus=c["cu_count"])


def expected(c, degl):
    n, nnz, world, rank, n_active = c["n"], c["nnz"], c["world"], c["rank"], c["n_active"]
    e = dict(limit="none")
    e["n_loc_pad"] = pad = pm.slice_len(n, world)
    e["ldq"], e["iolen"] = pad + 64, world * pad + 64
    e["n_loc_real"] = (n - rank + world - 1) // world if rank < n else 0
    # the first choice: the unset-option defaults, restated from the header's comments
    pb = c["pb_opt"] > 0 or (c["pb_opt"] < 0 and n >= 512 * KI and nnz // world >= 8 * MI)
    hub = c["hub_opt"] if c["hub_opt"] >= 0 else ((18 * KI if world == 1 and n >= 4 * MI else 16 * KI) if pb else 8 * KI)
    hub = min(hub, n, 20000) & ~1
    pb = pb and 0 < hub < n
    slots = hub + (2 if pb else 0)
    e.update(first_pb=int(pb), first_hub_real=hub, first_hub=slots, first_spmv_lds=(slots + 16) * 8, first_xs=pad, first_xlen=e["iolen"])
    e["hub_share_rows"] = min(hub, n) if pb and c["hub_opt"] < 0 and nnz > 0 else 0
    if e["hub_share_rows"] and c["hub_share"] * 100 < nnz and n > 2048:      # the 1 % rule
        hub, slots = 1024, 1026
    e.update(n_active=n_active, max_degree=c["max_degree"])
    # from here the models, with the choice so far as their set options
    pb_set, hub_set = int(pb), hub
    pb, hub_real = sm.staging(n, n_active, pb_set, hub_set)
    if hub > n_active:      # the cut to the vertices with an edge: the two zero slots stay if the handle still blocked at the cut
        slots = hub_real + (2 if pb_set and hub_real else 0)
    e.update(pb=int(pb), hub_real=hub_real, hub=slots, spmv_lds=(slots + 16) * 8)
    xfp32 = world > 1 and c["xfp32_opt"] > 0
    wanted = c["overlap_opt"] > 0 or (c["overlap_opt"] < 0 and c["comm_kind"] != 2)
    xs, xs0 = sm.exchange(n, n_active, world, pb_set, hub_set, column_band=c["pb_cb_opt"] if c["pb_cb_opt"] > 0 else None, overlap=wanted and not xfp32)
    rp_active = np.minimum(np.arange(n + 1), n_active)      # n_active vertices of degree 1
    if world > 1:
        assert pm.exchange_len(rp_active, world) == xs
        if pb and wanted and not xfp32 and (c["pb_cb_opt"] > 0 or (world * xs + 64) * 8 <= 16 * MI):     # partition_model knows the 16 Ki band
            assert pm.chunk0_len(rp_active, world, hub_set) == xs0
    live = (n_active - rank + world - 1) // world if n_active > rank else 0
    e.update(rows_live=min(pad, round_up(live, 64)), xs=xs, xs0=xs0, xlen=world * xs + 64 if world > 1 else e["iolen"], overlap=int(xs0 < xs),
             xfp32=int(xfp32), tie_sort=int(pb and n_active > hub_real and c["tie_sort_opt"] != 0),
             try_sparse=int(xs0 < xs and world > 1 and c["sparse_opt"] != 0), sentinel=hub_real if pb else slots + world * xs,
             sparse_xlen=world * xs0 + round_up(c["xc1"], 64) + 64)
    t = model_tables(c, degl, pb, hub_real)
    assert t.rows_live == e["rows_live"] and t.n_loc_pad == pad and t.n_loc_real == e["n_loc_real"]
    dp = round_up(t.degl[:t.n_long64], 4)
    long_ptr = np.concatenate([[0], np.cumsum(dp)])
    lists = dict(h_long_ptr=long_ptr, h_item_first=np.concatenate([[0], np.cumsum(t.row_items)]),
                 h_item_beg=np.asarray([long_ptr[r] + j * t.item_cap for r, k in enumerate(t.row_items.tolist()) for j in range(k)], dtype=np.int64),
                 h_item_len=t.item_len, h_slice_off=np.concatenate([[0], np.cumsum(t.slice_w * 64)])[:t.n_slices], h_slice_w=t.slice_w,
                 perm=t.perm, h_slice_w0=t.w0)
    e.update(long_thr=t.thr, n_long_true=t.n_long, n_long64=t.n_long64, n_slices=t.n_slices, n_items=t.n_items, long_elems=t.long_elems,
             sell_elems=t.sell_elems, classes=int(t.classes), ns_wide=t.ns_wide, ns_w8=t.ns_w8, ns_w4=t.ns_w4, per_cu=1 if pb else 4,
             spmv_grid=t.grid, fin_grid=t.fin_grid)
    for k, a in lists.items():
        e[k + "_len"], e[k + "_sum"] = len(a), int(np.asarray(a, dtype=np.int64).sum())
        if c["vectors"]:
            e[k] = [int(x) for x in a]
    return e, t


# ---- the program ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++, the host compiler of host/Makefile, is not installed"
    exe = str(tmp_path_factory.mktemp("prepare_plan") / "prepare_plan_check")
    # -static-libasan / -static-libubsan: with the runtimes inside the program it does not depend on ASan's check that its shared
    # runtime comes first among the loaded libraries; -fno-sanitize-recover: a finding of UBSan ends the program, as ASan's do
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "prepare_plan_check.cc"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def run(program, path, text):
    with open(path, "w") as f:
        f.write(text)
    done = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    out, name = {}, None
    for line in done.stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "begin":
            name = rest
            out[name] = {}
        elif key == "end":
            name = None
        elif name is not None:
            out[name][key] = rest if key == "limit" else [int(x) for x in rest.split()] if key in LISTS or key.endswith("_hash") or key == "round_up" else int(rest)
    assert done.stdout.splitlines()[-1] == f"{len(out)} cases planned"
    return out


def case_text(name, c, degl):
    change = np.flatnonzero(np.diff(degl)) + 1 if len(degl) else np.zeros(0, dtype=np.int64)
    starts = np.concatenate([[0], change]).astype(np.int64) if len(degl) else change
    counts = np.diff(np.concatenate([starts, [len(degl)]])) if len(degl) else change
    runs = " ".join(f"{int(degl[s])} {int(k)}" for s, k in zip(starts, counts))
    return f"case {name} " + " ".join(f"{k}={int(v)}" for k, v in c.items()) + f"\ndegl {runs}\n"


def test_the_planner_against_the_models(program, tmp_path):
    cases = sampled_cases() + boundary_cases()
    got = run(program, tmp_path / "cases.txt", "".join(case_text(*c) for c in cases + limit_cases()))
    assert got["limit_n"] == dict(limit="n = %llu: this build indexes vertices with 31 bits")
    assert got["limit_layout"] == dict(limit="exchange layout does not fit 32-bit codes")
    reached = dict.fromkeys(("pad_reached", "live_below_2mi", "live_at_2mi", "classes_by_count", "no_classes_by_count", "halved_grid", "full_grid",
                             "band_16k_at_16mib", "band_18k_above", "one_chunk", "two_chunks", "rule_taken", "rule_not_taken", "default_blocked",
                             "default_18k", "capped_20000", "cut_to_active", "w0", "w4", "w8", "wide", "sparse", "tie_sort", "wgs_cap"), False)
    for name, c, degl in cases:
        e, t = expected(c, degl)
        g = got[name]
        differ = {k: (g.get(k), v) for k, v in e.items() if g.get(k) != v}
        assert not differ, (name, c, differ)
        assert sorted(g) == sorted(e), (name, sorted(set(g) ^ set(e)))      # every printed quantity was compared
        cus = c["cu_count"]
        reached["pad_reached"] |= t.reaches_pad
        reached["live_below_2mi"] |= e["pb"] and e["rows_live"] == 2 * MI - 64 and e["long_thr"] == 256
        reached["live_at_2mi"] |= e["pb"] and e["rows_live"] == 2 * MI and e["long_thr"] == 1024
        reached["classes_by_count"] |= c["narrow_opt"] < 0 and e["classes"] and e["n_slices"] == 8 * cus * 16
        reached["no_classes_by_count"] |= c["narrow_opt"] < 0 and e["pb"] and not e["classes"] and e["n_slices"] == 8 * cus * 16 - 1
        reached["halved_grid"] |= e["pb"] and t.units == cus * 512 - 1 and e["spmv_grid"] == max(1, cus // 2)
        reached["full_grid"] |= e["pb"] and t.units == cus * 512 and e["spmv_grid"] == cus
        reached["band_16k_at_16mib"] |= e["xlen"] * 8 == 16 * MI and e["overlap"] and e["xs0"] % 16384 == 0
        reached["band_18k_above"] |= e["xlen"] * 8 > 16 * MI and e["overlap"] and e["xs0"] % 18432 == 0 and e["xs0"] % 16384 != 0
        reached["one_chunk"] |= e["pb"] and c["world"] > 1 and not e["overlap"]
        reached["two_chunks"] |= bool(e["overlap"])
        reached["rule_taken"] |= e["hub_share_rows"] > 0 and e["hub_real"] == 1024
        reached["rule_not_taken"] |= e["hub_share_rows"] > 0 and e["hub_real"] > 1024
        reached["default_blocked"] |= c["pb_opt"] < 0 and bool(e["pb"])
        reached["default_18k"] |= e["first_hub_real"] == 18 * KI
        reached["capped_20000"] |= e["hub_real"] == 20000
        reached["cut_to_active"] |= e["hub_real"] < e["first_hub_real"] and e["hub_share_rows"] == 0
        reached["w0"] |= len(t.w0) > 0
        reached["w4"] |= t.ns_w4 > 0
        reached["w8"] |= t.ns_w8 > 0
        reached["wide"] |= bool(t.classes) and t.ns_wide > 0
        reached["sparse"] |= bool(e["try_sparse"])
        reached["tie_sort"] |= bool(e["tie_sort"])
        reached["wgs_cap"] |= c["spmv_wgs_opt"] > 0 and e["spmv_grid"] == c["spmv_wgs_opt"]
    assert all(reached.values()), [k for k, v in reached.items() if not v]


def test_the_hashes_of_the_sparse_lists(program, tmp_path):
    rng = np.random.default_rng(3)
    world, pad = 3, 128
    send_off, recv_off = [0, 2, 2, 5], [0, 1, 4, 4]
    idx = rng.integers(0, pad, 5).tolist()
    where = [int(p * pad + rng.integers(0, pad)) for p in (0, 1, 1, 1)]
    text = f"hash lists world={world} n_loc_pad={pad}\nsend_off {' '.join(map(str, send_off))}\nrecv_off {' '.join(map(str, recv_off))}\n"
    text += f"idx {' '.join(map(str, idx))}\nmap {' '.join(map(str, where))}\n"
    got = run(program, tmp_path / "hash.txt", text)["lists"]
    send = [sum(mix64(idx[i] + ((i - send_off[p]) << 32)) for i in range(send_off[p], send_off[p + 1])) & MASK for p in range(world)]
    recv = [sum(mix64(where[i] - p * pad + ((i - recv_off[p]) << 32)) for i in range(recv_off[p], recv_off[p + 1])) & MASK for p in range(world)]
    assert got["send_hash"] == send and got["recv_hash"] == recv and send[1] == 0 and recv[2] == 0
    assert got["send_hash_sum"] == sum(send) & MASK and got["recv_hash_len"] == world
    assert got["round_up"] == [0, 64, 128]


def test_the_header_stands_alone():
    """host only: nothing of HIP and nothing of the project is included, so that a plain C++ program can include it"""
    with open(os.path.join(CSRC, "lzx_prepare_plan.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes and all(inc in ("<cstdint>", "<cstddef>", "<algorithm>", "<vector>") for inc in includes), includes
