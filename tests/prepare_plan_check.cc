// prepare_plan_check.cc -- csrc/lzx_prepare_plan.h, the decisions of the graph hand-over, on a CPU.  A program of its own
// (tests/test_prepare_plan_host.py compiles it with -fsanitize=address,undefined and runs it as a child process): it reads cases
// from the text file named on its command line and prints every planned quantity, one "name value ..." line each.
//
//   case <id> <name>=<value> ...      the inputs of lzx_plan_in by their names, and: n_active, max_degree, hub_share (what the
//                                     ranking measured), xc1 (packed length of a sparse chunk 1), vectors (0: the lists are
//                                     left out of the print, their sums stay)
//   degl <value> <count> ...          run-length form of degl, from local row 0; the rest of the n_loc_pad rows is 0
//   hash <id> world=.. n_loc_pad=..   followed by four lines "send_off ...", "recv_off ...", "idx ...", "map ..."
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "lzx_prepare_plan.h"

typedef std::map<std::string, long long> Values;

static Values read_values(std::istringstream &line)
{
    Values v;
    std::string tok;
    while (line >> tok) {
        const size_t eq = tok.find('=');
        v[tok.substr(0, eq)] = std::stoll(tok.substr(eq + 1));
    }
    return v;
}

static long long get(const Values &v, const char *name, long long otherwise)
{
    const auto it = v.find(name);
    return it == v.end() ? otherwise : it->second;
}

template <typename T>
static void print_list(const char *name, const std::vector<T> &a, bool whole)
{
    unsigned long long sum = 0;
    for (const T &x : a) sum += x;
    std::printf("%s_len %zu\n%s_sum %llu\n", name, a.size(), name, sum);
    if (!whole) return;
    std::printf("%s", name);
    for (const T &x : a) std::printf(" %llu", (unsigned long long)x);
    std::printf("\n");
}

static std::vector<u32> read_list(std::ifstream &in, const char *name)
{
    std::string text, word;
    std::getline(in, text);
    std::istringstream line(text);
    line >> word;
    if (word != name) {
        std::fprintf(stderr, "expected a line '%s', got '%s'\n", name, word.c_str());
        std::exit(2);
    }
    std::vector<u32> a;
    unsigned long long x;
    while (line >> x) a.push_back((u32)x);
    return a;
}

static void run_case(const Values &v, const std::vector<u32> &runs)
{
    lzx_plan P;
    lzx_plan_in &in = P.in;
    in.n = (u64)get(v, "n", 0);
    in.nnz = (u64)get(v, "nnz", 0);
    in.world = (u32)get(v, "world", 1);
    in.rank = (u32)get(v, "rank", 0);
    in.cu_count = (u32)get(v, "cu_count", 256);
    in.comm_kind = (int)get(v, "comm_kind", 1);
    in.force_multi = get(v, "force_multi", 0) != 0;
    in.pb_opt = get(v, "pb_opt", -1);
    in.hub_opt = get(v, "hub_opt", -1);
    in.overlap_opt = get(v, "overlap_opt", -1);
    in.xfp32_opt = get(v, "xfp32_opt", -1);
    in.pb_cb_opt = get(v, "pb_cb_opt", -1);
    in.sparse_opt = get(v, "sparse_opt", -1);
    in.tie_sort_opt = get(v, "tie_sort_opt", -1);
    in.long_row_opt = get(v, "long_row_opt", -1);
    in.item_opt = get(v, "item_opt", -1);
    in.narrow_opt = get(v, "narrow_opt", -1);
    in.wgs_per_cu_opt = get(v, "wgs_per_cu_opt", -1);
    in.spmv_wgs_opt = get(v, "spmv_wgs_opt", -1);
    const bool whole = get(v, "vectors", 1) != 0;

    const char *limit = lzx_plan_layout(P);
    std::printf("limit %s\n", limit ? limit : "none");
    if (limit) return;
    std::printf("n_loc_pad %u\nldq %u\niolen %llu\nn_loc_real %u\n", P.n_loc_pad, P.ldq, (unsigned long long)P.iolen, P.n_loc_real);
    std::printf("first_pb %d\nfirst_hub_real %u\nfirst_hub %u\nfirst_spmv_lds %zu\nfirst_xs %u\nfirst_xlen %llu\n", (int)P.pb, P.hub_real, P.hub,
                P.spmv_lds, P.xs, (unsigned long long)P.xlen);
    std::printf("hub_share_rows %u\n", lzx_plan_hub_share_rows(P));

    lzx_plan_ranked(P, (u64)get(v, "n_active", 0), (u32)get(v, "max_degree", 0), (u64)get(v, "hub_share", 0));
    std::printf("n_active %llu\nmax_degree %u\npb %d\nhub_real %u\nhub %u\nspmv_lds %zu\n", (unsigned long long)P.n_active, P.max_degree, (int)P.pb,
                P.hub_real, P.hub, P.spmv_lds);
    std::printf("rows_live %u\nxs %u\nxlen %llu\nxs0 %u\noverlap %d\nxfp32 %d\ntie_sort %d\ntry_sparse %d\nsentinel %u\n", P.rows_live, P.xs,
                (unsigned long long)P.xlen, P.xs0, (int)P.overlap, (int)P.xfp32, (int)P.tie_sort, (int)P.try_sparse, P.sentinel);
    std::printf("sparse_xlen %llu\n", (unsigned long long)lzx_plan_sparse_xlen(in.world, P.xs0, (u64)get(v, "xc1", 0)));

    std::vector<u32> degl;   // exactly n_loc_pad entries: a read past them is AddressSanitizer's finding
    degl.reserve(P.n_loc_pad);
    for (size_t i = 0; i + 1 < runs.size(); i += 2) degl.insert(degl.end(), runs[i + 1], runs[i]);
    if (degl.size() > P.n_loc_pad) {
        std::fprintf(stderr, "degl of %zu rows for n_loc_pad %u\n", degl.size(), P.n_loc_pad);
        std::exit(2);
    }
    degl.resize(P.n_loc_pad, 0);
    degl.shrink_to_fit();
    lzx_plan_rows(P, degl);
    lzx_plan_slice_order(P);
    lzx_plan_grid(P);
    const lzx_row_plan &R = P.rows;
    std::printf("long_thr %u\nn_long_true %u\nn_long64 %u\nn_slices %u\nn_items %u\nlong_elems %llu\nsell_elems %llu\n", R.long_thr, R.n_long_true,
                R.n_long64, R.n_slices, R.n_items, (unsigned long long)R.long_elems, (unsigned long long)R.sell_elems);
    print_list("h_long_ptr", R.h_long_ptr, whole);
    print_list("h_item_first", R.h_item_first, whole);
    print_list("h_item_beg", R.h_item_beg, whole);
    print_list("h_item_len", R.h_item_len, whole);
    print_list("h_slice_off", R.h_slice_off, whole);
    print_list("h_slice_w", R.h_slice_w, whole);
    std::printf("classes %d\nns_wide %u\nns_w8 %u\nns_w4 %u\n", (int)R.classes, R.ns_wide, R.ns_w8, R.ns_w4);
    print_list("perm", R.perm, whole);
    print_list("h_slice_w0", R.h_slice_w0, whole);
    std::printf("per_cu %u\nspmv_grid %u\nfin_grid %u\n", R.per_cu, R.spmv_grid, R.fin_grid);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: prepare_plan_check CASES\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string text, word, id;
    size_t cases = 0;
    while (std::getline(in, text)) {
        std::istringstream line(text);
        if (!(line >> word >> id)) continue;
        const Values v = read_values(line);
        std::printf("begin %s\n", id.c_str());
        if (word == "case") {
            run_case(v, read_list(in, "degl"));
        } else if (word == "hash") {
            const std::vector<u32> send_off = read_list(in, "send_off"), recv_off = read_list(in, "recv_off");
            const std::vector<u32> idx = read_list(in, "idx"), map = read_list(in, "map");
            std::vector<u64> hs, hr;
            lzx_plan_sx_hashes((u32)get(v, "world", 1), (u32)get(v, "n_loc_pad", 64), send_off, recv_off, idx, map, hs, hr);
            print_list("send_hash", hs, true);
            print_list("recv_hash", hr, true);
            std::printf("round_up %u %u %u\n", round_up(0, 64), round_up(64, 64), round_up(65, 64));
        } else {
            std::fprintf(stderr, "unknown line '%s'\n", word.c_str());
            return 2;
        }
        std::printf("end %s\n", id.c_str());
        ++cases;
    }
    std::printf("%zu cases planned\n", cases);
    return 0;
}
