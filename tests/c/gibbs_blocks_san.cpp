// gibbs_blocks_san.cpp -- the block tables of the NIPT block pass under AddressSanitizer + UBSan, as a stand-alone program.
//
// Built by tests/test_chain_cases_cpu.py with -fsanitize=address,undefined from this file, oracle/gibbs.c, oracle/fullpass.c and the
// host header csrc/gibbs_blocks.hpp (plain C++, no device runtime).  Input: one file of records (int64 byte count, bytes), written
// by the test:
//   header   int32 [n_tables, n_calls]
//   a table  int32 [G, R, radius], double [quantile], double rate2[G - 1], int32 L_grid[G], int32 wif[R]
//   a call   the oracle's sampler on one chain: see read_call below
// For every table -- the file's, then R in (0, 1, 2) x G in (1, 2, 3) built here -- qo_define_blocked_grids / qo_make_gibbs_considers
// and qa::define_blocked_grids / qa::make_gibbs_considers run on exactly-sized buffers and must return the same table, in which
// every block's read range is inside the chain's reads or empty (start 0, end -1).  Every call must return status 0.
// Prints one line per table and call, "gibbs blocks: ok" last; exit code 1 on a difference.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "oracle/quilt_oracle.h"
#include "quilt_amd/csrc/gibbs_blocks.hpp"

namespace {

struct Records {
    FILE *f;
    std::vector<char> next() {
        int64_t n = 0;
        if (fread(&n, sizeof n, 1, f) != 1 || n < 0) { fprintf(stderr, "short file\n"); exit(2); }
        std::vector<char> b((size_t)n);
        if (n && fread(b.data(), 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short record\n"); exit(2); }
        return b;
    }
    template <class T>
    std::vector<T> vec() {
        const std::vector<char> b = next();
        std::vector<T> v(b.size() / sizeof(T));
        if (!b.empty()) memcpy(v.data(), b.data(), v.size() * sizeof(T));
        return v;
    }
};

template <class T>
const T *ptr_or_null(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

int n_bad = 0;

void fail(const std::string &what, const char *why) {
    printf("%s: DIFFERENT: %s\n", what.c_str(), why);
    n_bad++;
}

void check_table(const std::string &what, int G, int R, int radius, double q, const std::vector<double> &rate2,
                 const std::vector<int32_t> &L, const std::vector<int32_t> &wif) {
    std::vector<int32_t> blocked_o((size_t)G), gs((size_t)G), ge((size_t)G), rs((size_t)G), re((size_t)G), where((size_t)G);
    qo_define_blocked_grids(rate2.data(), L.data(), G, radius, q, blocked_o.data());
    const int n = qo_make_gibbs_considers(blocked_o.data(), G, wif.data(), R, gs.data(), ge.data(), rs.data(), re.data(), where.data());
    const std::vector<int32_t> blocked_h = qa::define_blocked_grids(rate2.data(), L.data(), G, radius, q);
    const qa::BlockTable T = qa::make_gibbs_considers(blocked_h, wif.data(), R);
    if (blocked_h != blocked_o) fail(what, "blocked grids");
    if (T.n_blocks != n) { fail(what, "number of blocks"); return; }
    if (T.grid_where != where) fail(what, "grid_where");
    printf("%s: G=%d R=%d blocks=%d", what.c_str(), G, R, n);
    for (int b = 0; b < n; b++) {
        if (T.grid_start[b] != gs[b] || T.grid_end[b] != ge[b] || T.reads_start[b] != rs[b] || T.reads_end[b] != re[b]) fail(what, "a block");
        const bool empty = rs[b] == 0 && re[b] == -1;
        if (!empty && !(0 <= rs[b] && rs[b] <= re[b] && re[b] < R)) fail(what, "a block's read range leaves the chain's reads");
        if (!(0 <= gs[b] && ge[b] < G)) fail(what, "a block's grid range");
        printf(" [%d-%d|%d-%d]", gs[b], ge[b], rs[b], re[b]);
    }
    printf("\n");
}

// a call: int32 [K, G, T, nMaxDH, special_nrow, use_special, Ks, R, first_read, radius, n_burn, n_sample], double [ref_error, ff,
// quantile], then rhb_t, hapMatcher, hapMatcherR, distinctHapsB, distinctHapsIE, special_grid_which, special_ptr, special_values,
// special_matrix_helper, special_matrix, transMatRate_t, which, read_ptr, u, bq, wif, grid_has_read, runif_reads, runif_block,
// runif_resample, L_grid, H0, block iterations (an absent array is an empty record)
void run_call(Records &in, int i) {
    const std::vector<int32_t> n = in.vec<int32_t>();
    const std::vector<double> d = in.vec<double>();
    const auto rhb = in.vec<int32_t>();
    const auto hm = in.vec<int32_t>();
    const auto hmr = in.vec<uint8_t>();
    const auto dhb = in.vec<int32_t>();
    const auto dhie = in.vec<double>();
    const auto sgw = in.vec<int32_t>();
    const auto sptr = in.vec<int32_t>();
    const auto svals = in.vec<int32_t>();
    const auto smh = in.vec<int32_t>();
    const auto sm = in.vec<int32_t>();
    const auto tm = in.vec<double>();
    const auto which = in.vec<int32_t>();
    const auto read_ptr = in.vec<int32_t>();
    const auto u = in.vec<int32_t>();
    const auto bq = in.vec<int32_t>();
    const auto wif = in.vec<int32_t>();
    const auto ghr = in.vec<uint8_t>();
    const auto ru = in.vec<double>();
    const auto rb = in.vec<double>();
    const auto rr = in.vec<double>();
    const auto L = in.vec<int32_t>();
    std::vector<int32_t> H = in.vec<int32_t>();
    const auto its = in.vec<int32_t>();
    const int K = n[0], G = n[1], T = n[2], Ks = n[6], R = n[7];
    qo_panel_t p;
    memset(&p, 0, sizeof p);
    p.K = K; p.nGrids = G; p.nSNPs = T; p.nMaxDH = n[3];
    p.rhb_t = ptr_or_null(rhb); p.hapMatcher = ptr_or_null(hm); p.hapMatcherR = ptr_or_null(hmr);
    p.distinctHapsB = ptr_or_null(dhb); p.distinctHapsIE = ptr_or_null(dhie);
    p.eMatDH_special_grid_which = ptr_or_null(sgw); p.special_values_ptr = ptr_or_null(sptr); p.special_values = ptr_or_null(svals);
    p.eMatDH_special_matrix_helper = ptr_or_null(smh); p.eMatDH_special_matrix = ptr_or_null(sm);
    p.eMatDH_special_matrix_nrow = n[4]; p.use_eMatDH_special_symbols = n[5];
    p.transMatRate_t = ptr_or_null(tm); p.ref_error = d[0];
    qo_gibbs_args_t a;
    memset(&a, 0, sizeof a);
    a.Ks = Ks; a.nReads = R; a.which_haps_to_use_1based = which.data();
    a.read_ptr = read_ptr.data(); a.u = ptr_or_null(u); a.bq = ptr_or_null(bq); a.wif = ptr_or_null(wif); a.grid_has_read = ghr.data();
    a.ff = d[1]; a.Jmax = 10000; a.maxDifferenceBetweenReads = 1e10;
    a.n_gibbs_burn_in_its = n[10]; a.n_gibbs_sample_its = n[11];
    a.block_gibbs_iterations = its.data(); a.n_block_gibbs_iterations = (int)its.size();
    a.perform_block_gibbs = 1; a.do_shard_block_gibbs = 0; a.gibbs_initialize_iteratively = 0; a.sample_is_diploid = 0;
    a.disable_read_category_usage = 0; a.rescale_eMatRead_t = 1; a.class_sum_cutoff = 0.06;
    a.runif_reads = ptr_or_null(ru); a.first_read = n[8]; a.runif_shard = nullptr;
    a.L_grid = L.data(); a.shuffle_bin_radius = n[9]; a.block_gibbs_quantile_prob = d[2];
    a.runif_block = ptr_or_null(rb); a.runif_resample = ptr_or_null(rr);
    std::vector<std::vector<double>> al(3, std::vector<double>((size_t)Ks * G)), be = al, eg = al, c(3, std::vector<double>((size_t)G));
    double *alp[3] = {al[0].data(), al[1].data(), al[2].data()}, *bep[3] = {be[0].data(), be[1].data(), be[2].data()};
    double *egp[3] = {eg[0].data(), eg[1].data(), eg[2].data()}, *cp[3] = {c[0].data(), c[1].data(), c[2].data()};
    std::vector<double> eMatRead((size_t)Ks * R), hap((size_t)3 * T), gm((size_t)3 * T), gf((size_t)3 * T);
    std::vector<int32_t> Hc((size_t)R), cat((size_t)R);
    const int st = qo_gibbs(&p, &a, H.data(), Hc.data(), alp, bep, egp, cp, eMatRead.data(), cat.data(), hap.data(), gm.data(), gf.data());
    printf("call %d: G=%d R=%d status=%d H=", i, G, R, st);
    for (int r = 0; r < R && r < 8; r++) printf("%d", H[(size_t)r]);
    printf("\n");
    if (st != 0) { n_bad++; printf("call %d: status %d\n", i, st); }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    Records in{fopen(argv[1], "rb")};
    if (!in.f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::vector<int32_t> head = in.vec<int32_t>();
    for (int i = 0; i < head[0]; i++) {
        const std::vector<int32_t> n = in.vec<int32_t>();
        const std::vector<double> q = in.vec<double>();
        const std::vector<double> rate2 = in.vec<double>();
        const std::vector<int32_t> L = in.vec<int32_t>();
        const std::vector<int32_t> wif = in.vec<int32_t>();
        if ((int)rate2.size() != n[0] - 1 || (int)L.size() != n[0] || (int)wif.size() != n[1]) { fprintf(stderr, "table %d: sizes\n", i); return 2; }
        check_table("table " + std::to_string(i), n[0], n[1], n[2], q[0], rate2, L, wif);
    }
    for (int G = 1; G <= 3; G++)
        for (int R = 0; R <= 2; R++) {
            std::vector<double> rate2((size_t)(G - 1));
            std::vector<int32_t> L((size_t)G), wif((size_t)R);
            for (int g = 0; g < G - 1; g++) rate2[(size_t)g] = 0.3 + 0.4 * g;
            for (int g = 0; g < G; g++) L[(size_t)g] = 1000 + 3000 * g;
            for (int r = 0; r < R; r++) wif[(size_t)r] = R > 1 ? r * (G - 1) / (R - 1) : G - 1;
            for (double q : {0.5, 0.95})
                check_table("small G=" + std::to_string(G) + " R=" + std::to_string(R), G, R, 1000, q, rate2, L, wif);
        }
    for (int i = 0; i < head[1]; i++) run_call(in, i);
    fclose(in.f);
    if (n_bad) return 1;
    printf("gibbs blocks: ok\n");
    return 0;
}
