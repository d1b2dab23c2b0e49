// pass_layout.hpp -- the device scratch of one full-panel launch set (run_passes, fullpass.hip): every buffer of
// qa_panel::Scratch with its size rule, each written ONCE.  The launch planner sums the layout (bytes per pass -> passes per
// launch set) and run_passes carves the arena by walking the same entries, so what is planned is what is carved.
// Host-only: no HIP types.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace qa {

// (declared with their kernels in fullpass_dev.hpp; repeated so that this header stands without the HIP headers)
int fb64_spill_rows(int K);
size_t fb64_alpha_col_elems(int K);
size_t fb_ref_state_doubles(int Kq);

// Three families of kernels run a pass:
//   KIND_F32       fp32 state (k_fwd / k_bwd<float>): the dosage passes, any output
//   KIND_F64_RANK  fp64 state, the reference's lazy normalisation, fused top-K (fullpass64.hip): best-haplotype lists only
//   KIND_F64_DOS   fp64 state, the reference's lazy normalisation, alpha stored at every second grid (k_bwd64d re-forms the
//                  others: PassParams::fw_add), gamma histogram for the dosage
//                  (k_fwd64 + k_bwd64d, fullpass64.hip): the DOSAGE passes of qa_panel_set_dosage_precision(64)
//   KIND_F64_FULL  fp64 state through the generic kernels (k_fwd / k_bwd<double>, one wave per SIMD): any output in
//                  double (alphaHat_t / betaHat_t / gamma_t of the single-pass entry point in that mode); not tuned (it spills)
//   KIND_F64_REF   VALIDATION MODE (qa_panel_set_sum_order(panel, 1), fullpass_ref.hip): fp64 state, the reference's lazy
//                  normalisation, every K-wide sum added in the reference's order by one lane; any output; slow on purpose
enum PassKind { KIND_F32 = 0, KIND_F64_RANK = 1, KIND_F64_FULL = 2, KIND_F64_DOS = 3, KIND_F64_REF = 4, KIND_COUNT = 5 };
struct Geometry { int NT, NCH; PassKind kind; bool f64() const { return kind != KIND_F32; } };
// the kinds whose forward pass normalises lazily, on the reference's schedule (PassParams::lazy)
inline bool lazy_kind(PassKind k) { return k == KIND_F64_RANK || k == KIND_F64_DOS || k == KIND_F64_REF; }

constexpr int kLayoutMaxRow = 256;   // = kMaxRow (fullpass_dev.hpp; fullpass.hip asserts it)

struct PanelDims { int K, G, T, n_special, n_sp_grids; };

// the thinned grids of a call (gammaSmall_cols_to_get): columns = max + 1, and the grids that hold one
struct Thin { int n_thin = 0, n_grids = 0; };
inline Thin count_thin(const int32_t *thin_col, int G) {
    Thin t;
    for (int g = 0; g < G; g++)
        if (thin_col[g] >= 0) { t.n_thin = std::max(t.n_thin, thin_col[g] + 1); t.n_grids++; }
    return t;
}

// what the passes of one launch set ask of the scratch
struct PassRequest {
    bool stores_all = false;   // a pass with dosage / alpha / gamma / beta output: alpha at every grid, else at the thinned grids
    bool gamma = false, beta = false, gamma_col = false;
    bool lists = false;        // best-haplotype lists (thinned columns and K_top > 0)
    bool alpha_grid0 = false;  // a pass that stores alpha at the thinned grids only keeps grid 0's column too, in one more slot
                               // (the reference writes alphaHat_t column 0 whatever is asked, reference-single.cpp:2347-2354: the
                               // single-pass entry in validation mode, when grid 0 is not a thinned grid)
    Thin thin;
    int top_cap = 64;          // entries per list
};
// flags as in PassParams::flags
inline PassRequest make_request(const int32_t *flags, int P, const Thin &thin, int K_top, int top_cap, bool gamma_col,
                                bool alpha_grid0 = false) {
    PassRequest r;
    for (int p = 0; p < P; p++) {
        r.stores_all |= (flags[p] & 15) != 0;
        r.gamma |= (flags[p] & 4) != 0;
        r.beta |= (flags[p] & 8) != 0;
    }
    r.lists = thin.n_thin > 0 && K_top > 0;
    r.thin = thin;
    r.top_cap = top_cap;
    r.gamma_col = gamma_col;
    r.alpha_grid0 = alpha_grid0 && !r.stores_all;
    return r;
}

// Elements PER PASS of every Scratch buffer (THIN_COL: per launch set, charged to every pass by the plan), in carve order.
// Three carves lie outside the per-pass plan:
//   * the 1 MiB behind ALPHA (kAlphaSlack: k_bwd64d's idle lanes fetch a fixed line past a short column), once per launch
//     set: paid by plan_chunk's fixed term;
//   * the single-pass entry's un-permute staging (Scratch::unperm, K x G doubles): that entry adds it to the fixed term itself;
//   * TOP_IDX / TOP_VAL carved a second time with a larger top_cap by the non-truncating top-K retry (single passes and
//     qa_fullpass_batch only: pathological ties): plan_chunk's fixed term; the single-pass entry and the launch-set hook add
//     room for lists of all K haplotypes (a label without reads) to it themselves.
struct PassLayout {
    enum Buf { GL, THIN_COL, FLAGS, ALPHA_SLOT, EMAT, ESCALE0, EMIN, EMIN_B1, ESP, GSP, ALPHA, C, FW_ADD, FW_XS, MG, DOSAGE, GAMMA,
               BETA, BETA_THIN, GAMMA_COL, TOP_CNT, SPILL, TOP_IDX, TOP_VAL, N_BUF };
    static constexpr size_t kAlphaSlack = (size_t)1 << 20;
    struct Entry { size_t elems = 0, elem_bytes = 1; };
    Entry e[N_BUF];
    // what PassParams repeats of the layout
    size_t es = 4, Kq = 0, alpha_cols = 0, alpha_col_elems = 0, esp_stride = 0, spill_stride = 0;

    PassLayout(const PanelDims &d, const Geometry &geo, const PassRequest &r) {
        const PassKind kind = geo.kind;
        const size_t G = d.G, T = d.T, n_thin = r.thin.n_thin;
        es = geo.f64() ? 8 : 4;
        Kq = (size_t)geo.NT * geo.NCH * 16;
        // alpha checkpoints: all grids for dosage / gamma / beta passes (the fp64 dosage kernels: every second one, k_bwd64d
        // re-forms the odd grids'), the thinned grids otherwise
        alpha_cols = !r.stores_all ? (size_t)std::max(r.thin.n_grids, 1) + (r.alpha_grid0 ? 1 : 0) : kind == KIND_F64_DOS ? (G + 1) / 2 : G;
        alpha_col_elems = kind == KIND_F64_DOS ? fb64_alpha_col_elems(d.K) : Kq;
        esp_stride = (size_t)d.n_special + (lazy_kind(kind) ? 16 * (size_t)d.n_sp_grids : 0) + 16;
        spill_stride = kind == KIND_F64_REF ? fb_ref_state_doubles((int)Kq)   // the validation kernels' state (when not in LDS)
                       : lazy_kind(kind) ? (size_t)fb64_spill_rows(d.K) * 8192 : 0;   // chunk rows streamed through HBM
        e[GL] = {T * 2, 8};
        e[THIN_COL] = {G, 4};
        e[FLAGS] = {1, 4};
        e[ALPHA_SLOT] = {G, 4};
        e[EMAT] = {G * kLayoutMaxRow, es};
        e[ESCALE0] = {1, 8};
        e[EMIN] = {G, 8};
        e[EMIN_B1] = {1, 8};
        e[ESP] = {esp_stride, es};
        e[GSP] = {(size_t)std::max(d.n_special, 1), es};
        e[ALPHA] = {alpha_cols * alpha_col_elems, es};
        e[C] = {G, 8};
        e[FW_ADD] = e[FW_XS] = {kind == KIND_F64_DOS ? G : 0, 8};
        e[MG] = {G * kLayoutMaxRow, es};
        e[DOSAGE] = {T, 8};
        e[GAMMA] = {r.gamma ? G * Kq : 0, es};
        e[BETA] = {r.beta ? G * Kq : 0, es};
        e[BETA_THIN] = {r.lists ? n_thin * Kq : 0, es};
        e[GAMMA_COL] = {r.gamma_col ? Kq : 0, 8};
        e[TOP_CNT] = {std::max<size_t>(n_thin, 1), 4};
        e[SPILL] = {spill_stride, 8};
        set_top_cap(r.lists ? r.top_cap : 0, n_thin);
    }
    void set_top_cap(int cap, size_t n_thin) {
        e[TOP_IDX] = {n_thin * (size_t)cap, 4};
        e[TOP_VAL] = {n_thin * (size_t)cap, es};
    }
    // bytes of buffer b in a launch set of P passes
    size_t bytes(Buf b, int P) const { return e[b].elems * e[b].elem_bytes * (b == THIN_COL ? 1 : (size_t)P) + (b == ALPHA ? kAlphaSlack : 0); }
    // the plan: bytes one more pass adds, every buffer rounded to the arena's carve alignment
    size_t pass_bytes(size_t align) const {
        size_t sum = 0;
        for (const Entry &x : e) sum += (x.elems * x.elem_bytes + align - 1) / align * align;
        return sum;
    }
};

}  // namespace qa
