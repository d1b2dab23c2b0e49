// fullpass.hip -- full-panel haploid Li-Stephens forward/backward on gfx950 (MI355X).
//
// What it computes: QUILT/src/reference-single.cpp `Rcpp_haploid_dosage_versus_refs`
// (:2189-2413) = `Rcpp_build_eMatDH` (:272-329) + forward v3 (:878-1131) + backward v3
// (:1781-2179) + top-K picker (:129-194), for use_eMatDH = TRUE.
//
// How (MI355X-first, not the reference's loop nest):
//   * the recursion is sequential in the grid index g and needs one all-K sum per grid, so ONE
//     workgroup owns one (sample, chain, label) pass and keeps all K alpha (resp. beta) values in
//     VGPRs (fp32, 16 * NCH per lane); the per-grid sum is a wave-shuffle + LDS reduce with a single
//     s_barrier.  Hundreds of independent passes fill the 256 CUs -- no inter-workgroup traffic.
//   * per grid each lane streams 16 haplotype codes with one aligned 16-byte load of the uint8
//     `hapMatcherR` row (coalesced 1 KiB per wave instruction), gathers the emission of its code
//     from a <=256-entry fp32 table staged in LDS, and (dosage passes) checkpoints alpha to HBM in
//     a lane-interleaved order that makes every store a fully coalesced 1 KiB dwordx4 store.
//   * the backward pass re-reads that checkpoint, forms gamma = alpha * beta in registers, and
//     histograms gamma * sigma by haplotype code with fixed-point integer LDS atomics (32 bank-private
//     copies; ds_add_f32 is ~30x slower on gfx950); the histogram of grid g+1 is folded after the
//     block-sum barrier of grid g; the 32 x nMaxDH dosage mat-vec is off the serial path (k_dosage).
//   * the best-haplotype lists come from a second family of kernels with fp64 state (k_fwd64 / k_bwd64 /
//     k_topk<double>: register + LDS resident state, haplotype codes DMA'd global -> LDS): which of several
//     nearly tied haplotypes the reference (double arithmetic) reports decides the next small panel, and
//     fp32 state ranks them differently.  See the comment above those kernels.
//   * alpha/beta are renormalised every grid (the reference's always_normalize = TRUE semantics,
//     equivalent for dosage / gamma / sum(log c): test-unit-reference-single.R:588-642), which is
//     what makes fp32 state safe; emissions are built in fp64 and rounded once.
//
// Algorithmic HBM bytes: dosage pass 10 * K * G (1 B code + 4 B alpha store
// forward; 1 B code + 4 B alpha load backward), ranking pass (1 + 0.1 * 8) * 2 * K * G.
#include "fullpass_dev.hpp"
#include "fullpass_testhook.h"
#include "pass_layout.hpp"
#include "variants.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <memory>
#include <utility>

namespace {

// ---------------------------------------------------------------------------------------------
// k_emat: emission tables.  One block per (grid, pass); thread d computes the fp64 emission of
// distinct word d-1 (reference-single.cpp:294-327), the block finds min / max, applies
// normalize_emissions (:985-990) and writes the table.  Row 0 is written as 0: haplotypes with code 0
// ("specials") get their own emission from `esp` (:1002-1042).
// The per-SNP factors of the words' products are formed once per block (they do not depend on the
// word) and the block's min / max are wave reductions plus one 4-entry exchange (min and max are
// exact: any order gives the same value) -- the first form of this kernel evaluated the factors per
// word and SNP and ran three 8-step LDS trees with a barrier per step.
// ---------------------------------------------------------------------------------------------
template <typename TS>
__global__ __launch_bounds__(256) void k_emat(PassParams prm) {
    const int g = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    __shared__ double2 s_e[32];
    __shared__ double s_red[3][4];
    __shared__ int s_var;
    const int s = 32 * g;
    const int nLocal = min(32, prm.T - s);
    const double2 *gl = reinterpret_cast<const double2 *>(prm.gl) + (size_t)p * prm.T + s;
    if (t == 0) s_var = 0;
    __syncthreads();
    if (t < nLocal) {
        const double2 v = gl[t];   // x = P(reads | ref), y = P(reads | alt)
        const double eps = prm.ref_error, ome = 1.0 - eps;
        s_e[t] = make_double2(v.x * ome + v.y * eps, v.x * eps + v.y * ome);
        if (v.x != 1.0 || v.y != 1.0) s_var = 1;  // benign race: all writers store 1
    }
    __syncthreads();
    const bool has_variant = s_var != 0 || g == 1 || g == 0;
    TS *out = static_cast<TS *>(prm.emat) + ((size_t)p * prm.G + g) * kMaxRow;
    const int so = prm.sp_off[g], sn = prm.sp_off[g + 1] - so;
    // special emissions: the grid's list as it is, or (lazy: the fp64 ranking kernels) followed by 16 zero entries that
    // keep the zero-coded padding beyond K at 0 (fullpass64.hip)
    TS *esp_out = static_cast<TS *>(prm.esp) + (size_t)p * prm.esp_stride + so + (prm.lazy && sn > 0 ? 16 * prm.sp_gidx[g] : 0);
    if (prm.lazy && sn > 0 && t < 16) esp_out[sn + t] = TS(0);
    if (!has_variant) {
        // reference shortcut (:1078-1088): emission is 1 for every haplotype
        out[t] = t >= prm.nrow ? TS(0) : (t == 0) ? (sn > 0 ? TS(1) : TS(0)) : TS(1);
        for (int i = t; i < sn; i += 256) esp_out[i] = TS(1);
        if (prm.lazy && t == 0) prm.emin[(size_t)p * prm.G + g] = -1.0;   // "no variant": the forward takes the shortcut
        return;  // (never taken for g == 0)
    }
    const bool row = t >= 1 && t < prm.nrow;
    double e = 0;
    if (row) e = word_emission((uint32_t)prm.B[(size_t)g * prm.nMaxDH + (t - 1)], s_e, nLocal);
    // min over rows 1..nMaxDH (row 0 of the reference's table starts at 1 and takes the min), then the max with row 0 in it
    const int wv = t >> 6;
    const double wmin = wave_min(row ? e : 1.0);
    if ((t & 63) == 0) s_red[0][wv] = wmin;
    __syncthreads();
    const double row0 = fmin(fmin(s_red[0][0], s_red[0][1]), fmin(s_red[0][2], s_red[0][3]));
    const double wmax = wave_max(row ? e : row0);
    if ((t & 63) == 0) s_red[1][wv] = wmax;
    __syncthreads();
    const double emax = fmax(fmax(s_red[1][0], s_red[1][1]), fmax(s_red[1][2], s_red[1][3]));
    double scale = 1.0, sp_scale = 1.0;
    if (prm.normalize_emissions) {
        if (emax < 1.0) scale = 1.0 / emax;
        sp_scale = 1.0 / emax;  // specials are always divided by emission_max (:1034)
    }
    if (g == 0) {
        if (prm.lazy) {
            scale = sp_scale = 1.0;   // the reference initialises alpha(0) from the raw emissions (:2314-2347)
        } else {
            // state that cannot hold the raw emissions: scale by 1 / max here and fold the factor back into c[0] in k_fwd
            scale = sp_scale = 1.0 / emax;
        }
        if (t == 0) prm.escale0[p] = scale;
    }
    // row 0 (code 0): 0 normally, so the zero padding K..Kq and any stray code drop out; 1 on grids
    // that hold specials, whose own emission `esp` is applied by the kernels' rare path
    out[t] = t >= prm.nrow ? TS(0) : (t == 0) ? (sn > 0 ? TS(1) : TS(0)) : (TS)(e * scale);   // kMaxRow == blockDim
    double sp_min = 2.0;
    for (int i = t; i < sn; i += 256) {
        double es = word_emission(prm.sp_word[so + i], s_e, nLocal) * sp_scale;
        esp_out[i] = (TS)es;
        sp_min = fmin(sp_min, es);
    }
    if (prm.lazy) {
        // min_emission_prob of the grid (:1044-1057): the smallest table row after normalisation (row 0 holds the column
        // minimum, the initial 1 included), then the specials
        const double wsp = wave_min(sp_min);
        if ((t & 63) == 0) s_red[2][wv] = wsp;
        __syncthreads();
        if (t == 0) {
            const double m = fmin(row0 * scale, fmin(fmin(s_red[2][0], s_red[2][1]), fmin(s_red[2][2], s_red[2][3])));
            prm.emin[(size_t)p * prm.G + g] = m;
            if (g == 1) prm.emin_b1[p] = s_var != 0 ? m : -1.0;   // the backward pass does not force grid 1 (:1866-1877)
        }
    }
}

// Multiply the state of the haplotypes with code 0 ("specials": grids with more than nMaxDH distinct
// words) by their own emission (reference-single.cpp:1002-1042 / :1902-1964).  Row 0 of the LDS table
// is 1 on such grids, so x holds the un-emitted value.  A chunk's specials are consecutive entries of
// the grid's ascending list: one lower_bound per chunk that holds a zero code, then in order.
template <typename TS, int NCH>
__device__ __forceinline__ void apply_special_emissions(TS (&x)[NCH][16], const uint4 (&dh)[NCH], const PassParams &prm,
                                                        const TS *esp, int g, int NT, int t) {
    const int lo = prm.sp_off[g], hi = prm.sp_off[g + 1];
#pragma unroll
    for (int j = 0; j < NCH; j++) {
        if (!any_zero_code(dh[j])) continue;
        const int k0 = (j * NT + t) * 16;
        if (k0 >= prm.K) continue;
        int at = special_lower_bound(prm.sp_k, lo, hi, k0);
        const uint32_t w[4] = {dh[j].x, dh[j].y, dh[j].z, dh[j].w};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t code = (w[i >> 2] >> ((i & 3) * 8)) & 0xffu;
            if (code == 0 && k0 + i < prm.K) {
                x[j][i] *= esp[at];
                at++;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_fwd: forward recursion.  alpha_k <- (alpha_k + psi/sigma) * e_k, renormalised every grid
// (reference-single.cpp:935-1107 with always_normalize).  One block per pass.
// ---------------------------------------------------------------------------------------------
template <typename TS, int NCH, int MAXT>
__global__ __launch_bounds__(MAXT) void k_fwd(PassParams prm) {
    using V = typename Vec<TS>::V;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TS *etab = reinterpret_cast<TS *>(smem);                                     // [2][256]
    double *red = reinterpret_cast<double *>(smem + 2 * kMaxRow * sizeof(TS));   // [2][16]
    const int p = blockIdx.x, t = threadIdx.x, NT = blockDim.x, nwaves = NT >> 6;
    const int K = prm.K, G = prm.G;
    const int flags = prm.flags[p];
    const bool store_all = (flags & 15) != 0;
    const TS *emat = static_cast<const TS *>(prm.emat) + (size_t)p * G * kMaxRow;
    const TS *esp = static_cast<const TS *>(prm.esp) + (size_t)p * prm.esp_stride;
    V *aout = reinterpret_cast<V *>(static_cast<TS *>(prm.alpha) + (size_t)p * prm.alpha_pass_stride);
    const int32_t *slot = prm.alpha_slot + (size_t)p * G;
    const size_t col_vecs = (size_t)prm.Kq / Vec<TS>::EPV;

    TS a[NCH][16];
    uint4 dh[NCH];
    const TS invK = TS(1) / (TS)K;
    // Chunks past K carry 0 and must stay 0: their codes are 0 (never loaded), so they see a finite table entry, and the
    // additive term is switched off per chunk (one select per chunk instead of a compare per element).  `tail_star` < 16
    // marks the one lane whose chunk (row jstar) straddles K.
    uint32_t valid = 0;
    const int jstar = (K / 16) / NT;
    const int tail_star = ((K / 16) % NT == t && (K & 15)) ? (K & 15) : 16;
#pragma unroll
    for (int j = 0; j < NCH; j++) {
        const int k0 = (j * NT + t) * 16;
        valid |= (k0 < K ? 1u : 0u) << j;
#pragma unroll
        for (int i = 0; i < 16; i++) a[j][i] = (k0 + i < K) ? invK : TS(0);
        dh[j] = make_uint4(0, 0, 0, 0);
        if (k0 < K) dh[j] = *reinterpret_cast<const uint4 *>(prm.hm + k0);
    }
    for (int i = t; i < kMaxRow; i += NT) etab[i] = (i < prm.nrow) ? emat[i] : TS(0);
    __syncthreads();

    for (int g = 0; g < G; g++) {
        const TS *et = etab + (g & 1) * kMaxRow;
        TS etn[4] = {0, 0, 0, 0};  // next grid's table: rows t, t+NT, .. (NT >= 64, nrow <= 256)
        if (g + 1 < G) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (t + r * NT < prm.nrow) etn[r] = emat[(size_t)(g + 1) * kMaxRow + t + r * NT];
        }
        double sg = 0.0, sig = 1.0;
        if (g > 0) {
            sig = prm.sigma[g - 1];
            sg = (1.0 - sig) / (double)K / sig;  // psi / sigma with A_prev = 1
        }
        const TS s = (TS)sg;
#pragma unroll
        for (int j = 0; j < NCH; j++) {
            const uint32_t w[4] = {dh[j].x, dh[j].y, dh[j].z, dh[j].w};
            const TS sj = ((valid >> j) & 1u) ? s : TS(0);
            TS e[16];   // the 16 table look-ups first, back to back, then the arithmetic
#pragma unroll
            for (int i = 0; i < 16; i++) e[i] = et[(w[i >> 2] >> ((i & 3) * 8)) & 0xffu];
#pragma unroll
            for (int i = 0; i < 16; i++) a[j][i] = (a[j][i] + sj) * e[i];
        }
        if (prm.sp_off[g + 1] > prm.sp_off[g]) apply_special_emissions<TS, NCH>(a, dh, prm, esp, g, NT, t);
        TS psum = 0;
#pragma unroll
        for (int j = 0; j < NCH; j++) {
            if (j == jstar && tail_star < 16) {   // one lane of the block
#pragma unroll
                for (int i = 0; i < 16; i++) a[j][i] = i < tail_star ? a[j][i] : TS(0);
            }
#pragma unroll
            for (int i = 0; i < 16; i++) psum += a[j][i];
        }
        if (g + 1 < G) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (t + r * NT < kMaxRow) etab[((g + 1) & 1) * kMaxRow + t + r * NT] = etn[r];
        }
        const double A = block_sum((double)psum, red + (g & 1) * 16, t, nwaves);
        // the codes of the next grid: issued as early as the registers allow (temporaries are dead)
        if (g + 1 < G) {
#pragma unroll
            for (int j = 0; j < NCH; j++) {
                const int k0 = (j * NT + t) * 16;
                if (k0 < K) dh[j] = *reinterpret_cast<const uint4 *>(prm.hm + (size_t)(g + 1) * prm.Kp + k0);
            }
        }
        const double invA = 1.0 / A;
        const TS inv = (TS)invA;
        if (t == 0) prm.c[(size_t)p * G + g] = (g == 0) ? invA * prm.escale0[p] : invA / sig;
        const int sl = store_all ? g : slot[g];
#pragma unroll
        for (int j = 0; j < NCH; j++) {
#pragma unroll
            for (int i = 0; i < 16; i++) a[j][i] *= inv;
            if (sl >= 0 && (j * NT + t) * 16 < K) store_chunk<TS>(aout + (size_t)sl * col_vecs, a[j], j, NT, t);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_bwd: backward recursion; FULL adds gamma + the code histogram of the dosage passes; beta at the
// thinned grids goes to k_topk.  reference-single.cpp:1854-2177.
// ---------------------------------------------------------------------------------------------
template <typename TS, int NCH, int MAXT, bool FULL>
__global__ __launch_bounds__(MAXT) void k_bwd(PassParams prm) {
    using V = typename Vec<TS>::V;
    constexpr int EPV = Vec<TS>::EPV, NV = 16 / EPV;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    TS *etab = reinterpret_cast<TS *>(smem);                                     // [2][256]
    double *red = reinterpret_cast<double *>(smem + 2 * kMaxRow * sizeof(TS));   // [2][16]
    using Hist = typename Vec<TS>::Hist;   // uint32 at 2^-31 (fp32 state) / uint64 at 2^-62 (fp64 state)
    Hist *hist = reinterpret_cast<Hist *>(smem + 2 * kMaxRow * sizeof(TS) + 2 * 16 * 8);  // [2][kMaxRow][32] (FULL)
    const int p = blockIdx.x, t = threadIdx.x, NT = blockDim.x, nwaves = NT >> 6;
    const int lane = t & 63;
    const int K = prm.K, G = prm.G;
    const int flags = prm.flags[p];
    const bool want_dosage = FULL && (flags & 1) != 0;
    const bool store_all = (flags & 15) != 0;
    const bool want_gamma = FULL && (flags & 4) != 0, want_beta = FULL && (flags & 8) != 0;
    const TS *emat = static_cast<const TS *>(prm.emat) + (size_t)p * G * kMaxRow;
    const TS *esp = static_cast<const TS *>(prm.esp) + (size_t)p * prm.esp_stride;
    const V *ain = reinterpret_cast<const V *>(static_cast<const TS *>(prm.alpha) + (size_t)p * prm.alpha_pass_stride);
    const int32_t *slot = prm.alpha_slot + (size_t)p * G;
    const size_t col_vecs = (size_t)prm.Kq / EPV;
    const double *cvec = prm.c + (size_t)p * G;

    TS b[NCH][16];
    uint4 dh[NCH];  // codes of grid g+1 during the emission phase, then reloaded with grid g's
    uint32_t valid = 0;   // see k_fwd
    const int jstar = (K / 16) / NT;
    const int tail_star = ((K / 16) % NT == t && (K & 15)) ? (K & 15) : 16;
#pragma unroll
    for (int j = 0; j < NCH; j++) {
        const int k0 = (j * NT + t) * 16;
        valid |= (k0 < K ? 1u : 0u) << j;
#pragma unroll
        for (int i = 0; i < 16; i++) b[j][i] = (k0 + i < K) ? TS(1) : TS(0);
        dh[j] = make_uint4(0, 0, 0, 0);
    }
    // fold one grid's 32 bank-private histogram copies into prm.mg (thread = code; copies visited in a rotated order
    // so that a wave's reads spread over the banks), re-zeroing them
    auto fold_histogram = [&](int g_of) {
        Hist *h = hist + (g_of & 1) * kMaxRow * kHistCopies;
        Hist *mgo = static_cast<Hist *>(prm.mg) + ((size_t)p * G + g_of) * kMaxRow;
        for (int code = t; code < prm.nrow; code += NT) {
            Hist v = 0;
#pragma unroll 8
            for (int c = 0; c < kHistCopies; c++) {
                const int at = code * kHistCopies + ((c + lane) & (kHistCopies - 1));
                v += h[at];
                h[at] = 0;
            }
            mgo[code] = v;
        }
    };
    if (want_dosage)
        for (int i = t; i < 2 * kMaxRow * kHistCopies; i += NT) hist[i] = 0;
    for (int i = t; i < kMaxRow; i += NT)
        etab[((G - 1) & 1) * kMaxRow + i] = (i < prm.nrow) ? emat[(size_t)(G - 1) * kMaxRow + i] : TS(0);
    __syncthreads();

    for (int g = G - 1; g >= 0; --g) {
        double sig = 1.0;  // "not_jump_prob" of the reference: sigma_g, or 1 at the last grid
        if (g < G - 1) {
            TS etn[4] = {0, 0, 0, 0};  // table of grid g (the emission side of iteration g-1)
            if (g > 0) {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (t + r * NT < prm.nrow) etn[r] = emat[(size_t)g * kMaxRow + t + r * NT];
            }
            sig = prm.sigma[g];
            const TS *et = etab + ((g + 1) & 1) * kMaxRow;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
                const uint32_t w[4] = {dh[j].x, dh[j].y, dh[j].z, dh[j].w};
                TS e[16];   // look-ups first, back to back
#pragma unroll
                for (int i = 0; i < 16; i++) e[i] = et[(w[i >> 2] >> ((i & 3) * 8)) & 0xffu];
#pragma unroll
                for (int i = 0; i < 16; i++) b[j][i] *= e[i];
            }
            if (prm.sp_off[g + 2] > prm.sp_off[g + 1]) apply_special_emissions<TS, NCH>(b, dh, prm, esp, g + 1, NT, t);
            TS psum = 0;
#pragma unroll
            for (int j = 0; j < NCH; j++)
#pragma unroll
                for (int i = 0; i < 16; i++) psum += b[j][i];
            // codes of grid g: histogram side below (dosage passes), emission side of the next iteration.
            // Issued here, after the last use of grid g+1's codes, so one register set serves both.
#pragma unroll
            for (int j = 0; j < NCH; j++) {
                const int k0 = (j * NT + t) * 16;
                if (k0 < K) dh[j] = *reinterpret_cast<const uint4 *>(prm.hm + (size_t)g * prm.Kp + k0);
            }
            // buffer (g & 1) was last read in iteration g + 1, before that iteration's barrier
            if (g > 0) {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (t + r * NT < kMaxRow) etab[(g & 1) * kMaxRow + t + r * NT] = etn[r];
            }
            const double S = block_sum((double)psum, red + (g & 1) * 16, t, nwaves);
            // every wave is past its atomics of grid g+1 (they precede this barrier), and none reaches the atomics of
            // grid g-1 (same buffer) before the next barrier: fold grid g+1 here, without a barrier of its own
            if constexpr (FULL) {
                if (want_dosage && (store_all || slot[g + 1] >= 0)) fold_histogram(g + 1);
            }
            const TS add = (TS)((1.0 - sig) / (double)K / sig * S);
#pragma unroll
            for (int j = 0; j < NCH; j++) {
                const TS aj = ((valid >> j) & 1u) ? add : TS(0);
#pragma unroll
                for (int i = 0; i < 16; i++) b[j][i] += aj;
                if (j == jstar && tail_star < 16) {   // one lane of the block
#pragma unroll
                    for (int i = 0; i < 16; i++) b[j][i] = i < tail_star ? b[j][i] : TS(0);
                }
            }
        }

        if (g == G - 1) {
#pragma unroll
            for (int j = 0; j < NCH; j++) {
                const int k0 = (j * NT + t) * 16;
                if (k0 < K) dh[j] = *reinterpret_cast<const uint4 *>(prm.hm + (size_t)g * prm.Kp + k0);
            }
        }
        const int tcol = prm.thin_col[g];
        if constexpr (FULL) {
            const int sl = store_all ? g : slot[g];
            const bool need_gamma = (want_dosage || want_gamma) && sl >= 0;
            if (need_gamma) {
                const V *src = ain + (size_t)sl * col_vecs;
                const bool has_sp = prm.sp_off[g + 1] > prm.sp_off[g];
                Hist *h = hist + (g & 1) * kMaxRow * kHistCopies;
                const TS fs = (TS)sig;
                // alpha is streamed through a 2-chunk register pipeline: chunk j+1 is in flight while chunk
                // j is consumed (holding all 16 * NCH values would double the register footprint)
                V av[2][NV];
                if (t * 16 < K) {
#pragma unroll
                    for (int q = 0; q < NV; q++) av[0][q] = src[alpha_vec_index<NV>(0, q, NT, t)];
                }
#pragma unroll
                for (int j = 0; j < NCH; j++) {
                    const int k0 = (j * NT + t) * 16;
                    if (j + 1 < NCH && ((j + 1) * NT + t) * 16 < K) {
#pragma unroll
                        for (int q = 0; q < NV; q++) av[(j + 1) & 1][q] = src[alpha_vec_index<NV>(j + 1, q, NT, t)];
                    }
                    if (k0 < K) {
                        const uint32_t w[4] = {dh[j].x, dh[j].y, dh[j].z, dh[j].w};
                        int sp_at = 0;
                        if (want_dosage && has_sp && any_zero_code(dh[j]))
                            sp_at = special_lower_bound(prm.sp_k, prm.sp_off[g], prm.sp_off[g + 1], k0);
#pragma unroll
                        for (int q = 0; q < NV; q++) {
                            TS gq[EPV];
#pragma unroll
                            for (int r = 0; r < EPV; r++) {
                                const int i = EPV * q + r;
                                const TS gk = vget(av[j & 1][q], r) * b[j][i];  // 0 beyond K: b is 0 there
                                gq[r] = gk * fs;
                                if (want_dosage) {
                                    const uint32_t code = (w[i >> 2] >> ((i & 3) * 8)) & 0xffu;
                                    if constexpr (sizeof(TS) == 8)
                                        atomicAdd(&h[code * kHistCopies + (lane & 31)], (Hist)((double)gq[r] * kHistScale64 + 0.5));
                                    else
                                        atomicAdd(&h[code * kHistCopies + (lane & 31)], (Hist)((float)gq[r] * kHistScale + 0.5f));
                                    if (has_sp && code == 0 && k0 + i < K) {
                                        // gamma of a special haplotype goes to its own list (:2096-2128)
                                        static_cast<TS *>(prm.gsp)[(size_t)p * prm.n_special + sp_at] = gk;
                                        sp_at++;
                                    }
                                }
                            }
                            if (want_gamma) {
                                V *dst = reinterpret_cast<V *>(prm.gamma_out) + ((size_t)p * G + g) * col_vecs;
                                dst[alpha_vec_index<NV>(j, q, NT, t)] = vmake(gq);
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (tcol >= 0 && prm.beta_thin) {
            // thinned grid: hand the (unscaled) beta column to k_topk, which forms gamma = alpha * beta
            // and picks the top matches off the serial path (:2020-2031)
            V *dst = reinterpret_cast<V *>(prm.beta_thin) + ((size_t)p * prm.n_thin + tcol) * col_vecs;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
                if ((j * NT + t) * 16 >= K) continue;
                store_chunk<TS>(dst, b[j], j, NT, t);
            }
        }
        // beta *= c_g * sigma_g   (:2165-2166)
        const TS x = (TS)(cvec[g] * sig);
#pragma unroll
        for (int j = 0; j < NCH; j++) {
#pragma unroll
            for (int i = 0; i < 16; i++) b[j][i] *= x;
        }
        if (want_beta) {
            V *dst = reinterpret_cast<V *>(prm.beta_out) + ((size_t)p * G + g) * col_vecs;
#pragma unroll
            for (int j = 0; j < NCH; j++) store_chunk<TS>(dst, b[j], j, NT, t);
        }
    }
    if constexpr (FULL) {
        if (want_dosage && (store_all || slot[0] >= 0)) {
            __syncthreads();
            fold_histogram(0);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_topk: best haplotypes at one thinned grid of one pass (reference-single.cpp:129-194, :2020-2031).
// threshold = K_top-th largest gamma counted with multiplicity; every k with gamma >= threshold is
// reported with gamma * not_jump_prob.  One block per (thinned column, pass); alpha and beta columns
// are in the same lane-interleaved order, so gamma is an elementwise product of two coalesced streams.
// WIDE (K_top in kMaxTop + 1 .. kMaxTopWide): the per-lane lists stay kMaxTop deep, so the K_top-th largest of the 256 x
// kMaxTop retained values is only a lower bound T of the threshold.  It is the threshold unless some lane dropped a value
// above it, i.e. unless a lane's whole list lies above T; then the values above T are gathered in LDS (a column pass) and
// the threshold is their K_top-th largest by rank counting -- or T, when fewer than K_top lie above it.  A gather that
// outgrows the LDS list raises T to the K_top-th largest of what it caught (still a lower bound: of a subset) and repeats;
// each round drops at least kWideList - K_top values, and with at most 63 retained values above the first T no more than
// 7 lanes can hold dropped ones, so up to Kq = 72 448 the first gather already fits.  Lists of up to 64 entries are put
// in order by rank counting, an entry per thread (the narrow form: by thread 0).
// ---------------------------------------------------------------------------------------------
constexpr int kMaxTopWide = 64;   // QA_K_TOP_MATCHES_MAX
constexpr int kWideList = 2048;   // gathered values above the lower bound (LDS)

template <typename TS, bool WIDE = false>
__global__ __launch_bounds__(256) void k_topk(PassParams prm, int NT) {
    using V = typename Vec<TS>::V;
    constexpr int EPV = Vec<TS>::EPV, NV = 16 / EPV;
    // one block per (thinned column, pass), or per entry of the to-do list (the grids the fused picker of the fp64
    // ranking kernels handed over)
    const int tcol = prm.topk_todo ? prm.topk_todo[2 * blockIdx.x + 1] : blockIdx.x;
    const int p = prm.topk_todo ? prm.topk_todo[2 * blockIdx.x] : blockIdx.y;
    const int t = threadIdx.x, lane = t & 63;
    constexpr int kTopW = WIDE ? kMaxTopWide : kMaxTop;   // entries of a wave's merged list
    __shared__ TS s_top[4][kTopW];
    __shared__ int s_cnt;
    __shared__ int s_g;
    if (t == 0) {
        s_cnt = 0;
        int g = 0;
        for (int i = 0; i < prm.G; i++) if (prm.thin_col[i] == tcol) g = i;
        s_g = g;
    }
    __syncthreads();
    const int g = s_g;
    const int flags = prm.flags[p];
    const int sl = (flags & 15) ? g : prm.alpha_slot[(size_t)p * prm.G + g];
    const size_t col_vecs = (size_t)prm.Kq / EPV;
    const V *av = reinterpret_cast<const V *>(static_cast<const TS *>(prm.alpha) + (size_t)p * prm.alpha_pass_stride) + (size_t)sl * col_vecs;
    const V *bv = reinterpret_cast<const V *>(prm.beta_thin) + ((size_t)p * prm.n_thin + tcol) * col_vecs;
    const int Ktop = prm.K_top;
    const int nvec = prm.Kq / EPV;
    TS ltop[kMaxTop];
#pragma unroll
    for (int q = 0; q < kMaxTop; q++) ltop[q] = 0;
    auto k_of = [&](int v, int r) {
        const int j = v / (NT * NV), rem = v % (NT * NV);
        const int tt = (rem / (64 * NV)) * 64 + (rem & 63), q = (rem >> 6) % NV;
        return (j * NT + tt) * 16 + EPV * q + r;
    };
    auto gamma_of = [&](int v, TS (&gq)[EPV]) {
        const V a4 = av[v], b4 = bv[v];
#pragma unroll
        for (int r = 0; r < EPV; r++) gq[r] = vget(a4, r) * vget(b4, r);
    };
    for (int v = t; v < nvec; v += 256) {
        if (k_of(v, 0) >= prm.K) continue;
        TS gq[EPV];
        gamma_of(v, gq);
#pragma unroll
        for (int r = 0; r < EPV; r++) {
            TS x = (k_of(v, r) < prm.K) ? gq[r] : TS(0);
#pragma unroll
            for (int z = 0; z < kMaxTop; z++) {
                if (WIDE || z < Ktop) {
                    const TS hi = ltop[z] > x ? ltop[z] : x;
                    x = ltop[z] > x ? x : ltop[z];
                    ltop[z] = hi;
                }
            }
        }
    }
    const TS lane_min = ltop[kMaxTop - 1];   // (WIDE) everything this lane dropped is <= this
    // wave merge: pop the maximum Ktop times
    for (int r = 0; r < Ktop; r++) {
        const TS m = wave_max(ltop[0]);
        const unsigned long long owners = __ballot(ltop[0] == m);
        const int first = __ffsll((long long)owners) - 1;
        if (lane == first) {
#pragma unroll
            for (int q = 0; q < kMaxTop - 1; q++) ltop[q] = ltop[q + 1];
            ltop[kMaxTop - 1] = 0;
        }
        if (lane == 0) s_top[t >> 6][r] = m;
    }
    __syncthreads();
    TS thr = 0;
    {
        TS head = 0;
        int pos = 0;
        if (lane < 4) head = s_top[lane][0];
        for (int r = 0; r < Ktop; r++) {
            const TS m = wave_max(head);
            thr = m;
            const unsigned long long owners = __ballot(lane < 4 && head == m);
            const int first = __ffsll((long long)owners) - 1;
            if (lane == first) {
                pos++;
                head = (pos < Ktop) ? s_top[lane][pos] : TS(0);
            }
        }
    }
    if constexpr (WIDE) {
        __shared__ TS s_list[kWideList];
        __shared__ TS s_thr;
        bool dropped_above = lane_min > thr;
        while (__syncthreads_or(dropped_above)) {   // (the barrier also covers s_cnt = 0 and the last round's reads of s_list)
            for (int v = t; v < nvec; v += 256) {
                if (k_of(v, 0) >= prm.K) continue;
                TS gq[EPV];
                gamma_of(v, gq);
#pragma unroll
                for (int r = 0; r < EPV; r++) {
                    if (k_of(v, r) < prm.K && gq[r] > thr) {
                        const int at = atomicAdd(&s_cnt, 1);
                        if (at < kWideList) s_list[at] = gq[r];
                    }
                }
            }
            __syncthreads();
            const int n_gt = s_cnt, n = min(n_gt, kWideList);
            if (n >= Ktop) {
                // the Ktop-th largest of the list, counted with multiplicity: x with #(> x) < Ktop <= #(>= x)
                for (int i = t; i < n; i += 256) {
                    const TS x = s_list[i];
                    int gt = 0, ge = 0;
                    for (int j = 0; j < n; j++) { const TS y = s_list[j]; gt += y > x; ge += y >= x; }
                    if (gt < Ktop && Ktop <= ge) s_thr = x;   // (every writer writes the same value)
                }
            }
            __syncthreads();
            if (n >= Ktop) thr = s_thr;
            if (t == 0) s_cnt = 0;
            dropped_above = n_gt > kWideList;   // the list was a subset: thr is a better lower bound, gather again
        }
    }
    const TS fs = (g < prm.G - 1) ? (TS)prm.sigma[g] : TS(1);
    int32_t *oi = prm.top_idx + ((size_t)p * prm.n_thin + tcol) * prm.top_cap;
    TS *ov = static_cast<TS *>(prm.top_val) + ((size_t)p * prm.n_thin + tcol) * prm.top_cap;
    for (int v = t; v < nvec; v += 256) {
        if (k_of(v, 0) >= prm.K) continue;
        TS gq[EPV];
        gamma_of(v, gq);
#pragma unroll
        for (int r = 0; r < EPV; r++) {
            const int kk = k_of(v, r);
            if (kk < prm.K && gq[r] >= thr) {
                const int at = atomicAdd(&s_cnt, 1);
                if (at < prm.top_cap) { oi[at] = kk; ov[at] = gq[r] * fs; }
            }
        }
    }
    __syncthreads();
    const int n_all = s_cnt;
    if (n_all > prm.top_cap && prm.truncate_lists) {
        // More matches than the list holds (exact ties at the threshold, e.g. haplotypes identical over the
        // whole region).  Keep what the host logic can ever look at first: every gamma above the
        // threshold, then the tied ones by ascending haplotype -- i.e. the head of the ordered list.
        __shared__ int s_n;
        auto block_count = [&](int kb) {   // #matches with gamma > thr, or gamma == thr and k <= kb
            __syncthreads();
            if (t == 0) s_n = 0;
            __syncthreads();
            int mine = 0;
            for (int v = t; v < nvec; v += 256) {
                if (k_of(v, 0) >= prm.K) continue;
                TS gq[EPV];
                gamma_of(v, gq);
#pragma unroll
                for (int r = 0; r < EPV; r++) {
                    const int kk = k_of(v, r);
                    if (kk < prm.K && (gq[r] > thr || (gq[r] == thr && kk <= kb))) mine++;
                }
            }
            atomicAdd(&s_n, mine);
            __syncthreads();
            return s_n;
        };
        int lo = -1, hi = prm.K - 1;   // smallest kb with count(kb) >= top_cap (count(-1) < top_cap: fewer than K_top above thr)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (block_count(mid) >= prm.top_cap) hi = mid; else lo = mid;
        }
        const int kb = (block_count(lo) >= prm.top_cap) ? lo : hi;
        __syncthreads();
        if (t == 0) s_cnt = 0;
        __syncthreads();
        for (int v = t; v < nvec; v += 256) {
            if (k_of(v, 0) >= prm.K) continue;
            TS gq[EPV];
            gamma_of(v, gq);
#pragma unroll
            for (int r = 0; r < EPV; r++) {
                const int kk = k_of(v, r);
                if (kk < prm.K && (gq[r] > thr || (gq[r] == thr && kk <= kb))) {
                    const int at = atomicAdd(&s_cnt, 1);
                    if (at < prm.top_cap) { oi[at] = kk; ov[at] = gq[r] * fs; }
                }
            }
        }
        __syncthreads();
    }
    if constexpr (WIDE) {
        // the same order by rank counting, an entry per thread: thread 0's insertion sort below moves a list of 64 through global
        // memory about a thousand times (0.4 ms per block; a third of the kernel's time at K_top = 64)
        __shared__ int32_t s_oi[64];
        __shared__ TS s_ov[64];
        const int n = min(min(s_cnt, prm.top_cap), n_all);
        if (n <= 64 && (n_all <= prm.top_cap || prm.truncate_lists)) {   // (uniform over the block)
            if (t < n) { s_oi[t] = oi[t]; s_ov[t] = ov[t]; }
            __syncthreads();
            if (t < n) {
                const int ki = s_oi[t];
                const TS vi = s_ov[t];
                int rank = 0;
                for (int j = 0; j < n; j++) rank += (s_ov[j] > vi || (s_ov[j] == vi && s_oi[j] < ki)) ? 1 : 0;
                oi[rank] = ki;
                ov[rank] = vi;
            }
        }
        if (t == 0) prm.top_cnt[(size_t)p * prm.n_thin + tcol] = n_all;
        return;
    }
    if (t == 0) {
        prm.top_cnt[(size_t)p * prm.n_thin + tcol] = n_all;
        const int n = min(min(s_cnt, prm.top_cap), n_all);
        // order as everything_per_hap_rejig_haps does (functions.R:2161-2170): value descending, ties by
        // ascending haplotype (R's stable order() on the k-ascending list).  Lists are ~K_top long.
        if (n <= 64 && (n_all <= prm.top_cap || prm.truncate_lists)) {
            for (int i = 1; i < n; i++) {
                const int ki = oi[i];
                const TS vi = ov[i];
                int j = i - 1;
                while (j >= 0 && (ov[j] < vi || (ov[j] == vi && oi[j] > ki))) { oi[j + 1] = oi[j]; ov[j + 1] = ov[j]; j--; }
                oi[j + 1] = ki;
                ov[j + 1] = vi;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_dosage: dosage[32g + b] = sigma_g * ( sum_d IE[d, 32g+b] * mg[d] + sum_specials gamma * (bit ? 1-eps : eps) )
// (reference-single.cpp:2092-2139).
// One wave per four consecutive grids, a lane per (grid, pair of SNPs): the wave's 128 dosages are 1 KiB of consecutive
// memory, stored with one instruction (16 bytes per lane), a block's four waves write 4 KiB -- the rows usually lie in the
// caller's pinned buffer, across PCIe.  (The first form ran one block of 32 x 8 threads per grid, 256 bytes per block:
// 512 000 blocks per 256 passes, 8 ms per launch for 131 MB.)  The sums keep that form's order: the codes d = 1 + q,
// 9 + q, ... into partial sum q (q = 0..7), the partial sums added in order.
// ---------------------------------------------------------------------------------------------
constexpr int kDosageGridsPerBlock = 16;

template <typename TS>
__global__ __launch_bounds__(256) void k_dosage(PassParams prm) {
    using Hist = typename Vec<TS>::Hist;
    const int p = blockIdx.y;
    if (!(prm.flags[p] & 1)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * kDosageGridsPerBlock + wave * 4 + (lane >> 4);
    if (g >= prm.G) return;                 // (no barrier below)
    const int b0 = 2 * (lane & 15), b1 = b0 + 1;   // this lane's SNPs of the grid
    const int s = 32 * g;
    const int nLocal = min(32, prm.T - s);
    const Hist *mg = static_cast<const Hist *>(prm.mg) + ((size_t)p * prm.G + g) * kMaxRow;
    const double eps = prm.ref_error, ome = 1.0 - eps;
    const double unit = sizeof(TS) == 8 ? prm.hist_unit : 1.0 / (double)kHistScale;
    // per partial sum q: histogram part (already times sigma_g) of both SNPs, specials (raw gamma), the grid's mass
    double acc0[8], acc1[8], sp0[8], sp1[8], mass[8];
#pragma unroll
    for (int q = 0; q < 8; q++) acc0[q] = acc1[q] = sp0[q] = sp1[q] = mass[q] = 0;
    const int32_t *Bg = prm.B + (size_t)g * prm.nMaxDH;
    const double *IE0 = prm.IE ? prm.IE + (size_t)(s + min(b0, nLocal - 1)) * prm.nMaxDH : nullptr;
    const double *IE1 = prm.IE ? prm.IE + (size_t)(s + min(b1, nLocal - 1)) * prm.nMaxDH : nullptr;
    mass[0] += (double)mg[0] * unit;        // bin 0 holds the specials' share of the grid's total gamma * sigma
    for (int d0 = 1; d0 < prm.nrow; d0 += 8) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int d = d0 + q;
            if (d < prm.nrow) {
                const double m = (double)mg[d] * unit;
                mass[(q + 1) & 7] += m;     // (d & 7: d0 = 1 mod 8)
                double ie0, ie1;
                if (prm.IE) {
                    ie0 = IE0[d - 1];
                    ie1 = IE1[d - 1];
                } else {
                    const uint32_t w = (uint32_t)Bg[d - 1];
                    ie0 = ((w >> b0) & 1u) ? ome : eps;
                    ie1 = ((w >> b1) & 1u) ? ome : eps;
                }
                acc0[q] += ie0 * m;
                acc1[q] += ie1 * m;
            }
        }
    }
    const int so = prm.sp_off[g], sn = prm.sp_off[g + 1] - so;
    for (int i0 = 0; i0 < sn; i0 += 8) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const int i = i0 + q;
            if (i < sn) {
                const double gk = (double)static_cast<const TS *>(prm.gsp)[(size_t)p * prm.n_special + so + i];
                const uint32_t w = prm.sp_word[so + i];
                sp0[q] += gk * (((w >> b0) & 1u) ? ome : eps);
                sp1[q] += gk * (((w >> b1) & 1u) ? ome : eps);
            }
        }
    }
    const double sig = (g < prm.G - 1) ? prm.sigma[g] : 1.0;
    double tot0 = 0, tot1 = 0, ms = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        tot0 += acc0[q] + sp0[q] * sig;
        tot1 += acc1[q] + sp1[q] * sig;
        ms += mass[q];
    }
    // gamma * sigma_g of a grid (what the histogram accumulates) sums to 1 (reference-single.cpp:2048-2091, :2170-2176;
    // the reference's test suite checks colSums(gamma_t) == 1).  Dividing by the mass actually accumulated removes the
    // common-mode drift of the state's scale (with fp32 state ~3e-8 per grid, 6e-5 over 2 000 grids), which is all
    // the dosage of a long region would otherwise inherit from 2 000 renormalisations in single precision.
    if (ms > 0) {
        tot0 /= ms;
        tot1 /= ms;
    }
    double *dst = prm.dosage + (size_t)p * prm.T + s + b0;
    if (b1 < nLocal && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<double2 *>(dst) = make_double2(tot0, tot1);
    } else {
        if (b0 < nLocal) dst[0] = tot0;
        if (b1 < nLocal) dst[1] = tot1;
    }
}

// ---------------------------------------------------------------------------------------------
// k_make_gl: per-label genotype likelihoods of a pass from the sample's reads and the current read
// labels: make_gl_from_u_bq (QUILT/R/reference-single.R:19-42) + Rcpp_make_gl_bound
// (reference-single.cpp:68-94).  One thread per (SNP, pass); the bases covering a SNP come from a
// per-sample SNP-major index (built once on the host), in read order, so the product order is the
// reference's.
// ---------------------------------------------------------------------------------------------
struct GlParams {
    int P, T;
    const int32_t *pass_sample;  // [P]
    const int32_t *pass_label;   // [P] 1-based
    const int32_t *pass_hoff;    // [P] offset of the pass's chain into H
    const int32_t *snp_ptr;      // [n_sample][T + 1] (local offsets)
    const int32_t *ent_off;      // [n_sample] offset into ent_*
    const int32_t *ent_read;     // read index (within the sample) of each base
    const int32_t *ent_bq;       // its signed base quality
    const int32_t *H;            // labels
    const double *pR_tab, *pA_tab;
    double minGLValue;
    double *gl;                  // [P][T][2]
};

__global__ __launch_bounds__(256) void k_make_gl(GlParams p) {
    const int t = blockIdx.x * 256 + threadIdx.x, pi = blockIdx.y;
    if (t >= p.T) return;
    const int s = p.pass_sample[pi], lab = p.pass_label[pi];
    const int32_t *sp = p.snp_ptr + (size_t)s * (p.T + 1);
    const int32_t *er = p.ent_read + p.ent_off[s], *eb = p.ent_bq + p.ent_off[s];
    const int32_t *H = p.H + p.pass_hoff[pi];
    double a = 1.0, b = 1.0;
    for (int i = sp[t]; i < sp[t + 1]; i++) {
        const int bq = eb[i];
        if (bq == 0 || H[er[i]] != lab) continue;
        const int ab = bq < 0 ? -bq : bq;
        a *= p.pR_tab[(bq > 0 ? 256 : 0) + ab];
        b *= p.pA_tab[(bq > 0 ? 256 : 0) + ab];
    }
    if (p.minGLValue > 0 && (a < p.minGLValue || b < p.minGLValue)) {
        if (a > b) { b = b / a; a = 1; if (b < p.minGLValue) b = p.minGLValue; }
        else       { a = a / b; b = 1; if (a < p.minGLValue) a = p.minGLValue; }
    }
    double2 *out = reinterpret_cast<double2 *>(p.gl) + (size_t)pi * p.T + t;
    *out = make_double2(a, b);
}

// un-permute a lane-interleaved [cols][Kq] matrix into a K x cols double matrix (column-major)
template <typename TS>
__global__ void k_unpermute(const TS *src, double *dst, int K, int Kq, int NT, int cols, size_t dst_ld) {
    constexpr int EPV = Vec<TS>::EPV, NV = 16 / EPV;
    const int col = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K || col >= cols) return;
    const int chunk = k >> 4, e = k & 15;
    const int j = chunk / NT, t = chunk % NT;
    const size_t vec = alpha_vec_index<NV>(j, e / EPV, NT, t);
    dst[(size_t)col * dst_ld + k] = (double)src[(size_t)col * Kq + vec * EPV + (e % EPV)];
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct qa_panel::Scratch {
    qa::ABuf<double> gl, c, dosage, escale0, unperm, emin, emin_b1, spill, fw_add, fw_xs, gamma_col;
    qa::ABuf<char> emat, esp, alpha, gamma, beta, beta_thin, top_val, mg, gsp;   // fp32 or fp64 elements (the launch decides)
    qa::ABuf<int32_t> thin_col, flags, alpha_slot, top_cnt, top_idx;
    qa::DBuf<int32_t> todo;   // (grid, pass) pairs handed to k_topk: persistent, grow-only
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    explicit Scratch(qa::Arena *a) {
        gl.arena = c.arena = dosage.arena = escale0.arena = unperm.arena = emin.arena = emin_b1.arena = spill.arena = fw_add.arena = fw_xs.arena = a;
        gamma_col.arena = a;
        emat.arena = esp.arena = alpha.arena = mg.arena = gsp.arena = gamma.arena = beta.arena = beta_thin.arena = top_val.arena = a;
        thin_col.arena = flags.arena = alpha_slot.arena = top_cnt.arena = top_idx.arena = a;
    }
    ~Scratch() {
        for (auto &e : ev) if (e) (void)hipEventDestroy(e);
    }
};

void qa::drop_pass_scratch(qa_panel *p) {
    delete p->scratch;
    p->scratch = nullptr;
}

qa_panel::~qa_panel() {
    delete scratch;
    if (gibbs_stream) (void)hipStreamDestroy(gibbs_stream);
    if (pass_stream) (void)hipStreamDestroy(pass_stream);
    if (stream) (void)hipStreamDestroy(stream);
}

namespace {

thread_local double g_timing[6] = {0, 0, 0, 0, 0, 0};   // emat, forward, backward, dosage, separate top-K, total

// (the kinds of kernels that run a pass -- PassKind -- and the launch Geometry: pass_layout.hpp)
using qa::PassKind; using qa::KIND_F32; using qa::KIND_F64_RANK; using qa::KIND_F64_FULL; using qa::KIND_F64_DOS; using qa::KIND_F64_REF;
using qa::Geometry; using qa::PanelDims; using qa::PassLayout; using qa::Thin;
static_assert(qa::kLayoutMaxRow == kMaxRow, "pass_layout.hpp sizes emat / mg rows of kMaxRow");

// what a kind is called in messages, and its rows in the kernel profile
struct KindInfo { const char *name; int pk_fwd, pk_bwd; };
constexpr KindInfo kKindInfo[qa::KIND_COUNT] = {
    /* KIND_F32      */ {"fp32", qa::PK_FWD, qa::PK_BWD},
    /* KIND_F64_RANK */ {"fp64 ranking", qa::PK_FWD64, qa::PK_BWD64},
    /* KIND_F64_FULL */ {"generic fp64", qa::PK_FWD64G, qa::PK_BWD64G},
    /* KIND_F64_DOS  */ {"fp64 dosage", qa::PK_FWD64D, qa::PK_BWD64D},
    /* KIND_F64_REF  */ {"reference-order validation", qa::PK_FWD64G, qa::PK_BWD64G},
};

// Register-resident geometry: NT threads (multiple of 64) x NCH chunks of 16 haplotypes per lane.  fp32 state:
// NT <= 512 so that each wave may use 256 VGPRs.  The smallest NCH that covers K gives the most waves; tiny panels
// still get >= 2 chunks per lane for ILP.  KIND_F64_RANK: 512 threads, chunk rows of 8192 haplotypes (fullpass64.hip).
// KIND_F64_FULL: 256 threads, NCH = ceil(K / 4096) rounded up to a built variant.  KIND_F64_REF: the same up to the largest
// built variant (so that nothing moves there), NCH = ceil(K / 4096) beyond.
// The NCH values pick_geometry chooses from (whatever the build flavour: K -> geometry -> layout is the same in every build), and
// those this build holds kernels for: all of them, or with QA_FAST_BUILD one of each kind.
using Nch32 = qa::IntList<1, 2, 3, 4, 5, 6, 7, 8, 10, 12>;
using Nch64 = qa::IntList<1, 2, 4, 6, 8, 10, 12, 13, 14>;
#ifdef QA_FAST_BUILD
using Nch32Built = qa::IntList<2, 7>;
using Nch64Built = qa::IntList<2, 13>;
#else
using Nch32Built = Nch32;
using Nch64Built = Nch64;
#endif
Geometry pick_geometry(int K, PassKind kind = KIND_F32) {
    const int chunks = (K + 15) / 16;
    if (kind == KIND_F64_RANK || kind == KIND_F64_DOS) {
        int nch = qa::fb64_chunks(K);
        if (kind == KIND_F64_DOS && nch && qa::fb64_dos_lds_bytes(K) > 160 * 1024) nch = 0;
        return {nch ? 512 : 0, nch, kind};
    }
    if (kind == KIND_F64_FULL || kind == KIND_F64_REF) {   // (the validation kernels write the generic kernels' layout)
        const int need = (K + 4095) / 4096;
        for (int nch : Nch64::values) if (nch >= need) return {256, nch, kind};
        // The list is the generic kernels' BUILT variants.  The validation kernels take the layout's NT and Kq at run time and keep
        // a pass's state in HBM (PassParams::spill) once it exceeds LDS, so beyond the list they get the layout of exactly the
        // chunk rows K needs: any K.
        if (kind == KIND_F64_REF) return {256, need, kind};
        return {0, 0, kind};
    }
    auto fit = [&](int nch) -> int {
        int nt = (chunks + nch - 1) / nch;
        nt = std::max((nt + 63) / 64 * 64, 64);
        if (nt > 512) return 0;
        if (nch == 1 && chunks > 128) return 0;
        return nt;
    };
    for (int nch : Nch32::values) if (int nt = fit(nch)) return {nt, nch, kind};
    return {0, 0, kind};
}


// the calling thread's last launch set as planned and as carved (fullpass_testhook.h)
struct LastPlan { int64_t P = 0, per_pass = 0, fixed = 0, carved = 0, kind = 0; };
thread_local LastPlan g_last_plan;

PanelDims dims_of(const qa_panel *pn) { return {pn->K, pn->G, pn->T, pn->n_special, pn->n_sp_grids}; }

// the plan of a launch set of passes that all carry `flag`: bytes per pass
size_t plan_pass_bytes(const qa_panel *pn, const Geometry &geo, int32_t flag, const Thin &thin, int K_top, int top_cap = 64,
                       bool gamma_col = false, bool alpha_grid0 = false) {
    return PassLayout(dims_of(pn), geo, qa::make_request(&flag, 1, thin, K_top, top_cap, gamma_col, alpha_grid0)).pass_bytes(qa::Arena::kCarveAlign);
}

// how many homogeneous passes fit, and make the arena big enough for them.  The fixed term pays for what a launch set carves
// once (pass_layout.hpp lists it); extra_fixed: the single-pass entry's un-permute staging.
int plan_chunk(qa_panel *pn, size_t per_pass, int remaining, size_t extra_fixed = 0) {
    const size_t fixed = (size_t)pn->G * 8 + ((size_t)2 << 20) + extra_fixed;
    g_last_plan.per_pass = (int64_t)per_pass;
    g_last_plan.fixed = (int64_t)fixed;
    const size_t budget = pn->plan_budget();
    long n = budget > fixed ? (long)((budget - fixed) / per_pass) : 0;
    n = std::max<long>(1, std::min<long>(n, remaining));
    // One pass is one workgroup and a compute unit holds one such workgroup: a launch runs in rounds of n_cu passes.  When
    // the passes have to be split anyway, split at whole rounds (292 passes cost two rounds, 256 + 36, like 512 would).
    static const int n_cu = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
        return std::max(prop.multiProcessorCount, 1);
    }();
    if (n < remaining && n > n_cu) n = n / n_cu * n_cu;
    try {
        pn->require_scratch(fixed + (size_t)n * per_pass);
    } catch (const qa::HipError &e) {
        // not even the smallest launch set (n = 1 when the budget holds no pass) could be allocated: the panel is too large for
        // this device's memory, which is the only limit of the kinds that keep a pass's state in HBM
        (void)hipGetLastError();
        char b[768];
        snprintf(b, sizeof b, "K = %d, nGrids = %d: a launch set of %ld pass(es) needs %zu bytes of device scratch: %s", pn->K, pn->G, n,
                 fixed + (size_t)n * per_pass, e.what());
        throw qa::CapacityError(b);
    }
    pn->A().reset();
    return (int)n;
}

template <typename TS, int NCH, int MAXT, bool FULL>
void launch_fb(const PassParams &prm, int NT, hipStream_t s, hipEvent_t e_mid) {
    const size_t lds_f = 2 * kMaxRow * sizeof(TS) + 2 * 16 * 8;
    const size_t lds_b = lds_f + (FULL ? (size_t)2 * kMaxRow * kHistCopies * sizeof(typename Vec<TS>::Hist) : 0);
    hipLaunchKernelGGL((k_fwd<TS, NCH, MAXT>), dim3(prm.P), dim3(NT), lds_f, s, prm);
    QA_HIP(hipGetLastError());
    QA_HIP(hipEventRecord(e_mid, s));
    QA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_bwd<TS, NCH, MAXT, FULL>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    hipLaunchKernelGGL((k_bwd<TS, NCH, MAXT, FULL>), dim3(prm.P), dim3(NT), lds_b, s, prm);
    QA_HIP(hipGetLastError());
}

// ord: reference-order launch sets of two or more passes take the batched kernels (qa_panel_set_sum_order_batched)
void launch_fb_any(const Geometry &geo, const PassParams &prm, hipStream_t st, hipEvent_t e_mid, bool ord) {
    if (geo.kind == KIND_F64_DOS) {
        qa::launch_fb64_dosage(&prm, st, e_mid);
        return;
    }
    if (geo.kind == KIND_F64_RANK) {
        qa::launch_fb64(&prm, st, e_mid);
        return;
    }
    if (geo.kind == KIND_F64_REF) {
        if (ord && prm.P >= 2) qa::launch_fb_ord(&prm, geo.NT, st, e_mid);
        else qa::launch_fb_ref(&prm, geo.NT, st, e_mid);
        return;
    }
    const bool built = geo.kind == KIND_F64_FULL
        ? qa::dispatch(Nch64Built{}, geo.NCH, [&](auto nch) { launch_fb<double, decltype(nch)::value, 256, true>(prm, geo.NT, st, e_mid); })
        : qa::dispatch(Nch32Built{}, geo.NCH, [&](auto nch) { launch_fb<float, decltype(nch)::value, 512, true>(prm, geo.NT, st, e_mid); });
    if (!built) throw std::runtime_error("geometry not built");
}

// whether launch_fb_any holds a build for the geometry (fullpass_testhook.h reports it)
bool geometry_built(const Geometry &geo, int K) {
    if (geo.NT == 0) return false;
    if (geo.kind == KIND_F64_RANK || geo.kind == KIND_F64_DOS) {
        int g[6];
        qa::fb64_launch_geometry(K, geo.kind == KIND_F64_DOS, g);
        return g[5] != 0;
    }
    if (geo.kind == KIND_F64_REF) return true;   // NT and Kq at run time
    return geo.kind == KIND_F64_FULL ? qa::contains(Nch64Built{}, geo.NCH) : qa::contains(Nch32Built{}, geo.NCH);
}

// the kernels behind the dosage passes of a handle: fp32 state, or (qa_panel_set_dosage_precision(64)) the fp64 dosage
// kernels -- the generic fp64 kernels when K exceeds those kernels' on-chip capacity
PassKind dosage_kind(const qa_panel *pn) {
    if (pn->sum_order_ref) return KIND_F64_REF;
    // (panels beyond the fp32 kernels' 98 304 haplotypes: the fp64 dosage kernels, whose chunk rows past the seventh stream)
    if (!pn->dosage_fp64 && pick_geometry(pn->K, KIND_F32).NT) return KIND_F32;
    return pick_geometry(pn->K, KIND_F64_DOS).NT ? KIND_F64_DOS : KIND_F64_FULL;
}

// the kernels behind the best-haplotype lists of a handle with fp64 ranking
PassKind rank_kind(const qa_panel *pn) { return pn->sum_order_ref ? KIND_F64_REF : KIND_F64_RANK; }

// Which kernels serve a request on this handle.  The tuned fp64 dosage kernels yield the dosage (and c) only, and the fp64
// ranking kernels the lists only; every other kind yields anything.
struct KindChoice {
    PassKind dosage;   // the passes that yield the dosage (single-pass entry: and the K x nGrids matrices)
    PassKind lists;    // the passes that yield best-haplotype lists only
    bool one_pass;     // a pass that wants dosage and lists gets both from `dosage`; else it runs once with each kind
};
enum KindCaller { FOR_SINGLE_PASS, FOR_GL_BATCH, FOR_READS_BATCH };
KindChoice choose_kinds(const qa_panel *pn, KindCaller who, bool want_dosage, bool want_lists, bool want_matrices) {
    const bool rank64 = pn->rank_fp64 && want_lists;   // lists whose membership and order are the reference's: fp64 state
    PassKind d = dosage_kind(pn);
    if (who == FOR_SINGLE_PASS) {
        // a call that wants alpha / beta / gamma matrices, or no dosage, takes the generic fp64 kernels
        if (d == KIND_F64_DOS && (want_matrices || !want_dosage)) d = KIND_F64_FULL;
        if (d == KIND_F64_DOS) return {d, pn->rank_fp64 ? rank_kind(pn) : KIND_F32, false};
        if (rank64 && d == KIND_F32) return {d, rank_kind(pn), false};   // every other output comes from the fp32 pass
        return {d, d, true};   // fp32 state with fp32 ranking, or fp64 state through the generic / validation kernels
    }
    // the batched drivers: with fp32 ranking the lists come from the dosage pass itself
    if (d == KIND_F64_DOS && want_lists && !pn->rank_fp64) d = KIND_F64_FULL;
    // fp64 ranking passes beside the dosage passes (fp32 state, or the fp64 dosage kernels); with the generic fp64 kernels,
    // or fp32 ranking, one pass yields both
    if (rank64 && d != KIND_F64_FULL) return {d, rank_kind(pn), false};
    if (who == FOR_READS_BATCH) return {d, pn->rank_fp64 ? rank_kind(pn) : KIND_F32, true};
    // (list-only passes of the fp64-dosage mode still take the faster ranking kernels)
    return {d, rank64 && pick_geometry(pn->K, rank_kind(pn)).NT ? rank_kind(pn) : d, true};
}

struct BatchOut {
    double *dosage = nullptr;        // [P][T] (row p, or dosage_rows[p] when given)
    const int32_t *dosage_rows = nullptr;
    double *c = nullptr;             // [P][G]
    double *alphaHat_t = nullptr;    // single-pass API only
    double *betaHat_t = nullptr;
    double *gamma_t = nullptr;
    double *gammaSmall_t = nullptr;
    bool gamma_small_unscaled = false;  // gammaSmall_t without return_gamma_t: no sigma factor (:2170-2176)
    // best_haps_stuff_list of every (pass, thinned column), appended in pass-major order
    std::vector<std::vector<std::pair<int32_t, double>>> *lists = nullptr;
    bool truncate_lists = false;   // batched drivers: lists capped at top_cap entries (head of the ordered list)
    int top_cap = 64;              // initial (or, truncating, final) capacity per list
    // truncating drivers: the device arrays as they are, [P][n_thin][top_cap], instead of `lists`
    std::vector<int32_t> *flat_idx = nullptr;
    std::vector<double> *flat_val = nullptr;
    bool order_by_value = false;   // lists ordered as everything_per_hap_rejig_haps wants (else ascending k)
    std::vector<int32_t> *true_counts = nullptr;   // untruncated list lengths
    // hla_run: gamma_t_col of grid gamma_grid for every pass (fp64 dosage or validation passes), K doubles to row gamma_rows[p]
    // (p when null) of gamma_col
    double *gamma_col = nullptr;
    int gamma_grid = -1;
    const int32_t *gamma_rows = nullptr;
    // single-pass entry, validation mode: alpha at the thinned grids only, and at grid 0 (PassRequest::alpha_grid0)
    bool alpha_grid0 = false;
};

// ---- run_passes, stage by stage.  What the stages of one call share:
struct PassRun {
    qa_panel *pn;
    qa_panel::Scratch &S;
    hipStream_t st;
    int P;
    const int32_t *h_flags, *thin_col_h;   // per pass as in PassParams::flags; per grid
    const BatchOut &out;
    Geometry geo;
    PassLayout L;
    int n_thin;
    bool any_top;   // lists wanted
    bool fused;     // ... and the fp64 ranking kernels pick them themselves: only the ordered head of each list is wanted (the driver)
    int top_cap;
    PassParams prm;
    bool dosage_direct = false;   // k_dosage writes the caller's rows itself
    std::vector<int32_t> cnt;     // [P][n_thin] list lengths
    int n_handed_over = 0;        // fused: lists left to k_topk
    size_t es() const { return L.es; }
};

// K_top_matches beyond what the pickers are built for (QA_K_TOP_MATCHES_MAX): said by every entry before it allocates
static_assert(kMaxTopWide == QA_K_TOP_MATCHES_MAX, "k_topk's wide form covers the documented range");
int check_k_top(const char *who, int K_top) {
    if (K_top <= QA_K_TOP_MATCHES_MAX) return QA_OK;
    qa::set_error("%s: K_top_matches = %d is not built: every K_top_matches in 1..%d runs", who, K_top, QA_K_TOP_MATCHES_MAX);
    return QA_ERR_UNSUPPORTED;
}

// the request against what the kind can yield
void check_request(const qa_panel *pn, PassKind kind, int P, const int32_t *h_flags, int K_top, const BatchOut &out) {
    if (kind == KIND_F64_RANK)
        for (int p = 0; p < P; p++)
            if (h_flags[p] & 15) throw std::runtime_error("fp64 ranking passes carry no dosage / gamma / beta outputs");
    if (out.gamma_col) {
        if (kind != KIND_F64_DOS && kind != KIND_F64_REF) throw std::runtime_error("internal: a gamma column from passes other than the fp64 dosage passes");
        if (out.gamma_grid < 0 || out.gamma_grid >= pn->G) throw std::runtime_error("internal: gamma grid out of range");
        for (int p = 0; p < P; p++)
            if (!(h_flags[p] & 1)) throw std::runtime_error("internal: a gamma column from a pass without dosage");
    }
    if (kind == KIND_F64_DOS) {
        for (int p = 0; p < P; p++)
            if (!(h_flags[p] & 1) || (h_flags[p] & 12)) throw std::runtime_error("fp64 dosage passes yield the dosage (and c) only");
        if (K_top > 0) throw std::runtime_error("fp64 dosage passes carry no best-haplotype lists (the ranking passes do)");
    }
}

// alpha checkpoint slots [P][G]: all grids for dosage / gamma / beta passes, thinned grids otherwise (the column counts:
// PassLayout::alpha_cols)
std::vector<int32_t> plan_alpha_slots(const PassRun &r) {
    const int P = r.P, G = r.pn->G;
    std::vector<int32_t> slot((size_t)P * G, -1);
    for (int p = 0; p < P; p++) {
        int32_t *sl = slot.data() + (size_t)p * G;
        if ((r.h_flags[p] & 15) && r.geo.kind == KIND_F64_DOS) {   // every second column: k_bwd64d re-forms the odd grids' (PassParams::fw_add)
            for (int g = 0; g < G; g += 2) sl[g] = g / 2;
        } else if (r.h_flags[p] & 15) {
            for (int g = 0; g < G; g++) sl[g] = g;
        } else {
            int n = 0;
            for (int g = 0; g < G; g++) if (r.thin_col_h[g] >= 0) sl[g] = n++;
            if (r.out.alpha_grid0 && sl[0] < 0) sl[0] = n;   // (the thinned grids keep their slots)
        }
    }
    return slot;
}

// the only way a Scratch buffer gets its memory: buffer b of the layout, for P passes
template <typename T>
void carve(qa::ABuf<T> &buf, const PassLayout &L, PassLayout::Buf b, int P) { buf.ensure(L.bytes(b, P) / sizeof(T)); }

// every buffer of the layout in its order (a buffer the launch set does not use has no elements and stays null); gl: only
// for a host gl, else the caller has carved and filled S.gl on the device already (k_make_gl)
void carve_scratch(qa_panel::Scratch &S, const PassLayout &L, int P, bool gl) {
    using B = PassLayout;
    if (gl) carve(S.gl, L, B::GL, P);
    carve(S.thin_col, L, B::THIN_COL, P);
    carve(S.flags, L, B::FLAGS, P);
    carve(S.alpha_slot, L, B::ALPHA_SLOT, P);
    carve(S.emat, L, B::EMAT, P);
    carve(S.escale0, L, B::ESCALE0, P);
    carve(S.emin, L, B::EMIN, P);
    carve(S.emin_b1, L, B::EMIN_B1, P);
    carve(S.esp, L, B::ESP, P);
    carve(S.gsp, L, B::GSP, P);
    carve(S.alpha, L, B::ALPHA, P);
    carve(S.c, L, B::C, P);
    carve(S.fw_add, L, B::FW_ADD, P);
    carve(S.fw_xs, L, B::FW_XS, P);
    carve(S.mg, L, B::MG, P);
    carve(S.dosage, L, B::DOSAGE, P);
    carve(S.gamma, L, B::GAMMA, P);
    carve(S.beta, L, B::BETA, P);
    carve(S.beta_thin, L, B::BETA_THIN, P);
    carve(S.gamma_col, L, B::GAMMA_COL, P);
    carve(S.top_cnt, L, B::TOP_CNT, P);
    carve(S.spill, L, B::SPILL, P);
    carve(S.top_idx, L, B::TOP_IDX, P);
    carve(S.top_val, L, B::TOP_VAL, P);
}

void fill_params(PassRun &r, int K_top, int normalize_emissions, int always_normalize, double norm_threshold) {
    const qa_panel *pn = r.pn;
    const auto &S = r.S;
    const PassLayout &L = r.L;
    const PassKind kind = r.geo.kind;
    PassParams &prm = r.prm;
    prm = PassParams{};
    prm.hm = pn->hm.p; prm.B = pn->B.p; prm.sp_off = pn->sp_off.p; prm.sp_k = pn->sp_k.p;
    prm.sp_word = pn->sp_word.p; prm.sp_gidx = pn->sp_gidx.p; prm.sp_chunk_at = pn->sp_chunk_at.p;
    prm.sigma = pn->sigma.p; prm.tm1 = pn->tm1.p; prm.IE = pn->ie_derived ? nullptr : pn->IE.p;
    prm.K = pn->K; prm.Kp = pn->Kp; prm.G = pn->G; prm.T = pn->T; prm.nMaxDH = pn->nMaxDH; prm.nrow = pn->nrow;
    prm.n_special = pn->n_special; prm.ref_error = pn->ref_error;
    prm.P = r.P; prm.gl = S.gl.p; prm.thin_col = S.thin_col.p; prm.n_thin = r.n_thin; prm.flags = S.flags.p;
    prm.normalize_emissions = normalize_emissions;
    prm.lazy = qa::lazy_kind(kind) ? 1 : 0; prm.always_normalize = always_normalize; prm.norm_threshold = norm_threshold;
    prm.grid0_left_to_right = pn->sum_order_grid0_ltr ? 1 : 0;
    prm.emin = S.emin.p; prm.emin_b1 = S.emin_b1.p; prm.esp_stride = (int)L.esp_stride;

    // (a buffer the layout gave no elements is null)
    prm.spill = S.spill.p; prm.spill_pass_stride = L.spill_stride;
    prm.fw_add = S.fw_add.p; prm.fw_xs = S.fw_xs.p;
    prm.emat = S.emat.p; prm.esp = S.esp.p; prm.escale0 = S.escale0.p; prm.alpha = S.alpha.p; prm.alpha_slot = S.alpha_slot.p;
    prm.alpha_pass_stride = L.alpha_cols * L.alpha_col_elems; prm.Kq = (int)L.Kq; prm.alpha_col_elems = L.alpha_col_elems;
    prm.hist_unit = kind == KIND_F64_DOS ? 1.0 / 2251799813685248.0 /* 2^-51: k_bwd64d */ : 1.0 / kHistScale64; prm.c = S.c.p; prm.mg = S.mg.p; prm.gsp = S.gsp.p;
    prm.gamma_out = S.gamma.p; prm.beta_out = S.beta.p;
    prm.gamma_col = S.gamma_col.p; prm.gamma_grid = r.out.gamma_col ? r.out.gamma_grid : -1;
    prm.K_top = r.any_top ? K_top : 0;
    prm.beta_thin = S.beta_thin.p;
    prm.fused_topk = r.fused ? 1 : 0;
    prm.top_cap = r.top_cap;
    prm.truncate_lists = r.out.truncate_lists ? 1 : 0;
    if (r.any_top) { prm.top_cnt = S.top_cnt.p; prm.top_idx = S.top_idx.p; prm.top_val = S.top_val.p; }
}

// Dosage rows that go to consecutive rows of a qa_host_alloc buffer are written there by k_dosage itself (every element
// once, 4 KiB of consecutive bytes per workgroup): the transfer rides under the kernel instead of following it.  Else
// the staging rows of the scratch.
void choose_dosage_destination(PassRun &r) {
    const BatchOut &out = r.out;
    const int P = r.P, T = r.pn->T;
    bool direct = false;
    if (out.dosage && P > 0) {
        const size_t r0 = out.dosage_rows ? (size_t)out.dosage_rows[0] : 0;
        direct = true;
        for (int p = 0; p < P && direct; p++)
            direct = (r.h_flags[p] & 1) && (out.dosage_rows ? (size_t)out.dosage_rows[p] : (size_t)p) == r0 + (size_t)p;
        direct = direct && qa::pinned_registry().covers(out.dosage + r0 * T, sizeof(double) * (size_t)P * T);
        if (direct) r.prm.dosage = out.dosage + r0 * T;
    }
    if (!direct) r.prm.dosage = r.S.dosage.p;
    r.dosage_direct = direct;
}

// emission tables, forward / backward, dosage: events 0 .. 4 around them
void launch_passes(PassRun &r) {
    auto &S = r.S;
    const PassParams &prm = r.prm;
    const int P = r.P, G = r.pn->G;
    const bool f64 = r.geo.f64();
    hipStream_t st = r.st;
    QA_HIP(hipEventRecord(S.ev[0], st));
    if (f64) hipLaunchKernelGGL(k_emat<double>, dim3(G, P), dim3(256), 0, st, prm);
    else hipLaunchKernelGGL(k_emat<float>, dim3(G, P), dim3(256), 0, st, prm);
    QA_HIP(hipGetLastError());
    QA_HIP(hipEventRecord(S.ev[1], st));
    launch_fb_any(r.geo, prm, st, S.ev[2], r.pn->sum_order_batched);
    QA_HIP(hipEventRecord(S.ev[3], st));
    const dim3 dgrid((G + kDosageGridsPerBlock - 1) / kDosageGridsPerBlock, P);
    if (r.geo.kind == KIND_F64_REF) { /* the validation backward kernel wrote the dosage itself, sums in the reference's order */ }
    else if (f64) hipLaunchKernelGGL(k_dosage<double>, dgrid, dim3(256), 0, st, prm);
    else hipLaunchKernelGGL(k_dosage<float>, dgrid, dim3(256), 0, st, prm);
    QA_HIP(hipGetLastError());
    QA_HIP(hipEventRecord(S.ev[4], st));
}

// k_topk over `grid` blocks: the state's element type, and the wide form beyond the per-lane lists' kMaxTop
void launch_topk(const PassRun &r, dim3 grid) {
    const bool wide = r.prm.K_top > kMaxTop;
    if (r.geo.f64()) {
        if (wide) hipLaunchKernelGGL((k_topk<double, true>), grid, dim3(256), 0, r.st, r.prm, r.geo.NT);
        else hipLaunchKernelGGL(k_topk<double>, grid, dim3(256), 0, r.st, r.prm, r.geo.NT);
    } else {
        if (wide) hipLaunchKernelGGL((k_topk<float, true>), grid, dim3(256), 0, r.st, r.prm, r.geo.NT);
        else hipLaunchKernelGGL(k_topk<float>, grid, dim3(256), 0, r.st, r.prm, r.geo.NT);
    }
    QA_HIP(hipGetLastError());
}

// fused: the backward kernel wrote the lists; the grids whose candidates overflowed its LDS list (top_cnt = -1: ties)
// left their beta column for k_topk
void finish_fused_lists(PassRun &r) {
    auto &S = r.S;
    PassParams &prm = r.prm;
    hipStream_t st = r.st;
    const int n_thin = r.n_thin;
    r.cnt.resize((size_t)r.P * n_thin);
    S.top_cnt.download(r.cnt.data(), r.cnt.size(), st);
    std::vector<int32_t> todo;
    for (size_t i = 0; i < r.cnt.size(); i++)
        if (r.cnt[i] < 0) { todo.push_back((int32_t)(i / n_thin)); todo.push_back((int32_t)(i % n_thin)); }
    r.n_handed_over = (int)todo.size() / 2;
    if (!r.n_handed_over) return;
    S.todo.ensure(todo.size());
    S.todo.upload(todo.data(), todo.size(), st);
    prm.topk_todo = S.todo.p;
    launch_topk(r, dim3(r.n_handed_over));
    S.top_cnt.download(r.cnt.data(), r.cnt.size(), st);
    QA_HIP(hipStreamSynchronize(st));
    prm.topk_todo = nullptr;
}

// the separate picker over every (thinned column, pass); not truncating: once more with room for the longest list
void pick_lists_separately(PassRun &r) {
    auto &S = r.S;
    PassParams &prm = r.prm;
    hipStream_t st = r.st;
    const int P = r.P, n_thin = r.n_thin;
    for (int attempt = 0; attempt < 2; attempt++) {
        if (attempt) {   // (outside the per-pass plan: pass_layout.hpp)
            r.L.set_top_cap(r.top_cap, n_thin);
            carve(S.top_idx, r.L, PassLayout::TOP_IDX, P);
            carve(S.top_val, r.L, PassLayout::TOP_VAL, P);
        }
        prm.top_cap = r.top_cap;
        prm.top_cnt = S.top_cnt.p; prm.top_idx = S.top_idx.p; prm.top_val = S.top_val.p;
        launch_topk(r, dim3(n_thin, P));
        r.cnt.resize((size_t)P * n_thin);
        S.top_cnt.download(r.cnt.data(), r.cnt.size(), st);
        QA_HIP(hipStreamSynchronize(st));
        int mx = 0;
        for (int32_t v : r.cnt) mx = std::max(mx, v);
        if (mx <= r.top_cap || r.out.truncate_lists) break;
        r.top_cap = mx;  // pathological ties (e.g. a label without reads): redo with room for all
    }
}

// event times into g_timing, and the launch set's rows of the kernel profile
void add_profile_rows(const PassRun &r) {
    const auto &S = r.S;
    const int P = r.P, G = r.pn->G, T = r.pn->T, K = r.pn->K, n_thin = r.n_thin;
    const size_t es = r.es();
    const PassKind kind = r.geo.kind;
    float ms;
    for (int i = 0; i < 5; i++) {
        QA_HIP(hipEventElapsedTime(&ms, S.ev[i], S.ev[i + 1]));
        g_timing[i] = ms;
    }
    QA_HIP(hipEventElapsedTime(&ms, S.ev[0], S.ev[5]));
    g_timing[5] = ms;
    // algorithmic HBM bytes of this launch set: per cell 1 B code + one state element
    // (4 B, or 8 B with fp64 state) on every stored column, forward (alpha) and backward (alpha re-read) alike;
    // the separate top-K picker re-reads alpha and beta at the thinned grids twice (outside the SURVEY contract:
    // it is what the fused picker of the fp64 ranking kernels removes); k_dosage reads the code histograms
    double cells_all = 0, cells_thin = 0, n_dos = 0;
    for (int p = 0; p < P; p++) {
        if (r.h_flags[p] & 15) cells_all += (double)K * G; else cells_thin += (double)K * G;
        if (r.h_flags[p] & 1) n_dos += 1;
    }
    const double frac = G > 0 ? (double)n_thin / G : 0;
    const double per_dir = cells_all * (1.0 + es) + cells_thin * (1.0 + es * frac);
    const double topk_bytes = (r.any_top && !r.fused) ? (double)P * n_thin * K * es * 4.0
                                                      : (double)r.n_handed_over * K * es * 4.0;
    const double t_e = qa::profile_clock_ms(S.ev[0]);
    double at = t_e;
    qa::profile_add(qa::PK_EMAT, g_timing[0], (double)P * T * 16.0 + (double)P * G * kMaxRow * es, at); at += g_timing[0];
    // (the fp64 dosage forward stores every second column: half of the state bytes; its backward reads each stored column twice)
    const double per_dir_fwd = kind == KIND_F64_DOS ? cells_all * (1.0 + es * 0.5) : per_dir;
    qa::profile_add(kKindInfo[kind].pk_fwd, g_timing[1], per_dir_fwd, at); at += g_timing[1];
    qa::profile_add(kKindInfo[kind].pk_bwd, g_timing[2], per_dir, at); at += g_timing[2];
    if (n_dos > 0) qa::profile_add(qa::PK_DOSAGE, g_timing[3], n_dos * G * kMaxRow * (r.geo.f64() ? 8.0 : 4.0) + n_dos * T * 8.0, at);
    at += g_timing[3];
    if (topk_bytes > 0) qa::profile_add(qa::PK_TOPK, g_timing[4], topk_bytes, at);
}

// rows of Kq (the kernels' 16-byte stores) -> rows of K: one 2-D copy per run of consecutive destination rows
void download_gamma_column(const PassRun &r) {
    const BatchOut &out = r.out;
    const int P = r.P, K = r.pn->K;
    const size_t Kq = r.L.Kq;
    auto row_of = [&](int p) { return (size_t)(out.gamma_rows ? out.gamma_rows[p] : p); };
    for (int p = 0; p < P;) {
        int n = 1;
        while (p + n < P && row_of(p + n) == row_of(p) + (size_t)n) n++;
        QA_HIP(hipMemcpy2DAsync(out.gamma_col + row_of(p) * K, sizeof(double) * K, r.S.gamma_col.p + (size_t)p * Kq, sizeof(double) * Kq,
                                sizeof(double) * K, n, hipMemcpyDeviceToHost, r.st));
        p += n;
    }
    QA_HIP(hipStreamSynchronize(r.st));
}

// the staged dosage rows: runs of consecutive dosage passes come back in one staged transfer each, then scatter to their rows
// (a run whose destination rows are consecutive too -- the batch calls' layout -- lands in the caller's buffer
// directly: one transfer, staged piecewise or, for a qa_host_alloc buffer, written by the copy kernel itself)
void download_dosage_rows(const PassRun &r) {
    const BatchOut &out = r.out;
    const int P = r.P, T = r.pn->T;
    const int32_t *h_flags = r.h_flags;
    const int max_rows = std::max<int>(1, (int)(qa::kStagePiece / (sizeof(double) * T)));
    auto row_of = [&](int p) { return (size_t)(out.dosage_rows ? out.dosage_rows[p] : p); };
    std::vector<double> tmp;
    for (int p = 0; p < P;) {
        if (!(h_flags[p] & 1)) { p++; continue; }
        int n = 1;
        while (p + n < P && (h_flags[p + n] & 1) && row_of(p + n) == row_of(p) + (size_t)n) n++;
        if (n > 1 || max_rows == 1) {
            qa::staged_download(out.dosage + row_of(p) * T, r.S.dosage.p + (size_t)p * T, sizeof(double) * T * n, r.st);
            p += n;
            continue;
        }
        while (p + n < P && n < max_rows && (h_flags[p + n] & 1)) n++;
        tmp.resize((size_t)n * T);
        qa::staged_download(tmp.data(), r.S.dosage.p + (size_t)p * T, sizeof(double) * T * n, r.st);
        for (int i = 0; i < n; i++)
            memcpy(out.dosage + row_of(p + i) * T, tmp.data() + (size_t)i * T, sizeof(double) * T);
        p += n;
    }
}

// single-pass entry: the K x nGrids matrices, un-permuted on the device through one staging buffer (K x G doubles: outside
// the per-pass plan, pass_layout.hpp) that every matrix re-uses -- each transfer is complete before the next starts
void download_matrices(PassRun &r, const std::vector<int32_t> &slot) {
    const BatchOut &out = r.out;
    if (!out.alphaHat_t && !out.gamma_t && !out.betaHat_t && !out.gammaSmall_t) return;
    auto &S = r.S;
    const qa_panel *pn = r.pn;
    const int G = pn->G, K = pn->K, Kq = (int)r.L.Kq;
    const bool any_gamma = S.gamma.p != nullptr, any_beta = S.beta.p != nullptr;
    S.unperm.ensure((size_t)K * G);
    auto unpermute_to_host = [&](const char *base, size_t elem_off, int cols, double *dst) {
        if (r.geo.f64())
            hipLaunchKernelGGL(k_unpermute<double>, dim3((K + 255) / 256, cols), dim3(256), 0, r.st,
                               reinterpret_cast<const double *>(base) + elem_off, S.unperm.p, K, Kq, r.geo.NT, cols, (size_t)K);
        else
            hipLaunchKernelGGL(k_unpermute<float>, dim3((K + 255) / 256, cols), dim3(256), 0, r.st,
                               reinterpret_cast<const float *>(base) + elem_off, S.unperm.p, K, Kq, r.geo.NT, cols, (size_t)K);
        QA_HIP(hipGetLastError());
        S.unperm.download(dst, (size_t)K * cols, r.st);
        QA_HIP(hipStreamSynchronize(r.st));
    };
    if (out.alphaHat_t) {
        if (r.h_flags[0] & 15) {
            unpermute_to_host(S.alpha.p, 0, G, out.alphaHat_t);
        } else {
            // only column 0 and the thinned columns exist (reference-single.cpp:2264-2268)
            std::vector<double> col(K);
            for (int g = 0; g < G; g++) {
                const int sl = slot[g];
                if (sl < 0) continue;
                unpermute_to_host(S.alpha.p, (size_t)sl * Kq, 1, col.data());
                memcpy(out.alphaHat_t + (size_t)g * K, col.data(), sizeof(double) * K);
            }
        }
    }
    if (out.gamma_t && any_gamma) unpermute_to_host(S.gamma.p, 0, G, out.gamma_t);
    if (out.betaHat_t && any_beta) unpermute_to_host(S.beta.p, 0, G, out.betaHat_t);
    if (out.gammaSmall_t && any_gamma) {
        std::vector<double> col(K);
        for (int g = 0; g < G; g++) {
            if (r.thin_col_h[g] < 0) continue;
            unpermute_to_host(S.gamma.p, (size_t)g * Kq, 1, col.data());
            if (out.gamma_small_unscaled && g < G - 1)
                for (int k = 0; k < K; k++) col[k] /= pn->h_sigma[g];
            memcpy(out.gammaSmall_t + (size_t)r.thin_col_h[g] * K, col.data(), sizeof(double) * K);
        }
    }
}

// the lists to the caller: the device arrays as they are (flat_idx / flat_val) and / or list by list
void collect_lists(const PassRun &r) {
    const BatchOut &out = r.out;
    const int top_cap = r.top_cap;
    if (out.true_counts) *out.true_counts = r.cnt;
    if (!out.lists && !out.flat_idx) return;
    const size_t n = (size_t)r.P * r.n_thin;
    std::vector<int32_t> idx_local;
    std::vector<double> val_local;
    std::vector<int32_t> &idx = out.flat_idx ? *out.flat_idx : idx_local;
    std::vector<double> &val = out.flat_val ? *out.flat_val : val_local;
    idx.resize(n * top_cap);
    val.resize(n * top_cap);
    r.S.top_idx.download(idx.data(), idx.size(), r.st);
    if (r.geo.f64()) {
        qa::staged_download(val.data(), r.S.top_val.p, val.size() * 8, r.st);
    } else {
        std::vector<float> v32(val.size());
        qa::staged_download(v32.data(), r.S.top_val.p, v32.size() * 4, r.st);
        for (size_t i = 0; i < val.size(); i++) val[i] = v32[i];
    }
    for (size_t i = 0; out.lists && i < n; i++) {
        std::vector<std::pair<int32_t, double>> tmp;
        const int nq = std::min<int>(r.cnt[i], top_cap);
        tmp.reserve(nq);
        for (int q = 0; q < nq; q++) tmp.emplace_back(idx[i * top_cap + q], val[i * top_cap + q]);
        if (!out.order_by_value) {
            std::sort(tmp.begin(), tmp.end());  // ascending k, the reference's emission order
        } else if (nq > 64) {                    // (k_topk orders lists of up to 64 entries itself)
            std::sort(tmp.begin(), tmp.end(), [](const std::pair<int32_t, double> &a, const std::pair<int32_t, double> &b) {
                return a.second > b.second || (a.second == b.second && a.first < b.first);
            });
        }
        out.lists->push_back(std::move(tmp));
    }
}

// runs P passes; flags per pass as in PassParams
int run_passes(qa_panel *pn, int P, const double *gl, const int32_t *h_flags, const int32_t *thin_col_h,
               int K_top, int normalize_emissions, const BatchOut &out, PassKind kind = KIND_F32,
               int always_normalize = 0, double norm_threshold = 1e-100) {
    if (const int st = check_k_top("full-panel passes", K_top)) return st;   // (the public entries have said so already)
    const Geometry geo = pick_geometry(pn->K, kind);
    if (geo.NT == 0) {
        qa::set_error("K = %d exceeds the on-chip capacity of the %s full-pass kernels", pn->K, kKindInfo[kind].name);
        return QA_ERR_UNSUPPORTED;
    }
    if (!geometry_built(geo, pn->K)) {   // (a build without every variant: QA_FAST_BUILD) -- said before any device work
        qa::set_error("K = %d: this build of the library holds no %s full-pass kernels of that geometry", pn->K, kKindInfo[kind].name);
        return QA_ERR_UNSUPPORTED;
    }
    check_request(pn, kind, P, h_flags, K_top, out);
    QA_HIP(hipSetDevice(pn->device));
    if (!pn->scratch) pn->scratch = new qa_panel::Scratch(&pn->A());
    auto &S = *pn->scratch;
    hipStream_t st = pn->pass_stream ? pn->pass_stream : pn->stream;
    for (auto &e : S.ev) if (!e) QA_HIP(hipEventCreate(&e));
    const int G = pn->G, T = pn->T;
    const Thin thin = qa::count_thin(thin_col_h, G);
    const bool any_top = thin.n_thin > 0 && K_top > 0;
    PassRun r{pn, S, st, P, h_flags, thin_col_h, out, geo,
              PassLayout(dims_of(pn), geo, qa::make_request(h_flags, P, thin, K_top, out.top_cap, out.gamma_col != nullptr, out.alpha_grid0)),
              thin.n_thin, any_top,
              /* fused: k_bwd64's picker merges its eight waves' K_top maxima in one wave, K_top <= kMaxTop; wider goes to k_topk */
              any_top && kind == KIND_F64_RANK && out.truncate_lists && out.top_cap <= 64 && K_top <= kMaxTop,
              out.top_cap, PassParams{}};

    const std::vector<int32_t> slot = plan_alpha_slots(r);
    carve_scratch(S, r.L, P, gl != nullptr);
    if (gl) S.gl.upload(gl, (size_t)P * T * 2, st);
    S.thin_col.upload(thin_col_h, G, st);
    S.flags.upload(h_flags, P, st);
    S.alpha_slot.upload(slot.data(), (size_t)P * G, st);
    fill_params(r, K_top, normalize_emissions, always_normalize, norm_threshold);
    choose_dosage_destination(r);

    launch_passes(r);
    if (r.fused) finish_fused_lists(r);
    else if (any_top) pick_lists_separately(r);
    QA_HIP(hipEventRecord(S.ev[5], st));
    QA_HIP(hipStreamSynchronize(st));
    add_profile_rows(r);

    // ---- copy results back
    if (out.c) S.c.download(out.c, (size_t)P * G, st);
    if (out.gamma_col) download_gamma_column(r);
    if (out.dosage && !r.dosage_direct) download_dosage_rows(r);
    if (P == 1) download_matrices(r, slot);
    if (any_top) collect_lists(r);
    QA_HIP(hipStreamSynchronize(st));
    g_last_plan.P = P;
    g_last_plan.kind = kind;
    g_last_plan.carved = (int64_t)S.gl.arena->off;
    return QA_OK;
}

}  // namespace

// hla_run: can this handle's dosage passes keep a gamma column?  Only the fp64 dosage kernels (k_bwd64d) and the validation
// kernels (k_bwd_ro) store one; QA_ERR_UNSUPPORTED with the cause named otherwise.
int qa::gamma_column_check(const qa_panel *pn, const char *who) {
    const PassKind dk = dosage_kind(pn);
    if (dk == KIND_F64_REF || (dk == KIND_F64_DOS && pn->rank_fp64)) return QA_OK;
    if (dk == KIND_F32)
        qa::set_error("%s: the handle's dosage passes are fp32; the gamma column comes from the fp64 dosage passes: call "
                      "qa_panel_set_dosage_precision(64) on the handle first", who);
    else if (!pn->rank_fp64)
        qa::set_error("%s: with fp32 ranking the dosage passes run the generic fp64 kernels, which keep no gamma column: call "
                      "qa_panel_set_ranking_precision(panel, 64) first", who);
    else
        qa::set_error("%s: K = %d haplotypes is served by the generic fp64 kernels (the fp64 dosage kernels' on-chip layout does not "
                      "hold this K), which keep no gamma column", who, pn->K);
    return QA_ERR_UNSUPPORTED;
}

extern "C" {

int qa_last_fullpass_timing_ms(double out[5]) {
    if (!out) return QA_ERR_INVALID;
    for (int i = 0; i < 3; i++) out[i] = g_timing[i];
    out[3] = g_timing[3] + g_timing[4];
    out[4] = g_timing[5];
    return QA_OK;
}

// pack best-haps lists into the caller's CSR arrays
static int pack_lists(const std::vector<std::vector<std::pair<int32_t, double>>> &lists, int32_t *best_ptr,
                      int32_t *best_idx, double *best_val, int64_t best_cap) {
    if (!best_ptr) return QA_OK;
    int64_t total = 0;
    best_ptr[0] = 0;
    for (size_t i = 0; i < lists.size(); i++) {
        total += (int64_t)lists[i].size();
        best_ptr[i + 1] = (int32_t)total;
    }
    if (total > best_cap || !best_idx || !best_val) {
        qa::set_error("best-haps capacity %lld < needed %lld", (long long)best_cap, (long long)total);
        return QA_ERR_CAPACITY;
    }
    for (size_t i = 0; i < lists.size(); i++)
        for (size_t q = 0; q < lists[i].size(); q++) {
            best_idx[best_ptr[i] + q] = lists[i][q].first;
            best_val[best_ptr[i] + q] = (double)lists[i][q].second;
        }
    return QA_OK;
}

int qa_fullpass_last_plan(int64_t out[6]) {
    if (!out) return QA_ERR_INVALID;
    out[0] = g_last_plan.P; out[1] = g_last_plan.per_pass; out[2] = g_last_plan.fixed; out[3] = g_last_plan.carved;
    out[4] = PassLayout::N_BUF; out[5] = g_last_plan.kind;
    return QA_OK;
}

int qa_fullpass_geometry(int32_t K, int32_t kind, int32_t out[8]) {
    if (!out || K < 1 || kind < 0 || kind >= qa::KIND_COUNT) return QA_ERR_INVALID;
    for (int i = 0; i < 8; i++) out[i] = 0;
    const Geometry geo = pick_geometry(K, (PassKind)kind);
    if (geo.NT == 0) return QA_OK;
    out[0] = geo.NT; out[1] = geo.NCH;
    if (kind == KIND_F64_RANK || kind == KIND_F64_DOS) {
        int g[6];
        qa::fb64_launch_geometry(K, kind == KIND_F64_DOS, g);
        out[2] = g[1]; out[3] = g[2]; out[4] = g[3]; out[5] = g[4];
    }
    out[6] = geo.NT * geo.NCH * 16;   // PassLayout::Kq
    out[7] = geometry_built(geo, K);
    return QA_OK;
}

int qa_fullpass_launch_set(qa_panel_t *panel, int32_t n_pass, const double *gl, const int32_t *flags,
                           const int32_t *gammaSmall_cols_to_get, int32_t K_top_matches, int32_t always_normalize,
                           double *dosage, double *c, int32_t *best_ptr, int32_t *best_idx, double *best_val, int64_t best_cap) {
    if (!qa::device_ready()) return QA_ERR_NO_DEVICE;
    if (!panel || !gl || n_pass <= 0 || !flags || !gammaSmall_cols_to_get) {
        qa::set_error("qa_fullpass_launch_set: bad argument");
        return QA_ERR_INVALID;
    }
    if (const int st = check_k_top("qa_fullpass_launch_set", K_top_matches)) return st;
    int32_t any = 0;
    for (int i = 0; i < n_pass; i++) {
        if (flags[i] != 0 && flags[i] != 1) {
            qa::set_error("qa_fullpass_launch_set: flags must be 0 or 1");
            return QA_ERR_INVALID;
        }
        any |= flags[i];
    }
    return qa::guarded([&] {
        qa::GateHold hold;
        hold.acquire(panel->gate(), &panel->arena);
        QA_HIP(hipSetDevice(panel->device));
        const PassKind kind = dosage_kind(panel);
        const Thin thin = qa::count_thin(gammaSmall_cols_to_get, panel->G);
        // (fixed term: room for the non-truncating top-K retry at full length -- every haplotype of a pass without reads ties)
        const size_t retry = K_top_matches > 0 ? (size_t)n_pass * thin.n_thin * panel->K * 12 + 2 * qa::Arena::kCarveAlign : 0;
        if (plan_chunk(panel, plan_pass_bytes(panel, pick_geometry(panel->K, kind), any, thin, K_top_matches), n_pass, retry) < n_pass) {
            qa::set_error("qa_fullpass_launch_set: %d passes do not fit one launch set", n_pass);
            return (int)QA_ERR_CAPACITY;
        }
        std::vector<std::vector<std::pair<int32_t, double>>> lists;
        BatchOut out;
        out.dosage = dosage;
        out.c = c;
        out.lists = &lists;
        const int status = run_passes(panel, n_pass, gl, flags, gammaSmall_cols_to_get, K_top_matches, 1, out, kind, always_normalize);
        if (status != QA_OK) return status;
        return pack_lists(lists, best_ptr, best_idx, best_val, best_cap);
    });
}

int qa_Rcpp_haploid_dosage_versus_refs(
    qa_panel_t *panel, const double *gl, const int32_t *gammaSmall_cols_to_get,
    const qa_fullpass_opts_t *o, double *alphaHat_t, double *betaHat_t, double *c, double *gamma_t,
    double *gammaSmall_t, double *dosage, int32_t *best_ptr, int32_t *best_idx, double *best_val,
    int64_t best_cap) {
    if (!qa::device_ready()) return QA_ERR_NO_DEVICE;
    if (!panel || !gl || !o || !gammaSmall_cols_to_get) {
        qa::set_error("qa_Rcpp_haploid_dosage_versus_refs: null argument");
        return QA_ERR_INVALID;
    }
    if (o->get_best_haps_from_thinned_sites)
        if (const int st = check_k_top("qa_Rcpp_haploid_dosage_versus_refs", o->K_top_matches)) return st;
    // A C caller that zero-initialises the options would ask the lazily normalised fp64 passes never to renormalise between
    // grid 0 and the last grid: alpha underflows over a long region, 1 / run_total = inf, NaN dosages.  A threshold that is not
    // positive (or NaN) is therefore read as "not set" = the reference's default (reference-single.cpp:2216, 1e-100).
    const double norm_threshold = o->min_emission_prob_normalization_threshold > 0 ? o->min_emission_prob_normalization_threshold : 1e-100;
    return qa::guarded([&] {
        qa::GateHold hold;
        hold.acquire(panel->gate(), &panel->arena);
        const int G = panel->G;
        std::vector<int32_t> thin(G, -1);
        const bool use_thin = o->get_best_haps_from_thinned_sites || o->return_gammaSmall_t;
        if (use_thin) for (int g = 0; g < G; g++) thin[g] = gammaSmall_cols_to_get[g];
        int32_t f = 0;
        if (o->return_dosage) f |= 1;
        // reference-single.cpp:2264-2268: alpha is kept everywhere unless only thinned outputs are wanted
        const bool only_thin = use_thin && !o->return_gamma_t && !o->return_dosage && !o->return_betaHat_t;
        if (!only_thin) f |= 2;
        if (o->return_gamma_t || o->return_gammaSmall_t) f |= 4;
        if (o->return_betaHat_t) f |= 8;
        BatchOut out;
        out.dosage = o->return_dosage ? dosage : nullptr;
        out.c = c;
        out.alphaHat_t = alphaHat_t;
        out.betaHat_t = o->return_betaHat_t ? betaHat_t : nullptr;
        out.gamma_t = o->return_gamma_t ? gamma_t : nullptr;
        out.gammaSmall_t = o->return_gammaSmall_t ? gammaSmall_t : nullptr;
        out.gamma_small_unscaled = !o->return_gamma_t;
        // the reference writes alphaHat_t column 0 in its "only thinned outputs" form too (:2347-2354); validation mode, which
        // yields every output of the call, keeps that column when grid 0 is not among the thinned grids
        out.alpha_grid0 = panel->sum_order_ref && alphaHat_t && only_thin && thin[0] < 0;
        std::vector<std::vector<std::pair<int32_t, double>>> lists;
        QA_HIP(hipSetDevice(panel->device));
        const Thin thin_dims = qa::count_thin(thin.data(), G);
        const bool want_lists = o->get_best_haps_from_thinned_sites != 0;
        const int K_top = want_lists ? o->K_top_matches : 0;
        // one pass of `kind` with flags `flags`, thinned grids `th` and K_top `kt`, planned with the un-permute staging
        // (K x nGrids doubles) in the fixed term, and with room for the non-truncating top-K retry at full length (every
        // haplotype of a label without reads ties: n_thin lists of K entries, beyond the fixed term's 2 MiB on large panels)
        auto plan = [&](PassKind kind, int32_t flags, const Thin &th, int kt) {
            const Geometry geo1 = pick_geometry(panel->K, kind);
            if (geo1.NT == 0) throw std::runtime_error("K exceeds the on-chip capacity of the full-pass kernels");
            const size_t retry = kt > 0 ? (size_t)th.n_thin * panel->K * 12 + 2 * qa::Arena::kCarveAlign : 0;
            plan_chunk(panel, plan_pass_bytes(panel, geo1, flags, th, kt, 64, false, out.alpha_grid0), 1, (size_t)panel->K * G * 8 + retry);
        };
        // fp64 dosage: the tuned kernels yield dosage and c; a call that also wants alpha / beta / gamma matrices takes the
        // generic fp64 kernels
        const bool matrices = alphaHat_t || o->return_betaHat_t || o->return_gamma_t || o->return_gammaSmall_t;
        const KindChoice kinds = choose_kinds(panel, FOR_SINGLE_PASS, o->return_dosage != 0, want_lists, matrices);
        const PassKind main_kind = kinds.dosage;
        const bool lists_alone = want_lists && panel->rank_fp64 && only_thin;
        if (pick_geometry(panel->K, main_kind).NT == 0 && !lists_alone) {
            // K x nGrids outputs (alphaHat_t / betaHat_t / gamma_t / gammaSmall_t) come from kernels that keep the whole state
            // on chip; the dosage and the best-haplotype lists (what the driver path asks for) have no such limit
            qa::set_error("K = %d: alphaHat_t / betaHat_t / gamma_t / gammaSmall_t outputs are limited to K <= 57 344 haplotypes (state on "
                          "chip); dosage, c and best_haps_stuff_list are available for any K; validation mode "
                          "(qa_panel_set_sum_order(panel, 1)) serves these outputs at any K", panel->K);
            return QA_ERR_UNSUPPORTED;
        }
        int st;
        if (main_kind == KIND_F64_DOS) {
            std::vector<int32_t> no_thin(G, -1);
            const int32_t f1 = 1;
            plan(KIND_F64_DOS, f1, Thin{}, 0);
            st = run_passes(panel, 1, gl, &f1, no_thin.data(), 0, o->normalize_emissions, out, KIND_F64_DOS,
                            o->always_normalize, norm_threshold);
            if (st == QA_OK && want_lists) {
                BatchOut out2;
                out2.lists = &lists;
                const int32_t f0 = 0;
                plan(kinds.lists, f0, thin_dims, K_top);
                st = run_passes(panel, 1, gl, &f0, thin.data(), K_top, o->normalize_emissions, out2, kinds.lists,
                                o->always_normalize, norm_threshold);
            }
        } else if (lists_alone) {
            // only the lists (and alpha at the thinned grids, c): the fp64 ranking pass, which follows the reference's
            // normalisation schedule (always_normalize / min_emission_prob_normalization_threshold honoured)
            out.lists = &lists;
            plan(rank_kind(panel), f, thin_dims, K_top);
            st = run_passes(panel, 1, gl, &f, thin.data(), K_top, o->normalize_emissions, out, rank_kind(panel),
                            o->always_normalize, norm_threshold);
        } else if (want_lists && !kinds.one_pass) {
            // the best-haplotype lists come from a pass with fp64 state, so that their membership and order are
            // the reference's; every other output comes from the fp32 pass
            plan(KIND_F32, f, thin_dims, 0);
            st = run_passes(panel, 1, gl, &f, thin.data(), 0, o->normalize_emissions, out, KIND_F32);
            if (st != QA_OK) return st;
            BatchOut out2;
            out2.lists = &lists;
            const int32_t f0 = 0;
            plan(kinds.lists, f0, thin_dims, K_top);
            st = run_passes(panel, 1, gl, &f0, thin.data(), K_top, o->normalize_emissions, out2, kinds.lists,
                            o->always_normalize, norm_threshold);
        } else {
            // one pass yields everything: fp32 state with fp32 ranking, or fp64 state (qa_panel_set_dosage_precision(64))
            if (want_lists) out.lists = &lists;
            plan(main_kind, f, thin_dims, K_top);
            st = run_passes(panel, 1, gl, &f, thin.data(), K_top, o->normalize_emissions, out, main_kind,
                            o->always_normalize, norm_threshold);
        }
        if (st != QA_OK || !want_lists) return st;
        return pack_lists(lists, best_ptr, best_idx, best_val, best_cap);
    });
}

int qa_fullpass_batch(qa_panel_t *panel, int32_t n_pass, const double *gl, const int32_t *want_dosage,
                      const int32_t *gammaSmall_cols_to_get, int32_t K_top_matches, double *dosage,
                      int32_t *best_ptr, int32_t *best_idx, double *best_val, int64_t best_cap) {
    if (!qa::device_ready()) return QA_ERR_NO_DEVICE;
    if (!panel || !gl || n_pass <= 0 || !want_dosage || !gammaSmall_cols_to_get) {
        qa::set_error("qa_fullpass_batch: bad argument");
        return QA_ERR_INVALID;
    }
    if (const int st = check_k_top("qa_fullpass_batch", K_top_matches)) return st;
    return qa::guarded([&] {
        qa::GateHold hold;
        hold.acquire(panel->gate(), &panel->arena);
        std::vector<int32_t> f(n_pass);
        for (int i = 0; i < n_pass; i++) f[i] = want_dosage[i] ? 1 : 0;
        // chunk the passes so that the alpha checkpoints fit in HBM (K = 50 000, G = 2 000: 0.4 GB per dosage
        // pass, 0.08 GB per thin pass); chunks are homogeneous so that every pass of a chunk has the same footprint
        QA_HIP(hipSetDevice(panel->device));
        const KindChoice kinds = choose_kinds(panel, FOR_GL_BATCH, true, K_top_matches > 0, false);
        const PassKind main_kind = kinds.dosage;
        const bool exact = !kinds.one_pass;   // fp64 ranking passes for the lists beside the dosage passes
        const Geometry geo = pick_geometry(panel->K, main_kind), geo64 = pick_geometry(panel->K, rank_kind(panel));
        if (geo.NT == 0 || (exact && geo64.NT == 0))
            throw std::runtime_error("K exceeds the on-chip capacity of the full-pass kernels");
        const int G = panel->G, T = panel->T;
        const Thin thin = qa::count_thin(gammaSmall_cols_to_get, G);
        std::vector<std::vector<std::pair<int32_t, double>>> lists;
        std::vector<int32_t> zeros(n_pass, 0);
        int done = 0;
        int status = QA_OK;
        while (done < n_pass && status == QA_OK) {
            const bool dos = f[done] != 0;
            int run = 0;
            while (done + run < n_pass && (f[done + run] != 0) == dos) run++;
            if (!exact) {
                const PassKind kind = dos ? main_kind : kinds.lists;
                const int n = plan_chunk(panel, plan_pass_bytes(panel, pick_geometry(panel->K, kind), f[done], thin, K_top_matches), run);
                BatchOut out;
                out.dosage = dosage ? dosage + (size_t)done * T : nullptr;
                out.lists = &lists;
                status = run_passes(panel, n, gl + (size_t)done * T * 2, f.data() + done, gammaSmall_cols_to_get,
                                    K_top_matches, 1, out, kind);
                done += n;
                continue;
            }
            // fp64-state ranking passes for the lists; dosage passes separately
            const size_t rank_bytes = plan_pass_bytes(panel, geo64, 0, thin, K_top_matches);
            int n = plan_chunk(panel, rank_bytes, run);
            if (dos) n = std::min(n, plan_chunk(panel, plan_pass_bytes(panel, geo, 1, Thin{}, 0), run));
            if (dos) {
                BatchOut out;
                out.dosage = dosage ? dosage + (size_t)done * T : nullptr;
                std::vector<int32_t> no_thin(G, -1);
                status = run_passes(panel, n, gl + (size_t)done * T * 2, f.data() + done, no_thin.data(), 0, 1, out, main_kind);
                if (status != QA_OK) break;
                plan_chunk(panel, rank_bytes, n);
            }
            BatchOut out2;
            out2.lists = &lists;
            status = run_passes(panel, n, gl + (size_t)done * T * 2, zeros.data(), gammaSmall_cols_to_get, K_top_matches, 1,
                                out2, rank_kind(panel));
            done += n;
        }
        if (status != QA_OK) return status;
        return pack_lists(lists, best_ptr, best_idx, best_val, best_cap);
    });
}

}  // extern "C"

namespace {

// selection arguments of qa_fullpass_reads_select_batch (nullptr: plain qa_fullpass_reads_batch)
struct SelectArgs {
    int32_t Ksubset, Knew;
    const int32_t *which;
    const uint64_t *seed;
    int32_t *which_next, *status;
};

// the arguments of the qa_fullpass_reads_*batch entry points (include/quilt_amd.h has their meaning)
struct ReadsCall {
    qa_panel_t *panel;
    int32_t n_chain, n_label, n_sample;
    const int32_t *chain_sample, *read_off, *read_ptr, *u, *bq, *H, *want_dosage, *want_top, *gammaSmall_cols_to_get;
    int32_t K_top_matches;
    double minGLValue;
    double *dosage;
    int32_t top_width;
    int32_t *top_idx;
    float *top_val;
    int32_t *top_cnt;
    const SelectArgs *sel = nullptr;
    int32_t gamma_grid = -1;
    double *gamma_col = nullptr;
    bool wants_lists(int c) const { return K_top_matches > 0 && (!want_top || want_top[c] != 0); }
};

// per-sample SNP-major index of the bases (input marshalling, O(bases))
struct BaseIndex { std::vector<int32_t> snp_ptr, ent_off, ent_read, ent_bq; };
BaseIndex index_bases(const ReadsCall &c) {
    const int n_sample = c.n_sample, T = c.panel->T;
    const int32_t *read_off = c.read_off, *read_ptr = c.read_ptr, *u = c.u, *bq = c.bq;
    BaseIndex ix;
    std::vector<int32_t> base_off(n_sample + 1, 0);
    ix.snp_ptr.assign((size_t)n_sample * (T + 1), 0);
    ix.ent_off.assign(n_sample, 0);
    for (int s = 0; s < n_sample; s++) {
        const int R = read_off[s + 1] - read_off[s];
        base_off[s + 1] = base_off[s] + (read_ptr + read_off[s] + s)[R];
    }
    const int totB = base_off[n_sample];
    ix.ent_read.resize(std::max(totB, 1));
    ix.ent_bq.resize(std::max(totB, 1));
    // a counting sort per sample, samples independent: spread over host threads (0.3 s on one thread for 256 samples of
    // 50 000 bases -- in front of every full-panel launch set, and uncovered whenever one host thread has the device to itself)
    // (one task per thread, each taking every n_thr-th sample: `fill` is allocated once per thread, not once per sample)
    const int n_thr = std::max(1, std::min<int>(qa::host_threads(), n_sample));
    qa::parallel_for((size_t)n_thr, n_thr, [&](size_t tid) {
        std::vector<int32_t> fill;
        for (int s = (int)tid; s < n_sample; s += n_thr) {
            const int R = read_off[s + 1] - read_off[s];
            const int32_t *rp = read_ptr + read_off[s] + s;
            const int32_t *su = u + base_off[s], *sb = bq + base_off[s];
            int32_t *sp = ix.snp_ptr.data() + (size_t)s * (T + 1);
            ix.ent_off[s] = base_off[s];
            for (int i = 0; i < rp[R]; i++) {
                if (su[i] < 0 || su[i] >= T) throw std::runtime_error("SNP index out of range");
                if (sb[i] > 255 || sb[i] < -255) throw std::runtime_error("|base quality| > 255");
                sp[su[i] + 1]++;
            }
            for (int t = 0; t < T; t++) sp[t + 1] += sp[t];
            fill.assign(sp, sp + T);
            for (int r = 0; r < R; r++)
                for (int i = rp[r]; i < rp[r + 1]; i++) {
                    const int at = fill[su[i]]++;
                    ix.ent_read[(size_t)base_off[s] + at] = r;
                    ix.ent_bq[(size_t)base_off[s] + at] = sb[i];
                }
        }
    });
    return ix;
}

// chain -> offset of its labels in H (chains are laid out back to back, each with its sample's R)
std::vector<int32_t> label_offsets(const ReadsCall &c) {
    std::vector<int32_t> hoff(c.n_chain + 1, 0);
    for (int i = 0; i < c.n_chain; i++) {
        const int s = c.chain_sample[i];
        if (s < 0 || s >= c.n_sample) throw std::runtime_error("chain_sample out of range");
        hoff[i + 1] = hoff[i] + (c.read_off[s + 1] - c.read_off[s]);
    }
    return hoff;
}

// Work groups of passes (pass = chain x label).  With fp64 ranking (the default) the dosage comes from a pass
// with fp32 state and the best-haplotype lists from a pass with fp64 state; a chain that wants both runs both.
struct Group { std::vector<int32_t> ids; int32_t flag; int K_top; PassKind kind; };
std::vector<Group> form_groups(const ReadsCall &c) {
    const KindChoice kinds = choose_kinds(c.panel, FOR_READS_BATCH, true, true, false);
    Group gd{{}, 1, 0, kinds.dosage}, gdt{{}, 1, c.K_top_matches, kinds.dosage}, gt{{}, 0, c.K_top_matches, kinds.lists};
    for (int i = 0; i < c.n_chain; i++) {
        const bool dos = c.want_dosage[i] != 0, top = c.wants_lists(i);
        for (int l = 0; l < c.n_label; l++) {
            const int id = i * c.n_label + l;
            if (!kinds.one_pass) {
                if (dos) gd.ids.push_back(id);
                if (top) gt.ids.push_back(id);
            } else {
                if (dos && top) gdt.ids.push_back(id);
                else if (dos) gd.ids.push_back(id);
                else if (top) gt.ids.push_back(id);
            }
        }
    }
    std::vector<Group> groups;
    for (Group *g : {&gd, &gdt, &gt}) if (!g->ids.empty()) groups.push_back(std::move(*g));
    return groups;
}

// eps tables from the host libm (convertScaledBQtoProbs, as copied-from-stitch.cpp:166-175)
std::vector<double> quality_tables() {
    std::vector<double> tabs(4 * 256);
    for (int q = 0; q < 256; q++) {
        const double e = std::pow(10, -(double)q / 10);
        tabs[q] = 1 - e; tabs[256 + q] = e / 3; tabs[512 + q] = e / 3; tabs[768 + q] = 1 - e;
    }
    return tabs;
}

// Per-call device buffers, carved from the handle's grow-only side arena (no hipMalloc / hipFree per call).  ONE list of
// (buffer, count) gives both the arena's required size and the carves.
struct ReadsAux {
    qa::ABuf<int32_t> ps, pl, ph;        // [P] per pass of the group in hand: sample, label, offset of the chain's labels
    qa::ABuf<int32_t> sp, eo, er, eb, H; // the base index and the labels
    qa::ABuf<double> tabs;
    // with the device-side selection: the call-wide list table [chain * n_label + label][thinned grid][top_width], its
    // counts, the rows of the launch set in hand, and the selection's own arrays
    qa::ABuf<int32_t> top_all, cnt_all, rows, which, next, stat, want;
    qa::ABuf<uint64_t> seed;
};
struct AuxItem { size_t bytes; std::function<void()> carve; };
template <typename T>
AuxItem aux_item(qa::ABuf<T> &b, qa::Arena *arena, size_t n) {
    n = std::max<size_t>(n, 1);
    return {n * sizeof(T), [&b, arena, n] { b.arena = arena; b.ensure(n); }};
}
void carve_aux(const ReadsCall &c, ReadsAux &a, const BaseIndex &ix, size_t n_labels, size_t n_tabs, int n_thin) {
    qa::Arena *A = &c.panel->aux;
    const size_t P = (size_t)c.n_chain * c.n_label, n_out = P * n_thin, n_chain = c.n_chain;
    std::vector<AuxItem> items = {aux_item(a.ps, A, P), aux_item(a.pl, A, P), aux_item(a.ph, A, P), aux_item(a.sp, A, ix.snp_ptr.size()),
                                  aux_item(a.eo, A, c.n_sample), aux_item(a.er, A, ix.ent_read.size()),
                                  aux_item(a.eb, A, ix.ent_bq.size()), aux_item(a.H, A, n_labels), aux_item(a.tabs, A, n_tabs)};
    if (c.sel)
        for (const AuxItem &i : {aux_item(a.top_all, A, n_out * c.top_width), aux_item(a.cnt_all, A, n_out), aux_item(a.rows, A, P),
                            aux_item(a.which, A, n_chain * c.sel->Ksubset), aux_item(a.next, A, n_chain * c.sel->Ksubset),
                            aux_item(a.stat, A, n_chain), aux_item(a.want, A, n_chain), aux_item(a.seed, A, n_chain)})
            items.push_back(i);
    size_t need = 0;
    for (const AuxItem &i : items) need += (i.bytes + qa::Arena::kCarveAlign - 1) / qa::Arena::kCarveAlign * qa::Arena::kCarveAlign;
    if (need > A->cap) A->require(need + need / 4);
    A->reset();
    for (const AuxItem &i : items) i.carve();
}

// what the stages of one call share
struct ReadsWork {
    qa_panel::Scratch &S;
    hipStream_t st;
    Thin thin;
    std::vector<int32_t> hoff, no_thin;
    ReadsAux aux;
    bool lists_to_host;
    int status = QA_OK;
    double t_kern = 0, t_run = 0;
};
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// one group: its passes' likelihoods (k_make_gl), the passes, their lists to the call-wide device table and to the caller --
// launch set by launch set
void run_group(const ReadsCall &c, const Group &grp, ReadsWork &w) {
    qa_panel *panel = c.panel;
    auto &S = w.S;
    ReadsAux &a = w.aux;
    hipStream_t st = w.st;
    const int T = panel->T, n_label = c.n_label, n_thin = w.thin.n_thin, top_width = c.top_width;
    const Geometry geo = pick_geometry(panel->K, grp.kind);
    if (geo.NT == 0) throw std::runtime_error("K exceeds the on-chip capacity of the full-pass kernels");
    const int n_grp = (int)grp.ids.size();
    std::vector<int32_t> ps(n_grp), pl(n_grp), ph(n_grp), flags(n_grp, grp.flag);
    for (int i = 0; i < n_grp; i++) {
        const int ch = grp.ids[i] / n_label, l = grp.ids[i] % n_label;
        ps[i] = c.chain_sample[ch]; pl[i] = l + 1; ph[i] = w.hoff[ch];
    }
    QA_HIP(hipStreamSynchronize(st));   // the previous group's launches read ps / pl / ph
    a.ps.upload(ps.data(), n_grp, st); a.pl.upload(pl.data(), n_grp, st); a.ph.upload(ph.data(), n_grp, st);
    const bool gc = c.gamma_col && grp.flag != 0;
    const int32_t *thin_col = grp.K_top > 0 ? c.gammaSmall_cols_to_get : w.no_thin.data();
    // the layout run_passes will build for passes like these: the plan, and the carve of the likelihoods k_make_gl writes
    const PassLayout L(dims_of(panel), geo, qa::make_request(&grp.flag, 1, grp.K_top > 0 ? w.thin : Thin{}, grp.K_top, top_width, gc));
    int done = 0;
    while (done < n_grp && w.status == QA_OK) {
        const int n = plan_chunk(panel, L.pass_bytes(qa::Arena::kCarveAlign), n_grp - done);
        carve(S.gl, L, PassLayout::GL, n);
        GlParams gp{};
        gp.P = n; gp.T = T; gp.pass_sample = a.ps.p + done; gp.pass_label = a.pl.p + done; gp.pass_hoff = a.ph.p + done;
        gp.snp_ptr = a.sp.p; gp.ent_off = a.eo.p; gp.ent_read = a.er.p; gp.ent_bq = a.eb.p; gp.H = a.H.p;
        gp.pR_tab = a.tabs.p; gp.pA_tab = a.tabs.p + 512; gp.minGLValue = c.minGLValue; gp.gl = S.gl.p;
        hipLaunchKernelGGL(k_make_gl, dim3((T + 255) / 256, n), dim3(256), 0, st, gp);
        QA_HIP(hipGetLastError());
        BatchOut out;
        out.dosage = grp.flag ? c.dosage : nullptr;
        out.dosage_rows = grp.ids.data() + done;
        if (gc) {
            out.gamma_col = c.gamma_col;
            out.gamma_grid = c.gamma_grid;
            out.gamma_rows = grp.ids.data() + done;
        }
        std::vector<int32_t> fidx;
        std::vector<double> fval;
        if (w.lists_to_host) {   // with the selection on the device the lists need not cross PCIe
            out.flat_idx = &fidx;
            out.flat_val = &fval;
        }
        out.top_cap = top_width;      // k_topk keeps the ordered head of each list: all the driver reads
        out.order_by_value = true;
        out.truncate_lists = true;
        std::vector<int32_t> true_cnt;
        out.true_counts = &true_cnt;
        const double tr = now_s();
        w.status = run_passes(panel, n, nullptr, flags.data() + done, thin_col, grp.K_top, 1, out, grp.kind);
        w.t_run += now_s() - tr;
        w.t_kern += g_timing[5] / 1e3;
        if (w.status != QA_OK) break;
        // compact, already ordered lists: the first top_width entries of every (pass, thinned grid)
        if (grp.K_top > 0 && c.sel) {   // this launch set's lists to their rows of the call-wide device table
            a.rows.upload(grp.ids.data() + done, n, st);
            qa::launch_scatter_lists(S.top_idx.p, S.top_cnt.p, a.rows.p, n, n_thin, top_width, a.top_all.p, a.cnt_all.p, st);
            QA_HIP(hipStreamSynchronize(st));   // rows is re-used by the next launch set
        }
        if (grp.K_top > 0) {
            for (int i = 0; i < n * n_thin; i++) {
                const size_t o = (size_t)grp.ids[done + i / n_thin] * n_thin + (i % n_thin);
                const int len = w.lists_to_host ? std::min<int>(true_cnt[i], top_width) : 0;
                if (c.top_cnt) c.top_cnt[o] = true_cnt[i];
                for (int q = 0; q < len; q++) {
                    if (c.top_idx) c.top_idx[o * top_width + q] = fidx[(size_t)i * top_width + q];
                    if (c.top_val) c.top_val[o * top_width + q] = (float)fval[(size_t)i * top_width + q];
                }
            }
        }
        done += n;
    }
}

// launch_select launched nothing (tables beyond the LDS): every chain is left to the caller's host path -- status 1 for a chain
// that wanted a selection, -1 for one that did not, as k_select itself reports them
void statuses_when_not_launched(const int32_t *want, int n_chain, int32_t *status) {
    for (int i = 0; i < n_chain; i++) status[i] = want[i] ? 1 : -1;
}

// what a selection may be asked for: the public entries and the test hook (fullpass_testhook.h) refuse the same calls
bool selection_sizes_ok(int K, int Ksubset, int Knew, int K_top_matches) {
    return Ksubset >= 1 && Ksubset <= K && Knew >= 0 && Knew <= Ksubset && K_top_matches >= 1;
}
bool which_in_range(const int32_t *which, size_t n, int K) {
    for (size_t i = 0; i < n; i++)
        if (which[i] < 1 || which[i] > K) return false;
    return true;
}

// everything_select_good_haps for every chain that asked for lists (select.hip), on the lists still on the device
void select_on_device(const ReadsCall &c, ReadsWork &w) {
    const SelectArgs *sel = c.sel;
    ReadsAux &a = w.aux;
    hipStream_t st = w.st;
    const int n_chain = c.n_chain, n_thin = w.thin.n_thin;
    const size_t n_out = (size_t)n_chain * c.n_label * n_thin;
    std::vector<int32_t> want(n_chain);
    for (int i = 0; i < n_chain; i++) want[i] = c.wants_lists(i);
    a.which.upload(sel->which, (size_t)n_chain * sel->Ksubset, st);
    a.seed.upload(sel->seed, n_chain, st);
    a.want.upload(want.data(), n_chain, st);
    qa::SelectParams sp{};
    sp.n_label = c.n_label; sp.n_thin = n_thin; sp.top_width = c.top_width; sp.K_top_matches = c.K_top_matches; sp.K = c.panel->K;
    sp.Ksubset = sel->Ksubset; sp.Knew = sel->Knew; sp.top = a.top_all.p; sp.which = a.which.p; sp.seed = a.seed.p;
    sp.want = a.want.p; sp.out = a.next.p; sp.status = a.stat.p;
    hipEvent_t e0, e1;
    QA_HIP(hipEventCreate(&e0)); QA_HIP(hipEventCreate(&e1));
    QA_HIP(hipEventRecord(e0, st));
    const bool launched = qa::launch_select(sp, n_chain, st);
    QA_HIP(hipEventRecord(e1, st));
    if (launched) {
        a.next.download(sel->which_next, (size_t)n_chain * sel->Ksubset, st);
        a.stat.download(sel->status, n_chain, st);
    } else {
        statuses_when_not_launched(want.data(), n_chain, sel->status);
    }
    QA_HIP(hipStreamSynchronize(st));
    float ms = 0;
    QA_HIP(hipEventElapsedTime(&ms, e0, e1));
    qa::profile_add(qa::PK_SELECT, ms, (double)n_out * c.top_width * 4.0 + (double)n_chain * sel->Ksubset * 8.0,
                    qa::profile_clock_ms(e0), n_chain);
    QA_HIP(hipEventDestroy(e0)); QA_HIP(hipEventDestroy(e1));
    // a truncated list only matters to the exhausted branch, which the device leaves to the host (status 1)
}

int fullpass_reads_impl(const ReadsCall &c) {
    qa_panel_t *panel = c.panel;
    const SelectArgs *sel = c.sel;
    if (!qa::device_ready()) return QA_ERR_NO_DEVICE;
    if (const int st = check_k_top("qa_fullpass_reads_batch", c.K_top_matches)) return st;
    if (!panel || c.n_chain <= 0 || c.n_label < 1 || c.n_label > 3 || c.n_sample <= 0 || !c.chain_sample || !c.read_off || !c.read_ptr ||
        !c.u || !c.bq || !c.H || !c.want_dosage || !c.gammaSmall_cols_to_get || c.top_width < c.K_top_matches || c.top_width > 64) {
        qa::set_error("qa_fullpass_reads_batch: bad argument");
        return QA_ERR_INVALID;
    }
    if (sel && (!selection_sizes_ok(panel->K, sel->Ksubset, sel->Knew, c.K_top_matches) || !sel->which || !sel->seed ||
                !sel->which_next || !sel->status)) {
        qa::set_error("qa_fullpass_reads_select_batch: bad selection argument");
        return QA_ERR_INVALID;
    }
    if (c.gamma_col) {
        if (c.gamma_grid < 0 || c.gamma_grid >= panel->G) {
            qa::set_error("qa_fullpass_reads_select_gamma_batch: gamma_grid = %d outside [0, nGrids = %d)", c.gamma_grid, panel->G);
            return QA_ERR_INVALID;
        }
        const int st = qa::gamma_column_check(panel, "qa_fullpass_reads_select_gamma_batch");
        if (st != QA_OK) return st;
    }
    if (sel && !which_in_range(sel->which, (size_t)c.n_chain * sel->Ksubset, panel->K)) {
        qa::set_error("qa_fullpass_reads_select_batch: which_haps_to_use out of range");
        return QA_ERR_INVALID;
    }
    return qa::guarded([&] {
        QA_HIP(hipSetDevice(panel->device));
        if (!panel->scratch) panel->scratch = new qa_panel::Scratch(&panel->A());
        const int P = c.n_chain * c.n_label;
        const bool tmg = getenv("QA_TIMING") != nullptr;
        const double T0 = now_s();
        ReadsWork w{*panel->scratch, panel->pass_stream ? panel->pass_stream : panel->stream,
                    qa::count_thin(c.gammaSmall_cols_to_get, panel->G)};
        hipStream_t st = w.st;
        const BaseIndex ix = index_bases(c);
        w.hoff = label_offsets(c);
        const std::vector<Group> groups = form_groups(c);
        const std::vector<double> tabs = quality_tables();
        const int n_labels = w.hoff[c.n_chain];
        ReadsAux &a = w.aux;
        carve_aux(c, a, ix, n_labels, tabs.size(), w.thin.n_thin);
        a.sp.upload(ix.snp_ptr.data(), ix.snp_ptr.size(), st); a.eo.upload(ix.ent_off.data(), c.n_sample, st);
        a.er.upload(ix.ent_read.data(), ix.ent_read.size(), st); a.eb.upload(ix.ent_bq.data(), ix.ent_bq.size(), st);
        a.H.upload(c.H, n_labels, st); a.tabs.upload(tabs.data(), tabs.size(), st);

        const size_t n_out = (size_t)P * w.thin.n_thin;
        if (c.top_cnt) std::fill(c.top_cnt, c.top_cnt + n_out, 0);
        if (c.top_idx) std::fill(c.top_idx, c.top_idx + n_out * c.top_width, -1);
        if (c.top_val) std::fill(c.top_val, c.top_val + n_out * c.top_width, 0.f);
        w.no_thin.assign(panel->G, -1);
        // (no memset of the call-wide list table: the scatter kernel writes every entry of every row of a chain that wants
        // lists, -1 past the list's end, and the selection reads no other rows; the runtime's fill is a blit with 512-thread
        // workgroups, which waits for a compute unit free of the other host thread's Gibbs waves -- half a second per
        // occurrence in the r02 trace)
        w.lists_to_host = c.top_idx || c.top_val;
        // ---- everything above is host work and uploads into this handle's own buffers; the launch sets below have the
        // device (exclusive phases: queue behind the other handles' launch sets) and the arena
        const double T1q = now_s();
        qa::GateHold hold;
        hold.acquire(panel->gate(), &panel->arena);
        const double T1 = now_s();
        for (const Group &grp : groups) {
            run_group(c, grp, w);
            if (w.status != QA_OK) break;
        }
        if (sel && w.status == QA_OK) select_on_device(c, w);
        hold.release();
        if (tmg)
            fprintf(stderr, "[qa_fullpass_reads P=%d] index+uploads %.3f s, queued for the device %.3f s, run_passes %.3f s (device %.3f s), scatter etc %.3f s\n", P,
                    T1q - T0, T1 - T1q, w.t_run, w.t_kern, now_s() - T1 - w.t_run);
        return w.status;
    });
}

}  // namespace

extern "C" {

int qa_fullpass_reads_batch(qa_panel_t *panel, int32_t n_chain, int32_t n_label, int32_t n_sample,
                            const int32_t *chain_sample, const int32_t *read_off, const int32_t *read_ptr,
                            const int32_t *u, const int32_t *bq, const int32_t *H, const int32_t *want_dosage,
                            const int32_t *want_top, const int32_t *gammaSmall_cols_to_get, int32_t K_top_matches,
                            double minGLValue,
                            double *dosage, int32_t top_width, int32_t *top_idx, float *top_val, int32_t *top_cnt) {
    return fullpass_reads_impl(ReadsCall{panel, n_chain, n_label, n_sample, chain_sample, read_off, read_ptr, u, bq, H, want_dosage,
                                         want_top, gammaSmall_cols_to_get, K_top_matches, minGLValue, dosage, top_width, top_idx,
                                         top_val, top_cnt});
}

int qa_fullpass_reads_select_batch(qa_panel_t *panel, int32_t n_chain, int32_t n_label, int32_t n_sample,
                                   const int32_t *chain_sample, const int32_t *read_off, const int32_t *read_ptr,
                                   const int32_t *u, const int32_t *bq, const int32_t *H, const int32_t *want_dosage,
                                   const int32_t *want_top, const int32_t *gammaSmall_cols_to_get, int32_t K_top_matches,
                                   double minGLValue, double *dosage, int32_t top_width, int32_t *top_idx, float *top_val,
                                   int32_t *top_cnt, int32_t Ksubset, int32_t Knew, const int32_t *which_haps_to_use,
                                   const uint64_t *seed_select, int32_t *which_next, int32_t *select_status) {
    const SelectArgs sel{Ksubset, Knew, which_haps_to_use, seed_select, which_next, select_status};
    return fullpass_reads_impl(ReadsCall{panel, n_chain, n_label, n_sample, chain_sample, read_off, read_ptr, u, bq, H, want_dosage,
                                         want_top, gammaSmall_cols_to_get, K_top_matches, minGLValue, dosage, top_width, top_idx,
                                         top_val, top_cnt, &sel});
}

int qa_fullpass_reads_select_gamma_batch(qa_panel_t *panel, int32_t n_chain, int32_t n_label, int32_t n_sample,
                                         const int32_t *chain_sample, const int32_t *read_off, const int32_t *read_ptr,
                                         const int32_t *u, const int32_t *bq, const int32_t *H, const int32_t *want_dosage,
                                         const int32_t *want_top, const int32_t *gammaSmall_cols_to_get, int32_t K_top_matches,
                                         double minGLValue, double *dosage, int32_t top_width, int32_t *top_idx, float *top_val,
                                         int32_t *top_cnt, int32_t Ksubset, int32_t Knew, const int32_t *which_haps_to_use,
                                         const uint64_t *seed_select, int32_t *which_next, int32_t *select_status,
                                         int32_t gamma_grid, double *gamma_col) {
    if (!qa::device_ready()) return QA_ERR_NO_DEVICE;
    if (!gamma_col) {
        qa::set_error("qa_fullpass_reads_select_gamma_batch: gamma_col is NULL");
        return QA_ERR_INVALID;
    }
    const SelectArgs sel{Ksubset, Knew, which_haps_to_use, seed_select, which_next, select_status};
    return fullpass_reads_impl(ReadsCall{panel, n_chain, n_label, n_sample, chain_sample, read_off, read_ptr, u, bq, H, want_dosage,
                                         want_top, gammaSmall_cols_to_get, K_top_matches, minGLValue, dosage, top_width, top_idx,
                                         top_val, top_cnt, &sel, gamma_grid, gamma_col});
}

// fullpass_testhook.h: the selection kernel on lists the caller supplies
int qa_select_from_lists(int32_t n_chain, int32_t n_label, int32_t n_thin, int32_t top_width, int32_t K_top_matches, int32_t K,
                         int32_t Ksubset, int32_t Knew, const int32_t *top, const int32_t *which, const uint64_t *seed,
                         const int32_t *want, int32_t *which_next, int32_t *status) {
    if (!qa::device_ready()) return QA_ERR_NO_DEVICE;
    if (const int st = check_k_top("qa_select_from_lists", K_top_matches)) return st;
    if (n_chain <= 0 || n_label < 1 || n_label > 3 || n_thin < 1 || K < 1 || !top || !which || !seed || !want || !which_next || !status ||
        top_width < K_top_matches || top_width > 64) {
        qa::set_error("qa_select_from_lists: bad argument");
        return QA_ERR_INVALID;
    }
    if (!selection_sizes_ok(K, Ksubset, Knew, K_top_matches)) {
        qa::set_error("qa_select_from_lists: bad selection argument");
        return QA_ERR_INVALID;
    }
    const size_t n_top = (size_t)n_chain * n_label * n_thin * top_width, n_which = (size_t)n_chain * Ksubset;
    if (!which_in_range(which, n_which, K)) {
        qa::set_error("qa_select_from_lists: which_haps_to_use out of range");
        return QA_ERR_INVALID;
    }
    for (size_t i = 0; i < n_top; i++)   // (the product's table comes from k_topk; here from a caller)
        if (top[i] < -1 || top[i] >= K) {
            qa::set_error("qa_select_from_lists: list entry out of range");
            return QA_ERR_INVALID;
        }
    return qa::guarded([&] {
        qa::DBuf<int32_t> d_top(n_top), d_which(n_which), d_want(n_chain), d_next(n_which), d_stat(n_chain);
        qa::DBuf<uint64_t> d_seed(n_chain);
        hipStream_t st = nullptr;
        d_top.upload(top, n_top, st); d_which.upload(which, n_which, st); d_want.upload(want, n_chain, st);
        d_seed.upload(seed, n_chain, st);
        d_next.upload(which_next, n_which, st);   // rows of chains that are not wanted, or handed back, stay as the caller filled them
        qa::SelectParams sp{};
        sp.n_label = n_label; sp.n_thin = n_thin; sp.top_width = top_width; sp.K_top_matches = K_top_matches; sp.K = K;
        sp.Ksubset = Ksubset; sp.Knew = Knew; sp.top = d_top.p; sp.which = d_which.p; sp.seed = d_seed.p;
        sp.want = d_want.p; sp.out = d_next.p; sp.status = d_stat.p;
        if (qa::launch_select(sp, n_chain, st)) {
            d_next.download(which_next, n_which, st);
            d_stat.download(status, n_chain, st);
        } else {
            statuses_when_not_launched(want, n_chain, status);
        }
        QA_HIP(hipStreamSynchronize(st));
        return (int)QA_OK;
    });
}

}  // extern "C"
