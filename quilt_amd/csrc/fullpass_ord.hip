// fullpass_ord.hip -- the reference-order full-panel passes AT BATCH THROUGHPUT (qa_panel_set_sum_order_batched(panel, 1) on
// top of qa_panel_set_sum_order(panel, 1 | 2)): the arithmetic of fullpass_ref.hip operation for operation -- the same
// element-wise updates, every K-wide sum in the reference's order (the header of fullpass_ref.hip lists them) -- and hence
// the same bits, from kernels laid out for a launch set of many passes instead of for one.
//
// What the validation kernels cost a batch while a pass's state fits LDS: a 256-thread workgroup per pass with up to 144 KB
// of LDS, so a compute unit holds ONE pass, and three of its four waves wait while wave 0 walks a sum.  A prescribed order makes one
// pass's sum a chain of dependent adds, but the chains of different passes are independent.  Here:
//   * ONE WAVE PER PASS (a 64-thread workgroup).  Nothing inside a pass idles: the wave that updates the column is the wave
//     that adds it.
//   * The state (alpha resp. beta) and the gamma column live in the pass's HBM scratch -- PassParams::spill, the 2 Kq doubles
//     per pass that the REF kind always carves (pass_layout.hpp: no new buffer); only the grid's emission table and
//     matched_gammas sit in LDS (4 KB), so a SIMD holds its eight waves = eight passes and their add chains interleave in
//     the VALU: the latency of one pass's dependent add is filled by the others'.
//   * The element-wise update of a grid and its sum are ONE walk over the column: a lane forms its 64-block's value, stores
//     it and feeds it to the ordered adds from the register (v_readlane), so the column is not read a second time.  The
//     grid's specials, which the reference adds FIRST, are formed ahead of the walk by the same expression (same operands,
//     same operations: same bits as the value the walk then stores).
//   * matched_gammas: one walk over the column for all (up to 256) codes.  The code of haplotype k is wave-uniform, so lane
//     (code & 63) adds gamma(k) to its accumulator number (code >> 6) -- per code the adds come in k order, as the reference's.
//     The validation kernel's thread `code` also adds +0.0 for every other haplotype; m + 0.0 == m for every m that a sum
//     started at +0.0 can hold, so leaving those adds out changes no bit.
// Outputs in the layout of the generic kernels (geometry NT = 256), exactly as fullpass_ref.hip writes them.
//
// MEASURED (profiles/sum_order_batched.json): at K = 50 000 x 2 000 grids this form is NOT faster -- 0.85x the
// validation kernels' passes/s for ranking passes, 0.67x for dosage passes, in launch sets of 256 and of 1 024.  At that K the
// validation kernels keep their state in the spill scratch too (it exceeds LDS), so they already run several workgroups per
// compute unit, and their four waves share a pass's element-wise work; 1 024 passes are one wave per SIMD here, so no chains
// interleave.  The one-pass-per-compute-unit cost described above is that of panels whose state sits in LDS (Kq <= 8 192).
#include "fullpass_ref_dev.hpp"

namespace {

constexpr int kWT = 64;   // threads per pass: one wave

// the grid's emission table, global -> LDS
__device__ __forceinline__ void load_table(double *et, const double *src, int lane) {
    __syncthreads();   // the previous readers of the table are done; the pass's earlier stores to its scratch are visible
#pragma unroll
    for (int i = 0; i < kMaxRow / kWT; i++) et[lane + kWT * i] = src[lane + kWT * i];
    __syncthreads();
}

// s + value(list[0]) + value(list[1]) + ... : the grid's special haplotypes, in list order.  value(k): the updated state of k.
template <typename F>
__device__ __forceinline__ double specials_sum(const int32_t *list, int n, double s, int lane, F value) {
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const double x = i < n ? value(list[i]) : 0.0;
        s = add_lanes_in_order(s, x);
    }
    return s;
}
// state[k] <- value(k) for every k, and s + state[0] + ... + state[K-1] left to right in the same walk.  SKIP0: haplotypes
// with code 0 contribute an exact zero.  Lanes past K add +0.0.
template <bool SKIP0, typename F>
__device__ __forceinline__ double update_and_sum(double *state, const uint8_t *code, int K, double s, int lane, F value) {
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        double x = 0.0;
        if (k < K) {
            x = value(k);
            state[k] = x;
            if (SKIP0 && code[k] == 0) x = 0.0;
        }
        s = add_lanes_in_order(s, x);
    }
    return s;
}
// ... and Armadillo's arrayops::accumulate instead (fullpass_ref.hip, serial_sum_arma): even k into acc1, odd k into acc2
template <typename F>
__device__ __forceinline__ double update_and_sum_arma(double *state, int K, int lane, F value) {
    double acc1 = 0.0, acc2 = 0.0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        double x = 0.0;
        if (k < K) {
            x = value(k);
            state[k] = x;
        }
        static_for<32>([&](auto ic) {
            acc1 += lane_value<2 * decltype(ic)::value>(x);
            acc2 += lane_value<2 * decltype(ic)::value + 1>(x);
        });
    }
    return acc1 + acc2;
}

// ---------------------------------------------------------------------------------------------
// forward (k_fwd_ro)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWT) void k_fwd_ord(PassParams prm, int NT) {
    __shared__ double et[kMaxRow];
    const int p = blockIdx.x, lane = threadIdx.x;
    const int K = prm.K, G = prm.G;
    const double *emat = static_cast<const double *>(prm.emat) + (size_t)p * G * kMaxRow;
    const double *esp = static_cast<const double *>(prm.esp) + (size_t)p * prm.esp_stride;
    const double *emin = prm.emin + (size_t)p * G;
    double *aout = static_cast<double *>(prm.alpha) + (size_t)p * prm.alpha_pass_stride;
    const int32_t *slot = prm.alpha_slot + (size_t)p * G;
    double *state = prm.spill + (size_t)p * prm.spill_pass_stride;
    const double double_K = (double)K, one_over_K = 1 / (double)K;

    double prev_sum = 1, running_min = 1;
    for (int g = 0; g < G; g++) {
        const uint8_t *code = prm.hm + (size_t)g * prm.Kp;
        load_table(et, emat + (size_t)g * kMaxRow, lane);
        const GridEm E = grid_em(prm, et, esp, g);
        const double em = emin[g];
        const bool has_variant = g == 0 || em >= 0;   // (grid 1 is forced: k_emat, :964-966)
        double sig = 1.0, addend = 0.0;
        if (g > 0) {
            sig = prm.sigma[g - 1];
            const double jump_prob = prm.tm1[g - 1] / double_K;
            const double jump_prob_plus = prm.always_normalize ? jump_prob : jump_prob * prev_sum;
            addend = jump_prob_plus / sig;
        }
        double run_total;
        if (g == 0) {
            const auto first = [&](int k) { return E.at(k, code[k]) * one_over_K; };
            run_total = prm.grid0_left_to_right ? update_and_sum<false>(state, code, K, 0.0, lane, first)
                                                : update_and_sum_arma(state, K, lane, first);
        } else if (has_variant) {
            const auto step = [&](int k) { return (addend + state[k]) * E.at(k, code[k]); };
            run_total = specials_sum(E.sp_k, E.sn, 0.0, lane, step);
            run_total = update_and_sum<true>(state, code, K, run_total, lane, step);
        } else {
            for (int k = lane; k < K; k += kWT) state[k] = addend + state[k];
            run_total = prev_sum / sig;   // (:1078-1088)
        }
        double cg = 1.0;
        if (g > 0) {
            if (has_variant) running_min = running_min * em;
            cg = cg / sig;
        }
        const bool renorm = g == 0 || prm.always_normalize || running_min < prm.norm_threshold || g == G - 1;
        double xs = 1.0;
        if (renorm) {
            xs = 1 / run_total;
            cg = (g == 0) ? xs : cg / run_total;
            run_total = 1;
            running_min = 1;
        }
        prev_sum = run_total;
        if (lane == 0) prm.c[(size_t)p * G + g] = cg;
        const int sl = slot[g];
        if (renorm || sl >= 0) {
            double *dst = aout + (size_t)max(sl, 0) * prm.alpha_col_elems;
            for (int k = lane; k < K; k += kWT) {
                double v = state[k];
                if (renorm) {
                    v *= xs;
                    state[k] = v;
                }
                if (sl >= 0) dst[perm_index(k, NT)] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// backward (k_bwd_ro<GCOL>)
// ---------------------------------------------------------------------------------------------
template <bool GCOL>
__global__ __launch_bounds__(kWT) void k_bwd_ord(PassParams prm, int NT) {
    __shared__ double et[kMaxRow];
    __shared__ double mt[kMaxRow];   // matched_gammas
    const int p = blockIdx.x, lane = threadIdx.x;
    const int K = prm.K, G = prm.G, T = prm.T;
    const int flags = prm.flags[p];
    const bool want_dosage = (flags & 1) != 0, want_gamma = (flags & 4) != 0, want_beta = (flags & 8) != 0;
    const double *emat = static_cast<const double *>(prm.emat) + (size_t)p * G * kMaxRow;
    const double *esp = static_cast<const double *>(prm.esp) + (size_t)p * prm.esp_stride;
    const double *emin = prm.emin + (size_t)p * G;
    const double *ain = static_cast<const double *>(prm.alpha) + (size_t)p * prm.alpha_pass_stride;
    const int32_t *slot = prm.alpha_slot + (size_t)p * G;
    const double *cvec = prm.c + (size_t)p * G;
    double *state = prm.spill + (size_t)p * prm.spill_pass_stride;
    double *gam = state + prm.Kq;
    const double double_K = (double)K;
    const double eps = prm.ref_error, ome = 1 - eps;

    for (int k = lane; k < K; k += kWT) state[k] = 1.0;   // 1 / not_jump_prob, not_jump_prob = 1 (:1855-1857)
    double not_jump_prob = 1.0, B_prev = 1.0;
    double B_prev_star = double_K * cvec[G - 1] * not_jump_prob;
    for (int g = G - 1; g >= 0; --g) {
        const double c_g = cvec[g];
        bool add_val = false;
        double val = 0.0;
        if (g < G - 1) {
            const double jump_prob = prm.tm1[g] / double_K;
            not_jump_prob = prm.sigma[g];
            const bool has_variant = (g + 1 == 1 ? prm.emin_b1[p] : emin[g + 1]) >= 0;   // (grid 1 is not forced here: :1866-1877)
            if (has_variant) {
                const uint8_t *code1 = prm.hm + (size_t)(g + 1) * prm.Kp;
                load_table(et, emat + (size_t)(g + 1) * kMaxRow, lane);
                const GridEm E = grid_em(prm, et, esp, g + 1);
                const auto step = [&](int k) { return state[k] * E.at(k, code1[k]); };
                double s = specials_sum(E.sp_k, E.sn, 0.0, lane, step);
                s = update_and_sum<true>(state, code1, K, s, lane, step);
                val = jump_prob / not_jump_prob * s;
                B_prev = s;
            } else {
                val = jump_prob / not_jump_prob * B_prev_star;
                B_prev = B_prev_star;
            }
            add_val = true;
            B_prev_star = c_g * B_prev;
        }
        const uint8_t *code = prm.hm + (size_t)g * prm.Kp;
        const int tcol = prm.thin_col[g];
        const int sl = slot[g];
        const bool to_thin = tcol >= 0 && prm.K_top > 0 && prm.beta_thin;
        const bool gcol_here = GCOL && g == prm.gamma_grid;
        const bool form_gamma = (want_dosage || want_gamma || gcol_here) && sl >= 0;
        const bool dosage_here = want_dosage && sl >= 0;
        const double x = c_g * not_jump_prob;   // beta *= c_g * sigma_g (:2165-2166)
        {
            // the grid's element-wise work on beta(k), one walk: + val; the unscaled column to k_topk (which forms gamma =
            // alpha * beta and picks, :2020-2031: comparisons only); gamma(k); * c_g sigma_g
            double *thin_dst = to_thin ? static_cast<double *>(prm.beta_thin) + ((size_t)p * prm.n_thin + tcol) * prm.Kq : nullptr;
            const double *acol = form_gamma ? ain + (size_t)sl * prm.alpha_col_elems : nullptr;
            double *gamma_dst = want_gamma && form_gamma ? static_cast<double *>(prm.gamma_out) + ((size_t)p * G + g) * prm.Kq : nullptr;
            double *gcol_dst = gcol_here && form_gamma ? prm.gamma_col + (size_t)p * prm.Kq : nullptr;
            double *beta_dst = want_beta ? static_cast<double *>(prm.beta_out) + ((size_t)p * G + g) * prm.Kq : nullptr;
            for (int k = lane; k < K; k += kWT) {
                double b = state[k];
                if (add_val) b = b + val;
                const size_t pk = perm_index(k, NT);
                if (thin_dst) thin_dst[pk] = b;
                if (acol) {
                    const double gk = acol[pk] * b;
                    gam[k] = gk;
                    if (gamma_dst) gamma_dst[pk] = gk * not_jump_prob;
                    if (gcol_dst) gcol_dst[k] = gk * not_jump_prob;
                }
                b *= x;
                state[k] = b;
                if (beta_dst) beta_dst[pk] = b;
            }
        }
        if (dosage_here) {
            __syncthreads();   // gam is complete
            // matched_gammas(dh) = sum over k in order of gamma(k) [hapMatcher(k, g) == dh], then * not_jump_prob (:2083-2095):
            // lane l holds the sums of the codes l, l + 64, l + 128, l + 192
            double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
            for (int k0 = 0; k0 < K; k0 += 64) {
                const int k = k0 + lane;
                int cv = 0;
                double gv = 0.0;
                if (k < K) {
                    cv = code[k];
                    gv = gam[k];
                }
                static_for<64>([&](auto ic) {
                    constexpr int I = decltype(ic)::value;
                    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane(cv, I);
                    if (c) {   // (wave-uniform; code 0 -- a special, or past K -- is nobody's)
                        const double a = ((c & 63u) == (uint32_t)lane) ? lane_value<I>(gv) : 0.0;
                        switch (c >> 6) {
                            case 0: m0 += a; break;
                            case 1: m1 += a; break;
                            case 2: m2 += a; break;
                            default: m3 += a; break;
                        }
                    }
                });
            }
            const auto put = [&](int code_of, double m) { mt[code_of] = ((code_of >= 1 && code_of < prm.nrow) ? m : 0.0) * not_jump_prob; };
            put(lane, m0);
            put(lane + 64, m1);
            put(lane + 128, m2);
            put(lane + 192, m3);
            __syncthreads();
            const int s = 32 * g, nLocal = min(32, T - s);
            if (lane < nLocal) {
                double d = 0.0;
                const int so = prm.sp_off[g], sn = prm.sp_off[g + 1] - so;
                for (int i = 0; i < sn; i++) {   // (:2096-2128)
                    const double gk = gam[prm.sp_k[so + i]] * not_jump_prob;
                    const uint32_t w = prm.sp_word[so + i];
                    d += ((w >> lane) & 1u) ? gk * ome : gk * eps;
                }
                const int32_t *Bg = prm.B + (size_t)g * prm.nMaxDH;
                const double *IEs = prm.IE ? prm.IE + (size_t)(s + lane) * prm.nMaxDH : nullptr;
                for (int dh = 0; dh < prm.nMaxDH; dh++) {   // (:2129-2139)
                    const double ie = IEs ? IEs[dh] : ((((uint32_t)Bg[dh] >> lane) & 1u) ? ome : eps);
                    d += ie * mt[dh + 1];
                }
                prm.dosage[(size_t)p * T + s + lane] = d;
            }
            __syncthreads();   // before the next grid writes gam / mt
        }
    }
}

}  // namespace

namespace qa {

void launch_fb_ord(const void *pass_params, int NT, hipStream_t st, hipEvent_t e_mid) {
    const PassParams &prm = *static_cast<const PassParams *>(pass_params);
    if (!prm.spill || prm.spill_pass_stride < 2 * (size_t)prm.Kq)
        throw std::runtime_error("internal: the batched reference-order passes without their state scratch");
    hipLaunchKernelGGL(k_fwd_ord, dim3(prm.P), dim3(kWT), 0, st, prm, NT);
    QA_HIP(hipGetLastError());
    if (e_mid) QA_HIP(hipEventRecord(e_mid, st));
    if (prm.gamma_col) hipLaunchKernelGGL(k_bwd_ord<true>, dim3(prm.P), dim3(kWT), 0, st, prm, NT);
    else hipLaunchKernelGGL(k_bwd_ord<false>, dim3(prm.P), dim3(kWT), 0, st, prm, NT);
    QA_HIP(hipGetLastError());
}

}  // namespace qa
