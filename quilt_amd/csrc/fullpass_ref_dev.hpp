// fullpass_ref_dev.hpp -- device helpers shared by the two forms of the reference-order full-panel passes: fullpass_ref.hip
// (validation mode: one 256-thread workgroup per pass) and fullpass_ord.hip (the batched form: one wave per pass).  Unnamed
// namespace like fullpass_dev.hpp: each translation unit gets its own copy.
#pragma once

#include "fullpass_dev.hpp"

namespace {

// position of haplotype k in a lane-interleaved column (fullpass_dev.hpp: alpha_vec_index)
__device__ __forceinline__ size_t perm_index(int k, int NT) {
    const int chunk = k >> 4, e = k & 15;
    const int j = chunk / NT, t = chunk % NT;
    return alpha_vec_index<8>(j, e >> 1, NT, t) * 2 + (e & 1);
}

template <int I>
__device__ __forceinline__ double lane_value(double x) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), I);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), I);
    return __hiloint2double(hi, lo);
}
// s <- ((s + x[lane 0]) + x[lane 1]) + ... + x[lane 63]
__device__ __forceinline__ double add_lanes_in_order(double s, double x) {
    static_for<64>([&](auto ic) { s += lane_value<decltype(ic)::value>(x); });
    return s;
}

struct GridEm {
    const double *et;        // the grid's emission table (LDS)
    const double *esp_g;     // the grid's special emissions, list order
    const int32_t *sp_k;     // the grid's special list
    int sn;
    __device__ __forceinline__ double at(int k, uint32_t code) const {
        if (code) return et[code];
        const int i = special_lower_bound(sp_k, 0, sn, k);
        return esp_g[i];
    }
};
__device__ __forceinline__ GridEm grid_em(const PassParams &prm, const double *et, const double *esp_pass, int g) {
    const int so = prm.sp_off[g], sn = prm.sp_off[g + 1] - so;
    return GridEm{et, esp_pass + so + (sn > 0 ? 16 * prm.sp_gidx[g] : 0), prm.sp_k + so, sn};   // (k_emat, lazy layout)
}

}  // namespace
