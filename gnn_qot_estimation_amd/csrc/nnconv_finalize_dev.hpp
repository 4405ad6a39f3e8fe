// Second-stage sums of the H = 64 NNConv backward as a device body (used by roles.hip).
#pragma once
#include "common.hpp"

namespace qot {

constexpr int kAdjBlocksPerCu = 1;      // workgroups per CU of nnconv_adjoint_dw64 (= slabs per CU)

// The grad-h half of the second-stage sums: one wave per output sums the per-workgroup partials of nnconv_gradh64_kernel.
// (256-thread virtual block vb of ceil(hn / 4).)
__device__ __forceinline__ void nnconv_gradh_sum64_body(const float* __restrict__ hpart, int hblk, int hn, int KD,
                                                        float* __restrict__ gw1, float* __restrict__ gb1, int vb) {
    const int t = vb * 4 + (threadIdx.x >> 6);
    if (t >= hn) return;
    const float s = wave_sum_partials(hpart, hblk, hn, t);
    if ((threadIdx.x & 63) == 0) { if (t < KD) gw1[t] = s; else gb1[t - KD] = s; }
}

// The slab half: the per-workgroup weight-gradient slabs of nnconv_adjoint_dw64 (16 lanes per float4 stride over the slabs,
// fixed butterfly), written in the parameters' own layouts.  It reads what the adjoint wrote and nothing of grad-h, so the
// grad-h launch itself may carry it (kHostedSlabSum64 below).  (256-thread virtual block vb of nb1 = ceil(elems / 4 * 16 / 256).)
__device__ __forceinline__ void nnconv_slab_sum64_body(const float* __restrict__ slabs, int nslabs, int64_t elems,
                                                       float* __restrict__ dst, int K, int vb) {
    const int64_t gt = vb * (int64_t)256 + threadIdx.x;
    const int64_t t = gt >> 4;             // float4 index
    const int sub = (int)(gt & 15);
    const bool live = t * 4 < elems;
    float4 acc = f4zero();
    if (live) {
        // eight slabs requested before the first is added (one load -> wait -> add per trip was 16 dependent round trips)
        int sidx = sub;
        for (; sidx + 7 * 16 < nslabs; sidx += 8 * 16) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ld4(slabs + (int64_t)(sidx + 16 * u) * elems + 4 * t);
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = add4(acc, v[u]);
        }
        for (; sidx < nslabs; sidx += 16) acc = add4(acc, ld4(slabs + (int64_t)sidx * elems + 4 * t));
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        acc.x += __shfl_xor(acc.x, o); acc.y += __shfl_xor(acc.y, o);
        acc.z += __shfl_xor(acc.z, o); acc.w += __shfl_xor(acc.w, o);
    }
    if (!live || sub) return;
    const int64_t e = 4 * t;
    const int a0 = (int)(e & 63), o_ = (int)((e >> 6) & 63), kb = (int)(e >> 12);
    const float v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int a = a0 + c;
        int64_t idx;
        if (kb < K) idx = ((int64_t)a * 64 + o_) * K + kb;
        else if (kb == K) idx = (int64_t)4096 * K + a * 64 + o_;
        else idx = (int64_t)4096 * (K + 1) + o_ * 64 + a;
        dst[idx] = v[c];
    }
}

// One launch for both second-stage sums of the NNConv backward (H = 64): blocks [0, nb1) run the slab half, the remaining
// blocks the grad-h half.  Separately these were three dependent launches of ~5 us each behind kernels that had long finished.
// (256-thread virtual block vb of nb1 + ceil(hn / 4).)
__device__ __forceinline__ void nnconv_bwd_finalize64_body(const float* __restrict__ slabs, int nslabs, int64_t elems,
                                                           float* __restrict__ dst, int K, int nb1,
                                                           const float* __restrict__ hpart, int hblk, int hn, int KD,
                                                           float* __restrict__ gw1, float* __restrict__ gb1, int vb) {
    if (vb >= nb1) nnconv_gradh_sum64_body(hpart, hblk, hn, KD, gw1, gb1, vb - nb1);
    else nnconv_slab_sum64_body(slabs, nslabs, elems, dst, K, vb);
}

// Jobs hosted by the tail workgroups of nnconv_gradh64_kernel (nnconv_gradh64.hip): fixed-order sums of partials that EARLIER
// launches wrote, run in the slots the kernel's ragged last round leaves empty.  Passed by value in the kernel arguments and
// read there through a pointer, as RoleTable of roles.hip is; a job is what its body reads and nothing more.
constexpr int kHostedSumRows = 1;       // sum_rows_body: a = nblk, b = n, c = rows per group, flag = float4 columns
constexpr int kHostedSlabSum64 = 2;     // nnconv_slab_sum64_body: a = slabs, b = elems, flag = K
struct HostedJob {
    int32_t kind, flag;
    const float* src;
    float* dst;
    int64_t a, b, c;
};
struct HostedTable {
    int n;
    int first[QOT_MAX_ROLES + 1];       // tail workgroup range of job r: [first[r], first[r + 1]), counted from n_main
    HostedJob job[QOT_MAX_ROLES];
};

}  // namespace qot
