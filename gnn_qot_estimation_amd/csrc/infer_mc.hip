// Monte-Carlo dropout in one launch: T stochastic forwards of TopologicalGNN per graph, the draws that
// the engine's train mode would take at steps first_step, first_step + 1, ... on the same batch.
//
// Grid (B, ceil(T / chunk)), 256 threads.  A workgroup runs phases 1 - 2 of infer.hip for its graph ONCE, with the same
// code (infer_dev.hpp): index, edge MLP hidden layer, attention, TransformerConv + leaky_relu.  Nothing there depends on
// the draw -- the first dropout sits behind conv1's leaky_relu -- so the undropped x1 stays in LDS.  Per sample of its chunk:
//   a  x1d = dropout(x1) at site 1, a masked copy in LDS (one hash per float4; the operand rows of phase 3 read every x1
//      element (2D + 1) times per incoming edge, so masking at the read would hash that many times more)
//   b  phases 3 - 4 on x1d with dropout at site 2 (behind conv2's leaky_relu, before the pool) and at site 97 (read-out)
// The mask rule is include/qot_gnn.h's: keep = 16 bits of act_hash64(site seed, step, flat / 4) >= thr16, flat numbered
// row-major over the BATCH's [N, H] (conv sites) and [B, H] (read-out); kept values times 1 / (1 - p).  thr16 == 0 takes
// no multiply: with p_conv = p_head = 0 a sample is bit for bit qot_topological_infer's row.
#include "infer_dev.hpp"

namespace qot {

struct InferMcArgs {
    float* samples;                     // [T, B, O]
    int T, chunk;
    uint64_t first_step, seed_conv1, seed_conv2, seed_head;
    uint32_t thr_conv, thr_head;
    float scale_conv, scale_head;
};

template <int H, int D>
__global__ __launch_bounds__(kInferThreads) void topological_infer_mc_kernel(const InferArgs a, const InferMcArgs mc) {
    constexpr int NT = kInferThreads;
    extern __shared__ float4 infer_mc_lds_raw[];
    float* lds = reinterpret_cast<float*>(infer_mc_lds_raw);
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int t0 = (int)blockIdx.y * mc.chunk;                         // (T <= 4096: no overflow)
    const int t1 = t0 + mc.chunk < mc.T ? t0 + mc.chunk : mc.T;
    const int64_t tstride = a.B * a.O;
    float* orow = mc.samples + b * a.O;                                // + t * tstride: sample t's row of this graph

    const int64_t n0 = a.node_ptr[b], e0 = a.edge_ptr[b];
    const int64_t nn = a.node_ptr[b + 1] - n0, mm = a.edge_ptr[b + 1] - e0;
    int bad = infer_slices_ok(a, n0, e0, nn, mm) ? 0 : 2;
    const InferLds L = infer_lds(a.cap_n, a.cap_m, H, D, kInferMc);
    const int n = (int)nn, m = (int)mm;
    if (!bad) bad = infer_phases12<H, D>(a, lds, L, n0, e0, n, m);
    if (bad) {                                                         // as the eval kernel: flag, NaN rows, nothing else
        if (tid == 0 && a.status) atomicOr(a.status, bad);
        if (tid < a.O)
            for (int t = t0; t < t1; ++t) orow[t * tstride + tid] = __builtin_nanf("");
        return;
    }
    const float4* x1 = reinterpret_cast<const float4*>(lds + L.x1);
    float4* x1d = reinterpret_cast<float4*>(lds + L.x1d);
    const uint64_t q0 = ((uint64_t)n0 * H) >> 2;                       // first float4 of the graph's rows in [N, H]
    InferDrop dr;
    dr.seed_conv2 = mc.seed_conv2; dr.seed_head = mc.seed_head;
    dr.thr_conv = mc.thr_conv; dr.thr_head = mc.thr_head;
    dr.scale_conv = mc.scale_conv; dr.scale_head = mc.scale_head;
    dr.row0 = (uint64_t)n0; dr.graph = (uint64_t)b;
    for (int t = t0; t < t1; ++t) {
        dr.step = mc.first_step + (uint64_t)t;
        // (the previous sample's last reads of x1d lie before the barrier that ends its phase 3)
        for (int q = tid; q < n * (H / 4); q += NT) {
            float4 v = x1[q];
            if (mc.thr_conv) {
                const uint64_t z = act_hash64(mc.seed_conv1, dr.step, q0 + (uint64_t)q);
                v.x = ((uint32_t)z & 0xFFFFu) >= mc.thr_conv ? v.x * mc.scale_conv : 0.f;
                v.y = ((uint32_t)(z >> 16) & 0xFFFFu) >= mc.thr_conv ? v.y * mc.scale_conv : 0.f;
                v.z = ((uint32_t)(z >> 32) & 0xFFFFu) >= mc.thr_conv ? v.z * mc.scale_conv : 0.f;
                v.w = ((uint32_t)(z >> 48) & 0xFFFFu) >= mc.thr_conv ? v.w * mc.scale_conv : 0.f;
            }
            x1d[q] = v;
        }
        __syncthreads();
        infer_phases34<H, D, true>(a, lds, L, n, lds + L.x1d, orow + t * tstride, dr);
    }
}

// round(p * 65536) clamped to 65535 and 1 / (1 - p) in fp32, as make_act (common.hpp) states them
static void mc_threshold(float p, uint32_t* thr16, float* scale) {
    *thr16 = 0;
    *scale = 1.0f;
    if (p > 0.f) {
        const uint32_t thr = (uint32_t)(p * 65536.0f + 0.5f);
        *thr16 = thr > 65535u ? 65535u : thr;
        *scale = 1.0f / (1.0f - p);
    }
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_mc_supported(int n_max, int max_e, int H, int D, int O) {
    if (!infer_shape_ok(H, D, O) || n_max < 0 || n_max > kInferMaxN || max_e < 0) return 0;
    if (max_e > (1 << 20)) return 0;                   // (keeps the word count below 2^31)
    return (size_t)infer_lds(n_max, max_e, H, D, kInferMc).words * 4 <= kInferLdsMax ? 1 : 0;
}

extern "C" int qot_topological_infer_mc_max_edges(int n_max, int H, int D) {
    if (!qot_topological_infer_mc_supported(n_max, 0, H, D, 1)) return -1;
    int lo = 0, hi = 1 << 20;                          // the layout grows with max_e: largest accepted value by bisection
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (qot_topological_infer_mc_supported(n_max, mid, H, D, 1)) lo = mid; else hi = mid - 1;
    }
    return lo;
}

extern "C" int qot_topological_infer_mc(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                        const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B,
                                        int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm,
                                        const float* P, int V, const float* w_edge, const float* w1, const float* b1,
                                        const float* wcat, const float* bias2, const float* w0, const float* b0,
                                        const float* w3, const float* b3, float slope_conv, float slope_head, float* samples,
                                        int H, int D, int O, int32_t* status, int T, int64_t first_step, uint64_t base_seed,
                                        float p_conv, float p_head, int chunk, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N < 0 || E < 0 || B < 0 || n_max < 0 || max_e < 0 || V <= 0 || first_step < 0) return QOT_ERR_BADARG;
    if (!(p_conv >= 0.f && p_conv < 1.f) || !(p_head >= 0.f && p_head < 1.f)) return QOT_ERR_BADARG;
    if (T < 1 || T > 4096 || chunk < 1 || chunk > T) return QOT_ERR_UNSUPPORTED;
    const int chunks = (T + chunk - 1) / chunk;
    if (chunks > 65535) return QOT_ERR_UNSUPPORTED;
    if (!qot_topological_infer_mc_supported(n_max, max_e, H, D, O)) return QOT_ERR_UNSUPPORTED;
    if (B == 0) return QOT_OK;
    if (B > 0x7fffffff) return QOT_ERR_UNSUPPORTED;
    const int arc = infer_args_check(node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, t4, ld4, M, ldm, P, V, w_edge,
                                     w1, b1, wcat, bias2, w0, b0, w3, b3, samples, H);
    if (arc != QOT_OK) return arc;
    const InferArgs a{node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, B, n_max, max_e, t4, ld4, M, ldm, P, V,
                      w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, nullptr, O, status};
    const uint64_t golden = 0x9E3779B97F4A7C15ull;     // TopologicalGNN._act: site seed = base + golden * site (mod 2^64)
    InferMcArgs mc;
    mc.samples = samples; mc.T = T; mc.chunk = chunk; mc.first_step = (uint64_t)first_step;
    mc.seed_conv1 = base_seed + golden * 1; mc.seed_conv2 = base_seed + golden * 2; mc.seed_head = base_seed + golden * 97;
    mc_threshold(p_conv, &mc.thr_conv, &mc.scale_conv);
    mc_threshold(p_head, &mc.thr_head, &mc.scale_head);
    const size_t lds = (size_t)infer_lds(n_max, max_e, H, D, kInferMc).words * 4;
    const dim3 grid((unsigned)B, (unsigned)chunks);
#define QOT_INFER_MC_CASE(HH, DD)                                                                                         \
    case HH * 8 + DD: {                                                                                                   \
        static size_t allowed[kMaxDevices];                                                                               \
        const int lrc = ensure_dyn_lds(reinterpret_cast<const void*>(topological_infer_mc_kernel<HH, DD>), lds, allowed); \
        if (lrc != QOT_OK) return lrc;                                                                                    \
        topological_infer_mc_kernel<HH, DD><<<grid, kInferThreads, lds, stream>>>(a, mc);                                 \
    } break;
    switch (H * 8 + D) {
        QOT_INFER_MC_CASE(16, 1) QOT_INFER_MC_CASE(16, 2) QOT_INFER_MC_CASE(16, 3) QOT_INFER_MC_CASE(16, 4)
        QOT_INFER_MC_CASE(32, 1) QOT_INFER_MC_CASE(32, 2) QOT_INFER_MC_CASE(32, 3) QOT_INFER_MC_CASE(32, 4)
        QOT_INFER_MC_CASE(64, 1) QOT_INFER_MC_CASE(64, 2) QOT_INFER_MC_CASE(64, 3) QOT_INFER_MC_CASE(64, 4)
        default: return QOT_ERR_UNSUPPORTED;
    }
#undef QOT_INFER_MC_CASE
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
