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

    const InferGraph g = infer_prologue<H, D, kInferMc>(a, lds);
    const InferLds& L = g.L;
    if (g.bad) {                                                       // as the eval kernel: flag, NaN rows, nothing else
        for (int t = t0; t < t1; ++t) infer_refuse(a, g.bad, orow + t * tstride);
        return;
    }
    const int64_t n0 = g.n0;
    const int n = (int)g.n;
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

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_mc_supported(int n_max, int max_e, int H, int D, int O) {
    return infer_supported(kInferMc, n_max, max_e, H, D, O);
}

extern "C" int qot_topological_infer_mc_max_edges(int n_max, int H, int D) { return infer_max_edges(kInferMc, n_max, H, D); }

extern "C" int qot_topological_infer_mc(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                        const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B,
                                        int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm,
                                        const float* P, int V, const float* w_edge, const float* w1, const float* b1,
                                        const float* wcat, const float* bias2, const float* w0, const float* b0,
                                        const float* w3, const float* b3, float slope_conv, float slope_head, float* samples,
                                        int H, int D, int O, int32_t* status, int T, int64_t first_step, uint64_t base_seed,
                                        float p_conv, float p_head, int chunk, qot_stream_t stream_) {
    if (!infer_sizes_ok(N, E, B, n_max, max_e, V) || first_step < 0) return QOT_ERR_BADARG;
    if (!(p_conv >= 0.f && p_conv < 1.f) || !(p_head >= 0.f && p_head < 1.f)) return QOT_ERR_BADARG;
    if (T < 1 || T > 4096 || chunk < 1 || chunk > T) return QOT_ERR_UNSUPPORTED;
    const int chunks = (T + chunk - 1) / chunk;
    if (chunks > 65535) return QOT_ERR_UNSUPPORTED;
    if (!infer_supported(kInferMc, n_max, max_e, H, D, O)) return QOT_ERR_UNSUPPORTED;
    InferArgs a;                                       // (a.out = samples: the kernel writes through mc.samples)
    const int rc = infer_make_args(&a, node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, B, n_max, max_e, t4, ld4, M,
                                   ldm, P, V, w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, samples, H,
                                   O, status);
    if (rc != QOT_OK || B == 0) return rc;
    const uint64_t golden = 0x9E3779B97F4A7C15ull;     // TopologicalGNN._act: site seed = base + golden * site (mod 2^64)
    InferMcArgs mc;
    mc.samples = samples; mc.T = T; mc.chunk = chunk; mc.first_step = (uint64_t)first_step;
    mc.seed_conv1 = base_seed + golden * 1; mc.seed_conv2 = base_seed + golden * 2; mc.seed_head = base_seed + golden * 97;
    dropout_consts(p_conv, &mc.thr_conv, &mc.scale_conv);
    dropout_consts(p_head, &mc.thr_head, &mc.scale_head);
    QOT_INFER_DISPATCH(topological_infer_mc_kernel, H, D, dim3((unsigned)B, (unsigned)chunks),
                       infer_lds_bytes(kInferMc, n_max, max_e, H, D), (hipStream_t)stream_, a, mc)
}
