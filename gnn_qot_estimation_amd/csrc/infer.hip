// Single-launch inference: the whole eval-mode TopologicalGNN forward (topological_training/models.py:49-64, dropout off)
// of a block-diagonal batch, ONE workgroup of 256 threads per graph.
//
// Everything a graph needs is small (n <= 128 nodes, a few hundred edges): its destination-sorted index, its edge features,
// the edge MLP's hidden layer and the first convolution's output all live in LDS; what depends on the parameters only --
// the projected table [q|k|v|skip], the score matrix M / P of the graph form (tconv_graph_dev.hpp) and the NNConv operand
// Wcat -- is read from global memory, where it is shared by every graph of the launch (L2-resident: at H = 64 Wcat is 164 KB
// and would not fit LDS beside the graph).
//
// Phases of a workgroup (a __syncthreads between them):
//   1  index: node ids, edge features -> LDS; in-degree histogram with LDS atomics, block scan, placement, per-row sort by
//      edge id (graph_prep_dev.hpp's pieces; the sort makes the slot order, and so every sum below, independent of the
//      atomics' order); the edge MLP's first layer h_e = relu(w1 ea_e + b1) per edge
//   2  TransformerConv: logit of every slot = M[id_i, id_j] + <P[id_i], ea_e> (slot-parallel: one L2 round trip), softmax
//      per destination (one thread per row, LDS only, PyG's max-subtraction and + 1e-16), then per (row, channel)
//      x1 = leaky_relu(sum alpha v[id_j] + We (sum alpha ea) + skip[id_i])
//   3  NNConv (mean) in tiles of R destination rows: A[r] = [mean_e h_e[k] x1[j] (k < 2D) | mean_e x1[j] | x1[r]] in LDS,
//      then A Wcat with RPT rows per thread (each Wcat element read once per tile and used RPT times from a register), + bias,
//      leaky_relu; the thread adds its rows to its share of the pool sum as they are finished
//   4  mean pool (the row groups' shares summed in a fixed order), Linear -> leaky_relu -> Linear, one row of `out`
// Plain fp32 FMA: per graph the products are ~4 MFLOP at H = 64 and far less at the reference's width, the launch exists
// for the latency of ONE graph or a handful, and fp32 accumulation in a fixed order gives the bitwise batch independence
// the interface promises without the split-bf16 bookkeeping of nnconv_mfma.hip.
// The layout and the phases are device functions in infer_dev.hpp: infer_mc.hip (Monte-Carlo dropout) runs the same code.
#include "infer_dev.hpp"

namespace qot {

template <int H, int D>
__global__ __launch_bounds__(kInferThreads) void topological_infer_kernel(const InferArgs a) {
    extern __shared__ float4 infer_lds_raw[];
    float* lds = reinterpret_cast<float*>(infer_lds_raw);
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    float* orow = a.out + b * a.O;

    const int64_t n0 = a.node_ptr[b], e0 = a.edge_ptr[b];
    const int64_t nn = a.node_ptr[b + 1] - n0, mm = a.edge_ptr[b + 1] - e0;
    // host-side size bound violated, or slices that do not lie inside the arrays: flag, write NaN, touch nothing else
    if (!infer_slices_ok(a, n0, e0, nn, mm)) {
        if (tid == 0 && a.status) atomicOr(a.status, 2);
        if (tid < a.O) orow[tid] = __builtin_nanf("");
        return;
    }
    const int n = (int)nn, m = (int)mm;
    const InferLds L = infer_lds(a.cap_n, a.cap_m, H, D);
    const int bad = infer_phases12<H, D>(a, lds, L, n0, e0, n, m);
    if (bad) {
        if (tid == 0 && a.status) atomicOr(a.status, bad);
        if (tid < a.O) orow[tid] = __builtin_nanf("");
        return;
    }
    infer_phases34<H, D, false>(a, lds, L, n, lds + L.x1, orow, InferDrop{});
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_supported(int n_max, int max_e, int H, int D, int O) {
    if (!infer_shape_ok(H, D, O) || n_max < 0 || n_max > kInferMaxN || max_e < 0) return 0;
    if (max_e > (1 << 20)) return 0;                   // (keeps the word count below 2^31)
    return (size_t)infer_lds(n_max, max_e, H, D).words * 4 <= kInferLdsMax ? 1 : 0;
}

extern "C" int qot_topological_infer_max_edges(int n_max, int H, int D) {
    if (!qot_topological_infer_supported(n_max, 0, H, D, 1)) return -1;
    int lo = 0, hi = 1 << 20;                          // the layout grows with max_e: largest accepted value by bisection
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (qot_topological_infer_supported(n_max, mid, H, D, 1)) lo = mid; else hi = mid - 1;
    }
    return lo;
}

extern "C" int qot_topological_infer(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                     const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B,
                                     int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P,
                                     int V, const float* w_edge, const float* w1, const float* b1, const float* wcat,
                                     const float* bias2, const float* w0, const float* b0, const float* w3, const float* b3,
                                     float slope_conv, float slope_head, float* out, int H, int D, int O, int32_t* status,
                                     qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N < 0 || E < 0 || B < 0 || n_max < 0 || max_e < 0 || V <= 0) return QOT_ERR_BADARG;
    if (!qot_topological_infer_supported(n_max, max_e, H, D, O)) return QOT_ERR_UNSUPPORTED;
    if (B == 0) return QOT_OK;
    if (B > 0x7fffffff) return QOT_ERR_UNSUPPORTED;
    const int arc = infer_args_check(node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, t4, ld4, M, ldm, P, V, w_edge,
                                     w1, b1, wcat, bias2, w0, b0, w3, b3, out, H);
    if (arc != QOT_OK) return arc;
    const InferArgs a{node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, B, n_max, max_e, t4, ld4, M, ldm, P, V,
                      w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, out, O, status};
    const size_t lds = (size_t)infer_lds(n_max, max_e, H, D).words * 4;
#define QOT_INFER_CASE(HH, DD)                                                                                         \
    case HH * 8 + DD: {                                                                                                \
        static size_t allowed[kMaxDevices];                                                                            \
        const int lrc = ensure_dyn_lds(reinterpret_cast<const void*>(topological_infer_kernel<HH, DD>), lds, allowed); \
        if (lrc != QOT_OK) return lrc;                                                                                 \
        topological_infer_kernel<HH, DD><<<(int)B, kInferThreads, lds, stream>>>(a);                                   \
    } break;
    switch (H * 8 + D) {
        QOT_INFER_CASE(16, 1) QOT_INFER_CASE(16, 2) QOT_INFER_CASE(16, 3) QOT_INFER_CASE(16, 4)
        QOT_INFER_CASE(32, 1) QOT_INFER_CASE(32, 2) QOT_INFER_CASE(32, 3) QOT_INFER_CASE(32, 4)
        QOT_INFER_CASE(64, 1) QOT_INFER_CASE(64, 2) QOT_INFER_CASE(64, 3) QOT_INFER_CASE(64, 4)
        default: return QOT_ERR_UNSUPPORTED;
    }
#undef QOT_INFER_CASE
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
