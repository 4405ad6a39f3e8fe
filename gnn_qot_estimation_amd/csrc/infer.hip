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
    const InferGraph g = infer_prologue<H, D, kInferEval>(a, lds);
    float* orow = a.out + (int64_t)blockIdx.x * a.O;
    if (g.bad) {                                        // flag, a NaN row, nothing else
        infer_refuse(a, g.bad, orow);
        return;
    }
    // (the layout restated behind the check, not g.L: two SGPRs fewer at D = 3, which is an occupancy step there)
    const InferLds L = infer_lds(a.cap_n, a.cap_m, H, D);
    infer_phases34<H, D, false>(a, lds, L, (int)g.n, lds + L.x1, orow, InferDrop{});
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_supported(int n_max, int max_e, int H, int D, int O) {
    return infer_supported(kInferEval, n_max, max_e, H, D, O);
}

extern "C" int qot_topological_infer_max_edges(int n_max, int H, int D) { return infer_max_edges(kInferEval, n_max, H, D); }

extern "C" int qot_topological_infer(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                     const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B,
                                     int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P,
                                     int V, const float* w_edge, const float* w1, const float* b1, const float* wcat,
                                     const float* bias2, const float* w0, const float* b0, const float* w3, const float* b3,
                                     float slope_conv, float slope_head, float* out, int H, int D, int O, int32_t* status,
                                     qot_stream_t stream_) {
    if (!infer_sizes_ok(N, E, B, n_max, max_e, V)) return QOT_ERR_BADARG;
    if (!infer_supported(kInferEval, n_max, max_e, H, D, O)) return QOT_ERR_UNSUPPORTED;
    InferArgs a;
    const int rc = infer_make_args(&a, node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, B, n_max, max_e, t4, ld4, M,
                                   ldm, P, V, w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, out, H, O,
                                   status);
    if (rc != QOT_OK || B == 0) return rc;
    QOT_INFER_DISPATCH(topological_infer_kernel, H, D, dim3((unsigned)B), infer_lds_bytes(kInferEval, n_max, max_e, H, D),
                       (hipStream_t)stream_, a)
}
