// LightpathPredictor.what_if: the eval-mode LightpathGNN row of K CANDIDATES in one launch.  Candidate k
// names a node of the batch (lut_idx[k]), may replace that node's feature row (x_lut[k]), removes some edges of the node's
// graph (positions in the batch's edge_index) and appends messages add_src[.] -> node behind the surviving edges.  out[k] is
// qot_lightpath_infer's row of that node in the explicitly built graph, bit for bit: the row is infer_lightpath_dev.hpp's
// lp_row under the edit policy LpWhatIf -- the same walk with another x_i, the dropped slice positions skipped and the added
// sources as further chunks behind the slice, every sum one after the other by rising position, the self loop last.
//
// One wavefront (a workgroup of 64 threads) per candidate, rows mode only.  A candidate rescans its base graph's slice:
// O(m) per candidate; candidates of one node do not share the scan.  Every index taken from the lists is checked before it
// is used as an address: the list slices against A and R here, the drop positions against the graph's slice and the added
// sources against the graph's node range in lp_row.  No atomics beside the status word's; plain fp32 FMA.
#include "infer_lightpath_dev.hpp"

namespace qot {
namespace {

struct LpEditArgs {
    const float* x_lut;                 // [K, F]; null: every candidate keeps its node's row
    const int64_t* add_src;             // [A] batch node numbering
    const int64_t* add_ptr;             // [K + 1]; null: no additions
    int64_t A;
    const int64_t* drop;                // [R] positions in the batch's edge_index
    const int64_t* drop_ptr;            // [K + 1]; null: no removals
    int64_t R;
};

__global__ __launch_bounds__(kWave) void lightpath_infer_whatif_kernel(const LpArgs a, const LpEditArgs ed) {
    __shared__ LpLds L;
    __shared__ int64_t dl[kLpMaxDrop];
    const int lane = threadIdx.x;
    const int64_t k = blockIdx.x;
    float* orow = a.out + k * a.O;
    int64_t i = 0, g = 0;
    if (!lp_locate(a, k, orow, lane, i, g)) return;            // (the candidate's node and its graph: status bit 1)
    // the candidate's slices of the two lists (every value is uniform over the wave)
    const int64_t a0 = ed.add_ptr ? ed.add_ptr[k] : 0, na = ed.add_ptr ? ed.add_ptr[k + 1] - a0 : 0;
    const int64_t d0 = ed.drop_ptr ? ed.drop_ptr[k] : 0, nd = ed.drop_ptr ? ed.drop_ptr[k + 1] - d0 : 0;
    if (a0 < 0 || na < 0 || a0 > ed.A - na || d0 < 0 || nd < 0 || nd > kLpMaxDrop || d0 > ed.R - nd) {
        lp_refuse(a, orow, lane, 2);
        return;
    }
    LpWhatIf w;
    w.xi = ed.x_lut ? ed.x_lut + k * a.F : nullptr;
    w.add = ed.add_src + a0;                                   // (not read when na == 0)
    w.na = na;
    w.drop = ed.drop + d0;                                     // (not read when nd == 0)
    w.nd = (int)nd;
    w.dl = dl;
    w.mp = 0;
    LpRowRegs R;
    lp_row<false, LpWhatIf>(a, L, nullptr, i, g, orow, lane, R, w);
}

}  // namespace
}  // namespace qot

using namespace qot;

extern "C" int qot_lightpath_infer_whatif(const float* x, const int64_t* edge_index, const int64_t* batch,
                                          const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx, int64_t L,
                                          int64_t N, int64_t E, int64_t B, const float* w, const float* att_src,
                                          const float* att_dst, const float* conv_bias, float slope_att,
                                          const float* bn_weight, const float* bn_bias, const float* bn_mean,
                                          const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                                          const float* b3, float slope_head, float* out, int32_t* count, int F, int C, int O,
                                          int heads, int lut_col, int32_t* status, const float* x_lut, const int64_t* add_src,
                                          const int64_t* add_ptr, int64_t A, const int64_t* drop, const int64_t* drop_ptr,
                                          int64_t R, int64_t K, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (A < 0 || R < 0 || K < 0 || L != K) return QOT_ERR_BADARG;
    LpArgs a;
    int64_t rows = 0;
    static const int64_t no_rows = 0;                          // K == 0 is rows mode with no row, whatever lut_idx is
    const int rc = lp_args(x, edge_index, batch, node_ptr, edge_ptr, K == 0 ? &no_rows : lut_idx, L, N, E, B, w, att_src,
                           att_dst, conv_bias,
                           slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, w0, b0, w3, b3, slope_head, out, count, F, C,
                           O, heads, lut_col, status, 1, a, rows);
    if (rc != QOT_OK || K == 0) return rc;
    if (!lut_idx || count) return QOT_ERR_BADARG;              // rows mode only
    if ((A > 0 && (!add_src || !add_ptr)) || (R > 0 && (!drop || !drop_ptr))) return QOT_ERR_BADARG;
    const LpEditArgs ed{x_lut, add_src, add_ptr, A, drop, drop_ptr, R};
    lightpath_infer_whatif_kernel<<<(int)rows, kWave, 0, stream>>>(a, ed);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
