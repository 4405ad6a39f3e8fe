// Single-launch inference for LightpathGNN: the eval-mode forward (lightpath_training/models.py:7-45, dropout off) of the
// LUT rows only, ONE wavefront (a workgroup of 64 threads) per output row.  The row itself -- its steps,
// the order of its sums -- is infer_lightpath_dev.hpp's lp_row, shared with the sensitivity kernel
// (infer_lightpath_grad.hip).
#include "infer_lightpath_dev.hpp"

namespace qot {
namespace {

__global__ __launch_bounds__(kWave) void lightpath_infer_kernel(const LpArgs a) {
    __shared__ LpLds L;
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    float* orow = a.out + r * a.O;
    int64_t i = 0, g = 0;
    if (!lp_locate(a, r, orow, lane, i, g)) return;
    LpRowRegs R;
    lp_row<false>(a, L, nullptr, i, g, orow, lane, R);
}

}  // namespace
}  // namespace qot

using namespace qot;

extern "C" int qot_lightpath_infer(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                                   const int64_t* edge_ptr, const int64_t* lut_idx, int64_t L, int64_t N, int64_t E, int64_t B,
                                   const float* w, const float* att_src, const float* att_dst, const float* conv_bias,
                                   float slope_att, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                                   const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                                   const float* b3, float slope_head, float* out, int32_t* count, int F, int C, int O,
                                   int heads, int lut_col, int32_t* status, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LpArgs a;
    int64_t rows = 0;
    const int rc = lp_args(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, L, N, E, B, w, att_src, att_dst, conv_bias,
                           slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, w0, b0, w3, b3, slope_head, out, count, F, C,
                           O, heads, lut_col, status, 1, a, rows);
    if (rc != QOT_OK || rows == 0) return rc;
    lightpath_infer_kernel<<<(int)rows, kWave, 0, stream>>>(a);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
