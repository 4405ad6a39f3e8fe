// LightpathPredictor.from_status: the eval-mode LightpathGNN row of the lightpath under test of every network-status
// sample, straight from data[S, P, L, Q] (fp64) in ONE launch -- no graph in between, nothing read back.
// out[g] / count[g] are, bit for bit, what qot_lightpath_infer's graphs mode gives for the graph the device builder
// (status_graph.hip) makes of sample samples[g]: the sample's lightpaths are status_scan_dev.hpp's discover() table, the
// feature rows its sg_feature(), and the row is infer_lightpath_dev.hpp's lp_row under the policy LpStaged -- the same sums
// in the same order (the interferers one after the other by rising lightpath number, which is the builder's canonical link
// order into the LUT node; the self loop last).
//
// One workgroup (256 threads) per sample:
//   1  discover(): the first-seen table (conn, first channel) in LDS; thread t reads lightpath t's is_lut flag on its first
//      channel.  count[g] = flagged lightpaths; a = the lowest-numbered one (none: NaN row).
//   2  rescan of the conn_id row, 256 channels at a time: a wave takes the channels of `a` its lanes found, one after the
//      other; for such a channel (l, q1) its lanes walk the Q slots of link l, test 0 < |freq[q1] - freq[q2]| < threshold
//      in fp64 (the builder's compare), and for a slot that passes read the channel's conn, look it up in the table and set
//      that lightpath's byte in nb[256] -- plain stores of the same value, so an interferer is one message however many
//      links and slots the pair shares; a's own slots set nothing.  A channel whose conn_id value is 0 is occupied only
//      when another of its P values is not (the occupancy rule); any other value makes it occupied by itself, so only then
//      are the other rows looked at.
//   3  wave 0 alone (the others have ended; a barrier waits on the surviving waves only): the fp32 feature rows of a and of
//      its interferers by rising number -> LDS (at most 256 x 17 words), then lp_row.
// No workspace, no global scratch.  Nothing read from data is used as an index: a conn is only compared, and the channel
// numbers come from the loop counters.  All global writes are ordinary vector stores (the status word: one atomicOr).
//
// On the device: a conn_id that is not finite or beyond +-2^53 (QOT_LP_STATUS_BAD_CONN), more than 256 lightpaths
// (QOT_LP_STATUS_TOO_MANY), a sample number outside [0, S) (QOT_LP_STATUS_BAD_SAMPLE): the sample's row is NaN, its count 0.
// channel_conn, the slot walk and the staging are infer_lightpath_status_dev.hpp's, shared with infer_lightpath_place.hip.
#include "infer_lightpath_status_dev.hpp"

namespace qot {
namespace {

__global__ __launch_bounds__(sg::kThreads) void lightpath_infer_status_kernel(const LpArgs a, const LpStatusArgs st) {
    __shared__ sg::Table T;
    __shared__ double freq[sg::kQCap];
    __shared__ LpLds L;
    __shared__ float rows[sg::kCap * kLpXs];
    __shared__ float xi[kLpMaxF];
    __shared__ uint8_t nb[sg::kCap];
    __shared__ unsigned long long lut_mask[sg::kWaves];
    __shared__ int bad_all;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t g = blockIdx.x;
    float* orow = a.out + g * a.O;
    bool ok;
    const int64_t s = sg::sample_of(st.samples, g, st.S, ok);
    if (!ok) {                                                     // block-uniform
        if (w == 0) {
            if (lane == 0) st.count[g] = 0;
            lp_refuse(a, orow, lane, QOT_LP_STATUS_BAD_SAMPLE);
        }
        return;
    }
    const int LQ = st.L * st.Q;
    const double* d = st.data + s * (int64_t)st.P * LQ;
    for (int q = tid; q < st.Q; q += sg::kThreads) freq[q] = st.freq[q];
    nb[tid] = 0;
    if (tid == 0) bad_all = 0;

    // ---- phase 1: the lightpaths of the sample, their flags ----
    const int bad = sg::discover(d, st.P, LQ, st.conn_row, T, nullptr);      // (begins and ends with a barrier)
    if (bad) atomicOr(&bad_all, bad);
    const int n = T.n;
    const bool flag = tid < n && sg::sg_is_lut(d, LQ, st.osnr_row, st.snr_row, st.ber_row, T.first[tid]);
    const unsigned long long fm = __ballot(flag);
    if (lane == 0) lut_mask[w] = fm;
    __syncthreads();
    if (bad_all) {                                                 // block-uniform
        if (w == 0) {
            if (lane == 0) st.count[g] = 0;
            lp_refuse(a, orow, lane, ((bad_all & QOT_SG_BAD_CONN) ? QOT_LP_STATUS_BAD_CONN : 0) |
                                         ((bad_all & QOT_SG_TOO_MANY) ? QOT_LP_STATUS_TOO_MANY : 0));
        }
        return;
    }
    int cnt = 0, lut = -1;
#pragma unroll
    for (int k = 0; k < sg::kWaves; ++k) {
        const unsigned long long m = lut_mask[k];
        cnt += __popcll(m);
        if (lut < 0 && m) lut = k * 64 + __builtin_ctzll(m);
    }
    if (tid == 0) st.count[g] = cnt;
    if (lut < 0) {                                                 // no lightpath under test: block-uniform
        if (tid < a.O) orow[tid] = __builtin_nanf("");
        return;
    }

    // ---- phase 2: the interferers of lightpath `lut` ----
    const int64_t conn_a = T.conn[lut];
    for (int base = 0; base < LQ; base += sg::kThreads) {
        const int c = base + tid;
        bool mine = false;
        if (c < LQ) {
            int64_t conn;
            mine = channel_conn(d, st.P, LQ, st.conn_row, c, conn) && conn == conn_a;
        }
        unsigned long long mask = __ballot(mine);
        while (mask) {                                             // (wave-uniform: this wave's channels of the lightpath)
            const int c1 = base + w * 64 + __builtin_ctzll(mask);
            mask &= mask - 1;
            const int l = c1 / st.Q, q1 = c1 - l * st.Q;
            lp_mark_slots(d, st, LQ, l, q1, freq, T, n, conn_a, nb, lane);
        }
    }
    __syncthreads();
    if (w != 0) return;

    // ---- phase 3: the rows of the neighbourhood by rising lightpath number, then the row ----
    const int na = lp_stage_marked(d, st, LQ, a.F, T, n, nb, rows, lane);
    if (lane < a.F) xi[lane] = sg::sg_feature(d, st.P, LQ, st.osnr_row, st.snr_row, st.ber_row, st.cols, lane, T.first[lut]);
    __syncthreads();
    LpStaged ed;
    ed.xi = xi;
    ed.rows = rows;
    ed.na = na;
    LpRowRegs R;
    lp_row<false, LpStaged>(a, L, nullptr, 0, 0, orow, lane, R, ed);
}

}  // namespace
}  // namespace qot

using namespace qot;

extern "C" int qot_lightpath_infer_status(const float* x, const int64_t* edge_index, const int64_t* batch,
                                          const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut,
                                          int64_t N, int64_t E, int64_t G, const float* w, const float* att_src,
                                          const float* att_dst, const float* conv_bias, float slope_att,
                                          const float* bn_weight, const float* bn_bias, const float* bn_mean,
                                          const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                                          const float* b3, float slope_head, float* out, int64_t* count, int F, int C, int O,
                                          int heads, int lut_col, int32_t* status, const double* data, const double* freq,
                                          const int64_t* samples, int64_t S, int P, int64_t L, int64_t Q, int conn_row,
                                          int osnr_row, int snr_row, int ber_row, const double* cols, int ncol,
                                          double freq_threshold, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = lp_status_envelope(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, n_lut, N, E, G, F, C, O, heads, lut_col,
                                      S, P, L, Q, conn_row, osnr_row, snr_row, ber_row, ncol, freq_threshold);
    if (rc != QOT_OK) return rc;
    if (G == 0) return QOT_OK;
    const LpArgs a = lp_status_args(G, w, att_src, att_dst, conv_bias, slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps,
                                    w0, b0, w3, b3, slope_head, out, F, C, O, lut_col, status);
    if (!lp_weights_present(a) || !out || !count || !data || !freq || !cols || S == 0) return QOT_ERR_BADARG;
    const LpStatusArgs st{data, freq, samples, S, P, (int)L, (int)Q, conn_row, osnr_row, snr_row, ber_row, cols,
                          freq_threshold, count};
    lightpath_infer_status_kernel<<<(int)G, sg::kThreads, 0, stream>>>(a, st);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
