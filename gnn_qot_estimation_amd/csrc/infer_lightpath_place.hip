// LightpathPredictor.place: the eval-mode LightpathGNN row of K CANDIDATE lightpaths, each placed into a network-status
// sample data[S, P, L, Q] (fp64) that does not hold it yet, in ONE launch -- no edited sample, no graph, nothing read back
// (DESIGN.md 4.22).  Candidate k is the raw lp_feat vector values[k, P] written into the channels cells[:, cell_ptr[k] :
// cell_ptr[k + 1]] (link index, frequency index) of sample samples[k].  out[k] is, bit for bit, the row
// qot_lightpath_infer gives the candidate's node in the graph the device builder (status_graph.hip) makes of that edited
// sample, and count[k] the edited sample's flagged lightpaths (the sample's own plus the candidate).  The kernel never
// builds the edited sample: the candidate fills free channels only, so every other lightpath keeps its first channel and
// its place in first-seen order; its interferers are named by the rule of infer_lightpath_status.hip's phase 2 applied to
// the candidate's cells on the unedited sample (a pair of its own cells names nobody: they are free there), and their
// messages are summed by rising first-seen number, the self loop last -- infer_lightpath_status_dev.hpp's walk and staging,
// infer_lightpath_dev.hpp's lp_row under the policy LpStaged.
//
// One workgroup (256 threads) per candidate:
//   1  discover() on the unedited sample; thread t reads lightpath t's is_lut flag on its first channel (count[k] = the
//      flagged ones + 1) and compares its conn with the candidate's truncated conn.
//   2  wave w takes the cells lo + w, lo + w + 4, ...: range check, the channel must be free, then the wave's lanes walk
//      the Q slots of the cell's link and mark nb[] (lp_mark_slots).  A duplicate cell marks the same bytes again.
//   3  wave 0 alone: the interferers' rows by rising number -> LDS (lp_stage_marked), x_i from values[k] through the same
//      column scaling (sg_feature_vec), then lp_row.
// Cost: O(L Q) for discover plus O(cells Q) for the walk, per candidate; candidates of one sample do not share the scan.
// No workspace, no global scratch.  Nothing read from data or values is used as an index: a conn is only compared; the
// cell indices come from `cells` and are range-checked first.  All global writes are ordinary vector stores (the status
// word: one atomicOr).
//
// On the device, since nothing is read back (the candidate's row is NaN, its count 0, the other rows are untouched): a
// sample number outside [0, S) (QOT_LP_STATUS_BAD_SAMPLE); a cell_ptr slice that is empty, descending or beyond M, a link
// or frequency index outside [0, L) / [0, Q) (QOT_LP_PLACE_BAD_CELL); a cell whose channel is occupied
// (QOT_LP_PLACE_OCCUPIED); a candidate conn_id that is not finite or beyond +-2^53, or such a value in the sample
// (QOT_LP_STATUS_BAD_CONN); values[k] without osnr == snr == ber == -1 (QOT_LP_PLACE_NOT_LUT); a conn_id the sample holds
// already (QOT_LP_PLACE_CONN_TAKEN); a sample of 256 or more lightpaths -- the edited one would hold 257
// (QOT_LP_STATUS_TOO_MANY).
#include "infer_lightpath_status_dev.hpp"

namespace qot {
namespace {

__global__ __launch_bounds__(sg::kThreads) void lightpath_infer_place_kernel(const LpArgs a, const LpStatusArgs st,
                                                                             const sg::PlaceArgs pl) {
    __shared__ sg::Table T;
    __shared__ double freq[sg::kQCap];
    __shared__ LpLds L;
    __shared__ float rows[sg::kCap * kLpXs];
    __shared__ float xi[kLpMaxF];
    __shared__ uint8_t nb[sg::kCap];
    __shared__ unsigned long long lut_mask[sg::kWaves];
    __shared__ int bad_all;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t k = blockIdx.x;
    float* orow = a.out + k * a.O;

    // ---- phases 1 and 2 (infer_lightpath_status_dev.hpp, shared with the place_impact and place_release kernels) ----
    LpPlaceScan r;
    const int bad = lp_place_scan<false>(st, pl, sg::ReleaseArgs{}, k, T, freq, nb, lut_mask, &bad_all, nullptr, r);   // (block-uniform)
    if (w != 0) return;
    if (bad) {
        if (lane == 0) st.count[k] = 0;
        lp_refuse(a, orow, lane, bad);
        return;
    }
    const double* d = r.d;
    const double* v = r.v;
    const int LQ = r.LQ, n = r.n, cnt = r.cnt;
    if (lane == 0) st.count[k] = cnt;

    // ---- phase 3: the rows of the neighbourhood by rising lightpath number, then the row ----
    const int na = lp_stage_marked(d, st, LQ, a.F, T, n, nb, rows, lane);
    if (lane < a.F) xi[lane] = sg::sg_feature_vec(v, st.P, st.osnr_row, st.snr_row, st.ber_row, st.cols, lane);
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

extern "C" int qot_lightpath_infer_place(const float* x, const int64_t* edge_index, const int64_t* batch,
                                         const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut,
                                         int64_t N, int64_t E, int64_t K, const float* w, const float* att_src,
                                         const float* att_dst, const float* conv_bias, float slope_att, const float* bn_weight,
                                         const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps,
                                         const float* w0, const float* b0, const float* w3, const float* b3, float slope_head,
                                         float* out, int64_t* count, int F, int C, int O, int heads, int lut_col, int32_t* status,
                                         const double* data, const double* freq, const int64_t* samples, int64_t S, int P,
                                         int64_t L, int64_t Q, int conn_row, int osnr_row, int snr_row, int ber_row,
                                         const double* cols, int ncol, double freq_threshold, const double* values,
                                         const int64_t* cells, const int64_t* cell_ptr, int64_t M, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = lp_status_envelope(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, n_lut, N, E, K, F, C, O, heads, lut_col,
                                      S, P, L, Q, conn_row, osnr_row, snr_row, ber_row, ncol, freq_threshold);
    if (rc != QOT_OK) return rc;
    if (M < 0) return QOT_ERR_BADARG;
    if (K == 0) return QOT_OK;
    const LpArgs a = lp_status_args(K, w, att_src, att_dst, conv_bias, slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps,
                                    w0, b0, w3, b3, slope_head, out, F, C, O, lut_col, status);
    if (!lp_weights_present(a) || !out || !count || !data || !freq || !cols || S == 0 || !samples || !values || !cell_ptr ||
        (M > 0 && !cells))
        return QOT_ERR_BADARG;
    const LpStatusArgs st{data, freq, samples, S, P, (int)L, (int)Q, conn_row, osnr_row, snr_row, ber_row, cols,
                          freq_threshold, count};
    const sg::PlaceArgs pl{values, cells, cell_ptr, M};
    lightpath_infer_place_kernel<<<(int)K, sg::kThreads, 0, stream>>>(a, st, pl);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
