// LightpathPredictor.place(release=...): the eval-mode LightpathGNN row of K CANDIDATE lightpaths, each placed into a
// network-status sample data[S, P, L, Q] (fp64) from which some established lightpaths are RELEASED first, in ONE launch --
// a reroute, or an admission together with a tear-down; no edited sample, no graph, nothing read back.
// Candidate k is infer_lightpath_place.hip's (values[k, P] into cells[:, cell_ptr[k] : cell_ptr[k + 1]] of sample
// samples[k]) plus the conns release[release_ptr[k] : release_ptr[k + 1]]: the lightpaths of its sample with one of those
// trunc(conn_id) values are gone before it is placed.  out[k] is, bit for bit, the row qot_lightpath_infer gives the
// candidate's node in the graph the device builder makes of that edited sample, count[k] the flagged survivors plus one.
// The kernel never builds the edited sample.  Releasing zeroes whole channels and the candidate fills channels that are
// free afterwards, so a survivor keeps every channel it had: its first channel, hence its features, and its place among
// the survivors in first-seen order.  The candidate's interferers are therefore the marks of infer_lightpath_place.hip's
// walk on the UNEDITED sample with the gone lightpaths' marks cleared, staged by rising first-seen number of the unedited
// table -- the survivors' relative order -- with the self loop last.
//
// One workgroup (256 threads) per candidate.  Phases 0 to 2 are infer_lightpath_status_dev.hpp's lp_place_scan<true>, the
// scan of infer_lightpath_place.hip with the release interleaved; the release rule itself (the slice, who is gone, when an
// occupied cell is legal) does not depend on the model and is status_scan_dev.hpp's sg::release_* over sg::Release:
//   0  the release slice, checked against [0, R] and the cap of 32 before `release` is read, -> LDS.
//   1  discover() on the unedited sample; thread t compares lightpath t's conn with the slice (gone[t]; every slice entry
//      that meets a lightpath is ticked), and -- a survivor only -- reads its is_lut flag and compares its conn with the
//      candidate's.  A slice entry nobody ticked refuses the candidate.
//   2  wave w takes the cells lo + w, lo + w + 4, ...: range check; an occupied channel is legal when its owner is gone (one
//      table lookup, the wave's lanes share the table); then lp_mark_slots as it is.
//   3  wave 0 alone: clears the marks of the gone, then lp_stage_marked, x_i from values[k], lp_row.
// Cost: infer_lightpath_place.hip's plus O(32) compares per thread and one table lookup per occupied cell.  No workspace,
// no global scratch.  Nothing read from data, values or release is used as an index: conns are only compared; the cell
// indices come from `cells` and are range-checked first.  All global writes are ordinary vector stores (the status word:
// one atomicOr).
//
// On the device (the candidate's row is NaN, its count 0, the other rows are untouched): everything
// infer_lightpath_place.hip refuses, with these differences -- an occupied cell is refused only when its owner survives,
// QOT_LP_PLACE_CONN_TAKEN is tested against the survivors, QOT_LP_STATUS_TOO_MANY means survivors + 1 > 256 or more than
// 256 lightpaths in the unedited sample (the table cannot hold them) -- and: a released conn the sample does not hold
// (QOT_LP_PLACE_NO_SUCH_CONN); a release_ptr slice that is descending, beyond R or longer than 32
// (QOT_LP_PLACE_BAD_RELEASE).
#include "infer_lightpath_status_dev.hpp"

namespace qot {
namespace {

__global__ __launch_bounds__(sg::kThreads) void lightpath_infer_place_release_kernel(const LpArgs a, const LpStatusArgs st,
                                                                                     const sg::PlaceArgs pl,
                                                                                     const sg::ReleaseArgs rl) {
    __shared__ sg::Table T;
    __shared__ double freq[sg::kQCap];
    __shared__ LpLds L;
    __shared__ float rows[sg::kCap * kLpXs];
    __shared__ float xi[kLpMaxF];
    __shared__ uint8_t nb[sg::kCap];
    __shared__ sg::Release rs;
    __shared__ unsigned long long lut_mask[sg::kWaves];
    __shared__ int bad_all;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t k = blockIdx.x;
    float* orow = a.out + k * a.O;

    // ---- phases 0 to 2 (infer_lightpath_status_dev.hpp's scan in its release form) ----
    LpPlaceScan r;
    const int bad = lp_place_scan<true>(st, pl, rl, k, T, freq, nb, lut_mask, &bad_all, &rs, r);     // (block-uniform)
    if (w != 0) return;
    if (bad) {
        if (lane == 0) st.count[k] = 0;
        lp_refuse(a, orow, lane, bad);
        return;
    }
    const double* d = r.d;
    const double* v = r.v;
    const int LQ = r.LQ, n = r.n;
    if (lane == 0) st.count[k] = r.cnt;

    // ---- phase 3: the gone send no message; the survivors' rows by rising lightpath number, then the row ----
    for (int j = lane; j < n; j += kWave)                          // (lp_stage_marked's lane j reads the bytes lane j wrote)
        if (rs.gone[j]) nb[j] = 0;
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

extern "C" int qot_lightpath_infer_place_release(const float* x, const int64_t* edge_index, const int64_t* batch,
                                                 const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx,
                                                 int64_t n_lut, int64_t N, int64_t E, int64_t K, const float* w,
                                                 const float* att_src, const float* att_dst, const float* conv_bias,
                                                 float slope_att, const float* bn_weight, const float* bn_bias,
                                                 const float* bn_mean, const float* bn_var, float bn_eps, const float* w0,
                                                 const float* b0, const float* w3, const float* b3, float slope_head, float* out,
                                                 int64_t* count, int F, int C, int O, int heads, int lut_col, int32_t* status,
                                                 const double* data, const double* freq, const int64_t* samples, int64_t S,
                                                 int P, int64_t L, int64_t Q, int conn_row, int osnr_row, int snr_row,
                                                 int ber_row, const double* cols, int ncol, double freq_threshold,
                                                 const double* values, const int64_t* cells, const int64_t* cell_ptr, int64_t M,
                                                 const int64_t* release, const int64_t* release_ptr, int64_t R,
                                                 qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = lp_status_envelope(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, n_lut, N, E, K, F, C, O, heads, lut_col,
                                      S, P, L, Q, conn_row, osnr_row, snr_row, ber_row, ncol, freq_threshold);
    if (rc != QOT_OK) return rc;
    if (M < 0 || R < 0) return QOT_ERR_BADARG;
    if (K == 0) return QOT_OK;
    const LpArgs a = lp_status_args(K, w, att_src, att_dst, conv_bias, slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps,
                                    w0, b0, w3, b3, slope_head, out, F, C, O, lut_col, status);
    if (!lp_weights_present(a) || !out || !count || !data || !freq || !cols || S == 0 || !samples || !values || !cell_ptr ||
        (M > 0 && !cells) || !release_ptr || (R > 0 && !release))
        return QOT_ERR_BADARG;
    const LpStatusArgs st{data, freq, samples, S, P, (int)L, (int)Q, conn_row, osnr_row, snr_row, ber_row, cols,
                          freq_threshold, count};
    const sg::PlaceArgs pl{values, cells, cell_ptr, M};
    const sg::ReleaseArgs rl{release, release_ptr, R};
    lightpath_infer_place_release_kernel<<<(int)K, sg::kThreads, 0, stream>>>(a, st, pl, rl);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
