// What the two kernels that take a LightpathGNN row straight from a network-status sample share beyond the sample scan
// (status_scan_dev.hpp) and the row routine (infer_lightpath_dev.hpp): infer_lightpath_status.hip (from_status, DESIGN.md
// 4.20: the row of the lightpath under test that the sample holds) and infer_lightpath_place.hip (place, DESIGN.md 4.22:
// the row of a candidate that the sample does not hold yet).  Stated once here for both: the sample's arguments, who
// occupies a channel (channel_conn), the walk over the slots of one link that marks the interferers of one channel
// (lp_mark_slots) and the staging of the marked lightpaths' feature rows by rising lightpath number (lp_stage_marked) --
// so who interferes, and in which order the messages are summed, is the same code in both.
#pragma once
#include "infer_lightpath_dev.hpp"
#include "status_scan_dev.hpp"

namespace qot {

struct LpStatusArgs {
    const double* data; const double* freq; const int64_t* samples;
    int64_t S;
    int P, L, Q;
    int conn_row, osnr_row, snr_row, ber_row;
    const double* cols;                 // [F, 4]: lp_feat row (-1 = is_lut), min, max - min, has_range
    double thr;
    int64_t* count;
};

// who occupies channel c: the rule is status_scan_dev.hpp's, shared with infer_topological_place.hip; the lightpath
// kernels keep calling it by this name
__device__ __forceinline__ bool channel_conn(const double* __restrict__ d, int P, int LQ, int conn_row, int c, int64_t& conn) {
    return sg::channel_conn(d, P, LQ, conn_row, c, conn);
}

// One wave, one channel (l, q1) of lightpath conn_a: its lanes walk the Q slots of link l, test 0 < |freq[q1] - freq[q2]| <
// threshold in fp64 (the builder's compare), and for a slot that passes read the channel's conn, look it up in the table
// and set that lightpath's byte in nb -- plain stores of the same value, so an interferer is one mark however many links
// and slots the pair shares; conn_a's own slots and empty slots set nothing.  freq: the Q frequencies (LDS).
__device__ __forceinline__ void lp_mark_slots(const double* __restrict__ d, const LpStatusArgs& st, int LQ, int l, int q1,
                                              const double* freq, const sg::Table& T, int n, int64_t conn_a, uint8_t* nb,
                                              int lane) {
    const double f1 = freq[q1];
    for (int q2 = lane; q2 < st.Q; q2 += kWave) {
        const double df = fabs(f1 - freq[q2]);
        if (!(df > 0.0 && df < st.thr)) continue;
        int64_t conn;
        if (!channel_conn(d, st.P, LQ, st.conn_row, l * st.Q + q2, conn) || conn == conn_a) continue;
        for (int i = 0; i < n; ++i)
            if (T.conn[i] == conn) { nb[i] = 1; break; }
    }
}

// One wave: the fp32 feature rows of the marked lightpaths, by rising lightpath number, -> rows [.][kLpXs] (LDS).  Returns
// how many (the same in every lane); visible behind the caller's next barrier.
__device__ __forceinline__ int lp_stage_marked(const double* __restrict__ d, const LpStatusArgs& st, int LQ, int F,
                                               const sg::Table& T, int n, const uint8_t* nb, float* rows, int lane) {
    int na = 0;
    for (int base = 0; base < n; base += kWave) {
        const int j = base + lane;
        const bool is = j < n && nb[j] != 0;
        const unsigned long long m = __ballot(is);
        if (is) {
            float* r = rows + (na + sg::wave_prefix(m)) * kLpXs;
            const int c = T.first[j];
            for (int k = 0; k < F; ++k) r[k] = sg::sg_feature(d, st.P, LQ, st.osnr_row, st.snr_row, st.ber_row, st.cols, k, c);
        }
        na += __popcll(m);
    }
    return na;
}

// What both entry points check of the arguments they share behind `status` (before any launch; G rows are asked for)
inline int lp_status_envelope(const void* x, const void* edge_index, const void* batch, const void* node_ptr,
                              const void* edge_ptr, const void* lut_idx, int64_t n_lut, int64_t N, int64_t E, int64_t G,
                              int F, int C, int O, int heads, int lut_col, int64_t S, int P, int64_t L, int64_t Q, int conn_row,
                              int osnr_row, int snr_row, int ber_row, int ncol, double freq_threshold) {
    // there is no graph: the batch arguments of the common prefix must be empty
    if (x || edge_index || batch || node_ptr || edge_ptr || lut_idx || n_lut != 0 || N != 0 || E != 0) return QOT_ERR_BADARG;
    if (G < 0 || S < 0 || P < 1 || L < 1 || Q < 1) return QOT_ERR_BADARG;
    if (F < 1 || F > kLpMaxF) return QOT_ERR_UNSUPPORTED;
    if (C < 1 || C > kLpMaxC) return QOT_ERR_UNSUPPORTED;
    if (O < 1 || O > kLpMaxO) return QOT_ERR_UNSUPPORTED;
    if (heads != kLpHeads) return QOT_ERR_UNSUPPORTED;
    if (lut_col < 0 || lut_col >= F) return QOT_ERR_UNSUPPORTED;
    if (Q > QOT_SG_MAX_FREQS || L * Q >= (int64_t)1 << 31 || G >= (int64_t)1 << 31) return QOT_ERR_UNSUPPORTED;
    if (ncol != F) return QOT_ERR_BADARG;
    if (conn_row < 0 || conn_row >= P || osnr_row < 0 || osnr_row >= P || snr_row < 0 || snr_row >= P || ber_row < 0 ||
        ber_row >= P)
        return QOT_ERR_BADARG;
    if (!(freq_threshold > 0.0) || !(freq_threshold <= 1.7976931348623157e308)) return QOT_ERR_BADARG;
    return QOT_OK;
}

}  // namespace qot
