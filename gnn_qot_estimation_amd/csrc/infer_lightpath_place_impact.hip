// LightpathPredictor.place_impact: the admission decision's second half.  Beside the row of each of K CANDIDATE lightpaths
// placed into a network-status sample data[S, P, L, Q] (fp64) -- infer_lightpath_place.hip's out[k] and count[k], bit for
// bit -- the ESTABLISHED lightpaths the candidate lands next to are retested, in the same launch: no edited sample, no
// graph, nothing read back.  The candidate's interferers (nb[] behind phase 2) are, by symmetry of the
// interference rule, the only lightpaths whose own neighbourhood the candidate changes.  The first A = max_affected of them
// by rising first-seen number get a slot i: affected[k, i] is the lightpath's conn, before[k, i] its eval-mode row as the
// lightpath under test of the unedited sample, after[k, i] the same row once the candidate is established next to it;
// n_affected[k] is their true number, which may exceed A.  Bit for bit these are the rows qot_lightpath_infer gives the
// lightpath's node in the graph the device builder (status_graph.hip) makes of the sample in which the lightpath's channels
// carry osnr = snr = ber = -1 and -- after -- values[k] with osnr = snr = ber = 0 lies in the candidate's cells
// (infer.materialise_retest).  Neither sample is built: flagging a lightpath changes its is_lut column and nothing else
// (the caller refuses feature lists that hold osnr, snr or ber), and the candidate fills free channels only, so every
// lightpath keeps its first channel and its number; the candidate is first seen behind the `pos` lightpaths whose first
// channel lies below the smallest of its cells.
//
// One workgroup (256 threads) per candidate:
//   1, 2  infer_lightpath_status_dev.hpp's lp_place_scan, as infer_lightpath_place.hip: nb[] holds the interferers.
//   2b    all four waves: the marked lightpaths are ranked by rising number (slot i < A: the i-th); the conn_id row is
//         rescanned 256 channels at a time, as phase 2 of infer_lightpath_status.hip does; for a channel of the lightpath j
//         in slot i the wave that found it runs lp_mark_slots(conn_a = conn_j) into nb_i, that lightpath's own byte map
//         (A x 256 bytes of LDS; plain same-value stores).  The rescan is infer_lightpath_status_dev.hpp's
//         lp_mark_slotted, shared with infer_lightpath_retest.hip.  The walk runs on the unedited sample: the candidate
//         is not seen there, and is a source of every affected lightpath by symmetry.
//   3     wave 0 alone, the others have ended.  For each slot, one after the other: j's sources by rising number -> LDS
//         (lp_stage_marked), j's own row from its first channel with is_lut forced to 1, lp_row -> before[k, i]; then the
//         sources at or behind `pos` are staged again one row further (the marks below `pos` are cleared first; the rows
//         below stay where they are), the candidate's row from values[k] with is_lut forced to 0 goes into the gap, lp_row
//         -> after[k, i].  Then the candidate's own row and count exactly as infer_lightpath_place.hip computes them, and the
//         padding: -1 / NaN in the slots >= min(n_affected, A).
// Phase 3 must stay in ONE wave: lp_row holds __syncthreads() calls whose number depends on the message count, which is
// safe only because the other waves have ended before it runs; two live waves in lp_row on different lightpaths would hang.
// Cost: infer_lightpath_place.hip's plus O(L Q) for the rescan, O(Q) per channel of a slotted lightpath and two rows per
// slot.  No workspace, no global scratch.  Nothing read from data or values is used as an index: a conn is only compared;
// the cell indices come from `cells` and are range-checked first.  All global writes are ordinary vector stores (the status
// word: one atomicOr).
//
// On the device: everything infer_lightpath_place.hip refuses, with the same status bits and no new one -- the candidate's
// out row is NaN, its count and n_affected 0, its affected -1, its before and after NaN; the other candidates are untouched.
#include "infer_lightpath_status_dev.hpp"

namespace qot {
namespace {

constexpr int kLpMaxAffected = QOT_PLACE_MAX_AFFECTED;   // 32

struct LpImpactArgs {
    int64_t* affected;                  // [K, A] conn ids, -1 padded
    int64_t* n_affected;                // [K] the true number
    float* before;                      // [K, A, O]
    float* after;                       // [K, A, O]
    int A;                              // 1 .. kLpMaxAffected
};

// slots [from, A) of candidate k: no lightpath
__device__ __forceinline__ void lp_impact_pad(const LpArgs& a, const LpImpactArgs& im, int64_t k, int from, int lane) {
    for (int i = from + lane; i < im.A; i += kWave) im.affected[k * im.A + i] = -1;
    const int64_t base = k * im.A * a.O;
    for (int t = from * a.O + lane; t < im.A * a.O; t += kWave) {
        im.before[base + t] = __builtin_nanf("");
        im.after[base + t] = __builtin_nanf("");
    }
}

__global__ __launch_bounds__(sg::kThreads) void lightpath_infer_place_impact_kernel(const LpArgs a, const LpStatusArgs st,
                                                                                    const sg::PlaceArgs pl,
                                                                                    const LpImpactArgs im) {
    __shared__ sg::Table T;
    __shared__ double freq[sg::kQCap];
    __shared__ LpLds L;
    __shared__ float rows[sg::kCap * kLpXs];
    __shared__ float xi[kLpMaxF];
    __shared__ float xc[kLpMaxF];                                  // the candidate's row as an established neighbour
    __shared__ uint8_t nb[sg::kCap];
    __shared__ uint32_t nbs[kLpMaxAffected * sg::kCap / 4];        // the slotted lightpaths' byte maps [A][256]
    __shared__ int16_t slot_lp[kLpMaxAffected];                    // slot -> lightpath number
    __shared__ unsigned long long lut_mask[sg::kWaves];
    __shared__ int wave_marked[sg::kWaves];
    __shared__ int bad_all, cmin;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t k = blockIdx.x;
    float* orow = a.out + k * a.O;
    const int A = im.A;
    uint8_t* maps = reinterpret_cast<uint8_t*>(nbs);
    for (int t = tid; t < A * (sg::kCap / 4); t += sg::kThreads) nbs[t] = 0;
    if (tid == 0) cmin = 0x7fffffff;

    // ---- phases 1 and 2 (infer_lightpath_status_dev.hpp, shared with the place and place_release kernels) ----
    LpPlaceScan r;
    const int bad = lp_place_scan<false>(st, pl, sg::ReleaseArgs{}, k, T, freq, nb, lut_mask, &bad_all, nullptr, r);   // (block-uniform)
    if (bad) {
        if (w == 0) {
            if (lane == 0) {
                st.count[k] = 0;
                im.n_affected[k] = 0;
            }
            lp_refuse(a, orow, lane, bad);
            lp_impact_pad(a, im, k, 0, lane);
        }
        return;
    }
    const double* d = r.d;
    const double* v = r.v;
    const int LQ = r.LQ, n = r.n;

    // ---- phase 2b: the marked lightpaths by rising number; the smallest of the candidate's cells; the slotted lightpaths' maps ----
    const bool marked = tid < n && nb[tid] != 0;
    const unsigned long long mm = __ballot(marked);
    if (lane == 0) wave_marked[w] = __popcll(mm);
    int c0 = 0x7fffffff;
    for (int64_t c = r.lo + tid; c < r.hi; c += sg::kThreads) {    // (every cell has passed phase 2's range check)
        const int cc = (int)pl.cells[c] * st.Q + (int)pl.cells[pl.M + c];
        c0 = cc < c0 ? cc : c0;
    }
    if (c0 != 0x7fffffff) atomicMin(&cmin, c0);
    __syncthreads();
    int rank = sg::wave_prefix(mm), total = 0;
#pragma unroll
    for (int j = 0; j < sg::kWaves; ++j) {
        const int p = wave_marked[j];
        if (j < w) rank += p;
        total += p;
    }
    if (marked && rank < A) slot_lp[rank] = (int16_t)tid;
    const int ns = total < A ? total : A;                          // slots in use
    __syncthreads();
    lp_mark_slotted(d, st, LQ, freq, T, n, slot_lp, ns, maps);     // (infer_lightpath_status_dev.hpp; every slot < ns is in use)
    __syncthreads();
    if (w != 0) return;

    // ---- phase 3: the slots one after the other, then the candidate's own row ----
    if (lane == 0) {
        st.count[k] = r.cnt;
        im.n_affected[k] = total;
    }
    int pos = 0;                                                   // the lightpaths first seen before the candidate
    const int first_cell = cmin;
    for (int base = 0; base < n; base += kWave) {
        const int j = base + lane;
        pos += __popcll(__ballot(j < n && T.first[j] < first_cell));
    }
    if (lane < a.F) {
        const bool lut = (int)st.cols[4 * lane] < 0;
        xc[lane] = lut ? 0.0f : sg::sg_feature_vec(v, st.P, st.osnr_row, st.snr_row, st.ber_row, st.cols, lane);
    }
    LpRowRegs R;
    for (int i = 0; i < ns; ++i) {                                 // (wave-uniform)
        const int j = slot_lp[i];
        uint8_t* nbj = maps + i * sg::kCap;
        const int64_t at = (k * A + i) * a.O;
        // before: j's own interferers in the unedited sample
        const int na = lp_stage_marked(d, st, LQ, a.F, T, n, nbj, rows, lane);
        if (lane < a.F) {
            const bool lut = (int)st.cols[4 * lane] < 0;
            xi[lane] = lut ? 1.0f : sg::sg_feature(d, st.P, LQ, st.osnr_row, st.snr_row, st.ber_row, st.cols, lane, T.first[j]);
        }
        if (lane == 0) im.affected[k * A + i] = T.conn[j];
        __syncthreads();
        LpStaged ed;
        ed.xi = xi;
        ed.rows = rows;
        ed.na = na;
        lp_row<false, LpStaged>(a, L, nullptr, 0, 0, im.before + at, lane, R, ed);
        // after: the candidate's row at its first-seen position -- the rows below it stay, the others move one further
        int below = 0;
        for (int base = 0; base < pos; base += kWave) {            // (lp_stage_marked's lane j reads the bytes lane j wrote)
            const int t = base + lane;
            const bool is = t < pos && nbj[t] != 0;
            below += __popcll(__ballot(is));
            if (is) nbj[t] = 0;
        }
        lp_stage_marked(d, st, LQ, a.F, T, n, nbj, rows + (below + 1) * kLpXs, lane);
        if (lane < a.F) rows[below * kLpXs + lane] = xc[lane];
        __syncthreads();
        ed.na = na + 1;
        lp_row<false, LpStaged>(a, L, nullptr, 0, 0, im.after + at, lane, R, ed);
    }
    lp_impact_pad(a, im, k, ns, lane);

    // the candidate's own row, as infer_lightpath_place.hip's phase 3
    const int na = lp_stage_marked(d, st, LQ, a.F, T, n, nb, rows, lane);
    if (lane < a.F) xi[lane] = sg::sg_feature_vec(v, st.P, st.osnr_row, st.snr_row, st.ber_row, st.cols, lane);
    __syncthreads();
    LpStaged ed;
    ed.xi = xi;
    ed.rows = rows;
    ed.na = na;
    lp_row<false, LpStaged>(a, L, nullptr, 0, 0, orow, lane, R, ed);
}

}  // namespace
}  // namespace qot

using namespace qot;

extern "C" int qot_lightpath_infer_place_impact(const float* x, const int64_t* edge_index, const int64_t* batch,
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
                                                int64_t* affected, int64_t* n_affected, float* before, float* after,
                                                int max_affected, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = lp_status_envelope(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, n_lut, N, E, K, F, C, O, heads, lut_col,
                                      S, P, L, Q, conn_row, osnr_row, snr_row, ber_row, ncol, freq_threshold);
    if (rc != QOT_OK) return rc;
    if (M < 0 || max_affected < 1 || max_affected > kLpMaxAffected) return QOT_ERR_BADARG;
    if (K == 0) return QOT_OK;
    const LpArgs a = lp_status_args(K, w, att_src, att_dst, conv_bias, slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps,
                                    w0, b0, w3, b3, slope_head, out, F, C, O, lut_col, status);
    if (!lp_weights_present(a) || !out || !count || !data || !freq || !cols || S == 0 || !samples || !values || !cell_ptr ||
        (M > 0 && !cells) || !affected || !n_affected || !before || !after)
        return QOT_ERR_BADARG;
    const LpStatusArgs st{data, freq, samples, S, P, (int)L, (int)Q, conn_row, osnr_row, snr_row, ber_row, cols,
                          freq_threshold, count};
    const sg::PlaceArgs pl{values, cells, cell_ptr, M};
    const LpImpactArgs im{affected, n_affected, before, after, max_affected};
    lightpath_infer_place_impact_kernel<<<(int)K, sg::kThreads, 0, stream>>>(a, st, pl, im);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
