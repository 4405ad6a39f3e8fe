// LightpathPredictor.reroute_impact: place_impact with established lightpaths RELEASED in the same launch -- who a
// reroute, or an admission together with a tear-down, helps and whom it hurts.  Candidate k is
// infer_lightpath_place_release.hip's: values[k, P] into cells[:, cell_ptr[k] : cell_ptr[k + 1]] of sample samples[k], from
// which the lightpaths with one of the conns release[release_ptr[k] : release_ptr[k + 1]] are gone first; out[k] and
// count[k] are that kernel's, bit for bit.  Two sets of SURVIVORS change their neighbourhood: those the candidate
// interferes with gain a source (nb[] behind phase 2, the marks of the gone cleared), those a gone lightpath interfered
// with lose one.  Their union, by rising first-seen number, is the affected: the first A = max_affected get a slot i --
// affected[k, i] the conn, before[k, i] the lightpath's eval-mode row as the lightpath under test of the UNEDITED sample
// (the gone still send their messages: place_impact's before), after[k, i] the same row in the sample with the release
// applied and the candidate established (osnr = snr = ber = 0, is_lut 0), gains[k, i] whether the candidate is a source of
// after, lost[k, i] how many gone lightpaths were sources of before.  Bit for bit these are the rows qot_lightpath_infer
// gives the lightpath's node in the graphs of infer.materialise_retest's samples (release= for after).  No sample is
// built: releasing zeroes whole channels and the candidate fills channels that are free afterwards, so a survivor keeps
// its channels, its first channel and its place among the survivors; the sources of after are the surviving marks of the
// walk on the unedited sample by rising number, the candidate's row behind the lightpaths whose first channel lies below
// the smallest of its cells.  The interference rule is symmetric: the survivors a gone lightpath's walk marks are the
// lightpaths that had it as a source.
//
// One workgroup (256 threads) per candidate; kRelease = false (release_ptr is NULL: nobody is released) skips 0 and 2a:
//   0-2   infer_lightpath_status_dev.hpp's lp_place_scan<kRelease> with an sg::Release in LDS, as
//         infer_lightpath_place_release.hip; then the marks of the gone are cleared in nb[].
//   2a    all four waves: the gone lightpaths (at most 32) by rising number -> the slots; lp_mark_slotted marks their
//         neighbourhoods into the 32 x 256 B maps; thread t, a survivor, sums its column over the gone slots -> lost_lp[t];
//         the maps are zeroed again.  (The maps are used twice: a second array would not fit the 64 KB of static LDS.)
//   2b    marked = survivor && (nb[t] || lost_lp[t]), ranked by rising number into the slots; lp_mark_slotted for the
//         slots, as infer_lightpath_place_impact.hip.
//   3     wave 0 alone, the others have ended (lp_row's barriers: see infer_lightpath_place_impact.hip).  For each slot:
//         all marks -> LDS (lp_stage_marked), j's own row with is_lut forced to 1, lp_row -> before; the marks of the gone
//         are cleared from the slot's map and the survivors are staged AGAIN from row 0 -- a gone source below the
//         candidate's position moves every row behind it, so place_impact's "the rows below pos stay" does not hold -- in
//         two calls, the marks below `pos` (lp_stage_marked over the first pos lightpaths: `below` rows) and, those marks
//         cleared, the rest one row further where nb[j] is set: the candidate's row goes into the gap; lp_row -> after.
//         Then the candidate's own row exactly as infer_lightpath_place_release.hip's phase 3, and the padding.
// Cost: infer_lightpath_place_impact.hip's plus one more rescan of the conn_id row (2a), O(32) adds per thread and the
// restaged rows.  No workspace, no global scratch.  Nothing read from data, values or release is used as an index: conns
// are only compared; the cell indices come from `cells` and are range-checked first.  All global writes are ordinary
// vector stores (the status word: one atomicOr).
//
// On the device: everything infer_lightpath_place_release.hip refuses, with the same status bits and no new one -- the
// candidate's out row is NaN, its count and n_affected 0, its affected and lost -1, its gains 0, its before and after
// NaN; the other candidates are untouched.
#include "infer_lightpath_status_dev.hpp"

namespace qot {
namespace {

constexpr int kLpMaxAffected = QOT_PLACE_MAX_AFFECTED;   // 32
static_assert(sg::kMaxRelease <= kLpMaxAffected, "the gone lightpaths borrow the slots and their maps in phase 2a");

struct LpRerouteArgs {
    int64_t* affected;                  // [K, A] conn ids, -1 padded
    int64_t* n_affected;                // [K] the true number
    float* before;                      // [K, A, O]
    float* after;                       // [K, A, O]
    uint8_t* gains;                     // [K, A] the candidate is a source of after; 0 padded
    int64_t* lost;                      // [K, A] gone sources of before; -1 padded
    int A;                              // 1 .. kLpMaxAffected
};

// slots [from, A) of candidate k: no lightpath
__device__ __forceinline__ void lp_reroute_pad(const LpArgs& a, const LpRerouteArgs& im, int64_t k, int from, int lane) {
    for (int i = from + lane; i < im.A; i += kWave) {
        im.affected[k * im.A + i] = -1;
        im.lost[k * im.A + i] = -1;
        im.gains[k * im.A + i] = 0;
    }
    const int64_t base = k * im.A * a.O;
    for (int t = from * a.O + lane; t < im.A * a.O; t += kWave) {
        im.before[base + t] = __builtin_nanf("");
        im.after[base + t] = __builtin_nanf("");
    }
}

template <bool kRelease>
__global__ __launch_bounds__(sg::kThreads) void lightpath_infer_reroute_impact_kernel(const LpArgs a, const LpStatusArgs st,
                                                                                      const sg::PlaceArgs pl,
                                                                                      const sg::ReleaseArgs rl,
                                                                                      const LpRerouteArgs im) {
    __shared__ sg::Table T;
    __shared__ double freq[sg::kQCap];
    __shared__ LpLds L;
    __shared__ float rows[sg::kCap * kLpXs];
    __shared__ float xi[kLpMaxF];
    __shared__ float xc[kLpMaxF];                                  // the candidate's row as an established neighbour
    __shared__ uint8_t nb[sg::kCap];
    __shared__ uint8_t lost_lp[sg::kCap];                          // lightpath t: the gone lightpaths among its sources
    __shared__ uint32_t nbs[kLpMaxAffected * sg::kCap / 4];        // byte maps [32][256]: the gone's (2a), then the slots'
    __shared__ int16_t slot_lp[kLpMaxAffected];                    // slot -> lightpath number
    __shared__ sg::Release rs;
    __shared__ unsigned long long lut_mask[sg::kWaves];
    __shared__ int wave_marked[sg::kWaves];
    __shared__ int bad_all, cmin;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t k = blockIdx.x;
    float* orow = a.out + k * a.O;
    const int A = im.A;
    uint8_t* maps = reinterpret_cast<uint8_t*>(nbs);
    for (int t = tid; t < kLpMaxAffected * (sg::kCap / 4); t += sg::kThreads) nbs[t] = 0;
    lost_lp[tid] = 0;
    if (tid == 0) cmin = 0x7fffffff;

    // ---- phases 0 to 2 (infer_lightpath_status_dev.hpp's scan, in its release form when a release is given) ----
    LpPlaceScan r;
    const int bad = lp_place_scan<kRelease>(st, pl, rl, k, T, freq, nb, lut_mask, &bad_all, kRelease ? &rs : nullptr, r);   // (block-uniform)
    if (bad) {
        if (w == 0) {
            if (lane == 0) {
                st.count[k] = 0;
                im.n_affected[k] = 0;
            }
            lp_refuse(a, orow, lane, bad);
            lp_reroute_pad(a, im, k, 0, lane);
        }
        return;
    }
    const double* d = r.d;
    const double* v = r.v;
    const int LQ = r.LQ, n = r.n;
    bool gone = false;                                             // lightpath tid is released

    // ---- phase 2a: the gone send no message; who loses them as a source ----
    if constexpr (kRelease) {
        gone = tid < n && rs.gone[tid] != 0;
        if (gone) nb[tid] = 0;
        int grank = sg::wave_prefix(rs.gone_mask[w]), ng = 0;      // (gone_mask: lp_place_scan's, behind its barriers)
#pragma unroll
        for (int j = 0; j < sg::kWaves; ++j) {
            const int p = __popcll(rs.gone_mask[j]);
            if (j < w) grank += p;
            ng += p;
        }
        if (ng) {                                                  // (block-uniform; ng <= 32: a slice entry names one lightpath)
            if (gone && grank < kLpMaxAffected) slot_lp[grank] = (int16_t)tid;
            ng = ng < kLpMaxAffected ? ng : kLpMaxAffected;
            __syncthreads();
            lp_mark_slotted(d, st, LQ, freq, T, n, slot_lp, ng, maps);
            __syncthreads();
            if (tid < n && !gone) {
                int lost = 0;
                for (int g = 0; g < ng; ++g) lost += maps[g * sg::kCap + tid];
                lost_lp[tid] = (uint8_t)lost;
            }
            __syncthreads();                                       // (every column is summed before the maps are zeroed)
            for (int t = tid; t < ng * (sg::kCap / 4); t += sg::kThreads) nbs[t] = 0;
        }
    }

    // ---- phase 2b: the affected by rising number; the smallest of the candidate's cells; the slotted lightpaths' maps ----
    const bool marked = tid < n && !gone && (nb[tid] != 0 || lost_lp[tid] != 0);
    const unsigned long long mm = __ballot(marked);
    if (lane == 0) wave_marked[w] = __popcll(mm);
    int c0 = 0x7fffffff;
    for (int64_t c = r.lo + tid; c < r.hi; c += sg::kThreads) {    // (every cell has passed phase 2's range check)
        const int cc = (int)pl.cells[c] * st.Q + (int)pl.cells[pl.M + c];
        c0 = cc < c0 ? cc : c0;
    }
    if (c0 != 0x7fffffff) atomicMin(&cmin, c0);
    __syncthreads();                                               // (2a's slot_lp and maps are done with; nb, lost_lp complete)
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
        const int gain = nb[j] != 0 ? 1 : 0;                       // the candidate is a source of j
        // before: j's own interferers in the unedited sample, the gone among them
        const int na = lp_stage_marked(d, st, LQ, a.F, T, n, nbj, rows, lane);
        if (lane < a.F) {
            const bool lut = (int)st.cols[4 * lane] < 0;
            xi[lane] = lut ? 1.0f : sg::sg_feature(d, st.P, LQ, st.osnr_row, st.snr_row, st.ber_row, st.cols, lane, T.first[j]);
        }
        if (lane == 0) {
            im.affected[k * A + i] = T.conn[j];
            im.gains[k * A + i] = (uint8_t)gain;
            im.lost[k * A + i] = lost_lp[j];
        }
        __syncthreads();
        LpStaged ed;
        ed.xi = xi;
        ed.rows = rows;
        ed.na = na;
        lp_row<false, LpStaged>(a, L, nullptr, 0, 0, im.before + at, lane, R, ed);
        // after: the surviving sources staged again from row 0, the candidate's row at its first-seen position among them
        if constexpr (kRelease)
            for (int t = lane; t < n; t += kWave)                  // (lp_stage_marked's lane j reads the bytes lane j wrote)
                if (rs.gone[t]) nbj[t] = 0;
        const int below = lp_stage_marked(d, st, LQ, a.F, T, pos, nbj, rows, lane);     // (the marks below pos alone)
        for (int t = lane; t < pos; t += kWave) nbj[t] = 0;
        const int behind = lp_stage_marked(d, st, LQ, a.F, T, n, nbj, rows + (below + gain) * kLpXs, lane);
        if (gain && lane < a.F) rows[below * kLpXs + lane] = xc[lane];
        __syncthreads();
        ed.na = below + gain + behind;
        lp_row<false, LpStaged>(a, L, nullptr, 0, 0, im.after + at, lane, R, ed);
    }
    lp_reroute_pad(a, im, k, ns, lane);

    // the candidate's own row, as infer_lightpath_place_release.hip's phase 3 (the marks of the gone are cleared already)
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

extern "C" int qot_lightpath_infer_reroute_impact(const float* x, const int64_t* edge_index, const int64_t* batch,
                                                  const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx,
                                                  int64_t n_lut, int64_t N, int64_t E, int64_t K, const float* w,
                                                  const float* att_src, const float* att_dst, const float* conv_bias,
                                                  float slope_att, const float* bn_weight, const float* bn_bias,
                                                  const float* bn_mean, const float* bn_var, float bn_eps, const float* w0,
                                                  const float* b0, const float* w3, const float* b3, float slope_head,
                                                  float* out, int64_t* count, int F, int C, int O, int heads, int lut_col,
                                                  int32_t* status, const double* data, const double* freq,
                                                  const int64_t* samples, int64_t S, int P, int64_t L, int64_t Q, int conn_row,
                                                  int osnr_row, int snr_row, int ber_row, const double* cols, int ncol,
                                                  double freq_threshold, const double* values, const int64_t* cells,
                                                  const int64_t* cell_ptr, int64_t M, const int64_t* release,
                                                  const int64_t* release_ptr, int64_t R, int64_t* affected, int64_t* n_affected,
                                                  float* before, float* after, uint8_t* gains, int64_t* lost, int max_affected,
                                                  qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = lp_status_envelope(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, n_lut, N, E, K, F, C, O, heads, lut_col,
                                      S, P, L, Q, conn_row, osnr_row, snr_row, ber_row, ncol, freq_threshold);
    if (rc != QOT_OK) return rc;
    if (M < 0 || R < 0 || max_affected < 1 || max_affected > kLpMaxAffected) return QOT_ERR_BADARG;
    if (K == 0) return QOT_OK;
    const LpArgs a = lp_status_args(K, w, att_src, att_dst, conv_bias, slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps,
                                    w0, b0, w3, b3, slope_head, out, F, C, O, lut_col, status);
    if (!lp_weights_present(a) || !out || !count || !data || !freq || !cols || S == 0 || !samples || !values || !cell_ptr ||
        (M > 0 && !cells) || (R > 0 && (!release || !release_ptr)) || !affected || !n_affected || !before || !after || !gains ||
        !lost)
        return QOT_ERR_BADARG;
    const LpStatusArgs st{data, freq, samples, S, P, (int)L, (int)Q, conn_row, osnr_row, snr_row, ber_row, cols,
                          freq_threshold, count};
    const sg::PlaceArgs pl{values, cells, cell_ptr, M};
    const sg::ReleaseArgs rl{release, release_ptr, R};
    const LpRerouteArgs im{affected, n_affected, before, after, gains, lost, max_affected};
    if (release_ptr)
        lightpath_infer_reroute_impact_kernel<true><<<(int)K, sg::kThreads, 0, stream>>>(a, st, pl, rl, im);
    else                                                           // nobody is released: no slice to read
        lightpath_infer_reroute_impact_kernel<false><<<(int)K, sg::kThreads, 0, stream>>>(a, st, pl, rl, im);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
