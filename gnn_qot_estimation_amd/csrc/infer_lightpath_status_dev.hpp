// What the two kernels that take a LightpathGNN row straight from a network-status sample share beyond the sample scan
// (status_scan_dev.hpp) and the row routine (infer_lightpath_dev.hpp): infer_lightpath_status.hip (from_status, DESIGN.md
// 4.20: the row of the lightpath under test that the sample holds) and infer_lightpath_place.hip (place, DESIGN.md 4.22:
// the row of a candidate that the sample does not hold yet).  Stated once here for both: the sample's arguments, who
// occupies a channel (channel_conn), the walk over the slots of one link that marks the interferers of one channel
// (lp_mark_slots) and the staging of the marked lightpaths' feature rows by rising lightpath number (lp_stage_marked) --
// so who interferes, and in which order the messages are summed, is the same code in both.  infer_lightpath_place.hip,
// infer_lightpath_place_impact.hip (place_impact, DESIGN.md 4.25: the candidate's row and the retest of the lightpaths it
// disturbs) and infer_lightpath_place_release.hip (place(release=...)) further share phases 1 and 2 of a
// candidate (lp_place_scan<kRelease>; the candidate's and the release's arguments and the release rule itself are
// status_scan_dev.hpp's, shared with the topological place kernels); infer_lightpath_place_impact.hip and
// infer_lightpath_retest.hip (retest, DESIGN.md 4.26: every established lightpath of a sample as the lightpath under test)
// share the rescan that marks the neighbourhoods of up to 32 slotted lightpaths at once (lp_mark_slotted).
// infer_lightpath_reroute_impact.hip (reroute_impact, DESIGN.md 4.27: place_impact for a candidate that releases
// lightpaths) runs the scan in either form and the rescan twice, for the released lightpaths and for the affected.
// infer_lightpath_place_slots.hip (place_slots, DESIGN.md 4.28: a route swept over every start slot of the grid) takes the
// walk and the staging from here and marks up to 32 start slots' neighbourhoods behind one discover().  The seven
// entries share their envelope, the weight test and the LpArgs of a call without a batch (the host inlines at the end).
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

// The whole workgroup: the neighbourhoods of up to 32 SLOTTED lightpaths of one sample in one rescan of its conn_id row
// (phase 2b of infer_lightpath_place_impact.hip, phase 2 of infer_lightpath_retest.hip).  slot_lp[i], i < ns: the
// lightpath number slot i retests; -1: an empty slot.  256 channels at a time: a channel of the lightpath in slot i (the
// first slot that holds it) raises its lane in a ballot, and the wave that found it runs lp_mark_slots with conn_a = that
// lightpath's conn into maps + i * kCap, the slot's own byte map (zeroed by the caller; plain same-value stores).  The
// caller's barriers stand before (slot_lp, maps, T, freq complete) and behind (the maps complete) the call.
__device__ __forceinline__ void lp_mark_slotted(const double* __restrict__ d, const LpStatusArgs& st, int LQ, const double* freq,
                                                const sg::Table& T, int n, const int16_t* slot_lp, int ns, uint8_t* maps) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int base = 0; base < LQ; base += sg::kThreads) {
        const int c = base + tid;
        int slot = -1;
        if (c < LQ) {
            int64_t conn;
            if (channel_conn(d, st.P, LQ, st.conn_row, c, conn))
                for (int i = 0; i < ns; ++i) {
                    const int j = slot_lp[i];
                    if (j >= 0 && T.conn[j] == conn) { slot = i; break; }
                }
        }
        unsigned long long mask = __ballot(slot >= 0);
        while (mask) {                                             // (wave-uniform: this wave's channels of slotted lightpaths)
            const int src = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int i = __shfl(slot, src);                       // 0 .. ns - 1
            const int c1 = base + w * 64 + src;
            const int l = c1 / st.Q, q1 = c1 - l * st.Q;
            lp_mark_slots(d, st, LQ, l, q1, freq, T, n, T.conn[slot_lp[i]], maps + i * sg::kCap, lane);
        }
    }
}

// what lp_place_scan leaves for the phases behind it (every value is uniform over the block)
struct LpPlaceScan {
    const double* d;                    // the candidate's sample
    const double* v;                    // values[k]
    int64_t conn_a, lo, hi;             // the candidate's truncated conn, its slice of cells
    int LQ, n, cnt;                     // L * Q; the sample's lightpaths; its flagged ones (kRelease: survivors) + 1
};

// Phases 1 and 2 of candidate k (sg::PlaceArgs, status_scan_dev.hpp) by its whole workgroup: the
// candidate's own arguments; discover() on the unedited sample, thread t reads lightpath t's is_lut flag on its first
// channel and compares its conn with the candidate's; then wave w takes the cells lo + w, lo + w + 4, ...: range check, the
// channel must be free, and the wave's lanes walk the Q slots of the cell's link and mark nb[] (lp_mark_slots; a duplicate
// cell marks the same bytes again).
// kRelease (place(release=...); rl and rs are read and written in this form only): phase 0 checks the
// release slice and loads it; in phase 1 thread t first matches lightpath t against the slice (status_scan_dev.hpp's
// release_* routines: rs->gone, the ticks), only a survivor is flagged, counted and compared with the candidate's conn, a
// second round refuses a slice entry nobody ticked and survivors + 1 > 256; in phase 2 an occupied cell is legal when its
// owner is gone.  The marks of the gone stay in nb[]: the caller clears them (rs->gone) before it stages.
// T, freq [kQCap], nb [kCap], lut_mask [kWaves], bad_all and rs are the caller's LDS.  Returns the candidate's refusal bits
// (QOT_LP_STATUS_* / QOT_LP_PLACE_*), the same in every thread, behind a barrier: 0 -- T, freq, nb and r are complete;
// otherwise nothing has been written to global memory and the caller refuses the candidate.
template <bool kRelease>
__device__ __forceinline__ int lp_place_scan(const LpStatusArgs& st, const sg::PlaceArgs& pl, const sg::ReleaseArgs& rl,
                                             int64_t k, sg::Table& T, double* freq, uint8_t* nb, unsigned long long* lut_mask,
                                             int* bad_all, sg::Release* rs, LpPlaceScan& r) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const double* v = pl.values + k * (int64_t)st.P;

    // ---- what the candidate's own arguments say ----
    bool ok;
    const int64_t s = sg::sample_of(st.samples, k, st.S, ok);
    const int64_t lo = pl.cell_ptr[k], hi = pl.cell_ptr[k + 1];
    int64_t conn_a = 0, rlo = 0;
    int nr = 0;                                                    // the release slice's length, 0 .. 32
    int early = ok ? 0 : QOT_LP_STATUS_BAD_SAMPLE;
    if (lo < 0 || hi <= lo || hi > pl.M) early |= QOT_LP_PLACE_BAD_CELL;
    if constexpr (kRelease)
        if ((nr = sg::release_slice(rl, k, rlo)) < 0) early |= QOT_LP_PLACE_BAD_RELEASE;
    if (!sg::sg_conn(v[st.conn_row], conn_a)) early |= QOT_LP_STATUS_BAD_CONN;
    if (!sg::sg_is_lut_vec(v, st.osnr_row, st.snr_row, st.ber_row)) early |= QOT_LP_PLACE_NOT_LUT;
    if (early) return early;                                       // block-uniform
    const int LQ = st.L * st.Q;
    const double* d = st.data + s * (int64_t)st.P * LQ;
    for (int q = tid; q < st.Q; q += sg::kThreads) freq[q] = st.freq[q];
    nb[tid] = 0;
    if constexpr (kRelease) sg::release_load(*rs, rl, rlo, nr);
    if (tid == 0) *bad_all = 0;

    // ---- phase 1: the lightpaths of the unedited sample, their flags, the candidate's conn among them ----
    const int bad = sg::discover(d, st.P, LQ, st.conn_row, T, nullptr);      // (begins and ends with a barrier)
    const int n = T.n;
    int mine = ((bad & QOT_SG_BAD_CONN) ? QOT_LP_STATUS_BAD_CONN : 0) | ((bad & QOT_SG_TOO_MANY) ? QOT_LP_STATUS_TOO_MANY : 0);
    bool alive = tid < n;                                          // lightpath tid is in the edited sample
    if constexpr (kRelease) alive = sg::release_match(*rs, nr, alive, alive ? T.conn[tid] : 0);
    if (alive && T.conn[tid] == conn_a) mine |= QOT_LP_PLACE_CONN_TAKEN;
    if (!kRelease && tid == 0 && n >= sg::kCap) mine |= QOT_LP_STATUS_TOO_MANY;   // the edited sample would hold n + 1
    if (mine) atomicOr(bad_all, mine);
    const bool flag = alive && sg::sg_is_lut(d, LQ, st.osnr_row, st.snr_row, st.ber_row, T.first[tid]);
    const unsigned long long fm = __ballot(flag);
    if (lane == 0) lut_mask[w] = fm;
    __syncthreads();
    if constexpr (kRelease) {                                      // a second round: what needs every thread's match
        int first;
        const int n_gone = sg::release_gone(*rs, first);
        mine = sg::release_unmatched(*rs, nr) ? QOT_LP_PLACE_NO_SUCH_CONN : 0;
        if (tid == 0 && n - n_gone >= sg::kCap) mine |= QOT_LP_STATUS_TOO_MANY;   // the edited sample would hold 257
        if (mine) atomicOr(bad_all, mine);
        __syncthreads();
    }
    if (*bad_all) return *bad_all;                                 // block-uniform; nobody writes it again
    int cnt = 1;                                                   // the candidate itself
#pragma unroll
    for (int j = 0; j < sg::kWaves; ++j) cnt += __popcll(lut_mask[j]);
    __syncthreads();                                               // (bad_all is written again below)

    // ---- phase 2: the candidate's cells, a wave each ----
    for (int64_t c = lo + w; c < hi; c += sg::kWaves) {            // (wave-uniform)
        const int64_t l = pl.cells[c], q1 = pl.cells[pl.M + c];
        int cell = 0;
        int64_t conn;
        if (l < 0 || l >= st.L || q1 < 0 || q1 >= st.Q) {
            cell = QOT_LP_PLACE_BAD_CELL;
        } else if (channel_conn(d, st.P, LQ, st.conn_row, (int)l * st.Q + (int)q1, conn)) {
            if constexpr (kRelease) cell = sg::release_freed(*rs, T, n, conn, lane) ? 0 : QOT_LP_PLACE_OCCUPIED;
            else cell = QOT_LP_PLACE_OCCUPIED;
        }
        if (cell) {
            if (lane == 0) atomicOr(bad_all, cell);
            continue;
        }
        lp_mark_slots(d, st, LQ, (int)l, (int)q1, freq, T, n, conn_a, nb, lane);
    }
    __syncthreads();
    r.d = d; r.v = v; r.conn_a = conn_a; r.lo = lo; r.hi = hi;
    r.LQ = LQ; r.n = n; r.cnt = cnt;
    return *bad_all;
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

// the LpArgs of a call without a batch: G rows of out, no graph arguments
inline LpArgs lp_status_args(int64_t G, const float* w, const float* att_src, const float* att_dst, const float* conv_bias,
                             float slope_att, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                             const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                             const float* b3, float slope_head, float* out, int F, int C, int O, int lut_col, int32_t* status) {
    return LpArgs{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, G, w, att_src, att_dst, conv_bias, slope_att,
                  bn_weight, bn_bias, bn_mean, bn_var, bn_eps, w0, b0, w3, b3, slope_head, out, nullptr, F, C, O, lut_col,
                  status};
}

// all twelve weights of the model are present
inline bool lp_weights_present(const LpArgs& a) {
    return a.w && a.att_src && a.att_dst && a.conv_bias && a.bn_w && a.bn_b && a.bn_mean && a.bn_var && a.w0 && a.b0 && a.w3 && a.b3;
}

}  // namespace qot
