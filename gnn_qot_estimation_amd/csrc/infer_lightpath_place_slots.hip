// LightpathPredictor.place_slots: the step every routing-and-spectrum-assignment loop takes before it scores an
// assignment -- given a route, which frequency slot? -- in ONE launch: R routes, each swept over all Q start slots of the
// grid of a network-status sample data[S, P, L, Q] (fp64); no free-slot list, no candidate lists, nothing read back
// (DESIGN.md 4.28).  Route r is the links links[link_ptr[r] : link_ptr[r + 1]] in sample samples[r] with the raw lp_feat
// vector values[r, P]; a candidate that starts at slot q occupies the slots q .. q + width - 1 on every link of the route.
// free[r, q] is 1 when all those channels are free and q + width <= Q; out[r, q] is then, bit for bit, the row
// qot_lightpath_infer_place gives the candidate with those cells and values[r] -- with slot_row >= 0, values[r] with
// freq[q] in that lp_feat row, what a lightpath on slot q carries there -- and a NaN row otherwise.  An occupied slot is
// an answer, not an error: it sets no status bit.  count[r] is place's: the sample's flagged lightpaths + 1, the same at
// every slot.  All slots of a route share the sample, the first-seen table and the candidate's vector; they differ in who
// lies within the threshold, so one discover() serves a chunk of slots.
//
// R * ceil(Q / chunk) workgroups of 256 threads; workgroup (r, b) owns the start slots [b * chunk, min((b + 1) * chunk, Q)):
//   0/1  the route's own arguments -- the five block-uniform tests at the head of lp_place_scan, restated here: moving
//        them into a routine of the header for both changed the code the compiler gives the four existing instantiations
//        of the scan, and those stay as they are -- then discover(), the flag ballot, the conn-taken and too-many tests
//        of place and the range check of the route's links: the status bit is per route, so one bad link refuses the
//        whole route, before anything is written.  Block b == 0 writes count[r].  A refused route: every block pads its
//        own slots, block b == 0 sets the bits.
//   2    the work items (slot i of the chunk, link j of the route, offset t < width) are dealt to the four waves: channel
//        (l, q + t) occupied or q + t >= Q sets the slot's `taken` byte, otherwise the wave's lanes walk the Q slots of
//        link l and mark the slot's own byte map (lp_mark_slots; chunk x 256 bytes of LDS, zeroed first; same-value
//        stores, so a duplicate link marks the same bytes again).  A barrier, and waves 1-3 return.
//   3    wave 0 alone, slot by slot.  Taken: a NaN row, free = 0.  Else the sources by rising number -> LDS
//        (lp_stage_marked), x_i from values[r] (sg_feature_vec; the column whose lp_feat row is slot_row from freq[q]:
//        the doubles a channel holding the edited vector would give), lp_row -> out[r, q], free = 1.
// Phase 3 must stay in ONE wave: lp_row holds __syncthreads() calls whose number depends on the message count, which is safe
// only because the other waves have ended before it runs (infer_lightpath_retest.hip has the same shape).  Every early
// exit is block-uniform and lies behind the barrier that publishes what it depends on.  A slot's row is computed from the
// sample, the route and the slot alone, by one wave, in a fixed order: it does not depend on chunk.
// Cost per workgroup: O(L Q) for discover plus O(chunk * route * width * Q) for the walks.
// No workspace, no global scratch.  Nothing read from data or values is used as an index: a conn is only compared; a link
// index comes from `links` and is range-checked first.  All global writes are ordinary vector stores (free: bytes; the
// status word: one atomicOr per route at the most).
//
// On the device, per route (all Q rows NaN, free 0, count 0; the other routes are untouched), with place's bits: a sample
// number outside [0, S) (QOT_LP_STATUS_BAD_SAMPLE); a link_ptr slice that is empty, descending or beyond M, a link index
// outside [0, L) (QOT_LP_PLACE_BAD_CELL); a conn_id of values[r] that is not finite or beyond +-2^53, or such a value in
// the sample (QOT_LP_STATUS_BAD_CONN); values[r] without osnr == snr == ber == -1 (QOT_LP_PLACE_NOT_LUT); a conn_id the
// sample holds already (QOT_LP_PLACE_CONN_TAKEN); a sample of 256 or more lightpaths (QOT_LP_STATUS_TOO_MANY).
#include "infer_lightpath_status_dev.hpp"

namespace qot {
namespace {

constexpr int kLpSlotsChunk = QOT_LP_PLACE_SLOTS_MAX_CHUNK;        // 32
constexpr int kLpSlotsWidth = QOT_LP_PLACE_SLOTS_MAX_WIDTH;        // 8

struct LpSlotsArgs {
    const double* values;               // [R, P] raw lp_feat vectors
    const int64_t* links;               // [M] link indices
    const int64_t* link_ptr;            // [R + 1]
    int64_t M;
    uint8_t* free;                      // [R, Q]
    int slot_row, width, chunk, blocks; // blocks = ceil(Q / chunk)
};

// start slots [from, to) of route r: not free (wave 0)
__device__ __forceinline__ void lp_slots_pad(const LpArgs& a, const LpSlotsArgs& sl, int64_t r, int Q, int from, int to,
                                             int lane) {
    for (int q = from + lane; q < to; q += kWave) sl.free[r * Q + q] = 0;
    const int64_t base = r * Q * a.O;
    for (int t = from * a.O + lane; t < to * a.O; t += kWave) a.out[base + t] = __builtin_nanf("");
}

__global__ __launch_bounds__(sg::kThreads) void lightpath_infer_place_slots_kernel(const LpArgs a, const LpStatusArgs st,
                                                                                   const LpSlotsArgs sl) {
    __shared__ sg::Table T;
    __shared__ double freq[sg::kQCap];
    __shared__ LpLds L;
    __shared__ float rows[sg::kCap * kLpXs];
    __shared__ float xi[kLpMaxF];
    __shared__ uint32_t nbs[kLpSlotsChunk * sg::kCap / 4];         // the slots' byte maps [chunk][256]
    __shared__ uint32_t taken_w[kLpSlotsChunk / 4];                // the slots' taken bytes [chunk]
    __shared__ unsigned long long lut_mask[sg::kWaves];
    __shared__ int bad_all;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t r = blockIdx.x / sl.blocks;
    const int b = (int)(blockIdx.x - r * sl.blocks);
    const int s0 = b * sl.chunk;
    const int s1 = s0 + sl.chunk < st.Q ? s0 + sl.chunk : st.Q;
    const int ns = s1 - s0;                                        // 1 .. chunk
    uint8_t* maps = reinterpret_cast<uint8_t*>(nbs);
    uint8_t* taken = reinterpret_cast<uint8_t*>(taken_w);
    const double* v = sl.values + r * (int64_t)st.P;

    // ---- phase 0: what the route's own arguments say (the tests lp_place_scan makes of a candidate's; see the header) ----
    bool ok;
    const int64_t s = sg::sample_of(st.samples, r, st.S, ok);
    const int64_t lo = sl.link_ptr[r], hi = sl.link_ptr[r + 1];
    int64_t conn_a = 0;
    int refused = ok ? 0 : QOT_LP_STATUS_BAD_SAMPLE;               // block-uniform
    if (lo < 0 || hi <= lo || hi > sl.M) refused |= QOT_LP_PLACE_BAD_CELL;
    if (!sg::sg_conn(v[st.conn_row], conn_a)) refused |= QOT_LP_STATUS_BAD_CONN;
    if (!sg::sg_is_lut_vec(v, st.osnr_row, st.snr_row, st.ber_row)) refused |= QOT_LP_PLACE_NOT_LUT;
    int n = 0, cnt = 1, LQ = 0;                                    // (cnt: the candidate itself)
    const double* d = nullptr;
    if (!refused) {
        LQ = st.L * st.Q;
        d = st.data + s * (int64_t)st.P * LQ;
        for (int q = tid; q < st.Q; q += sg::kThreads) freq[q] = st.freq[q];
        for (int t = tid; t < ns * (sg::kCap / 4); t += sg::kThreads) nbs[t] = 0;
        if (tid < kLpSlotsChunk / 4) taken_w[tid] = 0;
        if (tid == 0) bad_all = 0;

        // ---- phase 1: the lightpaths of the sample, their flags, the candidate's conn among them, the route's links ----
        const int bad = sg::discover(d, st.P, LQ, st.conn_row, T, nullptr);  // (begins and ends with a barrier)
        n = T.n;
        int mine = ((bad & QOT_SG_BAD_CONN) ? QOT_LP_STATUS_BAD_CONN : 0) | ((bad & QOT_SG_TOO_MANY) ? QOT_LP_STATUS_TOO_MANY : 0);
        if (tid < n && T.conn[tid] == conn_a) mine |= QOT_LP_PLACE_CONN_TAKEN;
        if (tid == 0 && n >= sg::kCap) mine |= QOT_LP_STATUS_TOO_MANY;     // the edited sample would hold n + 1
        for (int64_t c = lo + tid; c < hi; c += sg::kThreads) {
            const int64_t l = sl.links[c];
            if (l < 0 || l >= st.L) mine |= QOT_LP_PLACE_BAD_CELL;
        }
        if (mine) atomicOr(&bad_all, mine);
        const bool flag = tid < n && sg::sg_is_lut(d, LQ, st.osnr_row, st.snr_row, st.ber_row, T.first[tid]);
        const unsigned long long fm = __ballot(flag);
        if (lane == 0) lut_mask[w] = fm;
        __syncthreads();
        refused = bad_all;                                         // block-uniform; nobody writes it again
    }
    if (refused) {
        if (w == 0) {
            if (lane == 0 && b == 0) {
                st.count[r] = 0;
                if (a.status) atomicOr(a.status, refused);
            }
            lp_slots_pad(a, sl, r, st.Q, s0, s1, lane);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < sg::kWaves; ++k) cnt += __popcll(lut_mask[k]);
    if (tid == 0 && b == 0) st.count[r] = cnt;

    // ---- phase 2: the items (slot of the chunk, link of the route, offset in the width), a wave each ----
    const int64_t per_slot = (hi - lo) * sl.width;
    const int64_t items = ns * per_slot;
    for (int64_t e = w; e < items; e += sg::kWaves) {              // (wave-uniform)
        const int i = (int)(e / per_slot);                         // 0 .. ns - 1
        const int64_t rem = e - i * per_slot;
        const int64_t j = rem / sl.width;
        const int q = s0 + i + (int)(rem - j * sl.width);
        const int l = (int)sl.links[lo + j];                       // in [0, L): checked in phase 1
        int64_t conn;
        if (q >= st.Q || channel_conn(d, st.P, LQ, st.conn_row, l * st.Q + q, conn)) {
            if (lane == 0) taken[i] = 1;
            continue;
        }
        lp_mark_slots(d, st, LQ, l, q, freq, T, n, conn_a, maps + i * sg::kCap, lane);
    }
    __syncthreads();
    if (w != 0) return;

    // ---- phase 3: the slots one after the other ----
    LpRowRegs R;
    for (int i = 0; i < ns; ++i) {                                 // (wave-uniform)
        const int q = s0 + i;
        if (taken[i]) {
            lp_slots_pad(a, sl, r, st.Q, q, q + 1, lane);
            continue;
        }
        const int na = lp_stage_marked(d, st, LQ, a.F, T, n, maps + i * sg::kCap, rows, lane);
        if (lane < a.F) {
            const double* col = st.cols + 4 * lane;
            const bool swept = sl.slot_row >= 0 && (int)col[0] == sl.slot_row;
            xi[lane] = swept ? sg::scaled(freq[q], col)
                             : sg::sg_feature_vec(v, st.P, st.osnr_row, st.snr_row, st.ber_row, st.cols, lane);
        }
        if (lane == 0) sl.free[r * st.Q + q] = 1;
        __syncthreads();
        LpStaged ed;
        ed.xi = xi;
        ed.rows = rows;
        ed.na = na;
        lp_row<false, LpStaged>(a, L, nullptr, 0, 0, a.out + (r * st.Q + q) * a.O, lane, R, ed);
    }
}

}  // namespace
}  // namespace qot

using namespace qot;

extern "C" int qot_lightpath_infer_place_slots(const float* x, const int64_t* edge_index, const int64_t* batch,
                                               const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx,
                                               int64_t n_lut, int64_t N, int64_t E, int64_t R, const float* w,
                                               const float* att_src, const float* att_dst, const float* conv_bias,
                                               float slope_att, const float* bn_weight, const float* bn_bias,
                                               const float* bn_mean, const float* bn_var, float bn_eps, const float* w0,
                                               const float* b0, const float* w3, const float* b3, float slope_head, float* out,
                                               int64_t* count, int F, int C, int O, int heads, int lut_col, int32_t* status,
                                               const double* data, const double* freq, const int64_t* samples, int64_t S, int P,
                                               int64_t L, int64_t Q, int conn_row, int osnr_row, int snr_row, int ber_row,
                                               const double* cols, int ncol, double freq_threshold, const double* values,
                                               const int64_t* links, const int64_t* link_ptr, int64_t M, int slot_row,
                                               int width, int chunk, uint8_t* free, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (R < 0 || (Q > 0 && R > (((int64_t)1 << 31) - 1) / Q)) return R < 0 ? QOT_ERR_BADARG : QOT_ERR_UNSUPPORTED;
    const int rc = lp_status_envelope(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, n_lut, N, E, R * Q, F, C, O, heads,
                                      lut_col, S, P, L, Q, conn_row, osnr_row, snr_row, ber_row, ncol, freq_threshold);
    if (rc != QOT_OK) return rc;
    if (M < 0 || slot_row < -1 || slot_row >= P || width < 1 || width > kLpSlotsWidth || chunk < 1 || chunk > kLpSlotsChunk)
        return QOT_ERR_BADARG;
    const int blocks = (int)((Q + chunk - 1) / chunk);
    if (R * blocks >= (int64_t)1 << 31) return QOT_ERR_UNSUPPORTED;
    if (R == 0) return QOT_OK;
    const LpArgs a = lp_status_args(R * Q, w, att_src, att_dst, conv_bias, slope_att, bn_weight, bn_bias, bn_mean, bn_var,
                                    bn_eps, w0, b0, w3, b3, slope_head, out, F, C, O, lut_col, status);
    if (!lp_weights_present(a) || !out || !count || !data || !freq || !cols || S == 0 || !samples || !values || !link_ptr ||
        (M > 0 && !links) || !free)
        return QOT_ERR_BADARG;
    const LpStatusArgs st{data, freq, samples, S, P, (int)L, (int)Q, conn_row, osnr_row, snr_row, ber_row, cols,
                          freq_threshold, count};
    const LpSlotsArgs sl{values, links, link_ptr, M, free, slot_row, width, chunk, blocks};
    lightpath_infer_place_slots_kernel<<<(int)(R * blocks), sg::kThreads, 0, stream>>>(a, st, sl);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
