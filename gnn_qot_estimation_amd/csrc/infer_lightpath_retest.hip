// LightpathPredictor.retest: the standing question about a network state -- what is the predicted QoT of each lightpath
// that is already lit? -- in ONE launch: every ESTABLISHED lightpath of a status sample data[S, P, L, Q] (fp64), or a named
// subset, retested as the lightpath under test; no edited sample, no graph, nothing read back.  Sample
// samples[g] has n[g] lightpaths; slot i < M of it holds a lightpath j: conn[g, i] is its conn and out[g, i] its eval-mode
// row -- bit for bit the row qot_lightpath_infer gives the lightpath's node in the graph the device builder
// (status_graph.hip) makes of the sample in which the lightpath's channels carry osnr = snr = ber = -1
// (infer.materialise_retest without values).  That sample is never built: flagging a lightpath changes its is_lut column
// and nothing else (the caller refuses feature lists that hold osnr, snr or ber), so the row is the lightpath's own feature
// row from its first channel with is_lut forced to 1 and the messages of its interferers, by rising first-seen number, with
// their is_lut as the sample has it.  This is `before` of infer_lightpath_place_impact.hip with another source of slots.
//   conns == NULL   slot i holds lightpath number i (first-seen order, the node order of the builder) while i < n[g];
//   conns [G, M]    slot i holds the lightpath whose conn is conns[g, i]; -1 is an empty slot; a conn the sample does not
//                   hold is an empty slot that sets QOT_LP_RETEST_NO_SUCH_CONN; a conn named twice gives equal rows.
// An empty slot holds conn -1 and a NaN row.  count[g] is from_status's: the sample's own flagged lightpaths.
//
// G * ceil(M / chunk) workgroups of 256 threads; workgroup (g, b) owns the slots [b * chunk, min((b + 1) * chunk, M)):
//   1  as infer_lightpath_status.hip: the sample pick, discover(), the flag ballot, the refusal mapping; block b == 0
//      writes n[g] and count[g].  The slot table: thread i < chunk takes lightpath number b * chunk + i, or looks its conn
//      up in T.conn[0 .. n).  A block without a lightpath in its slots writes its padding and ends.
//   2  infer_lightpath_status_dev.hpp's lp_mark_slotted, shared with infer_lightpath_place_impact.hip: one rescan of the
//      conn_id row marks every slotted lightpath's own byte map (chunk x 256 bytes of LDS, zeroed first).
//   3  wave 0 alone, the others have ended.  Per slot: the sources by rising number -> LDS (lp_stage_marked), the
//      lightpath's own row with is_lut forced to 1, lp_row -> out[g, i].  A slot that repeats a lightpath of an earlier slot
//      of the block stages from that slot's map (the rescan fills the first one only).
// Phase 3 must stay in ONE wave: lp_row holds __syncthreads() calls whose number depends on the message count, which is safe
// only because the other waves have ended before it runs.  Every early exit is block-uniform and lies behind the barrier
// that publishes what it depends on.  A slot's row is computed from the sample and the slot alone, by one wave, in a fixed
// order: it does not depend on chunk.
// No workspace, no global scratch.  Nothing read from data or conns is used as an index: a conn is only compared.  All
// global writes are ordinary vector stores (the status word: one atomicOr per workgroup at the most).
//
// On the device: what infer_lightpath_status.hip refuses, with the same bits -- all M rows of the sample NaN, its conn -1,
// n = count = 0; the other samples are untouched.
#include "infer_lightpath_status_dev.hpp"

namespace qot {
namespace {

constexpr int kLpRetestChunk = QOT_LP_RETEST_MAX_CHUNK;            // 32
constexpr int kLpRetestSlots = QOT_SG_MAX_LIGHTPATHS;              // 256

struct LpRetestArgs {
    const int64_t* conns;               // [G, M] or null
    int64_t* conn;                      // [G, M]
    int64_t* n;                         // [G]
    int M, chunk, blocks;               // blocks = ceil(M / chunk)
};

// slots [from, to) of sample g: no lightpath (wave 0)
__device__ __forceinline__ void lp_retest_pad(const LpArgs& a, const LpRetestArgs& rt, int64_t g, int from, int to, int lane) {
    for (int i = from + lane; i < to; i += kWave) rt.conn[g * rt.M + i] = -1;
    const int64_t base = g * rt.M * a.O;
    for (int t = from * a.O + lane; t < to * a.O; t += kWave) a.out[base + t] = __builtin_nanf("");
}

__global__ __launch_bounds__(sg::kThreads) void lightpath_infer_retest_kernel(const LpArgs a, const LpStatusArgs st,
                                                                              const LpRetestArgs rt) {
    __shared__ sg::Table T;
    __shared__ double freq[sg::kQCap];
    __shared__ LpLds L;
    __shared__ float rows[sg::kCap * kLpXs];
    __shared__ float xi[kLpMaxF];
    __shared__ uint32_t nbs[kLpRetestChunk * sg::kCap / 4];        // the slotted lightpaths' byte maps [chunk][256]
    __shared__ int16_t slot_lp[kLpRetestChunk];                    // slot -> lightpath number, -1: empty
    __shared__ unsigned long long lut_mask[sg::kWaves];
    __shared__ int bad_all, in_use;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t g = blockIdx.x / rt.blocks;
    const int b = (int)(blockIdx.x - g * rt.blocks);
    const int s0 = b * rt.chunk;
    const int s1 = s0 + rt.chunk < rt.M ? s0 + rt.chunk : rt.M;
    const int ns = s1 - s0;                                        // 1 .. chunk
    uint8_t* maps = reinterpret_cast<uint8_t*>(nbs);
    bool ok;
    const int64_t s = sg::sample_of(st.samples, g, st.S, ok);
    int refused = ok ? 0 : QOT_LP_STATUS_BAD_SAMPLE;               // block-uniform
    int n = 0, cnt = 0, LQ = 0;
    const double* d = nullptr;
    if (!refused) {
        LQ = st.L * st.Q;
        d = st.data + s * (int64_t)st.P * LQ;
        for (int q = tid; q < st.Q; q += sg::kThreads) freq[q] = st.freq[q];
        for (int t = tid; t < ns * (sg::kCap / 4); t += sg::kThreads) nbs[t] = 0;
        if (tid == 0) bad_all = 0;

        // ---- phase 1: the lightpaths of the sample, their flags ----
        const int bad = sg::discover(d, st.P, LQ, st.conn_row, T, nullptr);  // (begins and ends with a barrier)
        if (bad) atomicOr(&bad_all, bad);
        n = T.n;
        const bool flag = tid < n && sg::sg_is_lut(d, LQ, st.osnr_row, st.snr_row, st.ber_row, T.first[tid]);
        const unsigned long long fm = __ballot(flag);
        if (lane == 0) lut_mask[w] = fm;
        __syncthreads();
        if (bad_all)                                               // block-uniform; nobody writes it again
            refused = ((bad_all & QOT_SG_BAD_CONN) ? QOT_LP_STATUS_BAD_CONN : 0) |
                      ((bad_all & QOT_SG_TOO_MANY) ? QOT_LP_STATUS_TOO_MANY : 0);
    }
    if (refused) {
        if (w == 0) {
            if (lane == 0 && b == 0) {
                st.count[g] = 0;
                rt.n[g] = 0;
                if (a.status) atomicOr(a.status, refused);
            }
            lp_retest_pad(a, rt, g, s0, s1, lane);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < sg::kWaves; ++k) cnt += __popcll(lut_mask[k]);
    if (tid == 0 && b == 0) {
        st.count[g] = cnt;
        rt.n[g] = n;
    }

    // ---- the slot table ----
    if (w == 0) {
        int lp = -1;
        bool missing = false;
        if (lane < ns) {
            if (rt.conns) {
                const int64_t want = rt.conns[g * rt.M + s0 + lane];
                if (want != -1) {
                    for (int j = 0; j < n; ++j)
                        if (T.conn[j] == want) { lp = j; break; }
                    missing = lp < 0;
                }
            } else if (s0 + lane < n) {
                lp = s0 + lane;
            }
            slot_lp[lane] = (int16_t)lp;
        }
        const unsigned long long used = __ballot(lp >= 0), miss = __ballot(missing);
        if (lane == 0) {
            in_use = used != 0;
            if (miss && a.status) atomicOr(a.status, QOT_LP_RETEST_NO_SUCH_CONN);
        }
    }
    __syncthreads();
    if (!in_use) {                                                 // block-uniform: nobody to retest in these slots
        if (w == 0) lp_retest_pad(a, rt, g, s0, s1, lane);
        return;
    }

    // ---- phase 2: the slotted lightpaths' maps (infer_lightpath_status_dev.hpp, shared with infer_lightpath_place_impact.hip) ----
    lp_mark_slotted(d, st, LQ, freq, T, n, slot_lp, ns, maps);
    __syncthreads();
    if (w != 0) return;

    // ---- phase 3: the slots one after the other ----
    LpRowRegs R;
    for (int i = 0; i < ns; ++i) {                                 // (wave-uniform)
        const int j = slot_lp[i];
        if (j < 0) {
            lp_retest_pad(a, rt, g, s0 + i, s0 + i + 1, lane);
            continue;
        }
        int src = i;                                               // the first slot of the block that holds lightpath j
        for (int t = i - 1; t >= 0; --t)
            if (slot_lp[t] == j) src = t;
        const int na = lp_stage_marked(d, st, LQ, a.F, T, n, maps + src * sg::kCap, rows, lane);
        if (lane < a.F) {
            const bool lut = (int)st.cols[4 * lane] < 0;
            xi[lane] = lut ? 1.0f : sg::sg_feature(d, st.P, LQ, st.osnr_row, st.snr_row, st.ber_row, st.cols, lane, T.first[j]);
        }
        if (lane == 0) rt.conn[g * rt.M + s0 + i] = T.conn[j];
        __syncthreads();
        LpStaged ed;
        ed.xi = xi;
        ed.rows = rows;
        ed.na = na;
        lp_row<false, LpStaged>(a, L, nullptr, 0, 0, a.out + (g * rt.M + s0 + i) * a.O, lane, R, ed);
    }
}

}  // namespace
}  // namespace qot

using namespace qot;

extern "C" int qot_lightpath_infer_retest(const float* x, const int64_t* edge_index, const int64_t* batch,
                                          const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx, int64_t n_lut,
                                          int64_t N, int64_t E, int64_t G, const float* w, const float* att_src,
                                          const float* att_dst, const float* conv_bias, float slope_att,
                                          const float* bn_weight, const float* bn_bias, const float* bn_mean,
                                          const float* bn_var, float bn_eps, const float* w0, const float* b0, const float* w3,
                                          const float* b3, float slope_head, float* out, int64_t* count, int F, int C, int O,
                                          int heads, int lut_col, int32_t* status, const double* data, const double* freq,
                                          const int64_t* samples, int64_t S, int P, int64_t L, int64_t Q, int conn_row,
                                          int osnr_row, int snr_row, int ber_row, const double* cols, int ncol,
                                          double freq_threshold, const int64_t* conns, int64_t* conn, int64_t* n,
                                          int max_lightpaths, int chunk, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = lp_status_envelope(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, n_lut, N, E, G, F, C, O, heads, lut_col,
                                      S, P, L, Q, conn_row, osnr_row, snr_row, ber_row, ncol, freq_threshold);
    if (rc != QOT_OK) return rc;
    if (max_lightpaths < 1 || max_lightpaths > kLpRetestSlots || chunk < 1 || chunk > kLpRetestChunk) return QOT_ERR_BADARG;
    const int blocks = (max_lightpaths + chunk - 1) / chunk;
    if (G * blocks >= (int64_t)1 << 31) return QOT_ERR_UNSUPPORTED;
    if (G == 0) return QOT_OK;
    const LpArgs a = lp_status_args(G, w, att_src, att_dst, conv_bias, slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps,
                                    w0, b0, w3, b3, slope_head, out, F, C, O, lut_col, status);
    if (!lp_weights_present(a) || !out || !count || !data || !freq || !cols || S == 0 || !conn || !n) return QOT_ERR_BADARG;
    const LpStatusArgs st{data, freq, samples, S, P, (int)L, (int)Q, conn_row, osnr_row, snr_row, ber_row, cols,
                          freq_threshold, count};
    const LpRetestArgs rt{conns, conn, n, max_lightpaths, chunk, blocks};
    lightpath_infer_retest_kernel<<<(int)(G * blocks), sg::kThreads, 0, stream>>>(a, st, rt);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
