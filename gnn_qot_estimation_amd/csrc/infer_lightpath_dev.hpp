// The eval-mode forward of one LightpathGNN output row by one wavefront, shared by the single-launch inference kernel
// (infer_lightpath.hip) and the sensitivity kernel (infer_lightpath_grad.hip): both run
// lp_locate + lp_row, so the row they write is the same sums in the same order, bit for bit.  Stated once here for both:
// lp_dot4 (the four per-head dot products of a logit; per-head values live in float[kLpHeads], indexed by unrolled loops
// only), LpRowRegs (what a row leaves in registers for the adjoint) and lp_args (the entry points' envelope, argument
// checks and LpArgs block).
//
// The reference architecture is GATConv(heads = 4) -> BatchNorm (running statistics) -> ReLU -> LUT rows -> MLP, so an output
// row depends on nothing but the one-hop in-neighbourhood of its LUT node: no graph index, no other node's row.  Because
// z_j = W x_j, the aggregate of head h factors as out_i[h] = W_h u_h with u_h = sum_e alpha_e x_{j_e} (F numbers per head
// instead of C), and the logit of a message is leaky_relu(s_h . x_j + d_h . x_i) with s_h = W_h^T att_src_h and
// d_h = W_h^T att_dst_h.
//
// Steps of a row (destination i of graph g; a workgroup barrier between them, which for one wave is a wait on its own
// LDS traffic):
//   0  s_h, d_h [4][F]: lane (h, f) walks the C channels of its head; x_i -> LDS; a_dst_h = d_h . x_i and the self loop's logit
//   1  scan of the graph's edge slice, 64 edges per chunk, lane = offset mod 64: every edge's ends are checked against the
//      graph's node range; the messages (dst == i, src != i: PyG's remove_self_loops) give the per-head maximum
//   2  second scan: a message's lane leaves its weights exp(logit - max) and its source row in LDS; then lane (h, f) adds
//      the chunk's messages to its denominator and to u[h][f] ONE AFTER THE OTHER in slice order; the self loop (PyG's
//      add_self_loops: exactly one, appended) comes last, then u /= (denominator + 1e-16)
//   3  lane-strided over the 4C channels: W_h u_h + bias, BatchNorm on running statistics, ReLU -> LDS
//   4  Linear(4C -> C) + leaky_relu, Linear(C -> O): lanes stride the inner dimension (coalesced rows of the weight), the
//      64 partial sums of an output go through LDS and are added in lane order by one lane
// Every sum has one fixed order that depends on the edge's offset inside its graph's slice and on nothing else: a row is
// bitwise reproducible, and independent of the other graphs of the launch and of the mode that asked for it.  Widths are run
// time values (loops stride them by lane); the parameters are read in place, nothing is tabulated or cached.
//
// lp_row takes a compile-time EDIT POLICY.  LpNoEdit, the default, is empty: the two kernels above
// instantiate the row as it stands.  LpWhatIf (infer_lightpath_whatif.hip) is one candidate of LightpathPredictor.what_if:
// another x_i, some slice positions skipped, further sources behind the slice.  The scans then run the slice's chunks and
// after them the added list as further chunks of 64; the sums stay "one after the other by rising position, the self loop
// last", which is the order of the explicitly built graph (its surviving edges in their order, the additions behind them).
// LpStaged (infer_lightpath_status.hip) is the row without a graph: x_i and the sources' rows are staged in
// LDS by the caller, the slice is empty, and message t is staged row t -- the same scans over the staged list alone.
#pragma once
#include "common.hpp"

namespace qot {

constexpr int kLpMaxF = 16, kLpMaxC = 256, kLpMaxO = 8, kLpHeads = 4;
constexpr int kLpXs = kLpMaxF + 1;      // row stride of the staged source rows (odd: lanes of a chunk hit different banks)
constexpr int kLpTile = 32;             // outputs of a dense layer per pass
constexpr int kLpPs = kWave + 1;        // row stride of their partial sums

struct LpLds {
    float s[kLpHeads * kLpMaxF];        // s_h[f]
    float d[kLpHeads * kLpMaxF];        // d_h[f]
    float xi[kLpMaxF];                  // the destination's features
    float ps[kLpHeads];                 // the self loop's weight exp(logit - max)
    float u[kLpHeads * kLpMaxF];
    float pw[kLpHeads * kWave];         // a chunk's message weights [h][lane]
    float xs[kWave * kLpXs];            // a chunk's source rows [lane][f]
    float y[kLpHeads * kLpMaxC];        // relu(norm(conv)) of the row
    float h1[kLpMaxC];
    float part[kLpTile * kLpPs];
};

// what the adjoint needs of a row beyond LpLds (s, d, xi, ps, u and y stay valid after lp_row): LDS ...
struct LpKeep {
    float pre[kLpMaxC];                 // h1 before its leaky_relu
    float den[kLpHeads];                // the softmax denominators (without the 1e-16)
};

// ... and registers, the same in every lane
struct LpRowRegs {
    float mx[kLpHeads], adst[kLpHeads], rself[kLpHeads];    // the maximum logit, d_h . x_i, the self loop's raw logit
    int64_t n0, n1, e0, m;              // the graph's node range, the first edge and the length of its edge slice
};

struct LpArgs {
    const float* x; const int64_t* ei; const int64_t* batch; const int64_t* node_ptr; const int64_t* edge_ptr;
    const int64_t* lut_idx;
    int64_t L, N, E, B;
    const float* w; const float* att_src; const float* att_dst; const float* conv_bias; float slope_att;
    const float* bn_w; const float* bn_b; const float* bn_mean; const float* bn_var; float eps;
    const float* w0; const float* b0; const float* w3; const float* b3; float slope_head;
    float* out; int32_t* count;
    int F, C, O, lut_col;
    int32_t* status;
};

__device__ __forceinline__ float lp_leaky(float v, float slope) { return v > 0.f ? v : slope * v; }

// acc[h] += sum_t v[h][t] x[t] for the four heads, t rising, one accumulator per head (v: [4][kLpMaxF] in LDS).  `stage`
// (may be null) receives a copy of x[0 .. F).  The loops over h are unrolled: acc stays in registers.
__device__ __forceinline__ void lp_dot4(const float* v, const float* x, int F, float (&acc)[kLpHeads], float* stage = nullptr) {
    for (int t = 0; t < F; ++t) {
        const float xv = x[t];
        if (stage) stage[t] = xv;
#pragma unroll
        for (int h = 0; h < kLpHeads; ++h) acc[h] = fmaf(v[h * kLpMaxF + t], xv, acc[h]);
    }
}

__device__ __forceinline__ void lp_refuse(const LpArgs& a, float* orow, int lane, int bit) {
    if (lane == 0 && a.status) atomicOr(a.status, bit);
    if (lane < a.O) orow[lane] = __builtin_nanf("");
}

// dst[o] = sum_q w[o, q] in[q] + b[o] for o < M (leaky_relu behind it when `act`); `in` holds K floats in LDS.  `raw`
// (LDS, may be null) receives the sums in front of the activation.
__device__ __forceinline__ void lp_dense(const float* __restrict__ w, const float* __restrict__ b, const float* in, int K, int M,
                                         bool act, float slope, float* dst, float* raw, float* part, int lane) {
    for (int c0 = 0; c0 < M; c0 += kLpTile) {
        const int nt = M - c0 < kLpTile ? M - c0 : kLpTile;
        for (int t = 0; t < nt; ++t) {
            const float* wr = w + (int64_t)(c0 + t) * K;
            float p = 0.f;
            for (int q = lane; q < K; q += kWave) p = fmaf(wr[q], in[q], p);
            part[t * kLpPs + lane] = p;
        }
        __syncthreads();
        if (lane < nt) {
            float sum = 0.f;
#pragma unroll 16
            for (int k = 0; k < kWave; ++k) sum += part[lane * kLpPs + k];
            sum += b[c0 + lane];
            if (raw) raw[c0 + lane] = sum;
            dst[c0 + lane] = act ? lp_leaky(sum, slope) : sum;
        }
        __syncthreads();
    }
}

// the edit policy of a plain row: nothing is edited, every hook folds away
struct LpNoEdit {
    static constexpr bool kEdits = false;
    static constexpr bool kStaged = false;
};

constexpr int kLpMaxDrop = 32;          // removals of one candidate (their offsets are staged in LDS: 256 B)

// the edit policy of one what-if candidate.  The kernel fills xi, add, na, drop, nd (each list bounds-checked against its
// array) and dl; lp_row calls stage() once the graph's edge slice is known to lie inside the edge array.
struct LpWhatIf {
    static constexpr bool kEdits = true;
    static constexpr bool kStaged = false;
    const float* xi;                    // the candidate's feature row [F]; null: the node's own
    const int64_t* add;                 // its added sources [na], batch node numbering
    int64_t na;
    const int64_t* drop;                // its drop positions [nd] in the batch's edge_index
    int nd;                             // 0 ... kLpMaxDrop
    int64_t* dl;                        // LDS [kLpMaxDrop]: the drop positions as offsets into the slice
    int64_t mp;                         // the slice's length rounded up to whole chunks: the added list starts there

    // stages the drop offsets (visible behind the next barrier); false: a position outside the slice [e0, e0 + m)
    __device__ __forceinline__ bool stage(int64_t e0, int64_t m, int lane) {
        bool out = false;
        if (lane < nd) {
            const int64_t k = drop[lane] - e0;
            out = k < 0 || k >= m;
            dl[lane] = k;
        }
        mp = (m + kWave - 1) / kWave * kWave;
        return !__any(out);
    }
    __device__ __forceinline__ bool dropped(int64_t k) const {
        bool hit = false;
        for (int t = 0; t < nd; ++t) hit = hit || dl[t] == k;      // (every lane reads the same word: a broadcast)
        return hit;
    }
};

// the edit policy of a row whose neighbourhood the caller has staged (infer_lightpath_status.hip): there is
// no graph -- node_ptr, edge_ptr, edge_index and x are not read, i and g are not looked at.  The edge slice is empty, x_i is
// the staged row `xi`, and the "added sources" are the `na` staged rows themselves, in the order the messages are summed:
// message t is row t.  All of them are messages (the caller leaves the destination out).
struct LpStaged {
    static constexpr bool kEdits = false;                      // no slice: nothing to drop, nothing to stage
    static constexpr bool kStaged = true;
    const float* xi;                    // the destination's feature row [F] (LDS)
    const float* rows;                  // the sources' feature rows [na][kLpXs] (LDS)
    int64_t na;
};

// where the feature row of message source `src` is read from: row src of x, or staged row src
template <class Edit>
__device__ __forceinline__ const float* lp_src_row(const LpArgs& a, const Edit& ed, int64_t src, int F) {
    if constexpr (Edit::kStaged) {
        return ed.rows + src * kLpXs;
    } else {
        return a.x + src * F;
    }
}

// the messages of a chunk: lane `lane` looks at the edge at offset base + lane of the slice.  Returns 0 (no message),
// 1 (a message from `src`) or 2 (an edge that leaves the graph's node range: nothing is read through it).  With an edit:
// a dropped offset is no message and its ends are not read; offset ed.mp + t is added source t, with destination i.
// Staged: offset t < na is the message from staged row t.
template <class Edit = LpNoEdit>
__device__ __forceinline__ int lp_edge(const LpArgs& a, int64_t e0, int64_t m, int64_t k, int64_t n0, int64_t n1, int64_t i,
                                       int64_t& src, const Edit& ed = Edit{}) {
    if constexpr (Edit::kStaged) {
        src = k;
        return k < ed.na ? 1 : 0;                              // (nothing below is reached)
    }
    if constexpr (Edit::kEdits) {
        if (k >= ed.mp) {
            if (k - ed.mp >= ed.na) return 0;
            const int64_t s = ed.add[k - ed.mp];
            if (s < n0 || s >= n1) return 2;
            src = s;
            return s != i ? 1 : 0;
        }
    }
    if (k >= m) return 0;
    if constexpr (Edit::kEdits) {
        if (ed.dropped(k)) return 0;
    }
    const int64_t s = a.ei[e0 + k], d = a.ei[a.E + e0 + k];
    if (s < n0 || s >= n1 || d < n0 || d >= n1) return 2;
    src = s;
    return (d == i && s != i) ? 1 : 0;
}

// the output row of node i of graph g (0 <= i < N and 0 <= g < B are the caller's).  Returns 0: the row is written;
// 1 / 2: refused (NaN row, status bit set) -- 2 when the graph's edge slice R.e0, R.m itself lies inside the edge array.
// kKeep: K (LDS) and R are filled for the adjoint; the sums are the same either way.  Edit: the edit policy (above); an
// edited row is also refused (status bit 2) when its feature row does not carry exactly 1.0f in the LUT column.
template <bool kKeep, class Edit = LpNoEdit>
__device__ __forceinline__ int lp_row(const LpArgs& a, LpLds& L, LpKeep* K, int64_t i, int64_t g, float* orow, int lane,
                                      LpRowRegs& R, Edit ed = Edit{}) {
    const int F = a.F, C = a.C;
    int64_t n0 = 0, n1 = 0, e0 = 0, e1 = 0;                    // (staged: no graph, an empty slice)
    if constexpr (!Edit::kStaged) {
        n0 = a.node_ptr[g]; n1 = a.node_ptr[g + 1]; e0 = a.edge_ptr[g]; e1 = a.edge_ptr[g + 1];
    }
    const bool slice_ok = e0 >= 0 && e1 >= e0 && e1 <= a.E;
    R.n0 = n0; R.n1 = n1; R.e0 = e0; R.m = e1 - e0;
    if constexpr (!Edit::kStaged) {
        if (n0 < 0 || n1 > a.N || i < n0 || i >= n1 || !slice_ok) {
            lp_refuse(a, orow, lane, 2);
            return slice_ok ? 2 : 1;
        }
    }
    const int64_t m = e1 - e0;
    int64_t span = m;                                          // the offsets the scans run over
    if constexpr (Edit::kStaged) span = ed.na;
    if constexpr (Edit::kEdits) {
        if (!ed.stage(e0, m, lane)) {                          // (wave-uniform)
            lp_refuse(a, orow, lane, 2);
            return 2;
        }
        span = ed.mp + ed.na;
    }

    // ---- step 0: s_h, d_h, the destination's row ----
    const int h = lane / F, f = lane - h * F;                  // lanes below 4F own the pair (h, f)
    if (lane < kLpHeads * F) {
        const float* w = a.w + (int64_t)h * C * F + f;
        const float* as = a.att_src + h * C;
        const float* ad = a.att_dst + h * C;
        float s = 0.f, d = 0.f;
        for (int c = 0; c < C; ++c) {
            const float wv = w[c * F];
            s = fmaf(wv, as[c], s);
            d = fmaf(wv, ad[c], d);
        }
        L.s[h * kLpMaxF + f] = s;
        L.d[h * kLpMaxF + f] = d;
    }
    if constexpr (Edit::kStaged) {
        if (lane < F) L.xi[lane] = ed.xi[lane];
    } else if constexpr (Edit::kEdits) {
        if (lane < F) L.xi[lane] = ed.xi ? ed.xi[lane] : a.x[i * F + lane];
    } else {
        if (lane < F) L.xi[lane] = a.x[i * F + lane];
    }
    __syncthreads();
    if constexpr (Edit::kEdits) {
        if (L.xi[a.lut_col] != 1.0f) {                         // (wave-uniform: one LDS word)
            lp_refuse(a, orow, lane, 4);
            return 2;
        }
    }
    float adst[kLpHeads] = {}, lself[kLpHeads] = {};
    for (int t = 0; t < F; ++t) {                              // (two lp_dot4 in one pass over x_i: one LDS wait per t)
        const float xv = L.xi[t];
#pragma unroll
        for (int hh = 0; hh < kLpHeads; ++hh) {
            adst[hh] = fmaf(L.d[hh * kLpMaxF + t], xv, adst[hh]);
            lself[hh] = fmaf(L.s[hh * kLpMaxF + t], xv, lself[hh]);
        }
    }
#pragma unroll
    for (int hh = 0; hh < kLpHeads; ++hh) {
        R.adst[hh] = adst[hh];
        R.rself[hh] = lself[hh] + adst[hh];
        lself[hh] = lp_leaky(R.rself[hh], a.slope_att);
    }

    // ---- step 1: range check of the slice, per-head maximum over the messages and the self loop ----
    float mx[kLpHeads];
#pragma unroll
    for (int hh = 0; hh < kLpHeads; ++hh) mx[hh] = lself[hh];
    bool bad = false;
    for (int64_t base = 0; base < span; base += kWave) {
        int64_t src = 0;
        const int kind = lp_edge(a, e0, m, base + lane, n0, n1, i, src, ed);
        bad = bad || kind == 2;
        if (kind == 1) {
            float l[kLpHeads] = {};
            lp_dot4(L.s, lp_src_row(a, ed, src, F), F, l);
#pragma unroll
            for (int hh = 0; hh < kLpHeads; ++hh) mx[hh] = fmaxf(mx[hh], lp_leaky(l[hh] + adst[hh], a.slope_att));
        }
    }
    if (__any(bad)) {                                          // (wave-uniform)
        lp_refuse(a, orow, lane, 1);
        return 2;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {                  // (a maximum: exact in any order)
#pragma unroll
        for (int hh = 0; hh < kLpHeads; ++hh) mx[hh] = fmaxf(mx[hh], __shfl_xor(mx[hh], o));
    }
#pragma unroll
    for (int hh = 0; hh < kLpHeads; ++hh) {
        R.mx[hh] = mx[hh];
        if (lane == 0) L.ps[hh] = expf(lself[hh] - mx[hh]);
    }

    // ---- step 2: weights and source rows of a chunk -> LDS, then the sums in slice order ----
    float den = 0.f, u = 0.f;
    for (int64_t base = 0; base < span; base += kWave) {
        int64_t src = 0;
        const bool msg = lp_edge(a, e0, m, base + lane, n0, n1, i, src, ed) == 1;
        if (msg) {
            float l[kLpHeads] = {};
            lp_dot4(L.s, lp_src_row(a, ed, src, F), F, l, L.xs + lane * kLpXs);
#pragma unroll
            for (int hh = 0; hh < kLpHeads; ++hh)
                L.pw[hh * kWave + lane] = expf(lp_leaky(l[hh] + adst[hh], a.slope_att) - mx[hh]);
        }
        unsigned long long mask = __ballot(msg);
        __syncthreads();
        if (lane < kLpHeads * F) {
            while (mask) {                                     // (wave-uniform: the chunk's messages by rising offset)
                const int k = __builtin_ctzll(mask);
                mask &= mask - 1;
                const float p = L.pw[h * kWave + k];
                den += p;
                u = fmaf(p, L.xs[k * kLpXs + f], u);
            }
        }
        __syncthreads();
    }
    __syncthreads();                                           // (L.ps of lane 0, when the slice is empty)
    if (lane < kLpHeads * F) {
        const float p = L.ps[h];
        den += p;
        u = fmaf(p, L.xi[f], u);
        L.u[h * kLpMaxF + f] = u / (den + 1e-16f);
        if (kKeep && f == 0) K->den[h] = den;
    }
    __syncthreads();

    // ---- step 3: W_h u_h + bias, BatchNorm (running statistics), ReLU ----
    for (int q = lane; q < kLpHeads * C; q += kWave) {
        const float* wr = a.w + (int64_t)q * F;
        const float* uh = L.u + (q / C) * kLpMaxF;
        float v = 0.f;
        for (int t = 0; t < F; ++t) v = fmaf(wr[t], uh[t], v);
        v += a.conv_bias[q];
        v = (v - a.bn_mean[q]) / sqrtf(a.bn_var[q] + a.eps) * a.bn_w[q] + a.bn_b[q];
        L.y[q] = v > 0.f ? v : 0.f;
    }
    __syncthreads();

    // ---- step 4: the head ----
    lp_dense(a.w0, a.b0, L.y, kLpHeads * C, C, true, a.slope_head, L.h1, kKeep ? K->pre : nullptr, L.part, lane);
    lp_dense(a.w3, a.b3, L.h1, C, a.O, false, 0.f, orow, nullptr, L.part, lane);
    return 0;
}

// Which node and graph workgroup r computes.  Rows mode: entry r of lut_idx.  Graphs mode: the wave counts the LUT nodes
// of graph r (count[r]) and takes the lowest-indexed one.  Returns true with i, g; false when there is no row to compute:
// the out row is NaN then (a graph without a LUT node; or an index / slice outside the arrays, status bit 1 set).
__device__ __forceinline__ bool lp_locate(const LpArgs& a, int64_t r, float* orow, int lane, int64_t& i, int64_t& g) {
    if (a.lut_idx) {                                           // rows mode: one wave per entry of lut_idx
        i = a.lut_idx[r];
        if (i < 0 || i >= a.N) {
            lp_refuse(a, orow, lane, 2);
            return false;
        }
        g = a.batch[i];
        if (g < 0 || g >= a.B) {
            lp_refuse(a, orow, lane, 2);
            return false;
        }
        return true;
    }
    // graphs mode: one wave per graph; its LUT nodes are counted, the lowest-indexed one gives the row
    const int64_t n0 = a.node_ptr[r], n1 = a.node_ptr[r + 1];
    if (n0 < 0 || n1 < n0 || n1 > a.N) {
        if (lane == 0) a.count[r] = 0;
        lp_refuse(a, orow, lane, 2);
        return false;
    }
    int cnt = 0;
    int64_t first = -1;
    for (int64_t base = n0; base < n1; base += kWave) {
        const int64_t k = base + lane;
        const bool hit = k < n1 && a.x[k * a.F + a.lut_col] == 1.0f;
        const unsigned long long mask = __ballot(hit);
        cnt += __popcll(mask);
        if (first < 0 && mask) first = base + __builtin_ctzll(mask);
    }
    if (lane == 0) a.count[r] = cnt;
    if (first < 0) {
        if (lane < a.O) orow[lane] = __builtin_nanf("");
        return false;
    }
    i = first;
    g = r;
    return true;
}

// What both entry points do with the arguments they share, passed on in the ABI's order (Q: the eval entry passes 1):
// sizes first, then the envelope, then -- when there are rows -- the pointers every row reads through.  Returns QOT_OK
// with `a` and `rows` filled (rows == 0: an empty batch, nothing to launch), or the error.
inline int lp_args(const float* x, const int64_t* edge_index, const int64_t* batch, const int64_t* node_ptr,
                   const int64_t* edge_ptr, const int64_t* lut_idx, int64_t L, int64_t N, int64_t E, int64_t B, const float* w,
                   const float* att_src, const float* att_dst, const float* conv_bias, float slope_att, const float* bn_weight,
                   const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps, const float* w0,
                   const float* b0, const float* w3, const float* b3, float slope_head, float* out, int32_t* count, int F, int C,
                   int O, int heads, int lut_col, int32_t* status, int Q, LpArgs& a, int64_t& rows) {
    rows = 0;
    if (N < 0 || E < 0 || B < 0 || L < 0) return QOT_ERR_BADARG;
    if (F < 1 || F > kLpMaxF) return QOT_ERR_UNSUPPORTED;
    if (C < 1 || C > kLpMaxC) return QOT_ERR_UNSUPPORTED;
    if (O < 1 || O > kLpMaxO) return QOT_ERR_UNSUPPORTED;
    if (heads != kLpHeads) return QOT_ERR_UNSUPPORTED;
    if (lut_col < 0 || lut_col >= F) return QOT_ERR_UNSUPPORTED;
    if (Q < 1 || Q > O) return QOT_ERR_UNSUPPORTED;
    const int64_t n = lut_idx ? L : B;
    if (n == 0) return QOT_OK;
    if (n > 0x7fffffff) return QOT_ERR_UNSUPPORTED;
    if (!node_ptr || !edge_ptr || !w || !att_src || !att_dst || !conv_bias || !bn_weight || !bn_bias || !bn_mean || !bn_var ||
        !w0 || !b0 || !w3 || !b3 || !out)
        return QOT_ERR_BADARG;
    if ((N > 0 && !x) || (E > 0 && !edge_index)) return QOT_ERR_BADARG;
    if (lut_idx ? !batch : !count) return QOT_ERR_BADARG;
    a = LpArgs{x, edge_index, batch, node_ptr, edge_ptr, lut_idx, L, N, E, B, w, att_src, att_dst, conv_bias, slope_att,
               bn_weight, bn_bias, bn_mean, bn_var, bn_eps, w0, b0, w3, b3, slope_head, out, count, F, C, O, lut_col, status};
    rows = n;
    return QOT_OK;
}

}  // namespace qot
