// Device pieces of the single-launch TopologicalGNN forward, shared by the eval kernel (infer.hip), the
// Monte-Carlo dropout kernel (infer_mc.hip), the sensitivity kernel (infer_grad.hip) and the
// what-if kernel (infer_whatif.hip, DESIGN.md 4.18: the same phases over an edited edge list, see InferBaseEdges):
// the LDS layout, the argument block and the two halves of a workgroup's work on ONE graph --
//   infer_phases12: index, edge MLP hidden layer, TransformerConv + leaky_relu -> the undropped x1 in LDS
//   infer_phases34: NNConv (mean) in row tiles + leaky_relu, pooled on the fly, mean pool, read-out MLP -> one output row
// The second half is a template on MC: false compiles the eval forward (no dropout code at all), true applies the engine's
// counter-based dropout (common.hpp: act_hash64) behind conv2's leaky_relu and inside the read-out; conv1's dropout is a
// masked copy of x1 the caller hands in as `xin`.  Every sum runs in the same order in both.  GRAD (the sensitivity
// kernel) keeps the branches the two leaky_relus took -- nothing else changes, the sums are the eval forward's.
// Around the phases, stated once for the three: a kernel's first steps (infer_prologue, infer_refuse) and, at the end of
// this file, the host path of an entry point -- the envelope answers, the argument checks, the dispatch over (H, D).
#pragma once
#include "graph_prep_dev.hpp"

namespace qot {

constexpr int kInferThreads = 256;
constexpr int kInferMaxN = 128;                       // local node ids are packed 16 + 16 bits; one softmax thread per row
constexpr size_t kInferLdsMax = 160 * 1024 - 2048;    // the CU's LDS less the static words of the block scan and flags

__host__ __device__ constexpr int infer_rpt(int H) { return H == 64 ? 4 : 2; }                 // rows per thread of A Wcat
__host__ __device__ constexpr int infer_tile_rows(int H) { return infer_rpt(H) * (kInferThreads / H); }
__host__ __device__ constexpr int infer_pad4(int v) { return (v + 3) & ~3; }

// 4-byte word offsets of the LDS image for graphs of at most cap_n nodes / cap_m edges: the ONE statement of the budget
// (the kernels, the entry points and qot_topological_infer[_mc|_grad]_supported all read it).  Variants: the eval image,
// unchanged, followed by
//   kInferMc    x1d, the sample's masked copy of x1 (cap_n * H words)
//   kInferGrad  gx1 [cap_n, H] (the adjoint of x1, then of conv1's pre-activation), gy [R, H] (a row tile of conv2's
//               adjoint), dh [cap_m, K] (per edge: the adjoint of the edge MLP's hidden layer, later the edge's partial
//               result) and gs / gpool [H] (the read-out's adjoints)
enum InferVariant { kInferEval = 0, kInferMc = 1, kInferGrad = 2 };
struct InferLds {
    int atile, x1, ea, he, alpha, ends, key, cin, rp, lnid, part, pooled, h1, x1d, gx1, gy, dh, gs, gpool, words;
};
__host__ __device__ inline InferLds infer_lds(int cap_n, int cap_m, int H, int D, InferVariant var = kInferEval) {
    const int K = 2 * D;
    InferLds L;
    int o = 0;
    L.atile = o;  o += infer_tile_rows(H) * (K + 2) * H;       // [R][(K + 2) H], rows 16-byte aligned
    L.x1 = o;     o += infer_pad4(cap_n * H);                  // first convolution's output
    L.ea = o;     o += infer_pad4(cap_m * D);                  // edge features, edge order
    L.he = o;     o += infer_pad4(cap_m * K);                  // edge MLP hidden layer, edge order
    L.alpha = o;  o += cap_m;                                  // placement rank, then logits / attention weights per slot
    L.ends = o;   o += cap_m;                                  // local source << 16 | local destination, edge order
    L.key = o;    o += cap_m;                                  // edge of every slot
    L.cin = o;    o += cap_n;
    L.rp = o;     o += cap_n + 1;
    L.lnid = o;   o += cap_n;
    o = infer_pad4(o);
    L.part = o;   o += kInferThreads;                          // pool shares of the row groups
    L.pooled = o; o += H;
    L.h1 = o;     o += H;
    L.x1d = o;    if (var == kInferMc) o += infer_pad4(cap_n * H);   // 16-byte aligned: all above ends on a multiple of 4
    L.gx1 = L.gy = L.dh = L.gs = L.gpool = o;
    if (var == kInferGrad) {
        L.gx1 = o;    o += infer_pad4(cap_n * H);
        L.gy = o;     o += infer_tile_rows(H) * H;
        L.dh = o;     o += infer_pad4(cap_m * K);
        L.gs = o;     o += H;
        L.gpool = o;  o += H;
    }
    L.words = o;
    return L;
}

struct InferArgs {
    const int64_t* node_ids; const int64_t* ei; const float* edge_attr; const int64_t* node_ptr; const int64_t* edge_ptr;
    int64_t N, E, B;
    int cap_n, cap_m;
    const float* t4; int ld4; const float* M; int ldm; const float* P; int V;
    const float* w_edge; const float* w1; const float* b1; const float* wcat; const float* bias2;
    const float* w0; const float* b0; const float* w3; const float* b3;
    float slope_conv, slope_head;
    float* out; int O;
    int32_t* status;
};

// the dropout of one Monte-Carlo sample (include/qot_gnn.h: keep = hash(site seed, step, flat element) >= thr16)
struct InferDrop {
    uint64_t seed_conv2, seed_head, step;
    uint32_t thr_conv, thr_head;        // 0: that site keeps everything and multiplies nothing
    float scale_conv, scale_head;       // 1 / (1 - p) in fp32
    uint64_t row0, graph;               // the graph's first row in the batch's [N, H] activation; its row of [B, H]
};

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : slope * v; }

// dropout of the already activated value y, element `flat` of its activation: act_apply1's rule (common.hpp)
__device__ __forceinline__ float infer_drop1(float y, uint64_t seed, uint64_t step, uint64_t flat, uint32_t thr16,
                                             float scale) {
    if (thr16) {
        const uint64_t z = act_hash64(seed, step, flat >> 2);
        const bool keep = ((uint32_t)(z >> (16 * (flat & 3))) & 0xFFFFu) >= thr16;
        y = keep ? y * scale : 0.f;
    }
    return y;
}

// the graph's slices lie inside the arrays and inside the LDS image the host sized
__device__ __forceinline__ bool infer_slices_ok(const InferArgs& a, int64_t n0, int64_t e0, int64_t nn, int64_t mm) {
    return !(nn < 0 || mm < 0 || nn > a.cap_n || mm > a.cap_m || n0 < 0 || e0 < 0 || n0 + nn > a.N || e0 + mm > a.E);
}

// ---- where phase 1 takes the graph's m edges from.  The default: edge e is position e0 + e of the batch's arrays.  Another
// source (infer_whatif.hip: a base graph's slice less some positions, then edges of a second list) states the same four
// things; an edge it skips is neither staged nor counted, and keeps its number: the slots stay sorted by edge number.
struct InferBaseEdges {
    __device__ __forceinline__ float attr(const InferArgs& a, int64_t e0, int c, int D) const {
        return a.edge_attr[e0 * D + c];
    }
    // true: edge e is left out (its ends and rank were never written)
    __device__ __forceinline__ bool skips(int e) const { return false; }
    // the local (source j, target i) of edge e; false: skips(e)
    __device__ __forceinline__ bool ends_of(const InferArgs& a, int64_t n0, int64_t e0, int n, int e, int& j, int& i) const {
        j = (int)(a.ei[e0 + e] - n0);
        i = (int)(a.ei[a.E + e0 + e] - n0);
        return true;
    }
    // slots of the index: m edges, placed slots behind the scan (rp[n]) when some were skipped
    __device__ __forceinline__ int slots(int m, const int* rp, int n) const { return m; }
};

// ---- phases 1 and 2 of graph [n0, n0 + n) / [e0, e0 + m): returns 0 with x1, he, rp, key, ends in LDS, or the status bits
// of a breach (uniform over the workgroup; the image is then unusable and the caller writes NaN)
template <int H, int D, class Src = InferBaseEdges>
__device__ __forceinline__ int infer_phases12(const InferArgs& a, float* lds, const InferLds& L, int64_t n0, int64_t e0,
                                              int n, int m, const Src& src = Src()) {
    constexpr int NT = kInferThreads;
    constexpr int K = 2 * D;
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    float* x1 = lds + L.x1;
    float* ea = lds + L.ea;
    float* he = lds + L.he;
    float* alpha = lds + L.alpha;
    int* rank = reinterpret_cast<int*>(lds + L.alpha);
    unsigned int* ends = reinterpret_cast<unsigned int*>(lds + L.ends);
    int* key = reinterpret_cast<int*>(lds + L.key);
    int* cin = reinterpret_cast<int*>(lds + L.cin);
    int* rp = reinterpret_cast<int*>(lds + L.rp);
    int* lnid = reinterpret_cast<int*>(lds + L.lnid);

    // ---- phase 1: the graph's image and index ----
    if (tid == 0) s_bad = 0;
    int bad = 0;
    for (int t = tid; t < n; t += NT) {
        int64_t id = a.node_ids[n0 + t];
        if (id < 0 || id >= a.V) { bad |= 4; id = 0; }
        lnid[t] = (int)id;
        cin[t] = 0;
    }
    for (int c = tid; c < m * D; c += NT) ea[c] = src.attr(a, e0, c, D);
    __syncthreads();
    for (int e = tid; e < m; e += NT) {
        int j, i;
        if (!src.ends_of(a, n0, e0, n, e, j, i)) continue;
        if (i < 0 || i >= n || j < 0 || j >= n) { bad |= 1; continue; }      // (the workgroup leaves below: nothing reads it)
        ends[e] = ((unsigned int)j << 16) | (unsigned int)i;
        rank[e] = atomicAdd(&cin[i], 1);
        float f[D];
#pragma unroll
        for (int d = 0; d < D; ++d) f[d] = ea[e * D + d];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float h = a.b1[k];
#pragma unroll
            for (int d = 0; d < D; ++d) h = fmaf(a.w1[k * D + d], f[d], h);
            he[e * K + k] = h > 0.f ? h : 0.f;
        }
    }
    if (bad) atomicOr(&s_bad, bad);
    __syncthreads();
    if (s_bad) return s_bad;                                          // (uniform: every thread reads the same word)
    block_scan_into<NT>(cin, rp, n);
    for (int e = tid; e < m; e += NT)
        if (!src.skips(e)) key[rp[ends[e] & 0xFFFFu] + rank[e]] = e;
    __syncthreads();
    for (int r = tid; r < n; r += NT) sort_row_keys(key, rp[r], rp[r + 1]);
    __syncthreads();

    // ---- phase 2: TransformerConv + leaky_relu ----
    const int slots = src.slots(m, rp, n);
    for (int p = tid; p < slots; p += NT) {
        const int e = key[p];
        const unsigned int ji = ends[e];
        const int idi = lnid[ji & 0xFFFFu], idj = lnid[ji >> 16];
        float l = a.M[(int64_t)idi * a.ldm + idj];
#pragma unroll
        for (int d = 0; d < D; ++d) l = fmaf(a.P[(int64_t)idi * D + d], ea[e * D + d], l);
        alpha[p] = l;
    }
    __syncthreads();
    for (int r = tid; r < n; r += NT) {
        const int beg = rp[r], end = rp[r + 1];
        if (beg == end) continue;
        float mx = alpha[beg];
        for (int p = beg + 1; p < end; ++p) mx = fmaxf(mx, alpha[p]);
        float s = 0.f;
        for (int p = beg; p < end; ++p) {
            const float ex = expf(alpha[p] - mx);
            alpha[p] = ex;
            s += ex;
        }
        s += 1e-16f;
        for (int p = beg; p < end; ++p) alpha[p] = alpha[p] / s;
    }
    __syncthreads();
    {
        const float* tv = a.t4 + 2 * H;
        const float* ts = a.t4 + 3 * H;
        for (int idx = tid; idx < n * H; idx += NT) {
            const int r = idx / H, c = idx % H;
            const int beg = rp[r], end = rp[r + 1];
            float acc = 0.f;
            float aa[D];
#pragma unroll
            for (int d = 0; d < D; ++d) aa[d] = 0.f;
#pragma unroll 4
            for (int p = beg; p < end; ++p) {
                const int e = key[p];
                const float al = alpha[p];
                acc = fmaf(al, tv[(int64_t)lnid[ends[e] >> 16] * a.ld4 + c], acc);
#pragma unroll
                for (int d = 0; d < D; ++d) aa[d] = fmaf(al, ea[e * D + d], aa[d]);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) acc = fmaf(a.w_edge[c * D + d], aa[d], acc);
            acc += ts[(int64_t)lnid[r] * a.ld4 + c];
            x1[idx] = leaky(acc, a.slope_conv);
        }
    }
    __syncthreads();
    return 0;
}

// ---- a kernel's first steps on graph blockIdx.x: its slices as the arrays state them, checked, then phases 1 and 2.
// bad: 0, or the status bits of the breach (uniform); n and m fit an int when it is 0
struct InferGraph {
    int64_t n0, e0, n, m;
    int bad;
    InferLds L;                         // the variant's image for the launch's caps
};
template <int H, int D, InferVariant VAR>
__device__ __forceinline__ InferGraph infer_prologue(const InferArgs& a, float* lds) {
    const int64_t b = blockIdx.x;
    InferGraph g;
    g.n0 = a.node_ptr[b];
    g.e0 = a.edge_ptr[b];
    g.n = a.node_ptr[b + 1] - g.n0;
    g.m = a.edge_ptr[b + 1] - g.e0;
    // host-side size bound violated, or slices that do not lie inside the arrays: nothing else is touched
    g.bad = infer_slices_ok(a, g.n0, g.e0, g.n, g.m) ? 0 : 2;
    g.L = infer_lds(a.cap_n, a.cap_m, H, D, VAR);
    if (g.bad) return g;
    g.bad = infer_phases12<H, D>(a, lds, g.L, g.n0, g.e0, (int)g.n, (int)g.m);
    return g;
}

// a refused graph: flag the launch's status word, NaN in one output row
__device__ __forceinline__ void infer_refuse(const InferArgs& a, int bad, float* row) {
    const int tid = threadIdx.x;
    if (tid == 0 && a.status) atomicOr(a.status, bad);
    if (tid < a.O) row[tid] = __builtin_nanf("");
}

// ---- phases 3 and 4 on the first convolution's output `xin` [n, H] (LDS: x1 itself, or a sample's masked copy of it):
// writes orow[0 .. O).  Ends without a barrier; the LDS it wrote last (h1) is not written again before three barriers of
// the next call.  GRAD: *ybits gets one bit per row of this thread, (tile number) * RPT + u, set where conv2's
// pre-activation of (that row, column tid % H) is positive (at most 128 / R * RPT = 32 rows per thread), and part[c]
// (c < H) keeps the read-out's pre-activation s.
template <int H, int D, bool MC, bool GRAD = false>
__device__ __forceinline__ void infer_phases34(const InferArgs& a, float* lds, const InferLds& L, int n, const float* xin,
                                               float* orow, const InferDrop& dr, unsigned int* ybits = nullptr) {
    constexpr int NT = kInferThreads;
    constexpr int K = 2 * D, KT = (K + 2) * H;
    constexpr int RPT = infer_rpt(H), R = infer_tile_rows(H);
    const int tid = threadIdx.x;
    float* atile = lds + L.atile;
    const float* he = lds + L.he;
    const unsigned int* ends = reinterpret_cast<const unsigned int*>(lds + L.ends);
    const int* key = reinterpret_cast<const int*>(lds + L.key);
    const int* rp = reinterpret_cast<const int*>(lds + L.rp);
    float* part = lds + L.part;
    float* pooled = lds + L.pooled;
    float* h1 = lds + L.h1;

    // ---- phase 3: NNConv (mean) + leaky_relu, pooled on the fly ----
    const int o = tid % H, rg = tid / H;
    const float bias_o = a.bias2[o];
    float pool = 0.f;
    unsigned int ypos = 0;
    for (int r0 = 0; r0 < n; r0 += R) {
        for (int idx = tid; idx < R * (K + 1) * H; idx += NT) {
            const int rr = idx / ((K + 1) * H), rem = idx % ((K + 1) * H);
            const int k = rem / H, c = rem % H;
            const int r = r0 + rr;
            float v = 0.f;
            if (r < n) {
                const int beg = rp[r], end = rp[r + 1];
                for (int p = beg; p < end; ++p) {
                    const int e = key[p];
                    const float xj = xin[(ends[e] >> 16) * H + c];
                    v = k < K ? fmaf(he[e * K + k], xj, v) : v + xj;
                }
                if (end - beg > 1) v = v / (float)(end - beg);
            }
            atile[rr * KT + rem] = v;
        }
        for (int idx = tid; idx < R * H; idx += NT) {
            const int rr = idx / H, c = idx % H;
            atile[rr * KT + (K + 1) * H + c] = r0 + rr < n ? xin[(r0 + rr) * H + c] : 0.f;
        }
        __syncthreads();
        float acc[RPT];
#pragma unroll
        for (int u = 0; u < RPT; ++u) acc[u] = 0.f;
        const float* arow = atile + rg * RPT * KT;
        const float* wcol = a.wcat + o;
#pragma unroll 2
        for (int kk = 0; kk < KT; kk += 4) {
            const float w0 = wcol[(kk + 0) * H], w1 = wcol[(kk + 1) * H], w2 = wcol[(kk + 2) * H], w3 = wcol[(kk + 3) * H];
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const float4 av = *reinterpret_cast<const float4*>(arow + u * KT + kk);
                acc[u] = fmaf(av.x, w0, acc[u]);
                acc[u] = fmaf(av.y, w1, acc[u]);
                acc[u] = fmaf(av.z, w2, acc[u]);
                acc[u] = fmaf(av.w, w3, acc[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < RPT; ++u)
            if (r0 + rg * RPT + u < n) {
                float y = leaky(acc[u] + bias_o, a.slope_conv);
                if constexpr (GRAD) ypos |= (acc[u] + bias_o > 0.f ? 1u : 0u) << ((r0 / R) * RPT + u);
                if constexpr (MC)
                    y = infer_drop1(y, dr.seed_conv2, dr.step, (dr.row0 + (uint64_t)(r0 + rg * RPT + u)) * H + o, dr.thr_conv,
                                    dr.scale_conv);
                pool += y;
            }
        __syncthreads();
    }

    // ---- phase 4: mean pool and the read-out MLP ----
    part[tid] = pool;                                   // [rg][o]
    __syncthreads();
    if (tid < H) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < NT / H; ++g) s += part[g * H + tid];
        pooled[tid] = n > 0 ? s / (float)n : 0.f;
    }
    __syncthreads();
    if (tid < H) {
        float s = a.b0[tid];
        const float* w = a.w0 + tid * H;
#pragma unroll 8
        for (int c = 0; c < H; ++c) s = fmaf(w[c], pooled[c], s);
        float y = leaky(s, a.slope_head);
        if constexpr (MC) y = infer_drop1(y, dr.seed_head, dr.step, dr.graph * H + tid, dr.thr_head, dr.scale_head);
        h1[tid] = y;
        if constexpr (GRAD) part[tid] = s;              // (the row groups' shares were read before the last barrier)
    }
    if constexpr (GRAD) *ybits = ypos;
    __syncthreads();
    if (tid < a.O) {
        float s = a.b3[tid];
        const float* w = a.w3 + tid * H;
#pragma unroll 8
        for (int c = 0; c < H; ++c) s = fmaf(w[c], h1[c], s);
        orow[tid] = s;
    }
}

// ====================================================================== the host path of an entry point
// qot_topological_infer[_mc|_grad]_supported / _max_edges: one layout, one answer per variant
inline size_t infer_lds_bytes(InferVariant var, int n_max, int max_e, int H, int D) {
    return (size_t)infer_lds(n_max, max_e, H, D, var).words * 4;
}

inline int infer_supported(InferVariant var, int n_max, int max_e, int H, int D, int O) {
    const bool shape_ok = (H == 16 || H == 32 || H == 64) && D >= 1 && D <= 4 && O >= 1 && O <= 8;
    if (!shape_ok || n_max < 0 || n_max > kInferMaxN || max_e < 0) return 0;
    if (max_e > (1 << 20)) return 0;                   // (keeps the word count below 2^31)
    return infer_lds_bytes(var, n_max, max_e, H, D) <= kInferLdsMax ? 1 : 0;
}

inline int infer_max_edges(InferVariant var, int n_max, int H, int D) {
    if (!infer_supported(var, n_max, 0, H, D, 1)) return -1;
    int lo = 0, hi = 1 << 20;                          // the layout grows with max_e: largest accepted value by bisection
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (infer_supported(var, n_max, mid, H, D, 1)) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// An entry point checks in this order: infer_sizes_ok (else QOT_ERR_BADARG), its own arguments and its variant's
// infer_supported, then infer_make_args.
inline bool infer_sizes_ok(int64_t N, int64_t E, int64_t B, int n_max, int max_e, int V) {
    return !(N < 0 || E < 0 || B < 0 || n_max < 0 || max_e < 0 || V <= 0);
}

// The common arguments of an entry point, in the ABI's order (edge_dim is not needed here): QOT_OK with *a filled, or
// the error to return.  B == 0 is QOT_OK before any pointer is looked at; the caller launches nothing then.
inline int infer_make_args(InferArgs* a, const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                           const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B, int n_max,
                           int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P, int V,
                           const float* w_edge, const float* w1, const float* b1, const float* wcat, const float* bias2,
                           const float* w0, const float* b0, const float* w3, const float* b3, float slope_conv,
                           float slope_head, float* out, int H, int O, int32_t* status) {
    if (B == 0) return QOT_OK;
    if (B > 0x7fffffff) return QOT_ERR_UNSUPPORTED;
    if (ld4 < 4 * H || (ld4 & 3) || ldm < V) return QOT_ERR_BADARG;
    if (!node_ptr || !edge_ptr || !t4 || !M || !P || !w_edge || !w1 || !b1 || !wcat || !bias2 || !w0 || !b0 || !w3 || !b3 ||
        !out)
        return QOT_ERR_BADARG;
    if ((N > 0 && !node_ids) || (E > 0 && (!edge_index || !edge_attr))) return QOT_ERR_BADARG;
    *a = InferArgs{node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, B, n_max, max_e, t4, ld4, M, ldm, P, V,
                   w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, out, O, status};
    return QOT_OK;
}

// One launch of kernel instantiation Kernel, 256 threads per workgroup; more than 64 KB of dynamic LDS is allowed first
// (the attribute is per kernel and per device: every instantiation has its own table).
template <auto Kernel, class... Args>
inline int infer_launch(dim3 grid, size_t lds_bytes, hipStream_t stream, const Args&... args) {
    static size_t allowed[kMaxDevices];
    const int lrc = ensure_dyn_lds(reinterpret_cast<const void*>(Kernel), lds_bytes, allowed);
    if (lrc != QOT_OK) return lrc;
    Kernel<<<grid, kInferThreads, lds_bytes, stream>>>(args...);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

}  // namespace qot

// The (H, D) switch of the three entry points: returns infer_launch<KERNEL<H, D>>(grid, lds_bytes, stream, args...) from
// the calling function, QOT_ERR_UNSUPPORTED outside {16, 32, 64} x {1 .. 4}.
#define QOT_INFER_CASE(KERNEL, HH, DD, ...) \
    case HH * 8 + DD: return qot::infer_launch<KERNEL<HH, DD>>(__VA_ARGS__);
#define QOT_INFER_ROW(KERNEL, HH, ...) \
    QOT_INFER_CASE(KERNEL, HH, 1, __VA_ARGS__) QOT_INFER_CASE(KERNEL, HH, 2, __VA_ARGS__) \
    QOT_INFER_CASE(KERNEL, HH, 3, __VA_ARGS__) QOT_INFER_CASE(KERNEL, HH, 4, __VA_ARGS__)
#define QOT_INFER_DISPATCH(KERNEL, H, D, ...)                                                                       \
    switch ((H) * 8 + (D)) {                                                                                        \
        QOT_INFER_ROW(KERNEL, 16, __VA_ARGS__) QOT_INFER_ROW(KERNEL, 32, __VA_ARGS__) QOT_INFER_ROW(KERNEL, 64, __VA_ARGS__) \
        default: return QOT_ERR_UNSUPPORTED;                                                                        \
    }
