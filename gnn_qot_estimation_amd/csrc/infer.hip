// Single-launch inference: the whole eval-mode TopologicalGNN forward (topological_training/models.py:49-64, dropout off)
// of a block-diagonal batch, ONE workgroup of 256 threads per graph.
//
// Everything a graph needs is small (n <= 128 nodes, a few hundred edges): its destination-sorted index, its edge features,
// the edge MLP's hidden layer and the first convolution's output all live in LDS; what depends on the parameters only --
// the projected table [q|k|v|skip], the score matrix M / P of the graph form (tconv_graph_dev.hpp) and the NNConv operand
// Wcat -- is read from global memory, where it is shared by every graph of the launch (L2-resident: at H = 64 Wcat is 164 KB
// and would not fit LDS beside the graph).
//
// Phases of a workgroup (a __syncthreads between them):
//   1  index: node ids, edge features -> LDS; in-degree histogram with LDS atomics, block scan, placement, per-row sort by
//      edge id (graph_prep_dev.hpp's pieces; the sort makes the slot order, and so every sum below, independent of the
//      atomics' order); the edge MLP's first layer h_e = relu(w1 ea_e + b1) per edge
//   2  TransformerConv: logit of every slot = M[id_i, id_j] + <P[id_i], ea_e> (slot-parallel: one L2 round trip), softmax
//      per destination (one thread per row, LDS only, PyG's max-subtraction and + 1e-16), then per (row, channel)
//      x1 = leaky_relu(sum alpha v[id_j] + We (sum alpha ea) + skip[id_i])
//   3  NNConv (mean) in tiles of R destination rows: A[r] = [mean_e h_e[k] x1[j] (k < 2D) | mean_e x1[j] | x1[r]] in LDS,
//      then A Wcat with RPT rows per thread (each Wcat element read once per tile and used RPT times from a register), + bias,
//      leaky_relu; the thread adds its rows to its share of the pool sum as they are finished
//   4  mean pool (the row groups' shares summed in a fixed order), Linear -> leaky_relu -> Linear, one row of `out`
// Plain fp32 FMA: per graph the products are ~4 MFLOP at H = 64 and far less at the reference's width, the launch exists
// for the latency of ONE graph or a handful, and fp32 accumulation in a fixed order gives the bitwise batch independence
// the interface promises without the split-bf16 bookkeeping of nnconv_mfma.hip.
#include "graph_prep_dev.hpp"

namespace qot {

constexpr int kInferThreads = 256;
constexpr int kInferMaxN = 128;                       // local node ids are packed 16 + 16 bits; one softmax thread per row
constexpr size_t kInferLdsMax = 160 * 1024 - 2048;    // the CU's LDS less the static words of the block scan and flags

__host__ __device__ constexpr int infer_rpt(int H) { return H == 64 ? 4 : 2; }                 // rows per thread of A Wcat
__host__ __device__ constexpr int infer_tile_rows(int H) { return infer_rpt(H) * (kInferThreads / H); }
__host__ __device__ constexpr int infer_pad4(int v) { return (v + 3) & ~3; }

// 4-byte word offsets of the LDS image for graphs of at most cap_n nodes / cap_m edges: the ONE statement of the budget
// (the kernel, the entry point and qot_topological_infer_supported all read it)
struct InferLds {
    int atile, x1, ea, he, alpha, ends, key, cin, rp, lnid, part, pooled, h1, words;
};
__host__ __device__ inline InferLds infer_lds(int cap_n, int cap_m, int H, int D) {
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

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : slope * v; }

template <int H, int D>
__global__ __launch_bounds__(kInferThreads) void topological_infer_kernel(const InferArgs a) {
    constexpr int NT = kInferThreads;
    constexpr int K = 2 * D, KT = (K + 2) * H;
    constexpr int RPT = infer_rpt(H), R = infer_tile_rows(H);
    extern __shared__ float4 infer_lds_raw[];
    __shared__ int s_bad;
    float* lds = reinterpret_cast<float*>(infer_lds_raw);
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    float* orow = a.out + b * a.O;

    const int64_t n0 = a.node_ptr[b], e0 = a.edge_ptr[b];
    const int64_t nn = a.node_ptr[b + 1] - n0, mm = a.edge_ptr[b + 1] - e0;
    // host-side size bound violated, or slices that do not lie inside the arrays: flag, write NaN, touch nothing else
    if (nn < 0 || mm < 0 || nn > a.cap_n || mm > a.cap_m || n0 < 0 || e0 < 0 || n0 + nn > a.N || e0 + mm > a.E) {
        if (tid == 0 && a.status) atomicOr(a.status, 2);
        if (tid < a.O) orow[tid] = __builtin_nanf("");
        return;
    }
    const int n = (int)nn, m = (int)mm;
    const InferLds L = infer_lds(a.cap_n, a.cap_m, H, D);
    float* atile = lds + L.atile;
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
    float* part = lds + L.part;
    float* pooled = lds + L.pooled;
    float* h1 = lds + L.h1;

    // ---- phase 1: the graph's image and index ----
    if (tid == 0) s_bad = 0;
    int bad = 0;
    for (int t = tid; t < n; t += NT) {
        int64_t id = a.node_ids[n0 + t];
        if (id < 0 || id >= a.V) { bad |= 4; id = 0; }
        lnid[t] = (int)id;
        cin[t] = 0;
    }
    for (int c = tid; c < m * D; c += NT) ea[c] = a.edge_attr[e0 * D + c];
    __syncthreads();
    for (int e = tid; e < m; e += NT) {
        int j = (int)(a.ei[e0 + e] - n0), i = (int)(a.ei[a.E + e0 + e] - n0);
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
    if (s_bad) {                                                      // (uniform: every thread reads the same word)
        if (tid == 0 && a.status) atomicOr(a.status, s_bad);
        if (tid < a.O) orow[tid] = __builtin_nanf("");
        return;
    }
    block_scan_into<NT>(cin, rp, n);
    for (int e = tid; e < m; e += NT) key[rp[ends[e] & 0xFFFFu] + rank[e]] = e;
    __syncthreads();
    for (int r = tid; r < n; r += NT) sort_row_keys(key, rp[r], rp[r + 1]);
    __syncthreads();

    // ---- phase 2: TransformerConv + leaky_relu ----
    for (int p = tid; p < m; p += NT) {
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

    // ---- phase 3: NNConv (mean) + leaky_relu, pooled on the fly ----
    const int o = tid % H, rg = tid / H;
    const float bias_o = a.bias2[o];
    float pool = 0.f;
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
                    const float xj = x1[(ends[e] >> 16) * H + c];
                    v = k < K ? fmaf(he[e * K + k], xj, v) : v + xj;
                }
                if (end - beg > 1) v = v / (float)(end - beg);
            }
            atile[rr * KT + rem] = v;
        }
        for (int idx = tid; idx < R * H; idx += NT) {
            const int rr = idx / H, c = idx % H;
            atile[rr * KT + (K + 1) * H + c] = r0 + rr < n ? x1[(r0 + rr) * H + c] : 0.f;
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
            if (r0 + rg * RPT + u < n) pool += leaky(acc[u] + bias_o, a.slope_conv);
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
        h1[tid] = leaky(s, a.slope_head);
    }
    __syncthreads();
    if (tid < a.O) {
        float s = a.b3[tid];
        const float* w = a.w3 + tid * H;
#pragma unroll 8
        for (int c = 0; c < H; ++c) s = fmaf(w[c], h1[c], s);
        orow[tid] = s;
    }
}

static bool infer_shape_ok(int H, int D, int O) {
    return (H == 16 || H == 32 || H == 64) && D >= 1 && D <= 4 && O >= 1 && O <= 8;
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_supported(int n_max, int max_e, int H, int D, int O) {
    if (!infer_shape_ok(H, D, O) || n_max < 0 || n_max > kInferMaxN || max_e < 0) return 0;
    if (max_e > (1 << 20)) return 0;                   // (keeps the word count below 2^31)
    return (size_t)infer_lds(n_max, max_e, H, D).words * 4 <= kInferLdsMax ? 1 : 0;
}

extern "C" int qot_topological_infer_max_edges(int n_max, int H, int D) {
    if (!qot_topological_infer_supported(n_max, 0, H, D, 1)) return -1;
    int lo = 0, hi = 1 << 20;                          // the layout grows with max_e: largest accepted value by bisection
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (qot_topological_infer_supported(n_max, mid, H, D, 1)) lo = mid; else hi = mid - 1;
    }
    return lo;
}

extern "C" int qot_topological_infer(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                     const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B,
                                     int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm, const float* P,
                                     int V, const float* w_edge, const float* w1, const float* b1, const float* wcat,
                                     const float* bias2, const float* w0, const float* b0, const float* w3, const float* b3,
                                     float slope_conv, float slope_head, float* out, int H, int D, int O, int32_t* status,
                                     qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N < 0 || E < 0 || B < 0 || n_max < 0 || max_e < 0 || V <= 0) return QOT_ERR_BADARG;
    if (!qot_topological_infer_supported(n_max, max_e, H, D, O)) return QOT_ERR_UNSUPPORTED;
    if (B == 0) return QOT_OK;
    if (B > 0x7fffffff) return QOT_ERR_UNSUPPORTED;
    if (ld4 < 4 * H || (ld4 & 3) || ldm < V) return QOT_ERR_BADARG;
    if (!node_ptr || !edge_ptr || !t4 || !M || !P || !w_edge || !w1 || !b1 || !wcat || !bias2 || !w0 || !b0 || !w3 || !b3 ||
        !out)
        return QOT_ERR_BADARG;
    if ((N > 0 && !node_ids) || (E > 0 && (!edge_index || !edge_attr))) return QOT_ERR_BADARG;
    const InferArgs a{node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, B, n_max, max_e, t4, ld4, M, ldm, P, V,
                      w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, out, O, status};
    const size_t lds = (size_t)infer_lds(n_max, max_e, H, D).words * 4;
#define QOT_INFER_CASE(HH, DD)                                                                                         \
    case HH * 8 + DD: {                                                                                                \
        static size_t allowed[kMaxDevices];                                                                            \
        const int lrc = ensure_dyn_lds(reinterpret_cast<const void*>(topological_infer_kernel<HH, DD>), lds, allowed); \
        if (lrc != QOT_OK) return lrc;                                                                                 \
        topological_infer_kernel<HH, DD><<<(int)B, kInferThreads, lds, stream>>>(a);                                   \
    } break;
    switch (H * 8 + D) {
        QOT_INFER_CASE(16, 1) QOT_INFER_CASE(16, 2) QOT_INFER_CASE(16, 3) QOT_INFER_CASE(16, 4)
        QOT_INFER_CASE(32, 1) QOT_INFER_CASE(32, 2) QOT_INFER_CASE(32, 3) QOT_INFER_CASE(32, 4)
        QOT_INFER_CASE(64, 1) QOT_INFER_CASE(64, 2) QOT_INFER_CASE(64, 3) QOT_INFER_CASE(64, 4)
        default: return QOT_ERR_UNSUPPORTED;
    }
#undef QOT_INFER_CASE
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
