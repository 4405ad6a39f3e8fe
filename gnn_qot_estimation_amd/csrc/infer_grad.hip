// Per-link sensitivity in one launch: out [B, O] of the eval-mode TopologicalGNN forward AND, for Q requested outputs,
// jac[q, e, :] = d out[graph(e), outputs[q]] / d edge_attr[e, :].  ONE workgroup of 256 threads per graph.
//
// The forward half is infer.hip's, the same device functions with the same sums (infer_dev.hpp): `out` is the eval
// kernel's row bit for bit.  It leaves in LDS what an adjoint to the edge features needs -- the index, ea, he, alpha, x1
// -- and keeps the branches of the leaky_relus: conv1's is the sign of x1 (the slope is positive), conv2's one bit per
// element in a register of the thread that finished that element, the read-out's pre-activation in `part`.
//
// Back pass of output o (no parameter or embedding gradient is formed; notation of DESIGN.md 4.16):
//   1  g_s = W3[o] (.) leaky'(s);  g_pool = W0^T g_s / n
//   per tile of R destination rows, as the forward walks them:
//   2  g_y = g_pool (.) leaky'(y) -> LDS [R, H];  U = g_y Wcat^T -> LDS [R, (K + 2) H]  (one thread per column: its Wcat
//      row in registers, the g_y rows broadcast from LDS)
//   3  per (slot, k): dh_e[k] = <U_i^k, x1_j> / deg_i
//   4  g_x1[j] += (sum_k h_e[k] U_i^k + U_i^K) / deg_i and g_x1[i] += U_i^{K+1}.  NO atomics: element (j, a) of g_x1 is
//      owned by thread (a = tid % H, g = tid / H) with j % G == g, G = 256 / H; the owner walks the tile's slots in slot
//      order and takes the edges whose source is its own, then adds the root term of its rows.  One owner, a fixed order.
//   after the tiles:
//   5  g_z = g_x1 (.) leaky'(x1)
//   6  per slot: da_e = <g_z[i], v[id_j] + W_edge f_e>, w_i = W_edge^T g_z[i], G2_e = W1^T ((h_e > 0) (.) dh_e); the slot
//      keeps da_e and alpha_e w_i + G2_e.  Per row: delta_i = sum_e alpha_e da_e in slot order.
//   7  jac[q, e] = alpha_e (da_e - delta_i) P[id_i] + (alpha_e w_i + G2_e): one plain store per element.
// Every index the back pass uses was checked by phase 1; a flagged graph writes NaN to its out row, its jac slices and
// its alpha slice through the same uniform path.
#include "infer_dev.hpp"

namespace qot {

struct InferGradArgs {
    const int32_t* outputs; int Q;
    float* jac;                         // [Q, E, D]
    float* alpha;                       // [E] in edge order, or null
};

template <int H, int D>
__global__ __launch_bounds__(kInferThreads) void topological_infer_grad_kernel(const InferArgs a, const InferGradArgs ga) {
    constexpr int NT = kInferThreads;
    constexpr int K = 2 * D, KT = (K + 2) * H;
    constexpr int RPT = infer_rpt(H), R = infer_tile_rows(H);
    constexpr int G = NT / H;
    extern __shared__ float4 infer_grad_lds_raw[];
    float* lds = reinterpret_cast<float*>(infer_grad_lds_raw);
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    float* orow = a.out + b * a.O;

    const InferGraph g = infer_prologue<H, D, kInferGrad>(a, lds);
    const InferLds& L = g.L;
    const int64_t e0 = g.e0;
    if (g.bad) {                                        // flag, NaN in all three outputs of the graph, nothing else
        infer_refuse(a, g.bad, orow);
        // (slices that leave the arrays: the part of the edge range that lies inside them)
        const int64_t lo = e0 < 0 ? 0 : e0, hi = g.m < 0 ? lo : (e0 + g.m > a.E ? a.E : e0 + g.m);
        for (int64_t e = lo + tid; e < hi; e += NT) {
            if (ga.alpha) ga.alpha[e] = __builtin_nanf("");
            for (int q = 0; q < ga.Q; ++q)
                for (int d = 0; d < D; ++d) ga.jac[((int64_t)q * a.E + e) * D + d] = __builtin_nanf("");
        }
        return;
    }
    const int n = (int)g.n, m = (int)g.m;
    unsigned int ybits = 0;
    infer_phases34<H, D, false, true>(a, lds, L, n, lds + L.x1, orow, InferDrop{}, &ybits);
    if (m == 0) return;                                 // (uniform) no edge: nothing to differentiate

    float* atile = lds + L.atile;
    const float* x1 = lds + L.x1;
    const float* ea = lds + L.ea;
    const float* he = lds + L.he;
    const float* alpha = lds + L.alpha;
    const unsigned int* ends = reinterpret_cast<const unsigned int*>(lds + L.ends);
    const int* key = reinterpret_cast<const int*>(lds + L.key);
    const int* rp = reinterpret_cast<const int*>(lds + L.rp);
    const int* lnid = reinterpret_cast<const int*>(lds + L.lnid);
    float* delta = lds + L.cin;                         // (the in-degree histogram is dead after phase 1)
    const float* spre = lds + L.part;
    float* gx1 = lds + L.gx1;
    float* gy = lds + L.gy;
    float* dh = lds + L.dh;
    float* gs = lds + L.gs;
    float* gpool = lds + L.gpool;
    const int col = tid % H, rg = tid / H;

    if (ga.alpha)
        for (int p = tid; p < m; p += NT) ga.alpha[e0 + key[p]] = alpha[p];
    __syncthreads();                                    // the forward's last reads of h1 / part are done

    for (int q = 0; q < ga.Q; ++q) {
        const int o = ga.outputs[q];                    // (the host checked 0 <= o < O)
        float* jq = ga.jac + ((int64_t)q * a.E + e0) * D;
        // ---- 1: the read-out and the pool ----
        if (tid < H) gs[tid] = a.w3[o * H + tid] * (spre[tid] > 0.f ? 1.f : a.slope_head);
        for (int idx = tid; idx < n * H; idx += NT) gx1[idx] = 0.f;
        __syncthreads();
        if (tid < H) {
            float s = 0.f;
#pragma unroll 8
            for (int r = 0; r < H; ++r) s = fmaf(a.w0[r * H + tid], gs[r], s);
            gpool[tid] = s / (float)n;
        }
        __syncthreads();
        const float gp = gpool[col];

        for (int r0 = 0; r0 < n; r0 += R) {
            const int rows = n - r0 < R ? n - r0 : R;
            // ---- 2: the tile of g_y, then U = g_y Wcat^T ----
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const int rr = rg * RPT + u;
                const bool pos = (ybits >> ((r0 / R) * RPT + u)) & 1u;
                gy[rr * H + col] = rr < rows ? (pos ? gp : a.slope_conv * gp) : 0.f;
            }
            __syncthreads();                            // (also: the previous tile's readers of U are done)
            for (int c = tid; c < KT; c += NT) {
                float4 w[H / 4];
                const float4* wrow = reinterpret_cast<const float4*>(a.wcat + (int64_t)c * H);
#pragma unroll
                for (int v = 0; v < H / 4; ++v) w[v] = wrow[v];
                for (int rr = 0; rr < rows; ++rr) {
                    const float4* g4 = reinterpret_cast<const float4*>(gy + rr * H);
                    float acc = 0.f;
#pragma unroll
                    for (int v = 0; v < H / 4; ++v) {
                        const float4 gv = g4[v];
                        acc = fmaf(gv.x, w[v].x, acc);
                        acc = fmaf(gv.y, w[v].y, acc);
                        acc = fmaf(gv.z, w[v].z, acc);
                        acc = fmaf(gv.w, w[v].w, acc);
                    }
                    atile[rr * KT + c] = acc;
                }
            }
            __syncthreads();
            const int pbeg = rp[r0], pend = rp[r0 + rows];
            // ---- 3: the adjoint of the edge MLP's hidden layer ----
            for (int it = tid; it < (pend - pbeg) * K; it += NT) {
                const int p = pbeg + it / K, k = it % K;
                const int e = key[p];
                const unsigned int ji = ends[e];
                const int i = (int)(ji & 0xFFFFu), j = (int)(ji >> 16);
                const float4* u4 = reinterpret_cast<const float4*>(atile + (i - r0) * KT + k * H);
                const float4* x4 = reinterpret_cast<const float4*>(x1 + j * H);
                float acc = 0.f;
#pragma unroll 4
                for (int v = 0; v < H / 4; ++v) {
                    const float4 uv = u4[v], xv = x4[v];
                    acc = fmaf(uv.x, xv.x, acc);
                    acc = fmaf(uv.y, xv.y, acc);
                    acc = fmaf(uv.z, xv.z, acc);
                    acc = fmaf(uv.w, xv.w, acc);
                }
                const int deg = rp[i + 1] - rp[i];
                dh[e * K + k] = deg > 1 ? acc / (float)deg : acc;
            }
            // ---- 4: the scatter into g_x1, every element by its owner in slot order ----
            for (int p = pbeg; p < pend; ++p) {
                const int e = key[p];
                const unsigned int ji = ends[e];
                const int j = (int)(ji >> 16);
                if (j % G != rg) continue;
                const int i = (int)(ji & 0xFFFFu);
                const float* urow = atile + (i - r0) * KT;
                float v = urow[K * H + col];
#pragma unroll
                for (int k = 0; k < K; ++k) v = fmaf(he[e * K + k], urow[k * H + col], v);
                const int deg = rp[i + 1] - rp[i];
                gx1[j * H + col] += deg > 1 ? v / (float)deg : v;
            }
            for (int rr = rg; rr < rows; rr += G)       // (r0 is a multiple of G: row r0 + rr is this thread's)
                gx1[(r0 + rr) * H + col] += atile[rr * KT + (K + 1) * H + col];
            // (no barrier here: the next tile writes gy, which nothing above reads, and meets one before it writes U)
        }
        __syncthreads();
        // ---- 5: through conv1's leaky_relu ----
        for (int idx = tid; idx < n * H; idx += NT) gx1[idx] = x1[idx] > 0.f ? gx1[idx] : a.slope_conv * gx1[idx];
        __syncthreads();
        // ---- 6: TransformerConv, per slot ----
        {
            const float* tv = a.t4 + 2 * H;
            for (int p = tid; p < m; p += NT) {
                const int e = key[p];
                const unsigned int ji = ends[e];
                const int i = (int)(ji & 0xFFFFu), j = (int)(ji >> 16);
                const float* gz = gx1 + i * H;
                const float* tvj = tv + (int64_t)lnid[j] * a.ld4;
                float f[D], w[D];
#pragma unroll
                for (int d = 0; d < D; ++d) { f[d] = ea[e * D + d]; w[d] = 0.f; }
                float da = 0.f;
#pragma unroll 4
                for (int c = 0; c < H; ++c) {
                    const float g = gz[c];
                    float t = tvj[c];
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        const float we = a.w_edge[c * D + d];
                        t = fmaf(we, f[d], t);
                        w[d] = fmaf(we, g, w[d]);
                    }
                    da = fmaf(g, t, da);
                }
                float g2[D];
#pragma unroll
                for (int d = 0; d < D; ++d) g2[d] = 0.f;
#pragma unroll 2
                for (int k = 0; k < K; ++k) {                 // (not fully unrolled: K D uniform weights would spill SGPRs)
                    const float dk = he[e * K + k] > 0.f ? dh[e * K + k] : 0.f;
#pragma unroll
                    for (int d = 0; d < D; ++d) g2[d] = fmaf(a.w1[k * D + d], dk, g2[d]);
                }
                const float al = alpha[p];
#pragma unroll
                for (int d = 0; d < D; ++d) dh[e * K + d] = fmaf(al, w[d], g2[d]);
                dh[e * K + D] = da;                     // (K = 2 D > D)
            }
        }
        __syncthreads();
        for (int r = tid; r < n; r += NT) {
            float s = 0.f;
            for (int p = rp[r]; p < rp[r + 1]; ++p) s = fmaf(alpha[p], dh[key[p] * K + D], s);
            delta[r] = s;
        }
        __syncthreads();
        // ---- 7: one store per element of the graph's slice of jac[q] ----
        for (int p = tid; p < m; p += NT) {
            const int e = key[p];
            const int i = (int)(ends[e] & 0xFFFFu);
            const float ds = alpha[p] * (dh[e * K + D] - delta[i]);
            const float* Pi = a.P + (int64_t)lnid[i] * D;
#pragma unroll
            for (int d = 0; d < D; ++d) jq[(int64_t)e * D + d] = fmaf(ds, Pi[d], dh[e * K + d]);
        }
        __syncthreads();                                // dh, gx1, delta are rewritten by the next pass
    }
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_grad_supported(int n_max, int max_e, int H, int D, int O) {
    return infer_supported(kInferGrad, n_max, max_e, H, D, O);
}

extern "C" int qot_topological_infer_grad_max_edges(int n_max, int H, int D) {
    return infer_max_edges(kInferGrad, n_max, H, D);
}

extern "C" int qot_topological_infer_grad(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                          const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B,
                                          int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm,
                                          const float* P, int V, const float* w_edge, const float* w1, const float* b1,
                                          const float* wcat, const float* bias2, const float* w0, const float* b0,
                                          const float* w3, const float* b3, float slope_conv, float slope_head, float* out,
                                          int H, int D, int O, int32_t* status, const int32_t* outputs, int Q, float* jac,
                                          float* alpha, qot_stream_t stream_) {
    if (!infer_sizes_ok(N, E, B, n_max, max_e, V)) return QOT_ERR_BADARG;
    if (!infer_supported(kInferGrad, n_max, max_e, H, D, O)) return QOT_ERR_UNSUPPORTED;
    if (Q < 1 || Q > O) return QOT_ERR_UNSUPPORTED;
    if (!(slope_conv > 0.f)) return QOT_ERR_UNSUPPORTED;    // conv1's branch is read off the sign of its OUTPUT
    if (!outputs || (E > 0 && !jac)) return QOT_ERR_BADARG;
    InferArgs a;
    const int rc = infer_make_args(&a, node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, B, n_max, max_e, t4, ld4, M,
                                   ldm, P, V, w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, out, H, O,
                                   status);
    if (rc != QOT_OK || B == 0) return rc;
    const InferGradArgs ga{outputs, Q, jac, alpha};
    QOT_INFER_DISPATCH(topological_infer_grad_kernel, H, D, dim3((unsigned)B), infer_lds_bytes(kInferGrad, n_max, max_e, H, D),
                       (hipStream_t)stream_, a, ga)
}
