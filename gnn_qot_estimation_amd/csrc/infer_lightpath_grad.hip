// LightpathPredictor.sensitivity: the eval-mode forward of a LUT row (infer_lightpath_dev.hpp's lp_row, the row of
// qot_lightpath_infer bit for bit) followed, in the same wavefront, by its Jacobian wrt the node features of the row's
// one-hop in-neighbourhood, for Q requested outputs.  One workgroup of 64 threads per row.
//
// With out_i[h] = W_h u_h, u_h = sum_e alpha_{e,h} x_{j_e}, alpha = softmax over the messages and the self loop of
// lk_{e,h} = leaky_relu(raw_{e,h}), raw_{e,h} = s_h . x_j + d_h . x_i:
//   A  per output q (o = outputs[q]), one pass back through the head:
//        g_h1[c] = w3[o, c] * leaky'(pre[c])                                  lanes stride c
//        g_y[k]  = sum_c w0[c, k] g_h1[c], c rising                           lanes stride k (coalesced rows of w0)
//        g_v[k]  = g_y[k] * [y[k] > 0] * bn_w[k] / sqrt(bn_var[k] + eps)
//        g_u[q][h][f] = sum_c W[hC + c, f] g_v[hC + c], c rising              lane (h, f)
//      then gud[q][h] = g_u[q][h] . u_h
//   B  third scan of the edge slice: a message's lane recomputes its logits with the forward's arithmetic,
//        alpha_{e,h} = exp(lk - max) / (den + 1e-16),   b_{e,h} = alpha_{e,h} (g_u[h] . x_j - gud[h]) leaky'(raw_{e,h})
//        jac_edge[q, e, f] = sum_h (alpha_{e,h} g_u[q][h][f] + b_{e,h} s_h[f]), h rising
//      and leaves b in LDS; lane (q, h) adds the chunk's b ONE AFTER THE OTHER in slice order (the ballot walk from the
//      lowest bit, chunks in order): dsum[q][h], the weight of d_h in the destination's own derivative
//   C  the self loop, last as in the forward:
//        jac_self[q, r, f] = sum_h (alpha_s g_u[q][h][f] + b_s (s_h[f] + d_h[f]) + dsum[q][h] d_h[f]), h rising
// leaky' is the forward's own branch (v > 0 ? 1 : slope), relu' is [y > 0]: torch's rule at 0.  No atomics on floats:
// an edge has one destination, so every jac_edge / alpha_edge element has at most one writer, and every sum one order.
// Edges that are no message into a computed row are never written: the caller zero-fills jac_edge and alpha_edge.
#include "infer_lightpath_dev.hpp"

namespace qot {
namespace {

struct LpGradArgs {
    const int32_t* outputs; int Q;
    float* jac_self; float* jac_edge; float* alpha_self; float* alpha_edge;
};

constexpr int kLpGu = kLpHeads * kLpMaxF;   // floats of one output's g_u

struct LpGradLds {
    LpKeep keep;
    float gu[kLpMaxO * kLpGu];          // g_u[q][h][f]
    float gud[kLpMaxO * kLpHeads];      // g_u[q][h] . u_h
    float dsum[kLpMaxO * kLpHeads];     // sum over the messages of b_{e,h}
};
// L.part is free between the forward and the end of the kernel: phase A keeps g_v [4C] and g_h1 [C] there, phase B a
// chunk's b [Q * 4][64]
static_assert(kLpTile * kLpPs >= kLpHeads * kLpMaxC + kLpMaxC, "g_v and g_h1 live in LpLds::part");
static_assert(kLpTile * kLpPs >= kLpMaxO * kLpHeads * kWave, "a chunk's b lives in LpLds::part");

// a row that is not computed: NaN in its jac_self rows and its alpha_self row (its out row is NaN already)
__device__ __forceinline__ void lpg_nan_row(const LpArgs& a, const LpGradArgs& ga, int64_t r, int64_t rows, int lane) {
    const float nan = __builtin_nanf("");
    if (lane < a.F)
        for (int q = 0; q < ga.Q; ++q) ga.jac_self[((int64_t)q * rows + r) * a.F + lane] = nan;
    if (ga.alpha_self && lane < kLpHeads) ga.alpha_self[r * kLpHeads + lane] = nan;
}

// ... and, for a flagged row whose graph's edge slice [e0, e0 + m) lies inside the edge array, NaN in that slice
__device__ __forceinline__ void lpg_nan_slice(const LpArgs& a, const LpGradArgs& ga, int64_t e0, int64_t m, int lane) {
    const float nan = __builtin_nanf("");
    for (int q = 0; q < ga.Q; ++q) {
        float* je = ga.jac_edge + ((int64_t)q * a.E + e0) * a.F;
        for (int64_t k = lane; k < m * a.F; k += kWave) je[k] = nan;
    }
    if (ga.alpha_edge)
        for (int64_t k = lane; k < m * kLpHeads; k += kWave) ga.alpha_edge[e0 * kLpHeads + k] = nan;
}

__global__ __launch_bounds__(kWave) void lightpath_infer_grad_kernel(const LpArgs a, const LpGradArgs ga) {
    __shared__ LpLds L;
    __shared__ LpGradLds G;
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x, rows = gridDim.x;
    float* orow = a.out + r * a.O;
    int64_t i = 0, g = 0;
    if (!lp_locate(a, r, orow, lane, i, g)) {
        lpg_nan_row(a, ga, r, rows, lane);
        return;
    }
    LpRowRegs R;
    const int rc = lp_row<true>(a, L, &G.keep, i, g, orow, lane, R);
    if (rc != 0) {                                             // (wave-uniform)
        lpg_nan_row(a, ga, r, rows, lane);
        if (rc == 2) lpg_nan_slice(a, ga, R.e0, R.m, lane);
        return;
    }
    const int F = a.F, C = a.C, Q = ga.Q;
    const int h = lane / F, f = lane - h * F;                  // lanes below 4F own the pair (h, f)
    __syncthreads();                                           // (K.pre, and L.part is free again)

    // ---- phase A: the head's adjoint per requested output -> g_u, gud ----
    float* gv = L.part;
    float* gh1 = L.part + kLpHeads * kLpMaxC;
    for (int q = 0; q < Q; ++q) {
        const int o = ga.outputs[q];
        const bool o_ok = o >= 0 && o < a.O;                   // (the caller checks the contents; nothing is read through a bad one)
        for (int c = lane; c < C; c += kWave)
            gh1[c] = o_ok ? a.w3[(int64_t)o * C + c] * (G.keep.pre[c] > 0.f ? 1.f : a.slope_head) : __builtin_nanf("");
        __syncthreads();
        for (int k = lane; k < kLpHeads * C; k += kWave) {
            const float* wc = a.w0 + k;
            float acc = 0.f;
            for (int c = 0; c < C; ++c) acc = fmaf(wc[(int64_t)c * kLpHeads * C], gh1[c], acc);
            gv[k] = L.y[k] > 0.f ? acc * (a.bn_w[k] / sqrtf(a.bn_var[k] + a.eps)) : 0.f;
        }
        __syncthreads();
        if (lane < kLpHeads * F) {
            const float* w = a.w + (int64_t)h * C * F + f;
            const float* gvh = gv + h * C;
            float acc = 0.f;
            for (int c = 0; c < C; ++c) acc = fmaf(w[c * F], gvh[c], acc);
            G.gu[q * kLpGu + h * kLpMaxF + f] = acc;
        }
        __syncthreads();
    }
    if (lane < kLpHeads * Q) {                                 // lane (q, h)
        const float* gu = G.gu + (lane >> 2) * kLpGu + (lane & 3) * kLpMaxF;
        const float* uh = L.u + (lane & 3) * kLpMaxF;
        float acc = 0.f;
        for (int t = 0; t < F; ++t) acc = fmaf(gu[t], uh[t], acc);
        G.gud[lane] = acc;
    }
    __syncthreads();

    // ---- phase B: third scan of the edge slice ----
    const float sl = a.slope_att;
    float den[kLpHeads];
#pragma unroll
    for (int hh = 0; hh < kLpHeads; ++hh) den[hh] = G.keep.den[hh] + 1e-16f;
    float* bq = L.part;                                        // a chunk's b [q * 4 + h][lane]
    float dsum = 0.f;
    for (int64_t base = 0; base < R.m; base += kWave) {
        int64_t src = 0;
        const bool msg = lp_edge(a, R.e0, R.m, base + lane, R.n0, R.n1, i, src) == 1;
        if (msg) {
            const int64_t e = R.e0 + base + lane;
            float* xs = L.xs + lane * kLpXs;                   // (this lane's own row: no barrier needed)
            float l[kLpHeads] = {};
            lp_dot4(L.s, a.x + src * F, F, l, xs);
            float al[kLpHeads], dk[kLpHeads];
#pragma unroll
            for (int hh = 0; hh < kLpHeads; ++hh) {
                const float raw = l[hh] + R.adst[hh];
                al[hh] = expf(lp_leaky(raw, sl) - R.mx[hh]) / den[hh];
                dk[hh] = raw > 0.f ? 1.f : sl;
                if (ga.alpha_edge) ga.alpha_edge[e * kLpHeads + hh] = al[hh];
            }
            for (int q = 0; q < Q; ++q) {
                const float* gu = G.gu + q * kLpGu;
                float dt[kLpHeads] = {}, b[kLpHeads];
                lp_dot4(gu, xs, F, dt);
#pragma unroll
                for (int hh = 0; hh < kLpHeads; ++hh) {
                    b[hh] = al[hh] * (dt[hh] - G.gud[q * kLpHeads + hh]) * dk[hh];
                    bq[(q * kLpHeads + hh) * kWave + lane] = b[hh];
                }
                float* je = ga.jac_edge + ((int64_t)q * a.E + e) * F;
                for (int t = 0; t < F; ++t) {
                    float v = 0.f;
#pragma unroll
                    for (int hh = 0; hh < kLpHeads; ++hh) {
                        v = fmaf(al[hh], gu[hh * kLpMaxF + t], v);
                        v = fmaf(b[hh], L.s[hh * kLpMaxF + t], v);
                    }
                    je[t] = v;
                }
            }
        }
        unsigned long long mask = __ballot(msg);
        __syncthreads();
        if (lane < kLpHeads * Q) {
            while (mask) {                                     // (wave-uniform: the chunk's messages by rising offset)
                const int k = __builtin_ctzll(mask);
                mask &= mask - 1;
                dsum += bq[lane * kWave + k];
            }
        }
        __syncthreads();
    }
    if (lane < kLpHeads * Q) G.dsum[lane] = dsum;
    __syncthreads();

    // ---- phase C: the self loop and the destination's own row ----
    float as[kLpHeads], dks[kLpHeads];
#pragma unroll
    for (int hh = 0; hh < kLpHeads; ++hh) {
        as[hh] = L.ps[hh] / den[hh];
        dks[hh] = R.rself[hh] > 0.f ? 1.f : sl;
        if (ga.alpha_self && lane == hh) ga.alpha_self[r * kLpHeads + hh] = as[hh];
    }
    for (int q = 0; q < Q; ++q) {
        const float* gu = G.gu + q * kLpGu;
        float dt[kLpHeads] = {};
        lp_dot4(gu, L.xi, F, dt);
        if (lane < F) {
            float v = 0.f;
#pragma unroll
            for (int hh = 0; hh < kLpHeads; ++hh) {
                const float bs = as[hh] * (dt[hh] - G.gud[q * kLpHeads + hh]) * dks[hh];
                v = fmaf(as[hh], gu[hh * kLpMaxF + lane], v);
                v = fmaf(bs, L.s[hh * kLpMaxF + lane] + L.d[hh * kLpMaxF + lane], v);
                v = fmaf(G.dsum[q * kLpHeads + hh], L.d[hh * kLpMaxF + lane], v);
            }
            ga.jac_self[((int64_t)q * rows + r) * F + lane] = v;
        }
    }
}

}  // namespace
}  // namespace qot

using namespace qot;

extern "C" int qot_lightpath_infer_grad(const float* x, const int64_t* edge_index, const int64_t* batch,
                                        const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* lut_idx, int64_t L,
                                        int64_t N, int64_t E, int64_t B, const float* w, const float* att_src,
                                        const float* att_dst, const float* conv_bias, float slope_att, const float* bn_weight,
                                        const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps,
                                        const float* w0, const float* b0, const float* w3, const float* b3, float slope_head,
                                        float* out, int32_t* count, int F, int C, int O, int heads, int lut_col,
                                        int32_t* status, const int32_t* outputs, int Q, float* jac_self, float* jac_edge,
                                        float* alpha_self, float* alpha_edge, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LpArgs a;
    int64_t rows = 0;
    const int rc = lp_args(x, edge_index, batch, node_ptr, edge_ptr, lut_idx, L, N, E, B, w, att_src, att_dst, conv_bias,
                           slope_att, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, w0, b0, w3, b3, slope_head, out, count, F, C,
                           O, heads, lut_col, status, Q, a, rows);
    if (rc != QOT_OK || rows == 0) return rc;
    if (!outputs || !jac_self || (E > 0 && !jac_edge)) return QOT_ERR_BADARG;
    const LpGradArgs ga{outputs, Q, jac_self, jac_edge, alpha_self, alpha_edge};
    lightpath_infer_grad_kernel<<<(int)rows, kWave, 0, stream>>>(a, ga);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
