// Gradients wrt the EDGE FEATURES of TopologicalGNN's two convolutions (edge_attr.grad).  The training step never asks for
// them; these kernels run in addition to whichever parameter backward a form picks and recompute what they need from the
// tensors the forward saved and from grad_out, so the parameter gradients stay the same code.  Every edge has exactly one
// owner (the lane group of its destination) and is written with plain stores: bitwise reproducible, no zero fill.
//
// TransformerConv (heads = 1), edge e = (j -> i), rs = 1/sqrt(H), W_e = lin_edge.weight [H, D], g_i = grad at the conv
// output (the fused leaky_relu + dropout undone, mask regenerated as qot_act_bwd does):
//     s_e  = rs <q_i, k_j> + <u_i, ea_e>,          u_i = rs W_e^T q_i        ([D] per destination)
//     da_e = <g_i, v_j>    + <w_i, ea_e>,          w_i = W_e^T g_i           ([D] per destination)
//     alpha = softmax_i(s),  delta_i = sum_e alpha_e da_e,  ds_e = alpha_e (da_e - delta_i)
//     grad ea_e = ds_e u_i + alpha_e w_i
// One group of G = min(H/4, 16) lanes per destination (sums inside a DPP row), float4 channel groups per lane.  Two passes over the in-edges:
// the first forms max, sum and sum exp(s - max) da online, the second the per-edge result.  The logits are recomputed
// rather than read from the forward, whose forms leave different things behind (stats, alpha in slot order, nothing).
//
// NNConv (aggr = mean), r_e = W1 ea_e + b1 ([K], K = 2D), GA_i[k, a] = sum_o g_i[o] W2[a*Hout + o, k] (caller GEMM):
//     dh_e[k] = invdeg_i <GA_i[k, :], x_j>,        grad ea_e = W1^T ((r_e > 0) * dh_e)
// The per-edge quantity qot_nnconv_bwd_edge reduces into gw1 / gb1, written per edge instead (same lane layout: H/4 lanes
// per destination, GA row in registers).
#include "common.hpp"

namespace qot {

template <int H, int D>
__global__ __launch_bounds__(256) void tconv_edge_attr_grad_kernel(
    const float* __restrict__ g, const float* __restrict__ y, ActParams act, const float* __restrict__ qkvs, int ld,
    const int32_t* __restrict__ rowmap, const int32_t* __restrict__ col, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ eid, const float* __restrict__ ea, const float* __restrict__ w_edge,
    float* __restrict__ grad_ea, int64_t N) {
    constexpr int G = H / 4 < 16 ? H / 4 : 16;            // lanes per destination: the sums stay inside a DPP row
    constexpr int T4 = H / (4 * G);                       // float4 channel groups per lane: c = 4 (lane + G t)
    const int lane = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (i >= N) return;                                   // whole groups only: the sums below stay inside a group
    const float rs = rsqrtf((float)H);
    const uint64_t step = act.thr16 ? (uint64_t)act.step[0] : 0;
    const int64_t qrow = rowmap ? (int64_t)rowmap[i] : i;
    float4 gi[T4], qi[T4];
    float u[D], w[D];
#pragma unroll
    for (int d = 0; d < D; ++d) u[d] = w[d] = 0.f;
#pragma unroll
    for (int t = 0; t < T4; ++t) {
        const int c = 4 * (lane + G * t);
        const int64_t flat = i * H + c;
        float4 gv = ld4(g + flat);
        if (act.enabled) {                                // back through dropout(leaky_relu(.)), as qot_act_bwd
            const float4 yv = ld4(y + flat);
            const uint64_t z = act.thr16 ? act_hash64(act.seed, step, (uint64_t)flat >> 2) : 0;
            float gr[4] = {gv.x, gv.y, gv.z, gv.w};
            const float yr[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool keep = act.thr16 ? (((uint32_t)(z >> (16 * r)) & 0xFFFFu) >= act.thr16) : true;
                gr[r] = gr[r] * (keep ? act.keep_scale : 0.f) * (yr[r] > 0.f ? 1.0f : act.slope);
            }
            gv = make_float4(gr[0], gr[1], gr[2], gr[3]);
        }
        gi[t] = gv;
        qi[t] = ld4(qkvs + qrow * ld + c);
        const float gr[4] = {gv.x, gv.y, gv.z, gv.w};
        const float qr[4] = {qi[t].x, qi[t].y, qi[t].z, qi[t].w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float we = w_edge[(c + r) * D + d];
                u[d] = fmaf(we, qr[r], u[d]);
                w[d] = fmaf(we, gr[r], w[d]);
            }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        u[d] = group_sum<G>(u[d]) * rs;
        w[d] = group_sum<G>(w[d]);
    }
    const int beg = rowptr[i], end = rowptr[i + 1];
    // logit and dalpha of slot p (identical in both passes: same loads, same order)
    auto edge = [&](int p, float& s, float& da) {
        const int64_t jr = col[p];
        const int64_t e = eid[p];
        float qk = 0.f, gv = 0.f;
#pragma unroll
        for (int t = 0; t < T4; ++t) {
            const int c = 4 * (lane + G * t);
            qk += dot4(qi[t], ld4(qkvs + jr * ld + H + c));
            gv += dot4(gi[t], ld4(qkvs + jr * ld + 2 * H + c));
        }
        qk = group_sum<G>(qk);
        gv = group_sum<G>(gv);
        float su = 0.f, sw = 0.f;
        if (e >= 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float a = ea[e * D + d];
                su = fmaf(u[d], a, su);
                sw = fmaf(w[d], a, sw);
            }
        }
        s = fmaf(qk, rs, su);
        da = gv + sw;
    };
    float m = -INFINITY, l = 0.f, acc = 0.f;
    for (int p = beg; p < end; ++p) {
        float s, da;
        edge(p, s, da);
        const float mn = fmaxf(m, s);
        const float sc = __expf(m - mn), ex = __expf(s - mn);
        l = fmaf(l, sc, ex);
        acc = fmaf(acc, sc, ex * da);
        m = mn;
    }
    const float inv = 1.0f / (l + 1e-16f);
    const float delta = acc * inv;
    for (int p = beg; p < end; ++p) {
        float s, da;
        edge(p, s, da);
        const int64_t e = eid[p];
        const float alpha = __expf(s - m) * inv;
        const float ds = alpha * (da - delta);
        // lane d writes component d (at H = 16 a group has 4 lanes: they loop over D)
        for (int d = lane; d < D; d += G) {
            float r = 0.f;
#pragma unroll
            for (int dd = 0; dd < D; ++dd)
                if (d == dd) r = fmaf(ds, u[dd], alpha * w[dd]);
            if (e >= 0) grad_ea[e * D + d] = r;
        }
    }
}

template <int H, int D>
__global__ __launch_bounds__(256) void nnconv_edge_attr_grad_kernel(
    const float* __restrict__ GA, int ldga, const float* __restrict__ x, int ldx, const float* __restrict__ ea,
    const float* __restrict__ w1, const float* __restrict__ b1, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const int32_t* __restrict__ eid, const float* __restrict__ invdeg,
    float* __restrict__ grad_ea, int64_t N) {
    constexpr int K = 2 * D;
    constexpr int TPR = H / 4;
    constexpr int RPB = 256 / TPR;
    const int sub = threadIdx.x % TPR;
    const int64_t i = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
    if (i >= N) return;                                   // whole rows only: the shuffles stay inside a row
    const int c0 = 4 * sub;
    float w[K][D], b[K];
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
        b[kk] = b1[kk];
#pragma unroll
        for (int d = 0; d < D; ++d) w[kk][d] = w1[kk * D + d];
    }
    float4 ga[K];
#pragma unroll
    for (int kk = 0; kk < K; ++kk) ga[kk] = ld4(GA + i * ldga + kk * H + c0);
    const float sc = invdeg[i];
    const int beg = rowptr[i], end = rowptr[i + 1];
    for (int p = beg; p < end; ++p) {
        const int64_t j = col[p];
        const int64_t e = eid[p];
        const float4 xj = ld4(x + j * ldx + c0);
        float dk[K];
#pragma unroll
        for (int kk = 0; kk < K; ++kk) dk[kk] = dot4(ga[kk], xj);
#pragma unroll
        for (int o = TPR / 2; o > 0; o >>= 1)
#pragma unroll
            for (int kk = 0; kk < K; ++kk) dk[kk] += __shfl_xor(dk[kk], o);
        if (sub == 0 && e >= 0) {
            float ee[D], out[D];
#pragma unroll
            for (int d = 0; d < D; ++d) {
                ee[d] = ea[e * D + d];
                out[d] = 0.f;
            }
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
                float pre = b[kk];
#pragma unroll
                for (int d = 0; d < D; ++d) pre = fmaf(w[kk][d], ee[d], pre);
                const float gh = (pre > 0.f) ? dk[kk] * sc : 0.f;
#pragma unroll
                for (int d = 0; d < D; ++d) out[d] = fmaf(w[kk][d], gh, out[d]);
            }
#pragma unroll
            for (int d = 0; d < D; ++d) grad_ea[e * D + d] = out[d];
        }
    }
}

}  // namespace qot

using namespace qot;

extern "C" int qot_tconv_edge_attr_grad(const float* grad_out, const float* y_act, float act_slope, float act_p,
                                        uint64_t act_seed, const int64_t* act_step, const float* qkvs, int ld,
                                        const int32_t* rowmap, const int32_t* col, const int32_t* rowptr,
                                        const int32_t* eid, const float* edge_attr, const float* w_edge,
                                        float* grad_edge_attr, int64_t N, int H, int D, qot_stream_t stream) {
    if (N < 0 || H <= 0 || ld < 4 * H || (ld & 3)) return QOT_ERR_BADARG;
    if (N == 0) return QOT_OK;
    if (!grad_out || !qkvs || !col || !rowptr || !eid || !edge_attr || !w_edge || !grad_edge_attr) return QOT_ERR_BADARG;
    const ActParams act = make_act(y_act != nullptr, act_slope, act_p, act_seed, act_step);
    QOT_DISPATCH_H(H, QOT_DISPATCH_D(D, {
        constexpr int G = kH / 4 < 16 ? kH / 4 : 16;
        tconv_edge_attr_grad_kernel<kH, kD><<<grid_for(N, 256 / G), 256, 0, (hipStream_t)stream>>>(
            grad_out, y_act, act, qkvs, ld, rowmap, col, rowptr, eid, edge_attr, w_edge, grad_edge_attr, N);
    }));
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

extern "C" int qot_nnconv_edge_attr_grad(const float* GA, int ld_ga, const float* x, int ld_x, const float* edge_attr,
                                         const float* w1, const float* b1, const int32_t* rowptr, const int32_t* col,
                                         const int32_t* eid, const float* invdeg, float* grad_edge_attr, int64_t N, int H,
                                         int D, qot_stream_t stream) {
    if (N < 0 || !rowptr) return QOT_ERR_BADARG;
    if (N == 0) return QOT_OK;
    if (!GA || !x || !edge_attr || !w1 || !b1 || !col || !eid || !invdeg || !grad_edge_attr || (ld_ga & 3) || (ld_x & 3))
        return QOT_ERR_BADARG;
    if (ld_ga < 2 * D * H || ld_x < H) return QOT_ERR_BADARG;
    QOT_DISPATCH_H(H, QOT_DISPATCH_D(D, {
        constexpr int RPB = 256 / (kH / 4);
        nnconv_edge_attr_grad_kernel<kH, kD><<<grid_for(N, RPB), 256, 0, (hipStream_t)stream>>>(
            GA, ld_ga, x, ld_x, edge_attr, w1, b1, rowptr, col, eid, invdeg, grad_edge_attr, N);
    }));
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
