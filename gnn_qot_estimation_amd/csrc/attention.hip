// Attention weights of the two attention convolutions, as PyG's return_attention_weights=True returns them.  The forward
// kernels keep the softmax in whatever shape their form needs (CSR slot order, per-node statistics, nothing); these
// kernels recompute it from the rows the forward already built and write it in the caller's edge order.  Every edge has
// exactly one owner (its destination) and gets one plain store: no atomics, no zero fill, bitwise reproducible.
//
// TransformerConv (heads = 1), edge e = (j -> i), rs = 1/sqrt(H), W_e = lin_edge.weight [H, D]:
//     s_e = rs <q_i, k_j + W_e ea_e> = rs <q_i, k_j> + <u_i, ea_e>,   u_i = rs W_e^T q_i   ([D] per destination)
//     alpha_e = exp(s_e - max_i) / (sum_i + 1e-16)                    (oracle/sparse.py: segment_softmax)
// Lane layout of qot_tconv_edge_attr_grad: G = min(H/4, 16) lanes per destination (every sum inside a DPP row), a float4
// of channels per lane and step.  Pass 1 forms the logits, the online max and sum; lane k % G keeps the logit of the k-th
// in-edge in registers for k < KEEP G, so pass 2 writes those without touching the rows again; a destination with more
// in-edges recomputes the rest.
//
// GATConv (heads = 4), slot p of the self-looped index, j = col[p]:
//     s_p = leaky_relu(a_src[j] + a_dst[i], neg_slope),  alpha_p = softmax over i's slots   (oracle/sparse.py: GATConv)
// One thread per destination, the four heads as a float4.  Output row of slot p: pos[eid[p]] for an input edge (its
// index among the input's non-self-loop edges), num_kept + i for the inserted self loop (eid = -1): the order of
// remove_self_loops + add_self_loops (oracle.sparse.gat_edge_set).
#include "common.hpp"

namespace qot {

template <int H, int D>
__global__ __launch_bounds__(256) void tconv_attention_kernel(
    const float* __restrict__ qkvs, int ld, const int32_t* __restrict__ rowmap, const int32_t* __restrict__ col,
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ eid, const float* __restrict__ ea,
    const float* __restrict__ w_edge, float* __restrict__ alpha, int64_t N) {
    constexpr int G = H / 4 < 16 ? H / 4 : 16;            // lanes per destination: the sums stay inside a DPP row
    constexpr int T4 = H / (4 * G);                       // float4 channel groups per lane: c = 4 (lane + G t)
    constexpr int KEEP = 2;                               // logits kept per lane: in-edges k < KEEP G of a destination
    const int lane = threadIdx.x % G;
    const int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
    if (i >= N) return;                                   // whole groups only: the sums below stay inside a group
    const float rs = rsqrtf((float)H);
    const int64_t qrow = rowmap ? (int64_t)rowmap[i] : i;
    float4 qi[T4];
    float u[D];
#pragma unroll
    for (int d = 0; d < D; ++d) u[d] = 0.f;
#pragma unroll
    for (int t = 0; t < T4; ++t) {
        const int c = 4 * (lane + G * t);
        qi[t] = ld4(qkvs + qrow * ld + c);
        const float qr[4] = {qi[t].x, qi[t].y, qi[t].z, qi[t].w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int d = 0; d < D; ++d) u[d] = fmaf(w_edge[(c + r) * D + d], qr[r], u[d]);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) u[d] = group_sum<G>(u[d]) * rs;
    const int beg = rowptr[i], end = rowptr[i + 1];
    auto logit = [&](int p) {
        const int64_t jr = col[p];
        const int64_t e = eid[p];
        float qk = 0.f;
#pragma unroll
        for (int t = 0; t < T4; ++t) qk += dot4(qi[t], ld4(qkvs + jr * ld + H + 4 * (lane + G * t)));
        qk = group_sum<G>(qk);
        float su = 0.f;
        if (e >= 0) {
#pragma unroll
            for (int d = 0; d < D; ++d) su = fmaf(u[d], ea[e * D + d], su);
        }
        return fmaf(qk, rs, su);
    };
    float m = -INFINITY, l = 0.f, kept[KEEP];
#pragma unroll
    for (int t = 0; t < KEEP; ++t) kept[t] = 0.f;
    for (int p = beg; p < end; ++p) {
        const float s = logit(p);
        const int k = p - beg;
#pragma unroll
        for (int t = 0; t < KEEP; ++t)
            if (k == lane + G * t) kept[t] = s;
        const float mn = fmaxf(m, s);
        l = fmaf(l, __expf(m - mn), __expf(s - mn));
        m = mn;
    }
    // (each lane normalises with its own max and sum: the group sums may round differently per lane, so the logits a lane
    // writes and the statistics it divides by come from the same arithmetic)
    const float inv = 1.0f / (l + 1e-16f);
#pragma unroll
    for (int t = 0; t < KEEP; ++t) {
        const int p = beg + lane + G * t;
        if (p < end) {
            const int64_t e = eid[p];
            if (e >= 0) alpha[e] = __expf(kept[t] - m) * inv;
        }
    }
    for (int p = beg + KEEP * G; p < end; ++p) {
        const float s = logit(p);
        const int64_t e = eid[p];
        if (lane == 0 && e >= 0) alpha[e] = __expf(s - m) * inv;
    }
}

__device__ __forceinline__ float4 gat_logit(float4 a, float4 b, float ns) {
    const float s[4] = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
    float r[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) r[h] = s[h] > 0.f ? s[h] : s[h] * ns;
    return make_float4(r[0], r[1], r[2], r[3]);
}

__global__ __launch_bounds__(256) void gat_attention_kernel(
    const float4* __restrict__ a_src, const float4* __restrict__ a_dst, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const int32_t* __restrict__ eid, const int32_t* __restrict__ pos, int64_t num_kept,
    float4* __restrict__ alpha, int64_t N, float ns) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float4 ad = a_dst[i];
    const int beg = rowptr[i], end = rowptr[i + 1];
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, l[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = beg; p < end; ++p) {
        const float4 sv = gat_logit(a_src[col[p]], ad, ns);
        const float s[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const float mn = fmaxf(m[h], s[h]);
            l[h] = fmaf(l[h], __expf(m[h] - mn), __expf(s[h] - mn));
            m[h] = mn;
        }
    }
    float inv[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) inv[h] = 1.0f / (l[h] + 1e-16f);
    for (int p = beg; p < end; ++p) {
        const float4 sv = gat_logit(a_src[col[p]], ad, ns);
        const int64_t e = eid[p];
        const int64_t r = e >= 0 ? (int64_t)pos[e] : num_kept + i;
        alpha[r] = make_float4(__expf(sv.x - m[0]) * inv[0], __expf(sv.y - m[1]) * inv[1], __expf(sv.z - m[2]) * inv[2],
                               __expf(sv.w - m[3]) * inv[3]);
    }
}

}  // namespace qot

using namespace qot;

extern "C" int qot_tconv_attention(const float* qkvs, int ld, const int32_t* rowmap, const int32_t* col,
                                   const int32_t* rowptr, const int32_t* eid, const float* edge_attr, const float* w_edge,
                                   float* alpha, int64_t N, int H, int D, qot_stream_t stream) {
    if (N < 0 || H <= 0 || ld < 4 * H || (ld & 3)) return QOT_ERR_BADARG;
    if (N == 0) return QOT_OK;
    if (!qkvs || !col || !rowptr || !eid || !edge_attr || !w_edge || !alpha || ((uintptr_t)qkvs & 15))
        return QOT_ERR_BADARG;
    QOT_DISPATCH_H(H, QOT_DISPATCH_D(D, {
        constexpr int G = kH / 4 < 16 ? kH / 4 : 16;
        tconv_attention_kernel<kH, kD><<<grid_for(N, 256 / G), 256, 0, (hipStream_t)stream>>>(
            qkvs, ld, rowmap, col, rowptr, eid, edge_attr, w_edge, alpha, N);
    }));
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

extern "C" int qot_gat_attention(const float* a_src, const float* a_dst, const int32_t* rowptr, const int32_t* col,
                                 const int32_t* eid, const int32_t* edge_pos, int64_t num_kept, float* alpha, int64_t N,
                                 int heads, float neg_slope, qot_stream_t stream) {
    if (N < 0 || num_kept < 0) return QOT_ERR_BADARG;
    if (heads != 4) return QOT_ERR_UNSUPPORTED;
    if (N == 0) return QOT_OK;
    if (!a_src || !a_dst || !rowptr || !col || !eid || !alpha || (num_kept > 0 && !edge_pos)) return QOT_ERR_BADARG;
    if (((uintptr_t)a_src | (uintptr_t)a_dst | (uintptr_t)alpha) & 15) return QOT_ERR_BADARG;
    gat_attention_kernel<<<grid_for(N, 256), 256, 0, (hipStream_t)stream>>>(
        (const float4*)a_src, (const float4*)a_dst, rowptr, col, eid, edge_pos, num_kept, (float4*)alpha, N, neg_slope);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
