// grad of the edge MLP's first layer at H = 64 (nnconv_gradh64_kernel), split off nnconv_mfma.hip so that THIS kernel can be
// compiled with -mllvm -amdgpu-sched-strategy=max-ilp (Makefile): measured 87 -> 82 us at cfg2, while the same strategy costs
// the adjoint kernel 2.6 us and spills the forward one (r03; tools/experiments/r03_sched_bench.sh).
#include "common.hpp"
#include "mfma_tile.hpp"
#include "nnconv_finalize_dev.hpp"
#include "reduce_dev.hpp"
#include "split_bf16.hpp"

namespace qot {

// ---------------------------------------------------------------------------------------------
// grad of the edge MLP's first layer (nn.0.weight / nn.0.bias), fused.
//   dL/dh_e[k] = invdeg_i * < GA_i[k,:], x_j > ,  GA_i[k,a] = sum_o g_i[o] * W2[a*64+o, k]
// The unfused path materialises GA ([N, 512] fp32, a 6.7 GFLOP library GEMM measured at 291 us)
// and re-reads it per destination.  Here, per tile of 32 destinations:
//   1. g rows -> LDS in MFMA fragment order (fp32 form: 8 KB of fp32; split form: split once per tile by the thread
//      that loaded them, three bf16 planes in the bf16 MFMA's A-fragment order, 12.4 KB)
//   2. GA tile [32 x 512] = g_tile @ Bm on the matrix cores (4 waves x 4 column blocks,
//      128 v_mfma_f32_32x32x2_f32 per wave), accumulators -> LDS row-major (66 KB, padded rows)
//   3. the tile's edges, staged in LDS at the top of the tile, dealt evenly over the 32 lane groups (r03; r02
//      gave every destination a lane group: its GA rows stayed in registers, but a group walked its edges in
//      batches of dependent loads and idled behind the longest row of its wave): per edge the destination's GA
//      rows come from LDS, 8 partial dots, transpose-reduced over the 8 lanes (7 DPP moves) so lane s ends with
//      k = s; relu mask recomputed from the edge features; the source rows are requested before phase 2.
// Per-lane accumulators of (gw1[k,:], gb1[k]) live across the persistent loop; block partials
// are summed in a fixed order afterwards (bitwise reproducible, no float atomics).
constexpr int kGaLd = 516;    // padded GA row (floats): rows 4 banks apart

constexpr int kGhCap = 256;   // edges of a tile staged in LDS by the grad-h kernel (the rest is read directly)

// SPLIT: the GA products on the bf16 matrix pipe (split_bf16.hpp): Bs = Wk^T pre-split into three bf16 planes, each
// [nb][16-deep step][lane], bs_planes u32x4 apart.
// PRESPLIT (split form only): the g tile goes to LDS as three bf16 planes, each [step][lane] u32x4 -- every value split once
// per tile, an A fragment = three ds_read_b128.  false: the fp32 tile of the fp32 form, every fragment split after its
// read, by every wave for each of its blocks (16 times per value; kept for comparison, QOT_GRADH_SPLIT_AFTER_READ=1).
// The plane layout (kGhPlStep, kGhPlLd) and its store are split_bf16.hpp's: the forward kernel shares them.
//
// Hosted sums: the launch is n_main + (tail) workgroups.  The first n_main are the persistent workgroups of the tile walk; the
// walk's last round is ragged (3200 tiles over 512 workgroups at cfg2: a quarter of the slots runs a 7th tile), and workgroups
// are handed out in index order, so the tail workgroups start in the slots the others free, while that round finishes.  A tail
// workgroup runs one virtual block of a hosted job (nnconv_finalize_dev.hpp: HostedTable) and returns: streaming fixed-order
// sums of partials that EARLIER launches wrote, so neither when nor where it runs changes a bit of any result.  No workgroup
// waits for another.  Its 4 KB of scratch is the GA tile's storage: the kernel's static LDS is what it was.
__device__ __forceinline__ void gradh_hosted_tail(const HostedTable& t, int vt, float* __restrict__ scratch) {
    int r = 0;
    while (r + 1 < t.n && vt >= t.first[r + 1]) ++r;                    // uniform; <= QOT_MAX_ROLES scalar steps
    const HostedJob& jb = t.job[r];
    const int vb = vt - t.first[r];
    if (jb.kind == kHostedSumRows) sum_rows_body(jb.src, jb.dst, jb.a, jb.b, jb.c, jb.flag, vb, scratch);
    else if (jb.kind == kHostedSlabSum64) nnconv_slab_sum64_body(jb.src, (int)jb.a, jb.b, jb.dst, jb.flag, vb);
}

template <int D, bool SPLIT = false, bool PRESPLIT = false>
__global__ __launch_bounds__(256, 2) void nnconv_gradh64_kernel(
    const HostedTable hosted_by_value, int n_main,      // first, so that the table lies at offset 0 of the argument segment
    const float* __restrict__ g, int ldg, const float* __restrict__ x, int ldx, const float* __restrict__ ea,
    const float* __restrict__ w1, const float* __restrict__ b1, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const int32_t* __restrict__ eidx, const float* __restrict__ invdeg,
    const float* __restrict__ Bp, float* __restrict__ partials, int64_t N, const u32x4* __restrict__ Bs = nullptr,
    int64_t bs_planes = 0) {
    constexpr int K = 2 * D;
    static_assert(K <= 8, "one k per lane of the 8-lane group");
    constexpr int NB = K * 2;               // 32-column blocks of GA (K*64/32)
    constexpr int NBW = NB / 4;             // per wave
    constexpr int EPG = kGhCap / 32;        // staged edge slots per lane group
    constexpr int EPF = 5;                  // ... of which the source rows are requested in front of the MFMA phase
    static_assert(SPLIT || !PRESPLIT, "the planes are the split form's");
    // g tile (x 1/deg): fragment-grouped fp32, or the three bf16 planes
    __shared__ __attribute__((aligned(16))) float Gt[PRESPLIT ? 3 * kGhPlLd * 4 : 8 * 2 * 32 * 4];
    __shared__ __attribute__((aligned(16))) float GAt[32 * (K * 64 + 4)];  // GA tile, row-major padded
    // the tile's first kGhCap edges, staged once per tile: source row, local destination row, edge features
    __shared__ int sj[kGhCap], sr[kGhCap];
    // PRESPLIT: the staged edge features live in the planes' storage (written after the MFMA phase, when the planes are
    // dead, read in the dot phase): 12.4 + 4 KB next to the GA tile would leave no room for two workgroups per CU at D = 4
    __shared__ __attribute__((aligned(16))) float sea_own[PRESPLIT ? 4 : kGhCap * D];
    static_assert(!PRESPLIT || kGhCap * D <= 3 * kGhPlLd * 4, "sea fits the planes");
    float* const sea = PRESPLIT ? Gt : sea_own;
    __shared__ int rp_l[36];
    constexpr int LDGA = K * 64 + 4;
    float4* Gt4 = reinterpret_cast<float4*>(Gt);
    if ((int)blockIdx.x >= n_main) {
        // a tail workgroup: the table is read where it lies, in the kernel-argument segment (first argument: offset 0),
        // through a pointer, as roles_kernel reads its own
#if defined(__HIP_DEVICE_COMPILE__)
        typedef const HostedTable __attribute__((address_space(4))) * KernargTable;
        gradh_hosted_tail(*(const HostedTable*)(KernargTable)__builtin_amdgcn_kernarg_segment_ptr(), (int)blockIdx.x - n_main, GAt);
#else
        gradh_hosted_tail(hosted_by_value, (int)blockIdx.x - n_main, GAt);
#endif
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r31 = lane & 31, hi = lane >> 5;
    const int sub = threadIdx.x & 7, il = threadIdx.x >> 3;
    const int c0 = 8 * sub;
    const int64_t ntiles = (N + 31) / 32;

    // lane-owned slice of the first edge-MLP layer: row k = sub
    float wrow[D], brow, aw[D], ab = 0.f;
    brow = (sub < K) ? b1[sub] : 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) { wrow[d] = (sub < K) ? w1[sub * D + d] : 0.f; aw[d] = 0.f; }

    // One edge: dots of the destination's GA rows (LDS; 1/deg is in the g tile) with the source row's 8 channels of this
    // lane, transposed over the 8 lanes of the group (lane k ends with the total of k), relu mask from the edge features.
    auto edge = [&](int r, const float4& x0, const float4& x1, const float (&ee)[D]) {
        float pd[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float a = 0.f;
            if (k < K) {
                const float4 u0 = *reinterpret_cast<const float4*>(&GAt[r * LDGA + k * 64 + c0]);
                const float4 u1 = *reinterpret_cast<const float4*>(&GAt[r * LDGA + k * 64 + c0 + 4]);
                float a0 = u0.x * x0.x, a1 = u0.y * x0.y;        // two interleaved partial dots
                a0 = fmaf(u0.z, x0.z, a0); a1 = fmaf(u0.w, x0.w, a1);
                a0 = fmaf(u1.x, x1.x, a0); a1 = fmaf(u1.y, x1.y, a1);
                a0 = fmaf(u1.z, x1.z, a0); a1 = fmaf(u1.w, x1.w, a1);
                a = a0 + a1;
            }
            pd[k] = a;
        }
        float t4[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float keep = (sub & 4) ? pd[m + 4] : pd[m];
            const float send = (sub & 4) ? pd[m] : pd[m + 4];
            t4[m] = keep + dpp_move<0x141>(send);      // partner 7 - sub (bit 2 differs)
        }
        float t2[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const float keep = (sub & 2) ? t4[m + 2] : t4[m];
            const float send = (sub & 2) ? t4[m] : t4[m + 2];
            t2[m] = keep + dpp_move<0x4E>(send);       // partner sub ^ 2
        }
        const float keep = (sub & 1) ? t2[1] : t2[0];
        const float send = (sub & 1) ? t2[0] : t2[1];
        const float tot = keep + dpp_move<0xB1>(send);   // partner sub ^ 1; k = sub
        float pre = brow;
#pragma unroll
        for (int d = 0; d < D; ++d) pre = fmaf(wrow[d], ee[d], pre);
        const float gh = (pre > 0.f && sub < K) ? tot : 0.f;
        ab += gh;
#pragma unroll
        for (int d = 0; d < D; ++d) aw[d] = fmaf(gh, ee[d], aw[d]);
    };

#pragma unroll 1
    for (int64_t it = 0;; ++it) {
        const int64_t tile = xcd_tile(it, ntiles, (unsigned)n_main);
        if (tile < 0) break;
        const int64_t tile0 = tile * 32;
        const int64_t i = tile0 + il;
        const int64_t tend = (tile0 + 32 < N) ? tile0 + 32 : N;
        // Weight fragments of this wave's first GA block are requested before anything else of the tile, those of block
        // t + 1 before the MFMAs of block t (two buffers).
        // split form: the wave's NBW * 4 steps (16 deep each) as one sequence, fragments requested SL steps ahead into a
        // ring of SL + 1 (48 VGPRs; two whole split blocks in flight, as the fp32 form keeps, spilled)
        constexpr int SL = 3;            // SL + 1 = 4 steps per block: ring slots are compile-time in a rolled block loop
        float4 bf[2][8];                    // (dead in the split form, bsp in the fp32 one)
        Bf3 bsp[SL + 1];
        const u32x4* bsw = Bs + (int64_t)(wave * NBW) * 4 * 64 + lane;
        if constexpr (SPLIT) {
#pragma unroll
            for (int s = 0; s < SL; ++s) bsp[s] = load_split_b(bsw + s * 64, bs_planes);
        } else {
            const float4* bp = reinterpret_cast<const float4*>(Bp) + (int64_t)(wave * NBW) * 8 * 64 + lane;
#pragma unroll
            for (int gq = 0; gq < 8; ++gq) bf[0][gq] = bp[gq * 64];
        }
        // 1. the tile's edges, staged (r03): every thread one edge (coalesced col / edge id, then its features), every
        // destination marks its slots; the per-edge work is dealt EVENLY over the 32 lane groups afterwards (slot s ->
        // group s % 32) whatever the degrees -- its results are sums over all lanes, no group has to own a destination.
        const int e_t0 = rowptr[tile0], e_t1 = rowptr[tend];
        const int nt = e_t1 - e_t0;
        const int ncap = nt < kGhCap ? nt : kGhCap;
        int64_t my_e = 0;
        if ((int)threadIdx.x < ncap) {
            sj[threadIdx.x] = col[e_t0 + threadIdx.x];
            my_e = eidx[e_t0 + threadIdx.x];
        }
        if (threadIdx.x < 33) rp_l[threadIdx.x] = rowptr[tile0 + threadIdx.x < N ? tile0 + threadIdx.x : N];
        // g tile x 1/deg -> LDS (fragment-grouped, group index = sub)
        {
            float4 g0 = f4zero(), g1 = f4zero();
            if (i < N) {
                const float sc = invdeg[i];
                const int beg = rowptr[i], end = rowptr[i + 1];
                g0 = scale4(sc, ld4(g + i * ldg + c0)); g1 = scale4(sc, ld4(g + i * ldg + c0 + 4));
                const int lim = e_t0 + ncap;
                for (int p = beg + sub; p < end && p < lim; p += 8) sr[p - e_t0] = il;
            }
            if constexpr (PRESPLIT) {
                // This thread's 8 channels are group sub = 2 s + q of row il, split once (split_bf16.hpp: store_split_planes);
                // rows of absent nodes are zero planes.
                store_split_planes(Gt, sub, il, g0, g1);
            } else {
                // (store_fragment_grouped spelled out: through the helper the slot's v_or3_b32 takes its operands in the other order)
                Gt4[at4_slot(sub, 0, il)] = make_float4(g0.x, g0.z, g1.x, g1.z);
                Gt4[at4_slot(sub, 1, il)] = make_float4(g0.y, g0.w, g1.y, g1.w);
            }
        }
        float my_ea[D];
#pragma unroll
        for (int d = 0; d < D; ++d) my_ea[d] = ((int)threadIdx.x < ncap) ? ea[my_e * D + d] : 0.f;
        lds_barrier();
        // the group's first source rows are requested before the MFMA phase and used after it
        const int mine = (ncap - il + 31) / 32;           // staged slots il, il + 32, ... of this lane group
        float4 xr0[EPF], xr1[EPF];
#pragma unroll
        for (int t = 0; t < EPF; ++t) {
            if (t < mine) {
                const float* xp = x + (int64_t)sj[il + 32 * t] * ldx + c0;
                xr0[t] = ld4(xp); xr1[t] = ld4(xp + 4);
            }
        }
        // 2. GA tile on the matrix cores
        if (SPLIT) {
            // A fragments: three ds_read_b128 of the planes per step (PRESPLIT), or the fp32 tile's two, split after the read
            // once per block; split fragments held across the blocks (48 VGPRs) spill.
            // The block loop is rolled: unrolled, the blocks' MFMA chains were interleaved (four accumulators live).
            const u32x4* pla = reinterpret_cast<const u32x4*>(Gt) + lane;
#pragma unroll 1
            for (int t = 0; t < NBW; ++t) {
                const int nb = wave * NBW + t;
                // two accumulators (split_bf16.hpp: mfma_split6_two): GA feeds sums over every edge of a graph, where an
                // error shared by a graph's rows does not average out
                f32x16 c, cs;
#pragma unroll
                for (int r = 0; r < 16; ++r) { c[r] = 0.f; cs[r] = 0.f; }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int q = 4 * t + s;                  // step of the wave's sequence (blocks are contiguous in Bs)
                    if (q + SL < 4 * NBW) bsp[(s + SL) % (SL + 1)] = load_split_b(bsw + (q + SL) * 64, bs_planes);
                    if constexpr (PRESPLIT) {
                        mfma_split6_two(load_split_b(pla + s * kGhPlStep, kGhPlLd), bsp[s], c, cs);
                    } else {
                        const float4 a0 = Gt4[at4_slot(2 * s, hi, r31)], a1 = Gt4[at4_slot(2 * s + 1, hi, r31)];
                        mfma_split6_two(split8(a0, a1), bsp[s], c, cs);
                    }
                }
                c += cs;                                      // (one vector expression: packed adds)
#pragma unroll
                for (int r = 0; r < 16; ++r) GAt[acc_row(r, hi) * LDGA + nb * 32 + r31] = c[r];
            }
        } else {
            float4 af[8];
#pragma unroll
            for (int gq = 0; gq < 8; ++gq) af[gq] = Gt4[at4_slot(gq, hi, r31)];
#pragma unroll
            for (int t = 0; t < NBW; ++t) {
                const int nb = wave * NBW + t;
                if (t + 1 < NBW) {
                    const float4* bp = reinterpret_cast<const float4*>(Bp) +
                                       (int64_t)(nb + 1) * 8 * 64 + lane;
#pragma unroll
                    for (int gq = 0; gq < 8; ++gq) bf[(t + 1) & 1][gq] = bp[gq * 64];
                }
                f32x16 c;
#pragma unroll
                for (int r = 0; r < 16; ++r) c[r] = 0.f;
#pragma unroll
                for (int gq = 0; gq < 8; ++gq) c = mfma4(af[gq], bf[t & 1][gq], c);
#pragma unroll
                for (int r = 0; r < 16; ++r) GAt[acc_row(r, hi) * LDGA + nb * 32 + r31] = c[r];
            }
        }
        if constexpr (PRESPLIT) lds_barrier();       // every wave is through with the planes: sea overwrites them
        if ((int)threadIdx.x < ncap) {
#pragma unroll
            for (int d = 0; d < D; ++d) sea[threadIdx.x * D + d] = my_ea[d];
        }
        lds_barrier();
        // 3. per-edge dots: the staged slots of this group ...
#pragma unroll
        for (int t = 0; t < EPF; ++t) {
            if (t < mine) {
                const int s = il + 32 * t;
                float ee[D];
#pragma unroll
                for (int d = 0; d < D; ++d) ee[d] = sea[s * D + d];
                edge(sr[s], xr0[t], xr1[t], ee);
            }
        }
        for (int t = EPF; t < mine; ++t) {
            const int s = il + 32 * t;
            const float* xp = x + (int64_t)sj[s] * ldx + c0;
            const float4 y0 = ld4(xp), y1 = ld4(xp + 4);
            float ee[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ee[d] = sea[s * D + d];
            edge(sr[s], y0, y1, ee);
        }
        // ... and what the tile has beyond the staged ones (a hub's tile): straight from memory, destination by
        // bisection of the tile's row pointers
        for (int s = kGhCap + il; s < nt; s += 32) {
            const int pp = e_t0 + s;
            int lo = 0;
#pragma unroll
            for (int st = 16; st > 0; st >>= 1)
                if (rp_l[lo + st] <= pp) lo += st;
            const int64_t e = eidx[pp];
            const float* xp = x + (int64_t)col[pp] * ldx + c0;
            const float4 y0 = ld4(xp), y1 = ld4(xp + 4);
            float ee[D];
#pragma unroll
            for (int d = 0; d < D; ++d) ee[d] = ea[e * D + d];
            edge(lo, y0, y1, ee);
        }
        lds_barrier();        // GAt / Gt / the staged edges are rewritten by the next tile
    }
    // block partial: sum the 32 lane groups (fixed order) -> partials[blk][K*(D+1)]
    float* red = GAt;
#pragma unroll
    for (int d = 0; d < D; ++d) red[(d * 32 + il) * 8 + sub] = aw[d];
    red[(D * 32 + il) * 8 + sub] = ab;
    lds_barrier();
    if (threadIdx.x < (D + 1) * 8) {
        const int s8 = threadIdx.x & 7, d = threadIdx.x >> 3;
        float sum = 0.f;
        for (int g32 = 0; g32 < 32; ++g32) sum += red[(d * 32 + g32) * 8 + s8];
        if (s8 < K) partials[(int64_t)blockIdx.x * (K * (D + 1)) + (d < D ? s8 * D + d : K * D + s8)] = sum;
    }
}

}  // namespace qot

using namespace qot;

// launch of nnconv_gradh64_kernel (qot_nnconv_gradh_fused, nnconv_mfma.hip)
int qot_nnconv_gradh64_launch(const float* grad_out, int ld_g, const float* x, int ld_x, const float* edge_attr, const float* w1,
                              const float* b1, const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* invdeg,
                              const float* b_perm, const void* b_split, int64_t split_stride, float* workspace, int64_t N, int D,
                              int grid, const qot::HostedTable& hosted, hipStream_t stream) {
    // `grid` persistent workgroups, then the hosted jobs' (first[n] of them; none: an empty table)
    const int n_main = grid;
    grid += hosted.n > 0 ? hosted.first[hosted.n] : 0;
    if (b_split) {
        // The g tile is split once per tile on its way to LDS unless QOT_GRADH_SPLIT_AFTER_READ=1 (the earlier loop, same
        // results bit for bit).  Read per call, not cached: callers flip it inside one process.
        const char* sar_env = getenv("QOT_GRADH_SPLIT_AFTER_READ");
        const bool presplit = !(sar_env && sar_env[0] == '1' && sar_env[1] == '\0');
        QOT_DISPATCH_D(D, {
            if (kD <= 4) {
                if (presplit)
                    nnconv_gradh64_kernel<(kD <= 4 ? kD : 4), true, true><<<grid, 256, 0, stream>>>(
                        hosted, n_main, grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr, col, eid, invdeg, nullptr, workspace, N,
                        static_cast<const u32x4*>(b_split), split_stride / 8);
                else
                    nnconv_gradh64_kernel<(kD <= 4 ? kD : 4), true><<<grid, 256, 0, stream>>>(
                        hosted, n_main, grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr, col, eid, invdeg, nullptr, workspace, N,
                        static_cast<const u32x4*>(b_split), split_stride / 8);
            }
        });
        QOT_LAUNCH_CHECK();
        return QOT_OK;
    }
    QOT_DISPATCH_D(D, {
        if (kD <= 4)
            nnconv_gradh64_kernel<(kD <= 4 ? kD : 4)><<<grid, 256, 0, stream>>>(
                hosted, n_main, grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr, col, eid, invdeg, b_perm, workspace, N);
    });
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
