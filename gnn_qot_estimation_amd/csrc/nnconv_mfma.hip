// NNConv fused gather -> LDS operand tile -> fp32 MFMA  (H = 64).
//
// out[i,:] = bias + A_i @ Wcat,  A_i = [inv_i * sum_e h_e[k] x_j (k<K) | inv_i * sum_e x_j | x_i]
// (see nnconv.hip for the algebra; reference site topological_training/models.py:57).
// The unfused path writes A ([N, 640] fp32 = 262 MB at B=1024) to HBM and reads it back in
// a library GEMM; here a workgroup builds the 32 x 640 operand tile of 32 consecutive
// destinations directly in LDS and multiplies it on the matrix cores, so HBM sees only
// x (read), the edge features / CSR, and out (written).
//
//   phase 1  8 lanes per destination (2 x float4 = 64 channels), all 32 destinations at once;
//            blocks 0..K land in LDS in fragment-grouped order (at4_slot): two conflict-free
//            ds_write_b128 per lane per block.
//   phase 2  4 waves = 2 column halves x 2 K halves; each wave chains
//            v_mfma_f32_32x32x2_f32 on one 32x32 accumulator.  A fragments: ONE conflict-free
//            ds_read_b128 per 4 MFMAs (measured: a ds_read_b32 + swizzle per MFMA capped the
//            loop at ~105 of the ~135 TFLOP/s the register-fed loop reaches).
//            B fragment: Wcat pre-permuted on the host side into fragment order so a lane
//            reads 16 B = 4 consecutive k-steps, a wave 1 KiB contiguous (L2-resident, 160 KB).
//   root     the destination's own row (block K+1) is kept in registers during phase 2 and
//            then overwrites block 0's slots: 72 KB of LDS instead of 80 KB, which is what
//            lets TWO workgroups share a CU (2 x 80 KB needs every byte of the 160 KiB and
//            was measured to run one workgroup per CU: gather and MFMA phases serialised).
//   phase 3  K halves summed through LDS, bias added, 128-B row segments stored.
// (The split-bf16 forward, the production form, publishes the tile as bf16 planes in two equal K phases instead: PRESPLIT below.)
// One workgroup gathers while its CU-mate owns the MFMA pipes.  TRANSPOSE runs the adjoint (grad_x) over the CSC with the mean scale taken at
// the gathered end.
#include "common.hpp"
#include "mfma_tile.hpp"
#include "nnconv_finalize_dev.hpp"
#include "split_bf16.hpp"

namespace qot {

// Phase 1.  8 lanes per destination (2 x float4 = 64 channels each), so the 32 destinations of
// a tile are gathered in ONE pass by the 256 threads.  Lane `sub` of a destination's group
// prefetches the (source, edge id, edge features) of in-edge `sub` and evaluates that edge's
// h = relu(W1 ea + b1) once; the per-edge loop then only broadcasts (8-lane shuffles) and
// streams the 256-B source rows, four edges in flight per group.
// Returns the destination's own row (root block) in registers; blocks 0..K go to LDS.
// PRESPLIT: At holds bf16 planes of (K + 2) / 2 blocks (split_bf16.hpp: store_split_planes); the first half of the blocks is
// split and stored, the others are returned in park0 / park1 (fp32, as accumulated) for the kernel's second phase.
template <int D, bool TRANSPOSE, bool PRESPLIT = false>
__device__ __forceinline__ void nnconv_gather_tile(
    float* __restrict__ At, const float* __restrict__ x, int ldx, const float* __restrict__ ea,
    const float* __restrict__ w1, const float* __restrict__ b1, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const int32_t* __restrict__ eidx, const float* __restrict__ invdeg,
    int64_t tile0, int64_t N, float4& root0, float4& root1, float4* park0 = nullptr, float4* park1 = nullptr) {
    constexpr int K = 2 * D;
    const int sub = threadIdx.x & 7, il = threadIdx.x >> 3;
    const int c0 = 8 * sub;
    const int64_t i = tile0 + il;
    float4 acc0[K + 1], acc1[K + 1];        // written (not accumulated) by the first edge slot: no zero fill per tile
    root0 = f4zero(); root1 = f4zero();
    int beg = 0, end = 0;
    // the row's own loads (mean scale, root row) are issued BEFORE the edge loop: behind it they were one more
    // exposed memory round trip per tile
    float srow = 0.f;
    if (i < N) {
        beg = rowptr[i]; end = rowptr[i + 1];
        if (!TRANSPOSE) srow = invdeg[i];
        root0 = ld4(x + i * ldx + c0);
        root1 = ld4(x + i * ldx + c0 + 4);
    }
    const int own = (i < N) ? (int)i : 0;   // dead edge slots read the destination's own row (times zero)
    // One batch = up to 8 in-edges of every destination, one edge per lane: indices, edge features, edge-MLP hidden vector
    // (the mean scale 1/deg of the forward form is folded into it), then two blocks of four slots.  Lanes 0..7 of a group
    // hold edges base..base+7; broadcasts with compile-time source lanes run on the DPP path (as __shfl with a runtime lane
    // each was a ds_bpermute_b32 round trip: ten per edge).  Dead slots (lane p >= end) carry h = 0 and scale = 0: their
    // terms vanish without per-use selects.  FIRST: the batch that every destination runs (also one without in-edges); its
    // first slot WRITES the accumulators.
#define QOT_ACC(FIRSTSLOT, H, X, A) ((FIRSTSLOT) ? scale4((H), (X)) : fma4((H), (X), (A)))
#define QOT_EDGE4(U0, FIRST)                                                                            \
        {                                                                                               \
            float4 xa[4], xb[4];                                                                        \
            float sc[4];                                                                                \
            int jj[4];                                                                                  \
            jj[0] = group8_bcast<U0 + 0>(myj); jj[1] = group8_bcast<U0 + 1>(myj);                       \
            jj[2] = group8_bcast<U0 + 2>(myj); jj[3] = group8_bcast<U0 + 3>(myj);                       \
            sc[0] = group8_bcast<U0 + 0>(mysc); sc[1] = group8_bcast<U0 + 1>(mysc);                     \
            sc[2] = group8_bcast<U0 + 2>(mysc); sc[3] = group8_bcast<U0 + 3>(mysc);                     \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                             \
                const float* xr = x + (int64_t)jj[u] * ldx + c0;                                        \
                xa[u] = ld4(xr);                                                                        \
                xb[u] = ld4(xr + 4);                                                                    \
            }                                                                                           \
            _Pragma("unroll") for (int kk = 0; kk < K; ++kk) {                                          \
                const float h0 = group8_bcast<U0 + 0>(myh[kk]), h1 = group8_bcast<U0 + 1>(myh[kk]);     \
                acc0[kk] = QOT_ACC(FIRST, h0, xa[0], acc0[kk]); acc1[kk] = QOT_ACC(FIRST, h0, xb[0], acc1[kk]); \
                acc0[kk] = fma4(h1, xa[1], acc0[kk]); acc1[kk] = fma4(h1, xb[1], acc1[kk]);             \
            }                                                                                           \
            acc0[K] = QOT_ACC(FIRST, sc[0], xa[0], acc0[K]); acc1[K] = QOT_ACC(FIRST, sc[0], xb[0], acc1[K]); \
            acc0[K] = fma4(sc[1], xa[1], acc0[K]); acc1[K] = fma4(sc[1], xb[1], acc1[K]);               \
            /* four rows stay in flight, the vector work is skipped in pairs (a wave runs as many slots */ \
            /* as its highest-degree row needs, and VALU time is MFMA time on this part)                */ \
            if (cnt > U0 + 2) {                                                                         \
                _Pragma("unroll") for (int kk = 0; kk < K; ++kk) {                                      \
                    const float h2 = group8_bcast<U0 + 2>(myh[kk]), h3 = group8_bcast<U0 + 3>(myh[kk]); \
                    acc0[kk] = fma4(h2, xa[2], acc0[kk]); acc1[kk] = fma4(h2, xb[2], acc1[kk]);         \
                    acc0[kk] = fma4(h3, xa[3], acc0[kk]); acc1[kk] = fma4(h3, xb[3], acc1[kk]);         \
                }                                                                                       \
                _Pragma("unroll") for (int u = 2; u < 4; ++u) {                                         \
                    acc0[K] = fma4(sc[u], xa[u], acc0[K]);                                              \
                    acc1[K] = fma4(sc[u], xb[u], acc1[K]);                                              \
                }                                                                                       \
            }                                                                                           \
        }
#define QOT_FWD_BATCH(FIRST)                                                                            \
    {                                                                                                   \
        const int p = base + sub;                                                                       \
        int myj = own;                                                                                  \
        float myh[K], mysc = 0.f;                                                                       \
        _Pragma("unroll") for (int kk = 0; kk < K; ++kk) myh[kk] = 0.f;                                 \
        if (p < end) {                                                                                  \
            myj = col[p];                                                                               \
            mysc = TRANSPOSE ? invdeg[myj] : srow;                                                      \
            edge_hidden<D>(w1, b1, ea, (int64_t)eidx[p], mysc, myh);                                    \
        }                                                                                               \
        const int cnt = (end - base < 8) ? end - base : 8;                                              \
        QOT_EDGE4(0, FIRST)                                                                             \
        if (cnt > 4) QOT_EDGE4(4, false)                                                                \
    }
    int base = beg;
    QOT_FWD_BATCH(true)
    for (base = beg + 8; base < end; base += 8) QOT_FWD_BATCH(false)
#undef QOT_FWD_BATCH
#undef QOT_EDGE4
#undef QOT_ACC
    if constexpr (PRESPLIT) {
        constexpr int HB = (K + 2) / 2;
#pragma unroll
        for (int kk = 0; kk < HB; ++kk)
            store_split_planes(reinterpret_cast<u32x4*>(At) + kk * 3 * kGhPlLd, sub, il, acc0[kk], acc1[kk]);
#pragma unroll
        for (int kk = HB; kk <= K; ++kk) { park0[kk - HB] = acc0[kk]; park1[kk - HB] = acc1[kk]; }
    } else {
#pragma unroll
        for (int kk = 0; kk <= K; ++kk)         // channels c0+{0,2,4,6} -> hi 0 ; c0+{1,3,5,7} -> hi 1
            store_fragment_grouped(reinterpret_cast<float4*>(At), kk * 8 + sub, il, acc0[kk], acc1[kk]);
    }
}

// Root block (x_i itself, kept in registers during the main part) takes block 0's slots once everyone is done with blocks
// 0..K, and is published: the fp32 image is 72 KB instead of 80 KB.
__device__ __forceinline__ void root_restage(float* At, float4 root0, float4 root1) {
    lds_barrier();                         // everyone is done with blocks 0..K
    store_fragment_grouped(reinterpret_cast<float4*>(At), threadIdx.x & 7, threadIdx.x >> 3, root0, root1);
    __syncthreads();
}

// SPLIT (forward only): the products on the bf16 matrix pipe (split_bf16.hpp).  Ws: Wcat pre-split into three bf16
// planes ws_planes u32x4 apart (qot_nnconv_fused_split); the A fragments are split after their ds_read_b128, i.e. by both column-half waves.
// PRESPLIT (split form only): every value of the operand tile is split ONCE, by the gather thread that holds it, and LDS
// holds bf16 planes (split_bf16.hpp: store_split_planes) -- an A fragment is three ds_read_b128, no split8 in the MFMA loops.
// The K + 2 blocks of the inner dimension as planes are 6 B per value (120 KB at D = 4), so the tile is published in two
// equal halves: phase A = blocks 0 .. (K+2)/2 - 1, phase B = the others (root block last), which wait in registers as fp32
// and are split and stored into the same storage behind the barrier that ends phase A's reads.  Wave (nh, kh) takes steps
// kh (K+2) .. kh (K+2) + K + 1 of each phase; the B ring runs across the phase boundary.  63,360 B of planes + 8 KB for the
// K-half exchange (which can no longer alias the image) = 71,552 B at D = 4.  false: the split-after-read loop
// (QOT_NNCONV_FWD_SPLIT_AFTER_READ=1), every value split by both column-half waves.
// The three product loops (fp32, split-after-read, pre-split) and the epilogue stay inside the kernel body, and the gather's
// batches stay macros.  As __device__ __forceinline__ functions returning the accumulator the loops compiled to other code:
// 16 zero moves more per split form, another packing of the epilogue's adds, 1-3 VGPRs more (203 -> 204 at D = 1, 216 ->
// 218 at D = 2, 240 -> 243 for the fp32 form at D = 4); the epilogue as a function had its two `if (kh)` branches merged
// into one with runtime accumulator indices (a compare-select chain per register).  tools/regs.py --against shows it.
__host__ __device__ constexpr int fwd_plane_off(int p) { return (p / 4) * 3 * kGhPlLd + (p % 4) * kGhPlStep; }   // u32x4, phase-local step p

template <int D, bool TRANSPOSE, bool SPLIT = false, bool PRESPLIT = false>
__global__ __launch_bounds__(256, 2) void nnconv_mfma64_kernel(
    const float* __restrict__ x, int ldx, const float* __restrict__ ea, const float* __restrict__ w1,
    const float* __restrict__ b1, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ eidx, const float* __restrict__ invdeg, const float* __restrict__ Wp,
    const float* __restrict__ bias, float* __restrict__ out, int64_t N, ActParams act,
    const u32x4* __restrict__ Ws = nullptr, int64_t ws_planes = 0) {
    static_assert(!SPLIT || !TRANSPOSE, "split form: forward only");
    static_assert(!PRESPLIT || SPLIT, "the planes are the split form's");
    constexpr int K = 2 * D;
    constexpr int KM = (K + 1) * 64;        // inner dimension held in LDS (blocks 0..K)
    constexpr int GM = KM / 16;             // float4 B groups per wave for the main part
    constexpr int CH = 4;                       // prefetch chunk (GM = 8D+4 is divisible by 4); 6 spilled inside the MFMA loop
    constexpr int HB = (K + 2) / 2;             // PRESPLIT: blocks per phase
    constexpr int PLF = HB * 3 * kGhPlLd * 4;   // PRESPLIT: floats of the plane image; the K-half exchange follows it
    __shared__ __attribute__((aligned(16))) float At[PRESPLIT ? PLF + 4 * 8 * 64 : KM * 32];
    const int64_t ntiles = (N + 31) / 32;
    // read once per kernel: inside the tile loop each was a load consumed on the spot (an L2 round trip per tile)
    const float bz = bias ? bias[((threadIdx.x >> 6) & 1) * 32 + (threadIdx.x & 31)] : 0.f;
    const uint64_t drop_step = (act.enabled && act.thr16) ? (uint64_t)act.step[0] : 0;
    // persistent: 2 workgroups per CU walk the tiles; the two CU-mates drift out of phase so
    // one gathers while the other owns the MFMA pipes
#pragma unroll 1
    for (int64_t it = 0;; ++it) {
    const int64_t tile = xcd_tile(it, ntiles);
    if (tile < 0) break;
    const int64_t tile0 = tile * 32;
    float4 root0, root1;
    float4 park0[PRESPLIT ? HB : 1], park1[PRESPLIT ? HB : 1];      // PRESPLIT: phase B's blocks, root block last
    if constexpr (PRESPLIT) {
        nnconv_gather_tile<D, false, true>(At, x, ldx, ea, w1, b1, rowptr, col, eidx, invdeg, tile0, N, park0[HB - 1],
                                           park1[HB - 1], park0, park1);
    } else {
        nnconv_gather_tile<D, TRANSPOSE>(At, x, ldx, ea, w1, b1, rowptr, col, eidx, invdeg, tile0, N, root0, root1);
    }
    const float4* At4 = reinterpret_cast<const float4*>(At);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nh = wave & 1, kh = wave >> 1;
    const int r31 = lane & 31, hi = lane >> 5;
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    if constexpr (PRESPLIT) {
        // Ws as below.  The wave's steps of both phases are one sequence of 2 NCS chunks of SC steps; B fragments are requested
        // NBS - 1 chunks ahead into a ring with compile-time slots (fully unrolled), also across the phase boundary.
        constexpr int SP = K + 2;                  // steps per wave and phase (a phase has 2 SP = 4 HB steps)
        constexpr int ST = 4 * SP;                 // steps per column half
        constexpr int SC = 2;                      // steps per chunk
        constexpr int NCS = SP / SC;               // chunks per phase
        constexpr int NBS = 3;                     // buffers: 2 chunks (24 MFMAs) of lookahead
        // chunk j, step u: phase j / NCS, step (j % NCS) SC + u.  The wave's part of the address is kept scalar (the wave index
        // through readfirstlane), so a request is `global_load_dwordx4 v, lane * 16, s[base]` with SALU address arithmetic:
        // as per-lane 64-bit pointers the 6 NCS SC addresses were computed in front of the tile loop and spilled.
        const int wv = __builtin_amdgcn_readfirstlane(wave);
        const u32x4* wsp = Ws + ((int64_t)(wv & 1) * ST + (wv >> 1) * SP) * 64;
        const unsigned lane_u = lane;
        // A fragments: phase-local step kh SP + t at fwd_plane_off(kh SP + t).  SP is 0 or 2 mod 4, so the offset is a
        // compile-time one on top of two per-wave bases: one for the chunks with t = 0, 1 mod 4, one for t = 2, 3 mod 4.
        const u32x4* plane = reinterpret_cast<const u32x4*>(At) + lane;
        const u32x4* pl_e = plane + kh * (fwd_plane_off(SP) - fwd_plane_off(0));
        const u32x4* pl_o = plane + kh * (fwd_plane_off(SP + 2) - fwd_plane_off(2));
        Bf3 sb[NBS][SC];
#define QOT_FWD_BLOAD(J)                                                                                \
        _Pragma("unroll") for (int u = 0; u < SC; ++u)                                                  \
            sb[(J) % NBS][u] = load_split_b(wsp + (((J) / NCS) * 2 * SP + ((J) % NCS) * SC + u) * 64, lane_u, ws_planes);
#define QOT_FWD_ALOAD(J)                                                                                \
        _Pragma("unroll") for (int u = 0; u < SC; ++u) {                                                \
            const int t = ((J) % NCS) * SC + u;                                                         \
            af[(J) & 1][u] = load_split_b(((t & 2) ? pl_o : pl_e) + fwd_plane_off(t), kGhPlLd);         \
        }
        // One chunk: the ring's request NBS - 1 chunks ahead and the next chunk's A fragments (same phase) are issued in front
        // of this chunk's 6 SC MFMAs; the scheduling barriers keep them there (left to itself the scheduler sank the requests
        // next to their uses: `s_waitcnt vmcnt(0)` inside the chain)
#define QOT_FWD_CHUNK(J)                                                                                \
        {                                                                                               \
            if ((J) + NBS - 1 < 2 * NCS) { QOT_FWD_BLOAD((J) + NBS - 1) }                               \
            if (((J) + 1) % NCS != 0) { QOT_FWD_ALOAD((J) + 1) }                                        \
            __builtin_amdgcn_sched_barrier(0);                                                          \
            _Pragma("unroll") for (int u = 0; u < SC; ++u) c = mfma_split6(af[(J) & 1][u], sb[(J) % NBS][u], c); \
            __builtin_amdgcn_sched_barrier(0);                                                          \
        }
        Bf3 af[2][SC];
#pragma unroll
        for (int j = 0; j < NBS - 1; ++j) QOT_FWD_BLOAD(j)
        lds_barrier();                         // phase A's planes are published
        QOT_FWD_ALOAD(0)
#pragma unroll
        for (int j = 0; j < NCS; ++j) QOT_FWD_CHUNK(j)
        lds_barrier();                         // everyone is done with phase A's planes
        {
            const int sub = threadIdx.x & 7, il = threadIdx.x >> 3;
#pragma unroll
            for (int kk = 0; kk < HB; ++kk)
                store_split_planes(reinterpret_cast<u32x4*>(At) + kk * 3 * kGhPlLd, sub, il, park0[kk], park1[kk]);
        }
        lds_barrier();                         // phase B's planes are published (LDS only: the ring's requests stay in flight)
        QOT_FWD_ALOAD(NCS)
#pragma unroll
        for (int j = NCS; j < 2 * NCS; ++j) QOT_FWD_CHUNK(j)
#undef QOT_FWD_ALOAD
#undef QOT_FWD_CHUNK
#undef QOT_FWD_BLOAD
    } else if constexpr (SPLIT) {
        // Ws: 3 planes of ws_planes u32x4, each [nh][16-deep step s][lane]; step s = fp32 groups 2s, 2s + 1 (split_bf16.hpp).  The
        // native loop's structure: root fragments and NB - 1 chunks requested before the barrier, compile-time buffers.
        constexpr int ST = (K + 2) * 64 / 16;      // steps per column half
        constexpr int SM = GM / 2;                 // main steps per wave
        constexpr int SC = 2;                      // steps per chunk
        constexpr int NCS = SM / SC;
        constexpr int NBS = 3;                     // buffers: 2 chunks (24 MFMAs) of lookahead
        static_assert(GM % 4 == 0, "chunking");
        const u32x4* wsn = Ws + (int64_t)nh * ST * 64 + lane;
        const u32x4* wsp = wsn + (int64_t)kh * SM * 64;
        const u32x4* rsp = wsn + (int64_t)(2 * SM + 2 * kh) * 64;
        asm volatile("" : "+v"(rsp));
        Bf3 rbs[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) rbs[u] = load_split_b(rsp + u * 64, ws_planes);
        Bf3 sb[NBS][SC];
#pragma unroll
        for (int q = 0; q < NBS - 1; ++q)
#pragma unroll
            for (int u = 0; u < SC; ++u) sb[q][u] = load_split_b(wsp + (q * SC + u) * 64, ws_planes);
        lds_barrier();
        int ch = 0;
#pragma unroll 1
        for (; ch + NBS <= NCS; ch += NBS) {
#pragma unroll
            for (int q = 0; q < NBS; ++q) {
                if (ch + q + NBS - 1 < NCS) {
#pragma unroll
                    for (int u = 0; u < SC; ++u)
                        sb[(q + NBS - 1) % NBS][u] = load_split_b(wsp + ((ch + q + NBS - 1) * SC + u) * 64, ws_planes);
                }
#pragma unroll
                for (int u = 0; u < SC; ++u) c = mfma_split_step(At4, kh * GM + 2 * ((ch + q) * SC + u), hi, r31, sb[q][u], c);
            }
        }
#pragma unroll
        for (int q = 0; q < NBS - 1; ++q) {
            if (ch + q < NCS) {
#pragma unroll
                for (int u = 0; u < SC; ++u) c = mfma_split_step(At4, kh * GM + 2 * ((ch + q) * SC + u), hi, r31, sb[q][u], c);
            }
        }
        root_restage(At, root0, root1);
#pragma unroll
        for (int u = 0; u < 2; ++u) c = mfma_split_step(At4, kh * 4 + 2 * u, hi, r31, rbs[u], c);
    } else {
    // Wp: [nh][group g of 4 k-steps][lane][4]; wave (nh, kh) owns main groups kh*GM.. and
    // root groups (2*GM + kh*4)..
    const float4* wpn = reinterpret_cast<const float4*>(Wp) + (int64_t)nh * (2 * GM + 8) * 64 + lane;
    const float4* wp = wpn + (int64_t)kh * GM * 64;
    // one base pointer + immediate offsets (as separate expressions the four addresses were materialised
    // outside the tile loop, spilled, and reloaded from scratch -- with a full wait each -- every tile)
    const float4* rbp = wpn + (int64_t)(2 * GM + kh * 4) * 64;
    asm volatile("" : "+v"(rbp));          // opaque: one live base per tile, the four offsets stay immediates
    // The first weight fragments of the tile (root block + three chunks) are requested BEFORE the barrier that
    // publishes the operand tile, and that barrier orders LDS traffic only: requested behind a __syncthreads() their
    // L2 round trip was exposed once per tile, now it runs while the wave waits for the slowest gatherer.
    float4 rb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) rb[u] = rbp[u * 64];
    // B fragments are requested NB - 1 chunks (48 MFMAs, ~3000 cycles) ahead, NB buffers rotating with
    // compile-time roles: an L2 round trip is then covered by this wave's own MFMAs, so a workgroup keeps
    // the pipe fed while its CU-mate is gathering (with one chunk of lookahead the MFMA phase only ran at
    // full rate when both workgroups were in it).
    constexpr int NCH = GM / CH;
    constexpr int NB = 4;                      // buffers: fragments are requested NB - 1 chunks ahead
    float4 bb[NB][CH];
#pragma unroll
    for (int q = 0; q < NB - 1; ++q)
#pragma unroll
        for (int u = 0; u < CH; ++u) bb[q][u] = wp[(q * CH + u) * 64];
    lds_barrier();
    int ch = 0;
    // (r04, measured: the A fragment of group L + 1 read from LDS before the four MFMAs of group L instead of right in front
    //  of its use -- `ds_read_b128; s_waitcnt lgkmcnt(0)` before every group as it stands -- 96.0 -> 96.9 us: no gain, not kept)
#pragma unroll 1
    for (; ch + NB <= NCH; ch += NB) {
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            if (ch + q + NB - 1 < NCH) {
#pragma unroll
                for (int u = 0; u < CH; ++u) bb[(q + NB - 1) % NB][u] = wp[((ch + q + NB - 1) * CH + u) * 64];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) c = mfma_group(At4, kh * GM + (ch + q) * CH + u, hi, r31, bb[q][u], c);
        }
    }
    // tail: chunks ch .. NCH-1 are already in buffers 0 .. (their loads were issued above)
#pragma unroll
    for (int q = 0; q < NB - 1; ++q) {
        if (ch + q < NCH) {
#pragma unroll
            for (int u = 0; u < CH; ++u) c = mfma_group(At4, kh * GM + (ch + q) * CH + u, hi, r31, bb[q][u], c);
        }
    }
    root_restage(At, root0, root1);
#pragma unroll
    for (int u = 0; u < 4; ++u) c = mfma_group(At4, kh * 4 + u, hi, r31, rb[u], c);
    }
    // K halves meet through LDS; every wave finishes 8 of the 16 accumulator registers of its
    // (column half), so the stores are spread over all four waves
    float* red = At + (PRESPLIT ? PLF : 64 * 32);      // disjoint from block 0, which other waves may still read; PRESPLIT: behind the planes
    // (compile-time register indices in both branches: a runtime index into the accumulator
    //  vector would be lowered through scratch)
    if (kh) {
#pragma unroll
        for (int r = 0; r < 8; ++r) red[((2 + nh) * 8 + r) * 64 + lane] = c[r];
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) red[(nh * 8 + r) * 64 + lane] = c[8 + r];
    }
    lds_barrier();
    {
        const int colg = nh * 32 + r31;
        float v[8];
        if (kh) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = c[8 + r] + red[(nh * 8 + r) * 64 + lane] + bz;
        } else {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = c[r] + red[((2 + nh) * 8 + r) * 64 + lane] + bz;
        }
        // Dropout draws: one 64-bit hash serves the four columns of a float4 group, i.e. the four lanes of
        // a quad for the same row.  Each lane hashes two of its eight rows and the quad shares them through
        // quad_perm broadcasts (2 hashes + 12 DPP moves per lane instead of 8 hashes: the 64-bit
        // multiplies of the hash were ~5 % of this kernel's VALU time).
        uint32_t zlo[8], zhi[8];
        const bool drop = act.enabled && act.thr16;
        if (drop) {
            const int jq = r31 & 3;
            uint32_t mylo[2], myhi[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int rr = kh * 8 + 2 * jq + t;
                const int row = acc_row(rr, hi);
                const uint64_t flat = (uint64_t)((tile0 + row) * 64 + colg);
                const uint64_t z = act_hash64(act.seed, drop_step, flat >> 2);
                mylo[t] = (uint32_t)z; myhi[t] = (uint32_t)(z >> 32);
            }
            quad_share_draws<2, 2, 1>(mylo, myhi, zlo, zhi);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int rr = kh * 8 + r;
            const int row = acc_row(rr, hi);
            const int64_t i = tile0 + row;
            float y = v[r];
            if (act.enabled) {
                y = y > 0.f ? y : act.slope * y;
                if (drop) {
                    const uint64_t z = ((uint64_t)zhi[r] << 32) | zlo[r];
                    const bool keep = ((uint32_t)(z >> (16 * (colg & 3))) & 0xFFFFu) >= act.thr16;
                    y = keep ? y * act.keep_scale : 0.f;
                }
            }
            if (i < N) out[i * 64 + colg] = y;
        }
    }
    // `red` is consumed before the next tile's gather overwrites it.  PRESPLIT: `red` is storage of its own; the next tile's
    // plane stores follow the barrier above (every wave is through with phase B's reads when it writes `red`), its `red`
    // stores follow three more barriers
    if constexpr (!PRESPLIT) lds_barrier();
    }
}

// ---------------------------------------------------------------------------------------------
// Backward of NNConv, data AND weight gradients from ONE gather  (H = 64).
//   U_j = [ sum_{e: j->i} h_e[k] invdeg_i g_i (k<K) | sum_e invdeg_i g_i | g_j ]     (adjoint tile)
//   grad_x_j  = U_j @ WcatT                         (as nnconv_mfma64<TRANSPOSE>)
//   gWcat     = sum_j x_j (x) U_j  ("X^T U")        -- grad of nn.2.weight / nn.2.bias / lin.weight
// The separate path re-gathered the forward operand A ([N,640] = 262 MB written, then read by a
// split-K GEMM).  Here the U tile that the adjoint needs anyway is multiplied twice: rows as the
// A operand (grad_x) and, read transposed from the same LDS image, against the tile's own x rows
// (weight gradient).  512 threads = 8 waves, one workgroup per CU: every wave keeps 5 of the 40
// 32x32 accumulator tiles of gWcat^T across the persistent loop (80 VGPRs), partials go to one slab
// per workgroup and are summed in a fixed order afterwards (bitwise reproducible).

// SPLIT: the weight-gradient product as split-bf16 MFMAs (the production form).  The
// grad_x product is the fp32 loop either way: its B operand would be bf16 planes of WcatT, which this entry point
// does not receive.
template <int D, bool SPLIT>
__global__ __launch_bounds__(512, 2) void nnconv_adjoint_dw64_kernel(
    const float* __restrict__ g, int ldg, const float* __restrict__ xf, int ldx, const float* __restrict__ ea,
    const float* __restrict__ w1, const float* __restrict__ b1, const int32_t* __restrict__ rowptr_t,
    const int32_t* __restrict__ col_t, const int32_t* __restrict__ eid_t, const float* __restrict__ invdeg,
    const float* __restrict__ Wp, float* __restrict__ gx, float* __restrict__ slabs, int64_t N) {
    constexpr int K = 2 * D;
    constexpr int KT = (K + 2) * 64;        // all K+2 blocks live in LDS (one workgroup per CU: room)
    constexpr int GQ = KT / 8 / 4;          // float4 groups per K quarter (20 at D=4)
    constexpr int MB = KT / 32;             // 32-row blocks of gWcat^T (20)
    constexpr int TPW = MB * 2 / 8;         // dW tiles per wave (5)
    static_assert(GQ % 4 == 0 || GQ % 5 == 0, "chunking");
    constexpr int CH = (GQ % 4 == 0) ? 4 : 5;
    __shared__ __attribute__((aligned(16))) float Ut[KT * 32];
    __shared__ __attribute__((aligned(16))) float red[8 * 3 * 4 * 64];
    __shared__ __attribute__((aligned(16))) float xs[32 * 64];      // the tile's own x rows (B operand of X^T U)
    float4* Ut4 = reinterpret_cast<float4*>(Ut);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r31 = lane & 31, hi = lane >> 5;
    const int nh = wave & 1, kq = wave >> 1;                 // grad_x: column half x K quarter
    const int ah = wave & 1, mb0 = wave >> 1;                // dW: x-channel half, row blocks mb0 + 4t
    const int64_t ntiles = (N + 31) / 32;

    f32x16 dw[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dw[t][r] = 0.f;
    // Transposed-read addressing of the U tile for this lane's dW rows (kcol = 32*(mb0 + 4t) + r31).
    // Float index of U[row jj][kcol] = base(t) + ((jj ^ m) << 2) with base(t) = base(0) + 4096 t and the
    // XOR mask m = (4 mb0 + (r31 >> 3)) & 7 the same for every t.  With jj = 8a + 2b + hi the XOR only
    // touches b and hi: (jj ^ m) << 2 = 32 a + ((((b ^ (m >> 1)) << 1) | (hi ^ (m & 1))) << 2), so four
    // per-lane offsets (b = 0..3) plus compile-time immediates (a, t) address all 80 reads of a tile.
    int dwoff[4];
    {
        const int kcol = mb0 * 32 + r31;
        const int gg = kcol >> 3, within = kcol & 7;
        const int base0 = ((2 * gg + (within & 1)) * 32) * 4 + (within >> 1);
        const int m = gg & 7;
#pragma unroll
        for (int b = 0; b < 4; ++b) dwoff[b] = base0 + ((((b ^ (m >> 1)) << 1) | (hi ^ (m & 1))) << 2);
    }
    const float4* wp = reinterpret_cast<const float4*>(Wp) + ((int64_t)nh * (KT / 8) + kq * GQ) * 64 + lane;
    // (r04, measured and not kept, tools/ab_adjoint.py, interleaved rounds in one process: static `s_setprio 1` for waves 4-7
    // -- 172.7 us either way; the half index folded into the tile's XOR swizzle, i ^ ((g + 4 hi) & 7), which makes the
    // transposed reads of the X^T U loop conflict-free -- 171.9 us either way: that loop does not wait for LDS bandwidth)

#pragma unroll 1
    for (int64_t it = 0;; ++it) {
        const int64_t tile = xcd_tile(it, ntiles);
        if (tile < 0) break;
        const int64_t tile0 = tile * 32;
        // the tile's own x rows are requested BEFORE the gather and written to LDS behind it (loaded behind the
        // gather, as first written, the load was one exposed memory round trip per tile)
        float4 xown;
        {
            const int64_t j = tile0 + (threadIdx.x >> 4);
            xown = (j < N) ? ld4(xf + j * ldx + 4 * (threadIdx.x & 15)) : f4zero();
        }
        // ---- gather: 16 lanes per source node j (float4 = 64 channels), out-edges over the CSC
        {
            const int sub = threadIdx.x & 15, il = threadIdx.x >> 4;
            const int c0 = 4 * sub;
            const int64_t j = tile0 + il;
            float4 acc[K + 2];          // blocks 0..K are WRITTEN by the first edge slot: no zero fill per tile
            acc[K + 1] = f4zero();
            int beg = 0, end = 0;
            if (j < N) { beg = rowptr_t[j]; end = rowptr_t[j + 1]; acc[K + 1] = ld4(g + j * ldg + c0); }
            const int own = (j < N) ? (int)j : 0;   // dead slots read the node's own g row (times zero), never another node's
            // One batch = up to 16 out-edges of every node, one edge per lane of the row (zeros past the end); broadcasts with
            // compile-time source lanes are one DPP move each (row_newbcast) -- with a runtime lane (__shfl) every one of the
            // ten per edge was a ds_bpermute_b32 + s_waitcnt round trip.  FIRST: the batch every node runs (also one without
            // out-edges); its first slot writes the accumulators.
#define QOT_ADJ_EDGE(U)                                                                                  \
                {                                                                                        \
                    const int64_t i = (int64_t)row16_bcast<U>(myi);                                      \
                    gr[(U) & 3] = ld4(g + i * ldg + c0);                                                 \
                    sc[(U) & 3] = row16_bcast<U>(mysc);                                                  \
                }
#define QOT_ADJ_FMA(U, FIRSTSLOT)                                                                        \
                {                                                                                        \
                    _Pragma("unroll") for (int kk = 0; kk < K; ++kk)                                     \
                        acc[kk] = (FIRSTSLOT) ? scale4(row16_bcast<U>(myh[kk]), gr[(U) & 3])             \
                                              : fma4(row16_bcast<U>(myh[kk]), gr[(U) & 3], acc[kk]);     \
                    acc[K] = (FIRSTSLOT) ? scale4(sc[(U) & 3], gr[(U) & 3]) : fma4(sc[(U) & 3], gr[(U) & 3], acc[K]); \
                }
#define QOT_ADJ_EDGE4(U0, FIRST)                                                                         \
                {                                                                                        \
                    float4 gr[4];                                                                        \
                    float sc[4];                                                                         \
                    QOT_ADJ_EDGE(U0) QOT_ADJ_EDGE(U0 + 1) QOT_ADJ_EDGE(U0 + 2) QOT_ADJ_EDGE(U0 + 3)      \
                    QOT_ADJ_FMA(U0, FIRST) QOT_ADJ_FMA(U0 + 1, false)                                    \
                    /* four rows stay in flight, but the vector work is skipped in pairs: a wave runs as */ \
                    /* many slots as its highest-degree row needs, and VALU time is MFMA time here      */ \
                    if (cnt > U0 + 2) { QOT_ADJ_FMA(U0 + 2, false) QOT_ADJ_FMA(U0 + 3, false) }          \
                }
#define QOT_ADJ_BATCH(FIRST)                                                                             \
            {                                                                                            \
                const int p = base + sub;                                                                \
                int myi = own;                                                                           \
                float myh[K], mysc = 0.f;                                                                \
                _Pragma("unroll") for (int kk = 0; kk < K; ++kk) myh[kk] = 0.f;                          \
                if (p < end) {                                                                           \
                    myi = col_t[p];                                                                      \
                    mysc = invdeg[myi];                                                                  \
                    edge_hidden<D>(w1, b1, ea, (int64_t)eid_t[p], mysc, myh);                            \
                }                                                                                        \
                const int cnt = (end - base < 16) ? end - base : 16;                                     \
                QOT_ADJ_EDGE4(0, FIRST)                                                                  \
                if (cnt > 4) QOT_ADJ_EDGE4(4, false)                                                     \
                if (cnt > 8) QOT_ADJ_EDGE4(8, false)                                                     \
                if (cnt > 12) QOT_ADJ_EDGE4(12, false)                                                   \
            }
            int base = beg;
            QOT_ADJ_BATCH(true)
            for (base = beg + 16; base < end; base += 16) QOT_ADJ_BATCH(false)
#undef QOT_ADJ_BATCH
#undef QOT_ADJ_EDGE4
#undef QOT_ADJ_FMA
#undef QOT_ADJ_EDGE
            // channels c0..c0+3 of block kk: k = 64 kk + c0 + t -> group 8 kk + sub/2,
            // (r, hi) = (2 (sub&1) + t/2, t&1): two 8-byte stores per block, conflict-free
#pragma unroll
            for (int kk = 0; kk < K + 2; ++kk) {
                const int gg = kk * 8 + (sub >> 1);
                float2* s0 = reinterpret_cast<float2*>(&Ut4[at4_slot(gg, 0, il)]) + (sub & 1);
                float2* s1 = reinterpret_cast<float2*>(&Ut4[at4_slot(gg, 1, il)]) + (sub & 1);
                *s0 = make_float2(acc[kk].x, acc[kk].z);
                *s1 = make_float2(acc[kk].y, acc[kk].w);
            }
        }
        // x rows of the tile's own nodes (B operand of the weight-gradient product) go to LDS next to the U
        // tile (16 lanes per row, one float4 each): holding them in 16 VGPRs through both MFMA loops was
        // part of what pushed this kernel into scratch.
        {
            const int sub = threadIdx.x & 15, il = threadIdx.x >> 4;
            *reinterpret_cast<float4*>(&xs[il * 64 + 4 * sub]) = xown;
        }
        // WcatT fragments: two buffers used alternately, two chunks per trip of a rolled loop.  Written as
        // `bc = bn` copies the compiler put `s_waitcnt vmcnt(0)` at the top of every chunk, i.e. waited for
        // the prefetch it had just issued (fully unrolled it spilled instead).
        constexpr int NCH = GQ / CH;
        float4 bc[CH], bn[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) bc[u] = wp[u * 64];
        lds_barrier();
        // ---- grad_x: this wave's K quarter of U @ WcatT
        f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = 0.f;
        {
            int ch = 0;
#pragma unroll 1
            for (; ch + 1 < NCH; ch += 2) {
#pragma unroll
                for (int u = 0; u < CH; ++u) bn[u] = wp[((ch + 1) * CH + u) * 64];
#pragma unroll
                for (int u = 0; u < CH; ++u) c = mfma_group(Ut4, kq * GQ + ch * CH + u, hi, r31, bc[u], c);
                if (ch + 2 < NCH) {
#pragma unroll
                    for (int u = 0; u < CH; ++u) bc[u] = wp[((ch + 2) * CH + u) * 64];
                }
#pragma unroll
                for (int u = 0; u < CH; ++u) c = mfma_group(Ut4, kq * GQ + (ch + 1) * CH + u, hi, r31, bn[u], c);
            }
            if (NCH & 1) {
#pragma unroll
                for (int u = 0; u < CH; ++u) c = mfma_group(Ut4, kq * GQ + (NCH - 1) * CH + u, hi, r31, bc[u], c);
            }
        }
        // (published BEFORE the weight-gradient loop so that the 16 accumulator registers are dead there)
        // ---- K quarters of grad_x meet through LDS: quarter q finishes accumulator registers
        // 4q..4q+3 of its column half (hands the other 12 over), so all 8 waves share the stores.
        // red[((owner*2 + nh)*3 + slot)*4 + rr][lane], slot = which of the 3 other quarters wrote it
#define QOT_GIVE(OWNER, SLOT)                                                                        \
        _Pragma("unroll") for (int rr = 0; rr < 4; ++rr)                                             \
            red[((((OWNER) * 2 + nh) * 3 + (SLOT)) * 4 + rr) * 64 + lane] = c[4 * (OWNER) + rr];
        if (kq == 0) { QOT_GIVE(1, 0) QOT_GIVE(2, 0) QOT_GIVE(3, 0) }
        else if (kq == 1) { QOT_GIVE(0, 0) QOT_GIVE(2, 1) QOT_GIVE(3, 1) }
        else if (kq == 2) { QOT_GIVE(0, 1) QOT_GIVE(1, 1) QOT_GIVE(3, 2) }
        else { QOT_GIVE(0, 2) QOT_GIVE(1, 2) QOT_GIVE(2, 2) }
#undef QOT_GIVE
        // ---- weight gradient: gWcat^T[(k,o)][a] += sum_j U[j][(k,o)] x[j][a]
        // fp32 form (the else branch): step s = 4a + b multiplies tile rows 2s, 2s+1.  Software-pipelined by hand: the TPW transposed
        // reads of step s+1 are issued before the TPW MFMAs of step s (left to itself the compiler
        // reused ONE temporary and put `ds_read_b32; s_waitcnt lgkmcnt(0)` in front of every MFMA --
        // half of all MFMAs of this kernel waited for their own LDS read).
        if (SPLIT) {
            // Split form (split_bf16.hpp): both operands are in LDS already, so each is split after its read.  Step s
            // covers tile rows jj = 8a + 2b + hi with a = 2s + (j >> 2), b = j & 3, j = 0..7: the bf16 MFMA contracts
            // element j of lane half hi on BOTH operands, so A and B only have to use the same map.  Same 80 transposed
            // reads of Ut per wave and tile as the fp32 form, at the same addresses; tile rows >= N hold zeros in Ut
            // and xs, and zero splits to zero.  Rolled, with a sched_barrier per accumulator tile: fully unrolled, D = 4
            // took 256 VGPRs and spilled.
#pragma unroll 1
            for (int s = 0; s < 2; ++s) {
                float xv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    xv[j] = xs[(8 * (2 * s + (j >> 2)) + 2 * (j & 3) + hi) * 64 + ah * 32 + r31];
                const Bf3 xb = split8(make_float4(xv[0], xv[1], xv[2], xv[3]), make_float4(xv[4], xv[5], xv[6], xv[7]));
#pragma unroll
                for (int t = 0; t < TPW; ++t) {
                    float av[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) av[j] = Ut[dwoff[j & 3] + (2 * s + (j >> 2)) * 32 + t * 4096];
                    dw[t] = mfma_split6(
                        split8(make_float4(av[0], av[1], av[2], av[3]), make_float4(av[4], av[5], av[6], av[7])), xb, dw[t]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        } else {
            float abuf[2][TPW], xbuf[2];
            const float* xsl = xs + hi * 64 + ah * 32 + r31;          // row 2s + hi -> + 128 s
#pragma unroll
            for (int t = 0; t < TPW; ++t) abuf[0][t] = Ut[dwoff[0] + t * 4096];
            xbuf[0] = xsl[0];
#pragma unroll
            for (int sidx = 0; sidx < 16; ++sidx) {
                const int cur = sidx & 1;
                if (sidx + 1 < 16) {
                    const int sn = sidx + 1;
#pragma unroll
                    for (int t = 0; t < TPW; ++t) abuf[cur ^ 1][t] = Ut[dwoff[sn & 3] + (sn >> 2) * 32 + t * 4096];
                    xbuf[cur ^ 1] = xsl[sn * 128];
                }
                __builtin_amdgcn_sched_barrier(0);      // the reads of step s+1 stay in front of the MFMAs of step s
#pragma unroll
                for (int t = 0; t < TPW; ++t)
                    dw[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(abuf[cur][t], xbuf[cur], dw[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        lds_barrier();
        {
            float v[4];
            if (kq == 0) { v[0] = c[0]; v[1] = c[1]; v[2] = c[2]; v[3] = c[3]; }
            else if (kq == 1) { v[0] = c[4]; v[1] = c[5]; v[2] = c[6]; v[3] = c[7]; }
            else if (kq == 2) { v[0] = c[8]; v[1] = c[9]; v[2] = c[10]; v[3] = c[11]; }
            else { v[0] = c[12]; v[1] = c[13]; v[2] = c[14]; v[3] = c[15]; }
            const int colg = nh * 32 + r31;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
                for (int slot = 0; slot < 3; ++slot) v[rr] += red[(((kq * 2 + nh) * 3 + slot) * 4 + rr) * 64 + lane];
                const int reg = 4 * kq + rr;
                const int row = acc_row(reg, hi);
                const int64_t j = tile0 + row;
                if (j < N) gx[j * 64 + colg] = v[rr];
            }
        }
        lds_barrier();            // Ut / red are rewritten by the next tile
    }
    // slab[blk][(k,o) row][a]
    float* slab = slabs + (int64_t)blockIdx.x * KT * 64;
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, hi);
            slab[((mb0 + 4 * t) * 32 + row) * 64 + ah * 32 + r31] = dw[t][r];
        }
}

// level-1/level-2 slab sums (same scheme as gemm_tn.hip; duplicated signature, internal linkage).  (Both as wrappers of one
// __forceinline__ body: other address arithmetic in the loop -- two s_add_u32 / s_addc_u32 pairs for two v_lshl_add_u64 --
// so the copy stays.)
__global__ void adj_slab_reduce_kernel(const float* __restrict__ slabs, int nslabs, int per_group, int64_t elems,
                                       int64_t slab_stride, float* __restrict__ dst, int64_t dst_stride) {
    int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t * 4 >= elems) return;
    const int s0 = blockIdx.y * per_group;
    int s1 = s0 + per_group;
    if (s1 > nslabs) s1 = nslabs;
    float4 acc = f4zero();
    int sidx = s0;
    for (; sidx + 8 <= s1; sidx += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = ld4(slabs + (int64_t)(sidx + u) * slab_stride + 4 * t);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = add4(acc, v[u]);
    }
    for (; sidx < s1; ++sidx) acc = add4(acc, ld4(slabs + (int64_t)sidx * slab_stride + 4 * t));
    st4(dst + blockIdx.y * dst_stride + 4 * t, acc);
}

// final slab sum written straight into the parameters' own layouts (no permute/copy kernels after):
//   dst = [ g(nn.2.weight)[a*64+o, k] (64*64*K) | g(nn.2.bias)[a*64+o] (64*64) | g(lin.weight)[o, a] (64*64) ]
// from gWcat^T[kb*64 + o][a]
__global__ void adj_slab_final_params_kernel(const float* __restrict__ slabs, int nslabs, int64_t elems,
                                             int64_t slab_stride, float* __restrict__ dst, int K) {
    int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t * 4 >= elems) return;
    float4 acc = f4zero();
    for (int sidx = 0; sidx < nslabs; ++sidx) acc = add4(acc, ld4(slabs + (int64_t)sidx * slab_stride + 4 * t));
    const int64_t e = 4 * t;
    const int a0 = (int)(e & 63), o = (int)((e >> 6) & 63), kb = (int)(e >> 12);
    const float v[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int a = a0 + c;
        int64_t idx;
        if (kb < K) idx = ((int64_t)a * 64 + o) * K + kb;
        else if (kb == K) idx = (int64_t)4096 * K + a * 64 + o;
        else idx = (int64_t)4096 * (K + 1) + o * 64 + a;
        dst[idx] = v[c];
    }
}

// ---------------------------------------------------------------------------------------------
// grad of the edge MLP's first layer: nnconv_gradh64_kernel lives in nnconv_gradh64.hip (a translation unit of its own:
// it is built with another machine-scheduler strategy, see the Makefile)
__global__ void gradh_partial_sum_kernel(const float* __restrict__ partials, int nblk, int n, int KD,
                                         float* __restrict__ gw1, float* __restrict__ gb1) {
    const int t = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // one wave per output
    if (t >= n) return;
    const float s = wave_sum_partials(partials, nblk, n, t);
    if ((threadIdx.x & 63) == 0) { if (t < KD) gw1[t] = s; else gb1[t - KD] = s; }
}

}  // namespace qot

using namespace qot;

// width-generic kernels (nnconv_gen.hip)
int qot_nnconv_gen_launch(const float* x, int ld_x, const float* edge_attr, const float* w1, const float* b1,
                          const int32_t* rowptr, const int32_t* col, const int32_t* edge_ids, const float* invdeg,
                          int transpose, const float* w_perm, const float* bias, float* out, int64_t N, int H, int D,
                          const ActParams& ap, hipStream_t stream);
int qot_nnconv_gradh_gen_launch(const float* grad_out, int ld_g, const float* x, int ld_x, const float* edge_attr,
                                const float* w1, const float* b1, const int32_t* rowptr, const int32_t* col,
                                const int32_t* eid, const float* invdeg, const float* b_perm, float* gw1, float* gb1,
                                float* workspace, int64_t N, int H, int D, hipStream_t stream);

// Wp layout (built by the caller, see functional.nnconv_perm_index): with GT = (K+2)*64/8 groups
// of 4 k-steps, for column half nh, group g, lane l, r in 0..3:
//   Wp[((nh*GT + g)*64 + l)*4 + r] = Wcat[8*g + 2*r + (l>>5)][nh*32 + (l&31)]
// edge_ids[p] = original edge id of slot p of the index being walked (CSR: eid; CSC: eid_t).
extern "C" int qot_nnconv_fused(const float* x, int ld_x, const float* edge_attr, const float* w1,
                                const float* b1, const int32_t* rowptr, const int32_t* col,
                                const int32_t* edge_ids, const float* invdeg, int transpose,
                                const float* w_perm, const float* bias, float* out, int64_t N, int H, int D,
                                int act, float act_slope, float act_p, uint64_t act_seed,
                                const int64_t* act_step, qot_stream_t stream) {
    if (N < 0 || !rowptr) return QOT_ERR_BADARG;
    if (H != 16 && H != 32 && H != 64 && H != 128 && H != 256) return QOT_ERR_UNSUPPORTED;
    if (N == 0) return QOT_OK;
    if (!x || !w1 || !b1 || !invdeg || !w_perm || !out || (ld_x & 3)) return QOT_ERR_BADARG;
    if (H != 64 || transpose == 2 || transpose == 3) {
        // other widths (and, for A/B measurements, H = 64 with transpose = 2 / 3): the per-pass tile kernel
        if (D > 4) return QOT_ERR_UNSUPPORTED;
        return qot_nnconv_gen_launch(x, ld_x, edge_attr, w1, b1, rowptr, col, edge_ids, invdeg, transpose & 1, w_perm,
                                     bias, out, N, H, D, make_act(act, act_slope, act_p, act_seed, act_step),
                                     (hipStream_t)stream);
    }
    int grid = grid_for(N, 32);
    if (grid > 2 * num_cus()) grid = 2 * num_cus();
    const ActParams ap = make_act(act, act_slope, act_p, act_seed, act_step);
    QOT_DISPATCH_D(D, {
        if (transpose)
            nnconv_mfma64_kernel<kD, true><<<grid, 256, 0, (hipStream_t)stream>>>(
                x, ld_x, edge_attr, w1, b1, rowptr, col, edge_ids, invdeg, w_perm, bias, out, N, ap);
        else
            nnconv_mfma64_kernel<kD, false><<<grid, 256, 0, (hipStream_t)stream>>>(
                x, ld_x, edge_attr, w1, b1, rowptr, col, edge_ids, invdeg, w_perm, bias, out, N, ap);
    });
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

// The forward at H = 64 with the products on the bf16 matrix pipe: w_split = Wcat in three bf16 planes (split_bf16.hpp;
// functional.nnconv_split_index), everything else as qot_nnconv_fused(transpose = 0).
extern "C" int qot_nnconv_fused_split(const float* x, int ld_x, const float* edge_attr, const float* w1,
                                      const float* b1, const int32_t* rowptr, const int32_t* col,
                                      const int32_t* edge_ids, const float* invdeg, const void* w_split,
                                      int64_t split_stride, const float* bias, float* out, int64_t N, int H, int D,
                                      int act, float act_slope, float act_p, uint64_t act_seed,
                                      const int64_t* act_step, qot_stream_t stream) {
    if (N < 0 || !rowptr) return QOT_ERR_BADARG;
    if (H != 64 || D > 4) return QOT_ERR_UNSUPPORTED;
    if (N == 0) return QOT_OK;
    if (!x || !w1 || !b1 || !invdeg || !w_split || !out || (ld_x & 3) || ((uintptr_t)w_split & 15) || (split_stride & 7) ||
        split_stride < (int64_t)(2 * D + 2) * 4096)   // a plane holds Wcat: (K+2)*64*64
        return QOT_ERR_BADARG;
    int grid = grid_for(N, 32);
    if (grid > 2 * num_cus()) grid = 2 * num_cus();
    const ActParams ap = make_act(act, act_slope, act_p, act_seed, act_step);
    // The operand tile is split once per tile on its way to LDS, in two K phases, unless QOT_NNCONV_FWD_SPLIT_AFTER_READ=1 (the
    // earlier loop: another per-wave summation order, so the last bits differ).  Read per call, not cached: callers flip it
    // inside one process.
    const char* sar_env = getenv("QOT_NNCONV_FWD_SPLIT_AFTER_READ");
    const bool presplit = !(sar_env && sar_env[0] == '1' && sar_env[1] == '\0');
    QOT_DISPATCH_D(D, {
        if (kD <= 4) {
            if (presplit)
                nnconv_mfma64_kernel<(kD <= 4 ? kD : 4), false, true, true><<<grid, 256, 0, (hipStream_t)stream>>>(
                    x, ld_x, edge_attr, w1, b1, rowptr, col, edge_ids, invdeg, nullptr, bias, out, N, ap,
                    static_cast<const u32x4*>(w_split), split_stride / 8);
            else
                nnconv_mfma64_kernel<(kD <= 4 ? kD : 4), false, true><<<grid, 256, 0, (hipStream_t)stream>>>(
                    x, ld_x, edge_attr, w1, b1, rowptr, col, edge_ids, invdeg, nullptr, bias, out, N, ap,
                    static_cast<const u32x4*>(w_split), split_stride / 8);
        }
    });
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

// Bp layout: for 32-column block nb of GA (column n = k*64 + a), group gq of 4 k-steps over o,
// lane l, r:  Bp[((nb*8 + gq)*64 + l)*4 + r] = W2[a*64 + o, k]  with o = 8*gq + 2*r + (l>>5),
// n = nb*32 + (l&31)  (built by functional.nnconv_gradh_perm_index).
int qot_nnconv_gradh64_launch(const float* grad_out, int ld_g, const float* x, int ld_x, const float* edge_attr, const float* w1,
                              const float* b1, const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* invdeg,
                              const float* b_perm, const void* b_split, int64_t split_stride, float* workspace, int64_t N, int D,
                              int grid, const qot::HostedTable& hosted, hipStream_t stream);
int qot_hosted_take(qot::HostedTable* t, qot_role_t* planned);      // roles.hip (qot_nnconv_gradh_host_roles)
extern "C" size_t qot_nnconv_gradh_workspace_floats(int D) {
    return (size_t)2 * 256 * 2 * (size_t)(2 * D * (D + 1));
}

static int nnconv_gradh_impl(const float* grad_out, int ld_g, const float* x, int ld_x,
                             const float* edge_attr, const float* w1, const float* b1,
                             const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                             const float* invdeg, const float* b_perm, const void* b_split, int64_t split_stride,
                             float* gw1, float* gb1,
                             float* workspace, int64_t N, int H, int D, qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // The jobs qot_nnconv_gradh_host_roles left for this call are taken whatever becomes of it (an error drops them).
    HostedTable hosted;
    qot_role_t hosted_roles[QOT_MAX_ROLES];
    const int n_hosted = qot_hosted_take(&hosted, hosted_roles);
    if (N < 0 || !rowptr) return QOT_ERR_BADARG;
    if ((H != 16 && H != 32 && H != 64 && H != 128 && H != 256) || D > 4) return QOT_ERR_UNSUPPORTED;
    if (!grad_out || !x || !w1 || !b1 || !invdeg || !(b_perm || b_split) || (!gw1 != !gb1) || !workspace || (ld_g & 3) ||
        (ld_x & 3) || ((uintptr_t)b_split & 15) || (b_split && ((split_stride & 7) || split_stride < (int64_t)2 * D * 64 * 64)))
        return QOT_ERR_BADARG;
    if (b_split && H != 64) return QOT_ERR_UNSUPPORTED;
    if (!gw1 && H != 64) return QOT_ERR_UNSUPPORTED;
    // a hosted job may not read what this call writes: its partials must lie outside the workspace
    for (int r = 0; r < n_hosted; ++r) {
        const uintptr_t src = (uintptr_t)hosted.job[r].src, w0 = (uintptr_t)workspace;
        if (src >= w0 && src < w0 + qot_nnconv_gradh_workspace_floats(D) * sizeof(float)) return QOT_ERR_BADARG;
    }
    if (H != 64) {   // other widths: GA built 32 input channels at a time (nnconv_gen.hip); hosted jobs in a launch behind it
        const int rc = qot_nnconv_gradh_gen_launch(grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr, col, eid, invdeg, b_perm,
                                                   gw1, gb1, workspace, N, H, D, stream);
        if (rc != QOT_OK || n_hosted == 0) return rc;
        return qot_run_roles(hosted_roles, n_hosted, stream_);
    }
    int grid = grid_for(N > 0 ? N : 1, 32);
    if (grid > 2 * num_cus()) grid = 2 * num_cus();
    const int K = 2 * D;
    const int rc = qot_nnconv_gradh64_launch(grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr, col, eid, invdeg, b_perm,
                                             b_split, split_stride, workspace, N, D, grid, hosted, stream);
    if (rc != QOT_OK) return rc;
    QOT_LAUNCH_CHECK();
    if (!gw1) return QOT_OK;          // partials left in the workspace for qot_nnconv_bwd_finalize
    const int n = K * (D + 1);
    gradh_partial_sum_kernel<<<grid_for(n, 4), 256, 0, stream>>>(workspace, grid, n, K * D, gw1, gb1);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

extern "C" int qot_nnconv_gradh_fused(const float* grad_out, int ld_g, const float* x, int ld_x,
                                      const float* edge_attr, const float* w1, const float* b1,
                                      const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                                      const float* invdeg, const float* b_perm, float* gw1, float* gb1,
                                      float* workspace, int64_t N, int H, int D, qot_stream_t stream) {
    return nnconv_gradh_impl(grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr, col, eid, invdeg, b_perm, nullptr, 0, gw1, gb1,
                             workspace, N, H, D, stream);
}

// As qot_nnconv_gradh_fused at H = 64 with the GA products on the bf16 matrix pipe: b_split = Wk^T in three bf16 planes
// (split_bf16.hpp; functional.nnconv_split_index).
extern "C" int qot_nnconv_gradh_split(const float* grad_out, int ld_g, const float* x, int ld_x,
                                      const float* edge_attr, const float* w1, const float* b1,
                                      const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                                      const float* invdeg, const void* b_split, int64_t split_stride, float* gw1, float* gb1,
                                      float* workspace, int64_t N, int H, int D, qot_stream_t stream) {
    if (!b_split) return QOT_ERR_BADARG;
    return nnconv_gradh_impl(grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr, col, eid, invdeg, nullptr, b_split, split_stride,
                             gw1, gb1,
                             workspace, N, H, D, stream);
}

// Both second-stage sums of the H = 64 NNConv backward in one launch: after qot_nnconv_adjoint_dw(param_layout = 2:
// slabs left in adj_workspace) and qot_nnconv_gradh_fused(gw1 = gb1 = NULL: partials left in gradh_workspace).
extern "C" int qot_nnconv_bwd_finalize(const float* adj_workspace, const float* gradh_workspace, float* grad_params,
                                       float* gw1, float* gb1, int64_t N, int H, int D, qot_stream_t stream_) {
    if (N <= 0 || H != 64 || D < 1 || D > 4) return (H != 64 || D > 4) ? QOT_ERR_UNSUPPORTED : QOT_ERR_BADARG;
    qot_role_t r{};                      // nnconv_bwd_finalize64_body through the multi-role launch (roles.hip)
    r.kind = QOT_ROLE_NNCONV_FINALIZE64;
    r.p[0] = adj_workspace; r.p[1] = gradh_workspace; r.p[2] = grad_params; r.p[3] = gw1; r.p[4] = gb1;
    r.i[0] = N; r.i[1] = D;
    return qot_run_roles(&r, 1, stream_);
}

// grad_x + weight gradient of NNConv in one pass (H = 64, D <= 4).  w_perm: WcatT in fragment
// order (as for qot_nnconv_fused transpose=1).  gwcat_t[(K+2)*64, 64] receives gWcat^T per block:
// gwcat_t[k*64 + o][a] = d/dWcat[k*64 + a][o].  workspace: qot_nnconv_adjoint_dw_workspace_floats(D).
extern "C" size_t qot_nnconv_adjoint_dw_workspace_floats(int D) {
    return (size_t)(num_cus() > 256 ? num_cus() : 256) * kAdjBlocksPerCu * (size_t)((2 * D + 2) * 64) * 64;
}

extern "C" int qot_nnconv_adjoint_dw(const float* grad_out, int ld_g, const float* x, int ld_x,
                                     const float* edge_attr, const float* w1, const float* b1,
                                     const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t,
                                     const float* invdeg, const float* w_perm, float* grad_x, float* gwcat_t,
                                     int param_layout, float* workspace, int64_t N, int H, int D,
                                     qot_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (N <= 0 || !rowptr_t) return QOT_ERR_BADARG;
    if (H != 64 || D > 4) return QOT_ERR_UNSUPPORTED;
    if (!grad_out || !x || !w1 || !b1 || !invdeg || !w_perm || !grad_x || !gwcat_t || !workspace || (ld_g & 3))
        return QOT_ERR_BADARG;
    int grid = grid_for(N, 32);
    const int cap = num_cus() * kAdjBlocksPerCu;
    if (grid > cap) grid = cap;
    // The weight-gradient product runs as split-bf16 MFMAs unless QOT_NNCONV_F32_MFMA=1 (the switch
    // functional.nnconv_split_bf16 reads).  Read per call, not cached: callers flip it inside one process.
    const char* f32_env = getenv("QOT_NNCONV_F32_MFMA");
    const bool f32_mfma = f32_env && f32_env[0] == '1' && f32_env[1] == '\0';
    QOT_DISPATCH_D(D, {
        if (kD <= 4) {
            constexpr int kD4 = kD <= 4 ? kD : 4;
            if (f32_mfma)
                nnconv_adjoint_dw64_kernel<kD4, false><<<grid, 512, 0, stream>>>(
                    grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr_t, col_t, eid_t, invdeg, w_perm, grad_x,
                    workspace, N);
            else
                nnconv_adjoint_dw64_kernel<kD4, true><<<grid, 512, 0, stream>>>(
                    grad_out, ld_g, x, ld_x, edge_attr, w1, b1, rowptr_t, col_t, eid_t, invdeg, w_perm, grad_x,
                    workspace, N);
        }
    });
    QOT_LAUNCH_CHECK();
    if (param_layout == 2) return QOT_OK;      // profiling: main kernel only (slabs left unsummed)
    const int64_t elems = (int64_t)(2 * D + 2) * 64 * 64;
    const int per_group = 16;
    const int groups = (grid + per_group - 1) / per_group;
    adj_slab_reduce_kernel<<<dim3(grid_for(elems / 4, 256), groups), 256, 0, stream>>>(
        workspace, grid, per_group, elems, elems, workspace, (int64_t)per_group * elems);
    QOT_LAUNCH_CHECK();
    if (param_layout)
        adj_slab_final_params_kernel<<<grid_for(elems / 4, 256), 256, 0, stream>>>(
            workspace, groups, elems, (int64_t)per_group * elems, gwcat_t, 2 * D);
    else
        adj_slab_reduce_kernel<<<dim3(grid_for(elems / 4, 256), 1), 256, 0, stream>>>(
            workspace, groups, groups, elems, (int64_t)per_group * elems, gwcat_t, 0);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
