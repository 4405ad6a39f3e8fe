// fp32 products on the bf16 matrix pipe ("split-bf16"): the H = 64 NNConv kernels' default form.
//
// gfx950 has no xf32; its fp32-input MFMA (v_mfma_f32_32x32x2_f32) runs at 64 FLOP/clk/SIMD, the bf16 one
// (v_mfma_f32_32x32x16_bf16) at 1024.  An fp32 value is EXACTLY the sum of three bf16 values, each split rounding
// to nearest (v_cvt_pk_bf16_f32):
//   hi = bf16(x),  mid = bf16(x - hi),  lo = bf16(x - hi - mid)
// Why exact: let x in [2^e, 2^(e+1)), a multiple of u = 2^(e-23).  hi keeps 8 significant bits, so r = x - hi is a
// multiple of u with |r| <= 2^(e-8) (half an ulp of hi): at most 16 significant bits, and the subtraction is exact.
// mid = bf16(r) leaves r - mid, again a multiple of u, with |r - mid| <= 2^(e-16): at most 8 significant bits, so
// r - mid is exact and lo = bf16(r - mid) = r - mid.  (Holds while no part leaves bf16's exponent range, which is
// fp32's: |x| below ~3.4e38 and parts above the denormal range -- for |x| >= ~2^-110 every part is normal.)
// A product a*b is then a sum of 9 bf16 cross products, each exact in the MFMA's fp32 accumulation path.  The six
// largest are kept (hh, hm, mh, hl, lh, mm); |mid| <= 2^-8 |x| and |lo| <= 2^-16 |x|, so the three dropped ones (ml, lm,
// ll) sum to at most ~2^-23 |a b|, about one rounding of the fp32 MFMA (2^-24 per product).  The six are issued smallest first into ONE fp32 accumulator
// (mfma_split6), or the five small ones into an accumulator of their own (mfma_split6_two: the grad-h kernel).
// Cost per 32 x 32 output block and 16-deep K step: 6 x 32 cycles against 8 x 64 for the fp32 MFMA.
#pragma once
#include "mfma_tile.hpp"

namespace qot {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// One 16-deep operand fragment of the 32x32x16 bf16 MFMA in three planes (12 VGPRs)
struct Bf3 {
    bf16x8 h, m, l;
};

__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 p;
    p[0] = (__bf16)a;                     // v_cvt_pk_bf16_f32: round to nearest even
    p[1] = (__bf16)b;
    return __builtin_bit_cast(uint32_t, p);
}

// split3 of one value: the three bf16 bit patterns (weights, pre-split once per step: roles.hip)
__device__ __forceinline__ void split3(float x, uint16_t& h, uint16_t& m, uint16_t& l) {
    const __bf16 bh = (__bf16)x;
    const float r = x - (float)bh;
    const __bf16 bm = (__bf16)r;
    const __bf16 bl = (__bf16)(r - (float)bm);
    h = __builtin_bit_cast(uint16_t, bh);
    m = __builtin_bit_cast(uint16_t, bm);
    l = __builtin_bit_cast(uint16_t, bl);
}

// Packed split of 8 values (an A fragment of two fp32 fragment groups): 12 v_cvt_pk_bf16_f32, 16 unpacks, 16 v_sub_f32.
// The empty asm statements keep the packed words opaque (otherwise the compiler re-converts single elements to unpack
// them) and keep the subtractions scalar (paired into v_pk_add_f32 they cost more issue cycles beside the MFMAs).
__device__ __forceinline__ Bf3 split8(float4 a, float4 b) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t h[4], m[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h[j] = cvt_pk_bf16(v[2 * j], v[2 * j + 1]);
        asm("" : "+v"(h[j]));
        float r0 = v[2 * j] - __uint_as_float(h[j] << 16), r1 = v[2 * j + 1] - __uint_as_float(h[j] & 0xffff0000u);
        asm("" : "+v"(r0), "+v"(r1));
        m[j] = cvt_pk_bf16(r0, r1);
        asm("" : "+v"(m[j]));
        float q0 = r0 - __uint_as_float(m[j] << 16), q1 = r1 - __uint_as_float(m[j] & 0xffff0000u);
        asm("" : "+v"(q0), "+v"(q1));
        l[j] = cvt_pk_bf16(q0, q1);
    }
    Bf3 s;
    s.h = __builtin_bit_cast(bf16x8, (u32x4){h[0], h[1], h[2], h[3]});
    s.m = __builtin_bit_cast(bf16x8, (u32x4){m[0], m[1], m[2], m[3]});
    s.l = __builtin_bit_cast(bf16x8, (u32x4){l[0], l[1], l[2], l[3]});
    return s;
}

// The six kept cross products, smallest first, into one fp32 accumulator
__device__ __forceinline__ f32x16 mfma_split6(const Bf3& a, const Bf3& b, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.m, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.m, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, c, 0, 0, 0);
    return c;
}

// The same six products with the five small ones (at most 2^-8 of hh) in an accumulator of their own: summed over the K steps
// into ONE accumulator every product rounds at the full sum's magnitude (6 roundings per step); kept apart, the small
// ones round at their own magnitude and the full-size accumulator sees one rounding per step plus the final c + s.
__device__ __forceinline__ void mfma_split6_two(const Bf3& a, const Bf3& b, f32x16& c, f32x16& s) {
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.m, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.m, s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.h, s, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, c, 0, 0, 0);
}

// Pre-split B fragment of 16-deep step s: three planes of `ps` u32x4 each, 64 lanes per step (16 B per lane and plane).
// Plane layout (built by roles.hip's gather from functional.nnconv_split_index): element j = 4 q + r of lane l in step s
// holds the value the fp32 fragment-grouped layout puts at group 2 s + q, lane l, component r -- so the bf16 MFMA's
// hardware k = 8 (l >> 5) + j runs over the 16 k of two fp32 groups, the SAME permutation on both operands.
__device__ __forceinline__ Bf3 load_split_b(const u32x4* __restrict__ p, int64_t ps) {
    Bf3 b;
    b.h = __builtin_bit_cast(bf16x8, p[0]);
    b.m = __builtin_bit_cast(bf16x8, p[ps]);
    b.l = __builtin_bit_cast(bf16x8, p[2 * ps]);
    return b;
}

// The same with the step's address wave-uniform (scalar registers) and the lane as a 32-bit offset of its own
__device__ __forceinline__ Bf3 load_split_b(const u32x4* __restrict__ p, unsigned lane, int64_t ps) {
    Bf3 b;
    b.h = __builtin_bit_cast(bf16x8, p[lane]);
    b.m = __builtin_bit_cast(bf16x8, (p + ps)[lane]);
    b.l = __builtin_bit_cast(bf16x8, (p + 2 * ps)[lane]);
    return b;
}

// A 32-row x 64-channel operand block pre-split in LDS (grad-h's g tile, the forward's operand blocks): three bf16 planes
// kGhPlLd u32x4 apart, each [16-deep step s of 4][lane = 32 hi + row] u32x4 in the bf16 MFMA's A-fragment order, so that an
// A fragment is load_split_b(planes + s * kGhPlStep + lane, kGhPlLd).  The steps are 66 u32x4 apart (64 lanes + 32 B): a
// 16-lane group of the stores below holds two rows x four steps x two q, and with the steps exactly 1 KB apart all four
// steps would land on the same 8 banks; 32 B more shift step s by 8 banks -- conflict-free.
constexpr int kGhPlStep = 66;                // u32x4 per step of a plane
constexpr int kGhPlLd = 4 * kGhPlStep;       // u32x4 per plane

// The store: thread (il, sub) holds channels 8 sub .. 8 sub + 7 of row il in (c0, c1), i.e. fp32 fragment group sub =
// 2 s + q: elements 4 q + r of step s, components r of half hi = 0 (even channels) in words 2q, 2q + 1 of each plane and
// of hi = 1 (odd channels) likewise -- what mfma_split_step forms from groups 2 s and 2 s + 1.  Every value is split once;
// six 8-byte stores; a zero row gives zero planes.
__device__ __forceinline__ void store_split_planes(void* planes, int sub, int il, float4 c0, float4 c1) {
    const Bf3 gs = split8(make_float4(c0.x, c0.z, c1.x, c1.z), make_float4(c0.y, c0.w, c1.y, c1.w));
    uint2* pl = reinterpret_cast<uint2*>(planes) + 2 * ((sub >> 1) * kGhPlStep + il) + (sub & 1);
    const u32x4 ph = __builtin_bit_cast(u32x4, gs.h), pm = __builtin_bit_cast(u32x4, gs.m),
                plo = __builtin_bit_cast(u32x4, gs.l);
    pl[0] = make_uint2(ph[0], ph[1]);                      pl[64] = make_uint2(ph[2], ph[3]);
    pl[2 * kGhPlLd] = make_uint2(pm[0], pm[1]);            pl[2 * kGhPlLd + 64] = make_uint2(pm[2], pm[3]);
    pl[4 * kGhPlLd] = make_uint2(plo[0], plo[1]);          pl[4 * kGhPlLd + 64] = make_uint2(plo[2], plo[3]);
}

// One 16-deep step from a fragment-grouped fp32 LDS tile: the A fragments of groups g and g + 1 (two ds_read_b128), split
// after the read, times a pre-split B fragment.
__device__ __forceinline__ f32x16 mfma_split_step(const float4* __restrict__ At4, int g, int hi, int r31, const Bf3& b,
                                                  f32x16 c) {
    const float4 a0 = At4[at4_slot(g, hi, r31)], a1 = At4[at4_slot(g + 1, hi, r31)];
    return mfma_split6(split8(a0, a1), b, c);
}

}  // namespace qot
