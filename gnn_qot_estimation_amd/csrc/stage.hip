// Device-side staging of a slice of an HBM-resident shard into the static buffers of a batch slot
// (loader.StageSlot; the streamed replay of harness.StepReplayer).
//
// A captured train step reads its batch through fixed device pointers.  To run a DIFFERENT batch on every replay of
// ONE captured graph, the launch below -- captured in front of the step -- copies graphs [lo, lo + B) of the shard into
// those buffers, and takes `lo` from device memory: a control block holds this epoch's schedule of `lo` values and a
// position that the launch itself advances.  No kernel argument changes between replays, nothing is allocated, the
// host is not involved.
//
// Two kernels per call:
//   stage_plan_kernel   one workgroup.  Reads the position, takes schedule[position], validates the slice against
//                       the slot (range, node / edge totals, every graph within (max_nodes, max_edges)), writes the
//                       verdict -- `lo`, or -1 -- into the control block's snapshot word and advances the position
//                       (as step_advance_kernel does for the dropout counter: the copy's workgroups all read the
//                       snapshot, none can see a half-advanced position).  A violation ORs a bit into `status`.
//   stage_copy_kernel   the copy, grid-stride over every field.  Returns at once when the snapshot is -1, so a
//                       structural violation stages NOTHING.  Given the plan's checks every load stays inside the
//                       shard's arrays and every store inside the slot's buffers (sized exactly B, N, E).
//                       int64 fields (edge_index rows, ptr, edge_ptr, batch, node_ids) are copied two per lane with
//                       a 16-byte store (and a 16-byte load when the slice's byte offset allows: slices start at
//                       arbitrary e0 * 8 bytes; else two 8-byte loads), re-based on the way; fp32 fields (edge_attr, x,
//                       y) four dwords per lane likewise (slices start at e0 * D * 4 bytes), dword head / tail.
//                       A node id outside [0, V) is staged as 0 and flagged: the step that follows gathers no row
//                       outside the embedding table, and the host raises from `status` at the end of the epoch.
//
// Padded slots (qot_shard_stage_padded; loader.PaddedStageSlot): batches of B graphs whose edge totals DIFFER go through
// one slot of B + P graphs and E_cap edges.  The plan kernel accepts a slice that falls short of E_cap by at most
// P * max_m edges and publishes its edge total next to `lo` (no load it did not already make);
// stage_copy_padded_kernel copies the real slice as above and then writes P pad graphs that hold the spare edges as
// rings over their own n nodes, with zero edge features: computed from (E_real, E_cap, P, n, max_m), nothing loaded.
//
// Gather slots (qot_shard_stage_gather; loader.GatherStageSlot): the padded slot filled from a LIST of single graphs
// (shuffled batches).  The schedule holds graph ids, B per batch.  stage_plan_gather_kernel validates the batch's ids,
// forms the exclusive prefix sum of their edge counts (workgroup scan, carried between rounds of 256 graphs) into a
// scratch array owned by the slot -- not into the slot's edge_ptr: a refused batch leaves the previous one untouched --
// and accepts E_real as the padded plan does.  stage_copy_gather_kernel is the segmented copy: QOT_GATHER_LANES lanes per
// graph, grid-stride over the graphs, each group running the helpers below on its graph's segments (which start at
// arbitrary 8-byte / 4-byte alignment on BOTH sides: 16-byte stores, 16-byte loads where the source allows); then the
// pad graphs of the padded slot (stage_pad_graphs, shared).
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   stage_plan_kernel<false>  VGPRs 16, AGPRs 0, SGPRs 50,  scratch 0, LDS 272 B, occupancy 8 waves / SIMD
//   stage_plan_kernel<true>   VGPRs 16, AGPRs 0, SGPRs 52,  scratch 0, LDS 280 B, occupancy 8 waves / SIMD
//   stage_copy_kernel         VGPRs 18, AGPRs 0, SGPRs 92,  scratch 0, LDS 0,     occupancy 8 waves / SIMD
//   stage_copy_padded_kernel  VGPRs 26, AGPRs 0, SGPRs 105, scratch 0, LDS 0,     occupancy 7 waves / SIMD
//   stage_plan_gather_kernel  VGPRs 36, AGPRs 0, SGPRs 75,  scratch 0, LDS 48 B,  occupancy 8 waves / SIMD
//   stage_copy_gather_kernel  VGPRs 83, AGPRs 0, SGPRs 106, scratch 0, LDS 0,     occupancy 5 waves / SIMD
// At the headline shape (1024 graphs x 100 nodes / 400 edges, D = 4) the copy moves ~15 MB (read + write ~30 MB).
#include "common.hpp"

namespace qot {

typedef long long ll2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u4_t __attribute__((ext_vector_type(4)));

constexpr int kStagePos = 0, kStageCount = 1, kStageSnap = 2, kStageEdges = 3, kStageHeader = 4;

struct StageShard {
    const int64_t* node_ptr;        // [G + 1]
    const int64_t* edge_ptr;        // [G + 1]
    const int64_t* graph_of_node;   // [N_total]
    const int64_t* edge_index;      // [2, E_total]
    const uint32_t* edge_attr;      // [E_total, D] dwords, or NULL
    const int64_t* node_ids;        // [N_total], or NULL
    const uint32_t* x;              // [N_total, F] dwords, or NULL
    const uint32_t* y;              // [G, Y] dwords, or NULL
    int64_t G, N_total, E_total;
    int D, F, Y;
};

struct StageSlot {
    int64_t* edge_index;            // [2, E]
    uint32_t* edge_attr;
    int64_t* node_ids;
    uint32_t* x;
    uint32_t* y;
    int64_t* ptr;                   // [B + 1]
    int64_t* edge_ptr;              // [B + 1]
    int64_t* batch;                 // [N]
    int64_t B, N, E, max_n, max_m, V;
};

// PAD (qot_shard_stage_padded): N counts the REAL nodes, E is the slot's edge capacity and a slice may fall short of it by
// up to pad_cap edges; its own edge total -- already loaded for the check -- goes to the control block's fourth word.
template <bool PAD>
__global__ __launch_bounds__(256) void stage_plan_kernel(int64_t* __restrict__ ctl, int64_t sched_cap,
                                                         int32_t* __restrict__ status, const int64_t* __restrict__ node_ptr,
                                                         const int64_t* __restrict__ edge_ptr, int64_t G, int64_t N_total,
                                                         int64_t E_total, int64_t B, int64_t N, int64_t E, int64_t max_n,
                                                         int64_t max_m, int64_t pad_cap) {
    __shared__ int64_t s_lo;
    __shared__ int64_t s_edges;
    __shared__ int s_bits;
    if (threadIdx.x == 0) {
        int bits = 0;
        int64_t lo = -1, edges = 0;
        const int64_t pos = ctl[kStagePos];
        int64_t cnt = ctl[kStageCount];
        if (cnt > sched_cap) cnt = sched_cap;
        if (pos < 0 || pos >= cnt) {
            bits |= QOT_STAGE_BAD_RANGE;                 // the schedule is used up: the position stays where it is
        } else {
            lo = ctl[kStageHeader + pos];
            ctl[kStagePos] = pos + 1;
            if (lo < 0 || lo > G - B) {
                bits |= QOT_STAGE_BAD_RANGE;
            } else {
                const int64_t n0 = node_ptr[lo], n1 = node_ptr[lo + B], e0 = edge_ptr[lo], e1 = edge_ptr[lo + B];
                if (n0 < 0 || n1 > N_total || e0 < 0 || e1 > E_total) bits |= QOT_STAGE_BAD_RANGE;
                else if (!PAD && (n1 - n0 != N || e1 - e0 != E)) bits |= QOT_STAGE_BAD_SHAPE;
                else if (PAD && (n1 - n0 != N || e1 - e0 < 0 || e1 - e0 > E || E - (e1 - e0) > pad_cap)) bits |= QOT_STAGE_BAD_SHAPE;
                edges = e1 - e0;
            }
        }
        s_lo = bits ? -1 : lo;
        if (PAD) s_edges = edges;
        s_bits = bits;
    }
    __syncthreads();
    const int64_t lo = s_lo;
    int bad = 0;
    if (lo >= 0) {
        for (int64_t g = threadIdx.x; g < B; g += blockDim.x) {
            const int64_t n = node_ptr[lo + g + 1] - node_ptr[lo + g], m = edge_ptr[lo + g + 1] - edge_ptr[lo + g];
            if (n < 0 || n > max_n || m < 0 || m > max_m) bad = 1;
        }
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        const int bits = s_bits | (bad ? QOT_STAGE_BAD_SHAPE : 0);
        ctl[kStageSnap] = bits ? -1 : lo;
        if (PAD) ctl[kStageEdges] = bits ? 0 : s_edges;
        if (bits) atomicOr(status, bits);
    }
}

// dst[i] = src[i] - sub, i < n.  dst and src are 8-byte aligned.  CHECK: values outside [0, V) are stored as 0 and
// reported through the return value.
template <bool CHECK>
__device__ __forceinline__ bool stage_i64(int64_t* __restrict__ dst, const int64_t* __restrict__ src, int64_t n, int64_t sub,
                                          int64_t V, int64_t tid, int64_t nthreads) {
    bool flagged = false;
    auto fix = [&](int64_t v) -> int64_t {
        v -= sub;
        if (CHECK && (v < 0 || v >= V)) { flagged = true; v = 0; }
        return v;
    };
    if (n <= 0) return false;
    const int64_t head = (reinterpret_cast<uintptr_t>(dst) & 15u) ? 1 : 0;      // elements in front of the first 16-byte line
    const int64_t pairs = (n - head) >> 1;
    const bool src16 = (reinterpret_cast<uintptr_t>(src + head) & 15u) == 0;    // uniform over the launch
    if (src16) {
        for (int64_t p = tid; p < pairs; p += nthreads) {
            const int64_t i = head + 2 * p;
            const ll2_t v = *reinterpret_cast<const ll2_t*>(src + i);
            ll2_t o;
            o.x = fix(v.x);
            o.y = fix(v.y);
            *reinterpret_cast<ll2_t*>(dst + i) = o;
        }
    } else {
        for (int64_t p = tid; p < pairs; p += nthreads) {
            const int64_t i = head + 2 * p;
            ll2_t o;
            o.x = fix(src[i]);
            o.y = fix(src[i + 1]);
            *reinterpret_cast<ll2_t*>(dst + i) = o;
        }
    }
    if (tid == 0) {
        if (head) dst[0] = fix(src[0]);
        const int64_t done = head + 2 * pairs;
        if (done < n) dst[done] = fix(src[done]);
    }
    return flagged;
}

// dst[i] = src[i], i < n dwords.  dst and src are 4-byte aligned.
__device__ __forceinline__ void stage_u32(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int64_t n, int64_t tid,
                                          int64_t nthreads) {
    if (n <= 0) return;
    int64_t head = ((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const int64_t quads = (n - head) >> 2;
    const int64_t tail0 = head + 4 * quads;
    const bool src16 = (reinterpret_cast<uintptr_t>(src + head) & 15u) == 0;
    if (src16) {
        for (int64_t q = tid; q < quads; q += nthreads) {
            const int64_t i = head + 4 * q;
            *reinterpret_cast<u4_t*>(dst + i) = *reinterpret_cast<const u4_t*>(src + i);
        }
    } else {
        for (int64_t q = tid; q < quads; q += nthreads) {
            const int64_t i = head + 4 * q;
            u4_t o;
            o.x = src[i];
            o.y = src[i + 1];
            o.z = src[i + 2];
            o.w = src[i + 3];
            *reinterpret_cast<u4_t*>(dst + i) = o;
        }
    }
    if (tid < head) dst[tid] = src[tid];
    if (tid < n - tail0) dst[tail0 + tid] = src[tail0 + tid];
}

// dst[i] = f(i), i < n.  dst is 8-byte aligned (pad regions start wherever the real slice ends).
template <class F>
__device__ __forceinline__ void stage_fill_i64(int64_t* __restrict__ dst, int64_t n, F f, int64_t tid, int64_t nthreads) {
    if (n <= 0) return;
    const int64_t head = (reinterpret_cast<uintptr_t>(dst) & 15u) ? 1 : 0;
    const int64_t pairs = (n - head) >> 1;
    for (int64_t p = tid; p < pairs; p += nthreads) {
        const int64_t i = head + 2 * p;
        ll2_t o;
        o.x = f(i);
        o.y = f(i + 1);
        *reinterpret_cast<ll2_t*>(dst + i) = o;
    }
    if (tid == 0) {
        if (head) dst[0] = f(0);
        const int64_t done = head + 2 * pairs;
        if (done < n) dst[done] = f(done);
    }
}

// dst[i] = 0, i < n dwords.  dst is 4-byte aligned.
__device__ __forceinline__ void stage_zero_u32(uint32_t* __restrict__ dst, int64_t n, int64_t tid, int64_t nthreads) {
    if (n <= 0) return;
    int64_t head = ((16u - (reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const int64_t quads = (n - head) >> 2;
    const int64_t tail0 = head + 4 * quads;
    u4_t z;
    z.x = 0; z.y = 0; z.z = 0; z.w = 0;
    for (int64_t q = tid; q < quads; q += nthreads) *reinterpret_cast<u4_t*>(dst + head + 4 * q) = z;
    if (tid < head) dst[tid] = 0;
    if (tid < n - tail0) dst[tail0 + tid] = 0;
}

// What lies behind the real part of a padded slot: P pad graphs that take the E_cap - E_real spare edges, max_m apiece
// until they are used up, as rings over their own n nodes.  Computed from (E_real, E_cap, P, n, max_m): no load.  The pad
// regions are a few hundred elements (at most P * max_m edges, P * n nodes), so their 64-bit divisions do not show.
__device__ __forceinline__ void stage_pad_graphs(const StageShard& s, const StageSlot& d, int64_t E_real, int64_t P, int64_t tid,
                                                 int64_t nth) {
    const int64_t E_cap = d.E, n = d.max_n, max_m = d.max_m, B = d.B, N = d.N;
    const int64_t spare = E_cap - E_real;
    // pad edge j: pad graph p = j / max_m, its edge k = j mod max_m: (k mod n) -> ((k + 1) mod n) from node N + p n on
    auto ring = [&](int64_t j, int64_t step) -> int64_t {
        const int64_t p = j / max_m, k = j - p * max_m;
        return N + p * n + (k + step) % n;
    };
    stage_fill_i64(d.edge_index + E_real, spare, [&](int64_t j) { return ring(j, 0); }, tid, nth);
    stage_fill_i64(d.edge_index + E_cap + E_real, spare, [&](int64_t j) { return ring(j, 1); }, tid, nth);
    if (s.edge_attr) stage_zero_u32(d.edge_attr + E_real * s.D, spare * s.D, tid, nth);
    if (s.x) stage_zero_u32(d.x + N * s.F, P * n * s.F, tid, nth);
    if (s.node_ids) stage_fill_i64(d.node_ids + N, P * n, [&](int64_t i) { return i % n; }, tid, nth);
    stage_fill_i64(d.batch + N, P * n, [&](int64_t i) { return B + i / n; }, tid, nth);
    stage_fill_i64(d.ptr + B + 1, P, [&](int64_t p) { return N + (p + 1) * n; }, tid, nth);
    stage_fill_i64(d.edge_ptr + B + 1, P, [&](int64_t p) {
        const int64_t used = (p + 1) * max_m;
        return E_real + (used < spare ? used : spare);
    }, tid, nth);
}

// Graphs [lo, lo + B) of the shard -- N nodes, E edges -- into the front of the slot's buffers; ld_e: the slot's edge
// capacity (the distance between the two rows of its edge_index).
__device__ __forceinline__ void stage_slice(const StageShard& s, const StageSlot& d, int64_t lo, int64_t B, int64_t N, int64_t E,
                                            int64_t ld_e, int32_t* __restrict__ status, int64_t tid, int64_t nth) {
    const int64_t n0 = s.node_ptr[lo], e0 = s.edge_ptr[lo];
    stage_i64<false>(d.edge_index, s.edge_index + e0, E, n0, 0, tid, nth);
    stage_i64<false>(d.edge_index + ld_e, s.edge_index + s.E_total + e0, E, n0, 0, tid, nth);
    if (s.edge_attr) stage_u32(d.edge_attr, s.edge_attr + e0 * s.D, E * s.D, tid, nth);
    if (s.x) stage_u32(d.x, s.x + n0 * s.F, N * s.F, tid, nth);
    if (s.y) stage_u32(d.y, s.y + lo * s.Y, B * s.Y, tid, nth);
    stage_i64<false>(d.batch, s.graph_of_node + n0, N, lo, 0, tid, nth);
    stage_i64<false>(d.ptr, s.node_ptr + lo, B + 1, n0, 0, tid, nth);
    stage_i64<false>(d.edge_ptr, s.edge_ptr + lo, B + 1, e0, 0, tid, nth);
    if (s.node_ids) {
        bool flagged;
        if (d.V > 0) flagged = stage_i64<true>(d.node_ids, s.node_ids + n0, N, 0, d.V, tid, nth);
        else         flagged = stage_i64<false>(d.node_ids, s.node_ids + n0, N, 0, 0, tid, nth);
        if (flagged) atomicOr(status, QOT_STAGE_BAD_NODE_ID);
    }
}

__global__ __launch_bounds__(256) void stage_copy_kernel(const int64_t* __restrict__ ctl, int32_t* __restrict__ status,
                                                         StageShard s, StageSlot d) {
    const int64_t lo = ctl[kStageSnap];
    if (lo < 0) return;                                  // the plan refused the slice: nothing is staged
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    stage_slice(s, d, lo, d.B, d.N, d.E, d.E, status, tid, nth);
}

// The padded slot: d.B / d.N count the REAL graphs / nodes, d.E is the edge capacity, d.max_n the node count n of every
// graph; the buffers hold d.B + P graphs, (d.B + P) * n nodes, d.E edges.  The real slice, then the pad graphs.
__global__ __launch_bounds__(256) void stage_copy_padded_kernel(const int64_t* __restrict__ ctl, int32_t* __restrict__ status,
                                                                StageShard s, StageSlot d, int64_t P) {
    const int64_t lo = ctl[kStageSnap];
    if (lo < 0) return;                                  // the plan refused the slice: nothing is staged
    const int64_t E_real = ctl[kStageEdges];
    const int64_t E_cap = d.E, B = d.B, N = d.N;
    const int64_t spare = E_cap - E_real;
    if (E_real < 0 || spare < 0 || spare > P * d.max_m) return;    // what the plan accepted, once more: bounds every store below
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    stage_slice(s, d, lo, B, N, E_real, E_cap, status, tid, nth);
    stage_pad_graphs(s, d, E_real, P, tid, nth);
}

// ---- gather slots: a batch is a list of B graph ids ------------------------------------------------------------------
#ifndef QOT_GATHER_LANES
#define QOT_GATHER_LANES 64          // lanes per graph of the segmented copy (a power of two <= 64; measured: file header)
#endif
constexpr int kGatherLanes = QOT_GATHER_LANES;
static_assert(kGatherLanes >= 1 && kGatherLanes <= 64 && (kGatherLanes & (kGatherLanes - 1)) == 0, "lanes per graph");

// ctl: [position, batches in the schedule, snapshot, E_real], then B ids per batch.  Batch `position` is validated id by
// id -- 0 <= g < G (else RANGE), n nodes and 0 <= m_g <= max_m edges inside the arrays (else SHAPE) -- and offs[i]
// receives the exclusive prefix sum of the edge counts: 256 graphs per round, a wave scan, the four wave totals through
// LDS, the running total carried into the next round.  The verdict (the batch's number, or -1) goes to the snapshot
// word and E_real beside it, as stage_plan_kernel<true> publishes them; the position advances under the same rule.
__global__ __launch_bounds__(256) void stage_plan_gather_kernel(int64_t* __restrict__ ctl, int64_t sched_cap,
                                                                int32_t* __restrict__ status, int64_t* __restrict__ offs,
                                                                const int64_t* __restrict__ node_ptr,
                                                                const int64_t* __restrict__ edge_ptr, int64_t G, int64_t N_total,
                                                                int64_t E_total, int64_t B, int64_t n, int64_t E_cap,
                                                                int64_t max_m, int64_t pad_cap) {
    __shared__ int64_t s_pos;
    __shared__ int64_t s_wave[4];
    __shared__ int s_bits;
    if (threadIdx.x == 0) {
        int64_t pos = ctl[kStagePos];
        int64_t cnt = ctl[kStageCount];
        if (cnt > sched_cap) cnt = sched_cap;
        if (pos < 0 || pos >= cnt) {
            s_bits = QOT_STAGE_BAD_RANGE;                // the schedule is used up: the position stays where it is
            pos = -1;
        } else {
            s_bits = 0;
            ctl[kStagePos] = pos + 1;
        }
        s_pos = pos;
    }
    __syncthreads();
    const int64_t pos = s_pos;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    int bits = 0;
    if (pos >= 0) {
        const int64_t* ids = ctl + kStageHeader + pos * B;
        for (int64_t base = 0; base < B; base += 256) {  // uniform trip count: every thread meets every barrier
            const int64_t i = base + threadIdx.x;
            int64_t m = 0;
            if (i < B) {
                const int64_t g = ids[i];
                if (g < 0 || g >= G) {
                    bits |= QOT_STAGE_BAD_RANGE;
                } else {
                    const int64_t n0 = node_ptr[g], e0 = edge_ptr[g];
                    m = edge_ptr[g + 1] - e0;
                    if (n0 < 0 || n0 > N_total - n || e0 < 0 || m < 0 || m > E_total - e0) { bits |= QOT_STAGE_BAD_RANGE; m = 0; }
                    else if (node_ptr[g + 1] - n0 != n || m > max_m) { bits |= QOT_STAGE_BAD_SHAPE; m = 0; }
                }
            }
            int64_t incl = m;                            // inclusive scan over the wave
            for (int d = 1; d < 64; d <<= 1) {
                const int64_t up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            int64_t before = 0, total = 0;
            for (int w = 0; w < 4; ++w) {
                const int64_t t = s_wave[w];
                if (w < wave) before += t;
                total += t;
            }
            if (i < B) offs[i] = carry + before + incl - m;
            carry += total;
            __syncthreads();                             // s_wave is rewritten by the next round
        }
    }
    if (bits) atomicOr(&s_bits, bits);
    __syncthreads();
    if (threadIdx.x == 0) {
        int all = s_bits;
        const int64_t E_real = carry;
        if (!all && (E_real > E_cap || E_cap - E_real > pad_cap)) all |= QOT_STAGE_BAD_SHAPE;
        ctl[kStageSnap] = all ? -1 : pos;
        ctl[kStageEdges] = all ? 0 : E_real;
        if (all) atomicOr(status, all);
    }
}

// The segmented copy.  Graph i of the batch (id g, m edges, destination columns off_i ..) is copied by ONE group of
// kGatherLanes lanes running the helpers above with (lane in group, kGatherLanes); groups stride over the graphs.  d as in
// stage_copy_padded_kernel.  Every segment is checked against the slot once more before it is written (what the plan
// accepted: bounds every store below).  Then the pad graphs, by the whole grid.
__global__ __launch_bounds__(256) void stage_copy_gather_kernel(const int64_t* __restrict__ ctl, const int64_t* __restrict__ offs,
                                                                int32_t* __restrict__ status, StageShard s, StageSlot d,
                                                                int64_t P) {
    const int64_t k = ctl[kStageSnap];
    if (k < 0) return;                                   // the plan refused the batch: nothing is staged
    const int64_t E_real = ctl[kStageEdges];
    const int64_t E_cap = d.E, B = d.B, n = d.max_n;
    const int64_t spare = E_cap - E_real;
    if (E_real < 0 || spare < 0 || spare > P * d.max_m) return;
    const int64_t* ids = ctl + kStageHeader + k * B;
    const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * blockDim.x;
    const int64_t t = tid & (kGatherLanes - 1);
    bool flagged = false;
    for (int64_t i = tid / kGatherLanes; i < B; i += nth / kGatherLanes) {
        const int64_t g = ids[i], off = offs[i];
        if (g < 0 || g >= s.G) continue;
        const int64_t n0 = s.node_ptr[g], e0 = s.edge_ptr[g];
        const int64_t m = s.edge_ptr[g + 1] - e0;
        if (m < 0 || m > d.max_m || off < 0 || off > E_real - m) continue;
        const int64_t sub = n0 - i * n;                  // shard numbering -> batch numbering
        stage_i64<false>(d.edge_index + off, s.edge_index + e0, m, sub, 0, t, kGatherLanes);
        stage_i64<false>(d.edge_index + E_cap + off, s.edge_index + s.E_total + e0, m, sub, 0, t, kGatherLanes);
        if (s.edge_attr) stage_u32(d.edge_attr + off * s.D, s.edge_attr + e0 * s.D, m * s.D, t, kGatherLanes);
        if (s.x) stage_u32(d.x + i * n * s.F, s.x + n0 * s.F, n * s.F, t, kGatherLanes);
        if (s.y) stage_u32(d.y + i * s.Y, s.y + g * s.Y, s.Y, t, kGatherLanes);
        stage_fill_i64(d.batch + i * n, n, [&](int64_t) { return i; }, t, kGatherLanes);
        if (s.node_ids) {
            if (d.V > 0) flagged |= stage_i64<true>(d.node_ids + i * n, s.node_ids + n0, n, 0, d.V, t, kGatherLanes);
            else         stage_i64<false>(d.node_ids + i * n, s.node_ids + n0, n, 0, 0, t, kGatherLanes);
        }
        if (t == 0) {
            d.ptr[i] = i * n;
            d.edge_ptr[i] = off;
        }
    }
    if (flagged) atomicOr(status, QOT_STAGE_BAD_NODE_ID);
    if (tid == 0) {
        d.ptr[B] = B * n;
        d.edge_ptr[B] = E_real;
    }
    stage_pad_graphs(s, d, E_real, P, tid, nth);
}

}  // namespace qot

using namespace qot;

static void stage_structs(StageShard& s, StageSlot& d, const int64_t* node_ptr, const int64_t* edge_ptr,
                          const int64_t* graph_of_node, int64_t G, int64_t N_total, int64_t E_total, const int64_t* edge_index,
                          const void* edge_attr, int D, const int64_t* node_ids, const void* x, int F, const void* y, int Y,
                          int64_t B, int64_t N, int64_t E, int64_t max_nodes, int64_t max_edges, int64_t V,
                          int64_t* dst_edge_index, void* dst_edge_attr, int64_t* dst_node_ids, void* dst_x, void* dst_y,
                          int64_t* dst_ptr, int64_t* dst_edge_ptr, int64_t* dst_batch) {
    s.node_ptr = node_ptr; s.edge_ptr = edge_ptr; s.graph_of_node = graph_of_node; s.edge_index = edge_index;
    s.edge_attr = D > 0 ? (const uint32_t*)edge_attr : nullptr;
    s.node_ids = node_ids;
    s.x = F > 0 ? (const uint32_t*)x : nullptr;
    s.y = Y > 0 ? (const uint32_t*)y : nullptr;
    s.G = G; s.N_total = N_total; s.E_total = E_total; s.D = D; s.F = F; s.Y = Y;
    d.edge_index = dst_edge_index; d.edge_attr = (uint32_t*)dst_edge_attr; d.node_ids = dst_node_ids;
    d.x = (uint32_t*)dst_x; d.y = (uint32_t*)dst_y; d.ptr = dst_ptr; d.edge_ptr = dst_edge_ptr; d.batch = dst_batch;
    d.B = B; d.N = N; d.E = E; d.max_n = max_nodes; d.max_m = max_edges; d.V = V;
}

enum StageKind { kExactSlot, kPaddedSlot, kGatherSlot };

// What the three entry points refuse (QOT_ERR_BADARG) before anything is launched, on the structs stage_structs filled.
// Exact slot: any N >= 0, and the node buffers are needed only when N > 0.  Padded and gather slots: d.max_n is the node
// count n >= 1 of every graph and P the pad graphs; d.N is not read (the entry point forms B * n once both are bounded).
// The gather slot takes its scratch `offs` where the others take graph_of_node.
static bool stage_args_ok(StageKind kind, const int64_t* ctl, int64_t sched_cap, const int32_t* status, const int64_t* offs,
                          const StageShard& s, const StageSlot& d, int64_t P) {
    const bool exact = kind == kExactSlot;
    if (!ctl || !status || !s.node_ptr || !s.edge_ptr || !d.ptr || !d.edge_ptr) return false;
    if (kind == kGatherSlot ? !offs : !s.graph_of_node) return false;
    if (sched_cap < 1 || s.G < 1 || s.N_total < 0 || s.E_total < 0 || d.B < 1 || d.E < 0 || d.max_n < 0 || d.max_m < 0 || d.V < 0)
        return false;
    if (s.D < 0 || s.F < 0 || s.Y < 0) return false;
    if (exact && d.N < 0) return false;
    if (!exact) {
        if (d.max_n < 1 || P < 0) return false;
        if (P > 0 && (d.max_n < 2 || d.max_m < 1)) return false;       // a ring over one node is a self loop; no room to pad
        if (d.B > (INT64_MAX >> 24) || P > (INT64_MAX >> 24) || d.max_n > (1 << 20) || d.max_m > (1 << 20)) return false;
        if (kind == kGatherSlot && sched_cap > (INT64_MAX >> 4) / d.B) return false;      // sched_cap * B ids
    }
    const bool nodes = !exact || d.N > 0;
    if ((d.E > 0 && (!s.edge_index || !d.edge_index)) || (nodes && !d.batch)) return false;
    return !((s.edge_attr && d.E > 0 && !d.edge_attr) || (s.node_ids && nodes && !d.node_ids) || (s.x && nodes && !d.x) ||
             (s.y && !d.y));
}

// 16-byte units of the whole copy; four per thread, at most 1024 workgroups (4 per CU)
static int stage_grid(int64_t B, int64_t N, int64_t E, int D, int F, int Y) {
    const int64_t bytes = 16 * E + 4 * E * (int64_t)D + 16 * N + 4 * N * (int64_t)F + 4 * B * (int64_t)Y + 16 * (B + 1);
    int64_t grid = (bytes / 16 + 256 * 4 - 1) / (256 * 4);
    if (grid < 1) grid = 1;
    if (grid > 1024) grid = 1024;
    return (int)grid;
}

extern "C" int qot_shard_stage(int64_t* ctl, int64_t sched_cap, int32_t* status, const int64_t* node_ptr,
                               const int64_t* edge_ptr, const int64_t* graph_of_node, int64_t G, int64_t N_total,
                               int64_t E_total, const int64_t* edge_index, const void* edge_attr, int D,
                               const int64_t* node_ids, const void* x, int F, const void* y, int Y, int64_t B, int64_t N,
                               int64_t E, int64_t max_nodes, int64_t max_edges, int64_t V, int64_t* dst_edge_index,
                               void* dst_edge_attr, int64_t* dst_node_ids, void* dst_x, void* dst_y, int64_t* dst_ptr,
                               int64_t* dst_edge_ptr, int64_t* dst_batch, qot_stream_t stream) {
    StageShard s;
    StageSlot d;
    stage_structs(s, d, node_ptr, edge_ptr, graph_of_node, G, N_total, E_total, edge_index, edge_attr, D, node_ids, x, F, y, Y, B,
                  N, E, max_nodes, max_edges, V, dst_edge_index, dst_edge_attr, dst_node_ids, dst_x, dst_y, dst_ptr, dst_edge_ptr,
                  dst_batch);
    if (!stage_args_ok(kExactSlot, ctl, sched_cap, status, nullptr, s, d, 0)) return QOT_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    stage_plan_kernel<false><<<1, 256, 0, st>>>(ctl, sched_cap, status, node_ptr, edge_ptr, G, N_total, E_total, B, N, E,
                                                max_nodes, max_edges, 0);
    QOT_LAUNCH_CHECK();
    stage_copy_kernel<<<stage_grid(B, N, E, D, F, Y), 256, 0, st>>>(ctl, status, s, d);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

extern "C" int qot_shard_stage_padded(int64_t* ctl, int64_t sched_cap, int32_t* status, const int64_t* node_ptr,
                                      const int64_t* edge_ptr, const int64_t* graph_of_node, int64_t G, int64_t N_total,
                                      int64_t E_total, const int64_t* edge_index, const void* edge_attr, int D,
                                      const int64_t* node_ids, const void* x, int F, const void* y, int Y, int64_t B,
                                      int64_t n, int64_t E_cap, int64_t P, int64_t max_edges, int64_t V,
                                      int64_t* dst_edge_index, void* dst_edge_attr, int64_t* dst_node_ids, void* dst_x,
                                      void* dst_y, int64_t* dst_ptr, int64_t* dst_edge_ptr, int64_t* dst_batch,
                                      qot_stream_t stream) {
    StageShard s;
    StageSlot d;
    stage_structs(s, d, node_ptr, edge_ptr, graph_of_node, G, N_total, E_total, edge_index, edge_attr, D, node_ids, x, F, y, Y, B,
                  0, E_cap, n, max_edges, V, dst_edge_index, dst_edge_attr, dst_node_ids, dst_x, dst_y, dst_ptr, dst_edge_ptr,
                  dst_batch);
    if (!stage_args_ok(kPaddedSlot, ctl, sched_cap, status, nullptr, s, d, P)) return QOT_ERR_BADARG;
    d.N = B * n;
    hipStream_t st = (hipStream_t)stream;
    stage_plan_kernel<true><<<1, 256, 0, st>>>(ctl, sched_cap, status, node_ptr, edge_ptr, G, N_total, E_total, B, d.N, E_cap,
                                               n, max_edges, P * max_edges);
    QOT_LAUNCH_CHECK();
    stage_copy_padded_kernel<<<stage_grid(B + P, (B + P) * n, E_cap, D, F, Y), 256, 0, st>>>(ctl, status, s, d, P);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

// groups of kGatherLanes lanes: one per graph, at most 2048 workgroups (8 per CU); the pad part needs no more
static int stage_gather_grid(int64_t B) {
    const int64_t per_block = 256 / kGatherLanes;
    int64_t grid = (B + per_block - 1) / per_block;
    if (grid < 1) grid = 1;
    if (grid > 2048) grid = 2048;
    return (int)grid;
}

extern "C" int qot_shard_stage_gather(int64_t* ctl, int64_t sched_cap, int32_t* status, int64_t* offs, const int64_t* node_ptr,
                                      const int64_t* edge_ptr, int64_t G, int64_t N_total, int64_t E_total,
                                      const int64_t* edge_index, const void* edge_attr, int D, const int64_t* node_ids,
                                      const void* x, int F, const void* y, int Y, int64_t B, int64_t n, int64_t E_cap, int64_t P,
                                      int64_t max_edges, int64_t V, int64_t* dst_edge_index, void* dst_edge_attr,
                                      int64_t* dst_node_ids, void* dst_x, void* dst_y, int64_t* dst_ptr, int64_t* dst_edge_ptr,
                                      int64_t* dst_batch, qot_stream_t stream) {
    StageShard s;
    StageSlot d;
    stage_structs(s, d, node_ptr, edge_ptr, nullptr, G, N_total, E_total, edge_index, edge_attr, D, node_ids, x, F, y, Y, B, 0,
                  E_cap, n, max_edges, V, dst_edge_index, dst_edge_attr, dst_node_ids, dst_x, dst_y, dst_ptr, dst_edge_ptr,
                  dst_batch);
    if (!stage_args_ok(kGatherSlot, ctl, sched_cap, status, offs, s, d, P)) return QOT_ERR_BADARG;
    d.N = B * n;
    hipStream_t st = (hipStream_t)stream;
    stage_plan_gather_kernel<<<1, 256, 0, st>>>(ctl, sched_cap, status, offs, node_ptr, edge_ptr, G, N_total, E_total, B, n, E_cap,
                                                max_edges, P * max_edges);
    QOT_LAUNCH_CHECK();
    stage_copy_gather_kernel<<<stage_gather_grid(B), 256, 0, st>>>(ctl, offs, status, s, d, P);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
