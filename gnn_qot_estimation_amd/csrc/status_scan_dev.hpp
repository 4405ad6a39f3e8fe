// The scan of one network-status sample data[P, L, Q] (fp64) by one 256-thread workgroup, shared by the graph builder
// (status_graph.hip) and the status-to-row kernels (infer_lightpath_status.hip, DESIGN.md 4.20;
// infer_topological_status.hip; infer_lightpath_place.hip; infer_topological_place.hip,
// DESIGN.md 4.23; the two *_place_release.hip files): all run discover(), so the lightpaths of a sample,
// their numbering and their first channels are the same table in all.  Stated once here: the workgroup's geometry and caps, the first-seen
// table and its insert, the sample pick, the occupancy / conn rule of one channel (sg_conn, channel_conn), the fp64 column scaling
// (scaled), a candidate's and a release's kernel arguments for both models (PlaceArgs, ReleaseArgs), the release rule of
// place(release=...), which does not depend on the model (the LDS struct Release and the release_* routines; the lightpath
// scan runs them, infer_topological_place_release.hip states why it does not yet) and, for the topological representation,
// the block scan, the pair contest that fills the 75 x 75 winner matrix (topo_winners) and the row-major run of cells a
// thread walks (topo_run).
//
// Channels are scanned in the order c = l * Q + q, 256 at a time: occupied = any of the P values != 0; the distinct
// trunc(conn_id) values are appended, in first-seen order, to an LDS table (conn, first channel).
//
// Scaling is (v - min) / (max - min) in fp64 (IEEE division), one rounding to fp32.  The expression holds a subtraction
// and a division, nothing a contraction could fuse; `scaled` is compiled under `fp contract(off)` all the same, so it is
// the same code in a translation unit built with -ffp-contract=off (status_graph.hip) and in one that is not.
#pragma once
#include "common.hpp"

namespace qot {
namespace sg {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kCap = QOT_SG_MAX_LIGHTPATHS;      // 256
constexpr int kQCap = QOT_SG_MAX_FREQS;          // 1024
constexpr int kTopo = QOT_SG_NODES;              // 75
constexpr int kCells = kTopo * kTopo;            // 5625
static_assert(kCap == kThreads, "one thread per lightpath / adjacency row");

__device__ __forceinline__ int wave_prefix(uint64_t mask) {      // set bits of mask below this lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

struct Table {
    int64_t conn[kCap];
    int32_t first[kCap];
    int64_t chunk_conn[kThreads];
    unsigned long long new_mask[kWaves];
    int wave_new[kWaves];
    int n;
};

// The conn of a channel whose conn_id value is cv: false when the value is NaN, inf or beyond +-2^53 (the channel then
// counts as empty and the caller flags QOT_SG_BAD_CONN); truncation, as int(...) does.
__device__ __forceinline__ bool sg_conn(double cv, int64_t& conn) {
    if (!(fabs(cv) <= 9007199254740992.0)) return false;
    conn = (int64_t)cv;
    return true;
}

// whether channel c is occupied, and by which conn (bad conn values: the sample has been refused before this is asked)
__device__ __forceinline__ bool channel_conn(const double* __restrict__ d, int P, int LQ, int conn_row, int c, int64_t& conn) {
    const double cv = d[(int64_t)conn_row * LQ + c];
    if (cv != 0.0) return sg_conn(cv, conn);
    bool occ = false;
    for (int p = 0; p < P; ++p) occ |= (d[(int64_t)p * LQ + c] != 0.0);
    conn = 0;
    return occ;
}

// The lightpaths of one sample in first-seen order.  chan (optional): lightpath number of every channel, -1 when the
// channel is empty.  Returns status bits.
__device__ int discover(const double* __restrict__ d, int P, int LQ, int conn_row, Table& T, int16_t* __restrict__ chan) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int bad = 0;
    if (tid == 0) T.n = 0;
    __syncthreads();
    for (int base = 0; base < LQ; base += kThreads) {
        const int c = base + tid;
        bool occ = false;
        int64_t conn = 0;
        if (c < LQ) {
            for (int p = 0; p < P; ++p) occ |= (d[(int64_t)p * LQ + c] != 0.0);
            if (occ) {
                const double cv = d[(int64_t)conn_row * LQ + c];
                if (!sg_conn(cv, conn)) {                          // NaN, inf or beyond +-2^53
                    bad |= QOT_SG_BAD_CONN;
                    occ = false;
                }
            }
        }
        const int n0 = T.n;
        int idx = -1;
        if (occ)
            for (int i = 0; i < n0; ++i)
                if (T.conn[i] == conn) { idx = i; break; }
        const bool isnew = occ && idx < 0;
        T.chunk_conn[tid] = conn;
        const unsigned long long m = __ballot(isnew);
        if (lane == 0) T.new_mask[w] = m;
        __syncthreads();
        // the first channel of the chunk with this conn appends it
        bool first = isnew;
        if (isnew) {
            for (int ww = 0; ww <= w && first; ++ww) {
                unsigned long long mm = T.new_mask[ww];
                if (ww == w) mm &= (1ull << lane) - 1ull;
                while (mm) {
                    const int j = ww * 64 + __builtin_ctzll(mm);
                    mm &= mm - 1;
                    if (T.chunk_conn[j] == conn) { first = false; break; }
                }
            }
        }
        const unsigned long long fm = __ballot(first);
        if (lane == 0) T.wave_new[w] = __popcll(fm);
        __syncthreads();
        int rank = wave_prefix(fm), total = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            const int p = T.wave_new[k];
            if (k < w) rank += p;
            total += p;
        }
        if (first) {
            const int slot = n0 + rank;
            if (slot < kCap) {
                T.conn[slot] = conn;
                T.first[slot] = c;
                idx = slot;
            } else {
                bad |= QOT_SG_TOO_MANY;
            }
        }
        __syncthreads();                                           // table complete; everybody has read T.n
        const int n1 = n0 + total < kCap ? n0 + total : kCap;
        if (tid == 0) T.n = n1;
        if (isnew && !first)
            for (int i = n0; i < n1; ++i)
                if (T.conn[i] == conn) { idx = i; break; }
        if (chan && c < LQ) chan[c] = (int16_t)idx;
        __syncthreads();
    }
    return bad;
}

__device__ __forceinline__ int64_t sample_of(const int64_t* samples, int64_t g, int64_t S, bool& ok) {
    const int64_t s = samples ? samples[g] : g;
    ok = s >= 0 && s < S;
    return s;
}

// ---- a candidate lightpath and a release, for both models' place kernels ----
// One candidate of a predictor's place: the raw lp_feat vector values[k] in the channels cells[:, cell_ptr[k] :
// cell_ptr[k + 1]] of sample samples[k]
struct PlaceArgs {
    const double* values;               // [K, P] raw lp_feat vectors
    const int64_t* cells;               // [2, M]: link indices, then frequency indices
    const int64_t* cell_ptr;            // [K + 1]
    int64_t M;
};

// place(release=...): the lightpaths of candidate k's sample with one of the conns release[release_ptr[k] :
// release_ptr[k + 1]] are gone before it is placed.  A kernel parameter of the two release kernels only.
struct ReleaseArgs {
    const int64_t* release;             // [R] conn_id values
    const int64_t* release_ptr;         // [K + 1]
    int64_t R;
};

constexpr int kMaxRelease = QOT_PLACE_MAX_RELEASE;   // 32

// the LDS state of one candidate's release: the slice, its ticks, who is gone
struct Release {
    int64_t rel[kMaxRelease];
    unsigned long long gone_mask[kWaves];
    uint8_t gone[kCap];
    uint8_t found[kMaxRelease];
};

// The routines below state the rule and return conditions; the caller maps them to its model's status bits.
// the slice of candidate k, checked against [0, R] and the cap before `release` is read: its length, or -1 (bad slice)
__device__ __forceinline__ int release_slice(const ReleaseArgs& rl, int64_t k, int64_t& rlo) {
    rlo = rl.release_ptr[k];
    const int64_t rhi = rl.release_ptr[k + 1];
    return (rlo < 0 || rhi < rlo || rhi > rl.R || rhi - rlo > kMaxRelease) ? -1 : (int)(rhi - rlo);
}

// the slice -> LDS, nothing ticked (visible behind the caller's next barrier)
__device__ __forceinline__ void release_load(Release& rs, const ReleaseArgs& rl, int64_t rlo, int nr) {
    const int tid = threadIdx.x;
    if (tid < nr) {
        rs.rel[tid] = rl.release[rlo + tid];
        rs.found[tid] = 0;
    }
}

// Thread t and lightpath t (mine: t < n; conn: its conn): every slice entry that names it is ticked (a conn named twice:
// both entries), gone[t] and the wave's gone mask are written.  Returns whether the lightpath survives.
__device__ __forceinline__ bool release_match(Release& rs, int nr, bool mine, int64_t conn) {
    const int tid = threadIdx.x;
    bool g = false;
    if (mine)
        for (int j = 0; j < nr; ++j)
            if (rs.rel[j] == conn) {
                g = true;
                rs.found[j] = 1;
            }
    rs.gone[tid] = g ? 1 : 0;
    const unsigned long long gm = __ballot(g);
    if ((tid & 63) == 0) rs.gone_mask[tid >> 6] = gm;
    return mine && !g;
}

// behind the barrier that follows release_match: how many lightpaths are gone and the first gone one's number (-1: nobody)
__device__ __forceinline__ int release_gone(const Release& rs, int& first) {
    int n_gone = 0;
    first = -1;
#pragma unroll
    for (int j = kWaves - 1; j >= 0; --j) {
        const unsigned long long m = rs.gone_mask[j];
        n_gone += __popcll(m);
        if (m) first = j * kWave + __builtin_ctzll(m);
    }
    return n_gone;
}

// behind the same barrier: thread t's slice entry met no lightpath of the sample
__device__ __forceinline__ bool release_unmatched(const Release& rs, int nr) { return (int)threadIdx.x < nr && !rs.found[threadIdx.x]; }

// one wave: is the owner (conn) of an occupied channel gone?  The wave's lanes share the table.
__device__ __forceinline__ bool release_freed(const Release& rs, const Table& T, int n, int64_t conn, int lane) {
    bool freed = false;
    for (int i = lane; i < n; i += kWave) freed |= (T.conn[i] == conn && rs.gone[i] != 0);
    return __any(freed);
}

// the is_lut flag of a lightpath: osnr == snr == ber == -1 on its first channel c
__device__ __forceinline__ bool sg_is_lut(const double* __restrict__ d, int LQ, int osnr_row, int snr_row, int ber_row, int c) {
    return d[(int64_t)osnr_row * LQ + c] == -1.0 && d[(int64_t)snr_row * LQ + c] == -1.0 && d[(int64_t)ber_row * LQ + c] == -1.0;
}

// one output column: col = (lp_feat row, min, max - min, has_range)
__device__ __forceinline__ float scaled(double v, const double* col) {
#pragma clang fp contract(off)
    if (col[3] != 0.0) v = (v - col[1]) / col[2];
    return (float)v;
}

// column k of the feature row of the lightpath whose first channel is c (cols [ncol, 4]; lp_feat row -1: is_lut; a row
// outside the P rows of data reads as 0)
__device__ __forceinline__ float sg_feature(const double* __restrict__ d, int P, int LQ, int osnr_row, int snr_row, int ber_row,
                                            const double* __restrict__ cols, int k, int c) {
    const double* col = cols + 4 * k;
    const int r = (int)col[0];
    if (r < 0) return sg_is_lut(d, LQ, osnr_row, snr_row, ber_row, c) ? 1.0f : 0.0f;
    return r < P ? scaled(d[(int64_t)r * LQ + c], col) : 0.0f;
}

// The same two for a lightpath that is not in the sample: v is its raw lp_feat vector [P] (LightpathPredictor.place's
// candidate, infer_lightpath_place.hip).  The doubles that reach `scaled` are those a channel holding v would give.
__device__ __forceinline__ bool sg_is_lut_vec(const double* __restrict__ v, int osnr_row, int snr_row, int ber_row) {
    return v[osnr_row] == -1.0 && v[snr_row] == -1.0 && v[ber_row] == -1.0;
}

__device__ __forceinline__ float sg_feature_vec(const double* __restrict__ v, int P, int osnr_row, int snr_row, int ber_row,
                                                const double* __restrict__ cols, int k) {
    const double* col = cols + 4 * k;
    const int r = (int)col[0];
    if (r < 0) return sg_is_lut_vec(v, osnr_row, snr_row, ber_row) ? 1.0f : 0.0f;
    return r < P ? scaled(v[r], col) : 0.0f;
}

// exclusive prefix of v over the block's threads (thread order) and the block total; `part` holds kWaves + 1 ints
__device__ __forceinline__ int block_exscan(int v, int* part, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                  // part may still be read from an earlier call
    if (lane == 63) part[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const int p = part[k];
        if (k < w) base += p;
        tot += p;
    }
    total = tot;
    return base + inc - v;
}

// ---- the topological representation: which lightpath gives the link of every node pair.  Thread t reads the end nodes of
// lightpath t (t < n = T.n) on its first channel; among the lightpaths of one unordered node pair the one with the largest
// conn wins, and its number goes to mat[u][v] and mat[v][u] (a self loop: the one cell).  mat [kCells] holds -1 everywhere
// on entry; eu / ev [kCap] are scratch.  Nothing read from data is used as an index before the 1 .. 75 test.  Returns
// QOT_SG_BAD_ENDPOINT or 0 (per thread); ends with a barrier, behind which mat is complete.
// cand (optional): the raw lp_feat vector of one more lightpath that the sample does not hold (TopologicalPredictor.place's
// candidate, infer_topological_place.hip).  It joins the contest as lightpath n: the caller has n < kCap and its conn,
// distinct from the sample's, in T.conn[n]; thread n takes its end nodes from cand under the same test.
// gone (optional, [kCap] bytes): lightpaths released from the sample before the candidate is placed
// (infer_topological_place_release.hip).  A gone lightpath is not usable before its end nodes are looked at: it contests no
// pair and its end nodes flag nothing.  slot (with cand; -1: n, as above): the table slot the candidate takes instead -- a
// gone lightpath's, so that a full table still has room for it; the caller has its conn in T.conn[slot].
__device__ __forceinline__ int topo_winners(const double* __restrict__ d, int LQ, int src_row, int dst_row, const Table& T,
                                            int n, int16_t* mat, uint8_t* eu, uint8_t* ev,
                                            const double* __restrict__ cand = nullptr, const uint8_t* gone = nullptr,
                                            int slot = -1) {
    const int tid = threadIdx.x;
    int bad = 0;
    const bool is_cand = cand != nullptr && tid == (slot < 0 ? n : slot);
    if (cand && slot < 0) ++n;
    // end nodes of lightpath tid (255 = not usable)
    int u = 255, v = 255;
    if (tid < n && !(gone != nullptr && !is_cand && gone[tid] != 0)) {
        const int c = is_cand ? 0 : T.first[tid];
        const double sv = is_cand ? cand[src_row] : d[(int64_t)src_row * LQ + c];
        const double dv = is_cand ? cand[dst_row] : d[(int64_t)dst_row * LQ + c];
        // written so that a NaN fails the test
        const bool good = sv >= 1.0 && sv <= (double)kTopo && dv >= 1.0 && dv <= (double)kTopo && sv == trunc(sv) && dv == trunc(dv);
        if (good) {
            const int su = (int)sv - 1, dvv = (int)dv - 1;
            u = su < dvv ? su : dvv;
            v = su < dvv ? dvv : su;
        } else {
            bad |= QOT_SG_BAD_ENDPOINT;
        }
    }
    eu[tid] = (uint8_t)u;
    ev[tid] = (uint8_t)v;
    __syncthreads();
    if (u != 255) {
        const int64_t mine = T.conn[tid];
        bool win = true;
        for (int j = 0; j < n; ++j)
            if (eu[j] == u && ev[j] == v && T.conn[j] > mine) { win = false; break; }
        if (win) {                                                  // conn values are distinct: one winner per pair
            mat[u * kTopo + v] = (int16_t)tid;
            mat[v * kTopo + u] = (int16_t)tid;
        }
    }
    __syncthreads();
    return bad;
}

// Thread t's contiguous run [k0, k1) of the matrix's cells: row-major order is (source, target) order, so the exclusive
// scan of the runs' link counts numbers the directed links canonically.  Returns the links in the run.
constexpr int kTopoPer = (kCells + kThreads - 1) / kThreads;
__device__ __forceinline__ int topo_run(const int16_t* mat, int& k0, int& k1) {
    k0 = threadIdx.x * kTopoPer;
    k1 = k0 + kTopoPer < kCells ? k0 + kTopoPer : kCells;
    int cnt = 0;
    for (int k = k0; k < k1; ++k) cnt += mat[k] >= 0;
    return cnt;
}

}  // namespace sg
}  // namespace qot
