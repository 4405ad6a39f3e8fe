// Graph construction on the device: network-status samples data[S, P, L, Q] (fp64) -> the lightpath and the
// topological graph representation, packed as a PackedGraphs shard.  Host counterpart:
// to_graph.create_*_graph + dataset.*_data_from_graph + PackedGraphs.from_data_list.
//
// One workgroup (256 threads) per sample, two launches with the single host read between them:
//   count  scans the channels in order c = l * Q + q, 256 at a time: occupied = any of the P values != 0; the distinct
//          trunc(conn_id) values are appended, in first-seen order, to an LDS table (conn, first channel).
//          lightpath:   every channel's lightpath number goes to a 2-byte-per-channel workspace; then one wave per link
//                       tests all slot pairs of the link (fp64 |f1 - f2|, strict compares) and sets bits of a
//                       256 x 256 adjacency bit matrix in LDS.  Links with fewer than two distinct lightpaths are
//                       skipped, as the host does.
//          topological: every lightpath reads src/dst of its first channel; among the lightpaths of one unordered
//                       node pair the one with the largest conn wins; winners go to a 75 x 75 matrix.
//          The matrix and the first-channel table go to the sample's scratch slot; (nodes, links) to info[].
//   fill   after the host has read info[] and allocated the outputs: walks the matrix row-major -- which is the
//          canonical (source, target) order -- and writes edge_index, x / edge_attr, node_ids, y.
// Everything a sample produces depends on that sample alone, so a graph is bit-identical in any chunk.
//
// Scaling is (v - min) / (max - min) in fp64 (IEEE division), one rounding to fp32; the file is compiled with
// -ffp-contract=off.  The scan, the table, the scaling, the topological pair contest and the walk's runs are
// status_scan_dev.hpp's, shared with infer_lightpath_status.hip and infer_topological_status.hip (4.21).
#include "status_scan_dev.hpp"

namespace qot {
namespace sg {

// (the workgroup's geometry, kCap / kQCap, kTopo / kCells, the first-seen table, discover(), sample_of(), scaled(), the block
// scan, the pair contest topo_winners() and the walk's run topo_run(): status_scan_dev.hpp)
constexpr int kAdjWords = kCap * kCap / 32;      // 2048

// scratch slot of one sample: first[kCap] int32, then the matrix (adjacency bits or int16 winners)
constexpr size_t kMatBytes = kCells * 2 > kAdjWords * 4 ? (size_t)((kCells * 2 + 15) / 16 * 16) : (size_t)kAdjWords * 4;
constexpr size_t kSlotBytes = (size_t)kCap * 4 + kMatBytes;

struct CountArgs {
    const double* data;
    const double* freq;
    const int64_t* samples;
    int64_t S;
    int P, L, Q;
    int conn_row, src_row, dst_row;
    double thr;
    char* scratch;
    int16_t* chan;
    int32_t* info;
};

__global__ __launch_bounds__(kThreads) void count_lightpath(CountArgs a) {
    __shared__ Table T;
    __shared__ double freq[kQCap];
    __shared__ int16_t row[kWaves][kQCap];
    __shared__ uint32_t adj[kAdjWords];
    __shared__ int part[kWaves + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t g = blockIdx.x;
    int32_t* first_out = reinterpret_cast<int32_t*>(a.scratch + (size_t)g * kSlotBytes);
    uint32_t* adj_out = reinterpret_cast<uint32_t*>(a.scratch + (size_t)g * kSlotBytes + (size_t)kCap * 4);
    bool ok;
    const int64_t s = sample_of(a.samples, g, a.S, ok);
    if (!ok) {                                                     // block-uniform
        if (tid == 0) {
            atomicOr(&a.info[0], QOT_SG_BAD_SAMPLE);
            a.info[2 + 2 * g] = 0;
            a.info[3 + 2 * g] = 0;
        }
        return;
    }
    const int LQ = a.L * a.Q;
    const double* d = a.data + s * (int64_t)a.P * LQ;
    int16_t* chan = a.chan + g * (int64_t)LQ;
    for (int q = tid; q < a.Q; q += kThreads) freq[q] = a.freq[q];
    for (int k = tid; k < kAdjWords; k += kThreads) adj[k] = 0u;
    int bad = discover(d, a.P, LQ, a.conn_row, T, chan);            // ends with a barrier: chan is visible to the block
    const int n = T.n;
    // one wave per link: all pairs of occupied slots
    for (int l0 = 0; l0 < a.L; l0 += kWaves) {
        const int l = l0 + w;
        int lo = kCap, hi = -1;
        if (l < a.L) {
            for (int q = lane; q < a.Q; q += 64) {
                const int v = chan[(int64_t)l * a.Q + q];
                row[w][q] = (int16_t)v;
                if (v >= 0) {
                    lo = v < lo ? v : lo;
                    hi = v > hi ? v : hi;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int tl = __shfl_xor(lo, o), th = __shfl_xor(hi, o);
                lo = tl < lo ? tl : lo;
                hi = th > hi ? th : hi;
            }
        }
        __syncthreads();                                           // the wave's row is complete
        if (l < a.L) {
            if (hi > lo) {                                         // two distinct lightpaths at least
                for (int q1 = lane; q1 < a.Q; q1 += 64) {
                    const int v1 = row[w][q1];
                    if (v1 < 0) continue;
                    const double f1 = freq[q1];
                    for (int q2 = q1 + 1; q2 < a.Q; ++q2) {
                        const int v2 = row[w][q2];
                        if (v2 < 0) continue;
                        const double df = fabs(f1 - freq[q2]);
                        if (df > 0.0 && df < a.thr) {
                            atomicOr(&adj[v1 * (kCap / 32) + (v2 >> 5)], 1u << (v2 & 31));
                            atomicOr(&adj[v2 * (kCap / 32) + (v1 >> 5)], 1u << (v1 & 31));
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    // degree of row tid, self loop, totals
    int deg = 0;
#pragma unroll
    for (int k = 0; k < kCap / 32; ++k) deg += __popc(adj[tid * (kCap / 32) + k]);
    const bool self = (adj[tid * (kCap / 32) + (tid >> 5)] >> (tid & 31)) & 1u;
    int total;
    (void)block_exscan(deg, part, total);
    first_out[tid] = tid < n ? T.first[tid] : 0;
    for (int k = tid; k < kAdjWords; k += kThreads) adj_out[k] = adj[k];
    if (bad) atomicOr(&a.info[0], bad);
    if (self) atomicOr(&a.info[1], 1);
    if (tid == 0) {
        a.info[2 + 2 * g] = n;
        a.info[3 + 2 * g] = total;
    }
}

__global__ __launch_bounds__(kThreads) void count_topological(CountArgs a) {
    __shared__ Table T;
    __shared__ int16_t mat[kCells];
    __shared__ uint8_t eu[kCap], ev[kCap];
    __shared__ int part[kWaves + 1];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    int32_t* first_out = reinterpret_cast<int32_t*>(a.scratch + (size_t)g * kSlotBytes);
    int16_t* mat_out = reinterpret_cast<int16_t*>(a.scratch + (size_t)g * kSlotBytes + (size_t)kCap * 4);
    bool ok;
    const int64_t s = sample_of(a.samples, g, a.S, ok);
    if (!ok) {
        if (tid == 0) {
            atomicOr(&a.info[0], QOT_SG_BAD_SAMPLE);
            a.info[2 + 2 * g] = 0;
            a.info[3 + 2 * g] = 0;
        }
        return;
    }
    const int LQ = a.L * a.Q;
    const double* d = a.data + s * (int64_t)a.P * LQ;
    for (int k = tid; k < kCells; k += kThreads) mat[k] = -1;
    int bad = discover(d, a.P, LQ, a.conn_row, T, nullptr);
    const int n = T.n;
    bad |= topo_winners(d, LQ, a.src_row, a.dst_row, T, n, mat, eu, ev);
    int cnt = 0, self = 0;
    for (int k = tid; k < kCells; k += kThreads)
        if (mat[k] >= 0) {
            ++cnt;
            self |= (k / kTopo == k % kTopo);
        }
    int total;
    (void)block_exscan(cnt, part, total);
    first_out[tid] = tid < n ? T.first[tid] : 0;
    for (int k = tid; k < kCells; k += kThreads) mat_out[k] = mat[k];
    if (bad) atomicOr(&a.info[0], bad);
    if (self) atomicOr(&a.info[1], 1);
    if (tid == 0) {
        a.info[2 + 2 * g] = kTopo;
        a.info[3 + 2 * g] = total;
    }
}

struct FillArgs {
    const double* data;
    const double* target;
    const int64_t* samples;
    int64_t S;
    int P, L, Q, M;
    int osnr_row, snr_row, ber_row;
    const double* cols;       // [ncol, 4]: lp_feat row (-1 = is_lut), min, max - min, has_range
    int ncol;
    const double* tcols;      // [3, 4]: target column (-1 = absent, reads 0.0), min, max - min, has_range
    const char* scratch;
    const int32_t* info;
    const int64_t* node_ptr;
    const int64_t* edge_ptr;
    int64_t n_total, e_total;
    int64_t* edge_index;      // [2, e_total]
    float* feat;              // lightpath: x [n_total, ncol]; topological: edge_attr [e_total, ncol]
    int64_t* node_ids;        // topological: [n_total]
    float* y;                 // [G, 3]
};

__device__ __forceinline__ void fill_y(const FillArgs& a, int64_t g, int64_t s) {
    if (threadIdx.x < 3) {
        const double* col = a.tcols + 4 * threadIdx.x;
        const int m = (int)col[0];
        const double v = (m >= 0 && m < a.M) ? a.target[s * a.M + m] : 0.0;
        a.y[g * 3 + threadIdx.x] = scaled(v, col);
    }
}

__global__ __launch_bounds__(kThreads) void fill_lightpath(FillArgs a) {
    __shared__ uint32_t adj[kAdjWords];
    __shared__ int part[kWaves + 1];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    bool ok;
    const int64_t s = sample_of(a.samples, g, a.S, ok);
    if (!ok) return;
    const int32_t* first = reinterpret_cast<const int32_t*>(a.scratch + (size_t)g * kSlotBytes);
    const uint32_t* adj_in = reinterpret_cast<const uint32_t*>(a.scratch + (size_t)g * kSlotBytes + (size_t)kCap * 4);
    const int n = a.info[2 + 2 * g], m = a.info[3 + 2 * g];
    const int64_t nb = a.node_ptr[g], eb = a.edge_ptr[g];
    // the offsets are the host's prefix sums of info[]: refuse to write when they do not match
    if (n < 0 || n > kCap || m < 0 || nb < 0 || eb < 0 || a.node_ptr[g + 1] - nb != n || a.edge_ptr[g + 1] - eb != m ||
        nb + n > a.n_total || eb + m > a.e_total)
        return;
    const int LQ = a.L * a.Q;
    const double* d = a.data + s * (int64_t)a.P * LQ;
    for (int k = tid; k < kAdjWords; k += kThreads) adj[k] = adj_in[k];
    fill_y(a, g, s);
    if (tid < n) {
        const int c = first[tid];
        if (c >= 0 && c < LQ) {
            for (int k = 0; k < a.ncol; ++k)
                a.feat[(nb + tid) * a.ncol + k] = sg_feature(d, a.P, LQ, a.osnr_row, a.snr_row, a.ber_row, a.cols, k, c);
        }
    }
    __syncthreads();
    int deg = 0;
#pragma unroll
    for (int k = 0; k < kCap / 32; ++k) deg += __popc(adj[tid * (kCap / 32) + k]);
    int total;
    int e = block_exscan(deg, part, total);
    if (total != m) return;
    for (int k = 0; k < kCap / 32; ++k) {
        uint32_t bits = adj[tid * (kCap / 32) + k];
        while (bits) {
            const int b = k * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            a.edge_index[eb + e] = nb + tid;
            a.edge_index[a.e_total + eb + e] = nb + b;
            ++e;
        }
    }
}

__global__ __launch_bounds__(kThreads) void fill_topological(FillArgs a) {
    __shared__ int16_t mat[kCells];
    __shared__ int part[kWaves + 1];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    bool ok;
    const int64_t s = sample_of(a.samples, g, a.S, ok);
    if (!ok) return;
    const int32_t* first = reinterpret_cast<const int32_t*>(a.scratch + (size_t)g * kSlotBytes);
    const int16_t* mat_in = reinterpret_cast<const int16_t*>(a.scratch + (size_t)g * kSlotBytes + (size_t)kCap * 4);
    const int n = a.info[2 + 2 * g], m = a.info[3 + 2 * g];
    const int64_t nb = a.node_ptr[g], eb = a.edge_ptr[g];
    if (n != kTopo || m < 0 || nb < 0 || eb < 0 || a.node_ptr[g + 1] - nb != n || a.edge_ptr[g + 1] - eb != m ||
        nb + n > a.n_total || eb + m > a.e_total)
        return;
    const int LQ = a.L * a.Q;
    const double* d = a.data + s * (int64_t)a.P * LQ;
    for (int k = tid; k < kCells; k += kThreads) mat[k] = mat_in[k];
    fill_y(a, g, s);
    if (tid < kTopo) a.node_ids[nb + tid] = tid;
    __syncthreads();
    // thread t owns a contiguous run of cells: row-major order is (source, target) order
    int k0, k1;
    const int cnt = topo_run(mat, k0, k1);
    int total;
    int e = block_exscan(cnt, part, total);
    if (total != m) return;
    for (int k = k0; k < k1; ++k) {
        const int i = mat[k];
        if (i < 0) continue;
        a.edge_index[eb + e] = nb + k / kTopo;
        a.edge_index[a.e_total + eb + e] = nb + k % kTopo;
        const int c = i < kCap ? first[i] : -1;
        if (c >= 0 && c < LQ)
            for (int j = 0; j < a.ncol; ++j) {
                const double* col = a.cols + 4 * j;
                const int r = (int)col[0];
                a.feat[(eb + e) * a.ncol + j] = (r >= 0 && r < a.P) ? scaled(d[(int64_t)r * LQ + c], col) : 0.0f;
            }
        ++e;
    }
}

inline bool shape_ok(int64_t G, int64_t S, int P, int64_t L, int64_t Q) {
    return G >= 0 && S >= 0 && P >= 1 && L >= 1 && Q >= 1;
}

}  // namespace sg
}  // namespace qot

using namespace qot;

extern "C" size_t qot_status_graph_scratch_bytes(int64_t G, int64_t L, int64_t Q, int representation) {
    if (G < 0 || L < 0 || Q < 0) return 0;
    size_t bytes = (size_t)G * sg::kSlotBytes;
    if (representation == QOT_SG_LIGHTPATH) bytes += ((size_t)G * (size_t)L * (size_t)Q * 2 + 15) / 16 * 16;
    return bytes;
}

extern "C" int qot_status_graph_count(const double* data, const double* freq, const int64_t* samples, int64_t G, int64_t S,
                                      int P, int64_t L, int64_t Q, int conn_row, int src_row, int dst_row,
                                      double freq_threshold, int representation, void* scratch, size_t scratch_bytes,
                                      int32_t* info, qot_stream_t stream) {
    if (!sg::shape_ok(G, S, P, L, Q)) return QOT_ERR_BADARG;
    if (representation != QOT_SG_LIGHTPATH && representation != QOT_SG_TOPOLOGICAL) return QOT_ERR_UNSUPPORTED;
    if (Q > QOT_SG_MAX_FREQS || L * Q >= (int64_t)1 << 31 || G >= (int64_t)1 << 31) return QOT_ERR_UNSUPPORTED;
    if (conn_row < 0 || conn_row >= P) return QOT_ERR_BADARG;
    if (representation == QOT_SG_TOPOLOGICAL && (src_row < 0 || src_row >= P || dst_row < 0 || dst_row >= P)) return QOT_ERR_BADARG;
    if (G == 0) return QOT_OK;
    if (!data || !freq || !scratch || !info || S == 0) return QOT_ERR_BADARG;
    if (scratch_bytes < qot_status_graph_scratch_bytes(G, L, Q, representation)) return QOT_ERR_BADARG;
    sg::CountArgs a;
    a.data = data; a.freq = freq; a.samples = samples; a.S = S; a.P = P; a.L = (int)L; a.Q = (int)Q;
    a.conn_row = conn_row; a.src_row = src_row; a.dst_row = dst_row; a.thr = freq_threshold;
    a.scratch = static_cast<char*>(scratch);
    a.chan = reinterpret_cast<int16_t*>(static_cast<char*>(scratch) + (size_t)G * sg::kSlotBytes);
    a.info = info;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (representation == QOT_SG_LIGHTPATH)
        hipLaunchKernelGGL(sg::count_lightpath, dim3((unsigned)G), dim3(sg::kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(sg::count_topological, dim3((unsigned)G), dim3(sg::kThreads), 0, st, a);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}

extern "C" int qot_status_graph_fill(const double* data, const double* target, const int64_t* samples, int64_t G, int64_t S,
                                     int P, int64_t L, int64_t Q, int M, int osnr_row, int snr_row, int ber_row,
                                     const double* cols, int ncol, const double* tcols, int representation,
                                     const void* scratch, const int32_t* info, const int64_t* node_ptr,
                                     const int64_t* edge_ptr, int64_t n_total, int64_t e_total, int64_t* edge_index,
                                     float* feat, int64_t* node_ids, float* y, qot_stream_t stream) {
    if (!sg::shape_ok(G, S, P, L, Q) || M < 0 || ncol < 0 || n_total < 0 || e_total < 0) return QOT_ERR_BADARG;
    if (representation != QOT_SG_LIGHTPATH && representation != QOT_SG_TOPOLOGICAL) return QOT_ERR_UNSUPPORTED;
    if (Q > QOT_SG_MAX_FREQS || L * Q >= (int64_t)1 << 31 || G >= (int64_t)1 << 31) return QOT_ERR_UNSUPPORTED;
    if (representation == QOT_SG_LIGHTPATH &&
        (osnr_row < 0 || osnr_row >= P || snr_row < 0 || snr_row >= P || ber_row < 0 || ber_row >= P))
        return QOT_ERR_BADARG;
    if (G == 0) return QOT_OK;
    if (!data || !target || !tcols || !scratch || !info || !node_ptr || !edge_ptr || !y || S == 0) return QOT_ERR_BADARG;
    if (ncol > 0 && (!cols || !feat) && (representation == QOT_SG_LIGHTPATH ? n_total > 0 : e_total > 0)) return QOT_ERR_BADARG;
    if (e_total > 0 && !edge_index) return QOT_ERR_BADARG;
    if (representation == QOT_SG_TOPOLOGICAL && !node_ids) return QOT_ERR_BADARG;
    sg::FillArgs a;
    a.data = data; a.target = target; a.samples = samples; a.S = S; a.P = P; a.L = (int)L; a.Q = (int)Q; a.M = M;
    a.osnr_row = osnr_row; a.snr_row = snr_row; a.ber_row = ber_row; a.cols = cols; a.ncol = ncol; a.tcols = tcols;
    a.scratch = static_cast<const char*>(scratch); a.info = info; a.node_ptr = node_ptr; a.edge_ptr = edge_ptr;
    a.n_total = n_total; a.e_total = e_total; a.edge_index = edge_index; a.feat = feat; a.node_ids = node_ids; a.y = y;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (representation == QOT_SG_LIGHTPATH)
        hipLaunchKernelGGL(sg::fill_lightpath, dim3((unsigned)G), dim3(sg::kThreads), 0, st, a);
    else
        hipLaunchKernelGGL(sg::fill_topological, dim3((unsigned)G), dim3(sg::kThreads), 0, st, a);
    QOT_LAUNCH_CHECK();
    return QOT_OK;
}
