// TopologicalPredictor.place(release=...): the eval-mode TopologicalGNN row of K CANDIDATE lightpaths, each placed into a
// network-status sample data[S, P, L, Q] (fp64) from which some established lightpaths are RELEASED first, in ONE launch --
// a reroute, or an admission together with a tear-down; no edited sample, no graph, nothing read back.
// Candidate k is infer_topological_place.hip's (values[k, P] into cells[:, cell_ptr[k] : cell_ptr[k + 1]] of sample
// samples[k]) plus the conns release[release_ptr[k] : release_ptr[k + 1]]: the lightpaths of its sample with one of those
// trunc(conn_id) values are gone before it is placed.  out[k] / links[k] are, bit for bit, what
// qot_topological_infer_status gives for that edited sample.  The kernel never builds it.  Releasing zeroes whole channels
// and the candidate fills channels that are free afterwards, so a survivor keeps every channel it had: its first channel,
// hence its conn, end nodes and features.  The graph is topo_winners' pair contest over the survivors and the candidate:
// a gone lightpath is not usable before its end nodes are looked at, so it contests no pair (the pair goes to the largest
// surviving conn, to the candidate, or disappears) and a bad end node of it flags nothing.  The candidate takes the table
// slot of the first gone lightpath, or slot n when nobody is gone: a table of 256 with one released has room for it.  Its
// number is free to choose: the forward sums the links in canonical (source, target) order, whatever a lightpath's number.
//
// One workgroup (256 threads) per candidate.  The candidate's and the release's arguments are status_scan_dev.hpp's
// (sg::PlaceArgs, sg::ReleaseArgs), shared with the lightpath kernels.  Steps 1 to 3 state the release rule in this file,
// over LDS arrays of its own; it is the rule status_scan_dev.hpp states as sg::release_* for the lightpath scan, and a
// change to one belongs in the other (DESIGN.md 4.24 says why the two are not one yet).
//   1  block-uniform checks of the candidate's own arguments: sample number, cell_ptr slice, conn_id, and the release_ptr
//      slice against [0, R] and the cap of 32 before `release` is read; the slice -> LDS.
//   2  discover() on the unedited sample; thread t compares lightpath t's conn with the slice (gone[t]; every slice entry
//      that meets a lightpath is ticked) and, a survivor only, with the candidate's conn.  A slice entry nobody ticked
//      refuses the candidate; so do survivors + 1 > 256.
//   3  wave w takes the cells lo + w, lo + w + 4, ...: range check first; an occupied channel is legal when its owner is
//      gone (one table lookup, the wave's lanes share the table).
//   4  topo_winners over the survivors and the candidate, then topo_status_forward.
// Cost: infer_topological_place.hip's plus O(32) compares per thread and one table lookup per occupied cell.  No
// workspace, no global scratch.  Nothing read from data, values or release is used as an index before it is checked: conns
// are only compared, the end nodes pass the 1 .. 75 test first, the cell indices come from `cells` and are range-checked
// first.  All global writes are ordinary vector stores (the status word: one atomicOr).
//
// On the device (the candidate's row is NaN, its links 0, the other rows are untouched): everything
// infer_topological_place.hip refuses, with these differences -- an occupied cell is refused only when its owner survives,
// QOT_TOPO_PLACE_CONN_TAKEN and QOT_TOPO_STATUS_BAD_ENDPOINT are tested against the survivors (and the candidate),
// QOT_TOPO_STATUS_TOO_MANY means survivors + 1 > 256 or more than 256 lightpaths in the unedited sample (the table cannot
// hold them) -- and: a released conn the sample does not hold (QOT_TOPO_PLACE_NO_SUCH_CONN); a release_ptr slice that is
// descending, beyond R or longer than 32 (QOT_TOPO_PLACE_BAD_RELEASE).
#include "infer_topological_status_dev.hpp"

namespace qot {

constexpr int kTopoMaxRelease = sg::kMaxRelease;         // 32
// the static LDS this kernel adds to kTopoStatusStatic: gone, the slice, its ticks, the gone masks
constexpr size_t kTopoReleaseStatic = sg::kCap + (size_t)kTopoMaxRelease * 9 + sg::kWaves * 8;

template <int H, int D>
__global__ __launch_bounds__(kInferThreads) void topological_infer_place_release_kernel(const InferArgs a,
                                                                                        const TopoStatusArgs st,
                                                                                        const sg::PlaceArgs pl,
                                                                                        const sg::ReleaseArgs rl) {
    static_assert(kInferThreads == sg::kThreads, "the scan and the forward share one workgroup");
    extern __shared__ float4 infer_place_release_lds_raw[];
    float* lds = reinterpret_cast<float*>(infer_place_release_lds_raw);
    __shared__ sg::Table T;
    __shared__ int16_t mat[sg::kCells];
    __shared__ uint8_t eu[sg::kCap], ev[sg::kCap];
    __shared__ int part[sg::kWaves + 1];
    __shared__ uint32_t rec[kTopoStatusLinks];
    __shared__ uint8_t gone[sg::kCap];
    __shared__ int64_t rel[kTopoMaxRelease];
    __shared__ uint8_t found[kTopoMaxRelease];
    __shared__ unsigned long long gone_mask[sg::kWaves];
    __shared__ int bad_all;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t k = blockIdx.x;
    float* orow = a.out + k * a.O;
    const double* v = pl.values + k * (int64_t)st.P;

    // ---- step 1: what the candidate's own arguments say (every value is uniform over the block) ----
    bool ok;
    const int64_t s = sg::sample_of(st.samples, k, st.S, ok);
    const int64_t lo = pl.cell_ptr[k], hi = pl.cell_ptr[k + 1];
    const int64_t rlo = rl.release_ptr[k], rhi = rl.release_ptr[k + 1];
    int64_t conn_a = 0;
    int early = ok ? 0 : QOT_TOPO_STATUS_BAD_SAMPLE;
    if (lo < 0 || hi <= lo || hi > pl.M) early |= QOT_TOPO_PLACE_BAD_CELL;
    if (rlo < 0 || rhi < rlo || rhi > rl.R || rhi - rlo > kTopoMaxRelease) early |= QOT_TOPO_PLACE_BAD_RELEASE;
    if (!sg::sg_conn(v[st.conn_row], conn_a)) early |= QOT_TOPO_STATUS_BAD_CONN;
    if (early) {                                                   // block-uniform
        topo_status_refuse(a, early, orow, st.links + k);
        return;
    }
    const int nr = (int)(rhi - rlo);                               // 0 .. 32
    const int LQ = st.L * st.Q;
    const double* d = st.data + s * (int64_t)st.P * LQ;
    for (int c = tid; c < sg::kCells; c += sg::kThreads) mat[c] = -1;
    if (tid < nr) {
        rel[tid] = rl.release[rlo + tid];
        found[tid] = 0;
    }
    if (tid == 0) bad_all = 0;

    // ---- step 2: the lightpaths of the unedited sample; who is gone; the candidate's conn among the survivors ----
    int bad = topo_status_bits(sg::discover(d, st.P, LQ, st.conn_row, T, nullptr));      // (begins and ends with a barrier)
    const int n = T.n;
    bool g = false;
    if (tid < n) {
        const int64_t conn = T.conn[tid];
        for (int j = 0; j < nr; ++j)
            if (rel[j] == conn) {                                  // (a conn named twice: both entries are ticked)
                g = true;
                found[j] = 1;
            }
        if (!g && conn == conn_a) bad |= QOT_TOPO_PLACE_CONN_TAKEN;
    }
    gone[tid] = g ? 1 : 0;
    const unsigned long long gm = __ballot(g);
    if (lane == 0) gone_mask[w] = gm;
    __syncthreads();
    int n_gone = 0, slot = -1;                                     // the first gone lightpath's slot goes to the candidate
#pragma unroll
    for (int j = sg::kWaves - 1; j >= 0; --j) {
        const unsigned long long m = gone_mask[j];
        n_gone += __popcll(m);
        if (m) slot = j * kWave + __builtin_ctzll(m);
    }
    if (tid < nr && !found[tid]) bad |= QOT_TOPO_PLACE_NO_SUCH_CONN;
    if (tid == 0 && n - n_gone >= sg::kCap) bad |= QOT_TOPO_STATUS_TOO_MANY;  // the edited sample would hold 257

    // ---- step 3: the candidate's cells, a wave each ----
    for (int64_t c = lo + w; c < hi; c += sg::kWaves) {            // (wave-uniform)
        const int64_t l = pl.cells[c], q = pl.cells[pl.M + c];
        int64_t conn;
        if (l < 0 || l >= st.L || q < 0 || q >= st.Q) {
            bad |= QOT_TOPO_PLACE_BAD_CELL;
        } else if (sg::channel_conn(d, st.P, LQ, st.conn_row, (int)l * st.Q + (int)q, conn)) {
            bool freed = false;                                    // occupied: legal when its owner is gone
            for (int i = lane; i < n; i += kWave) freed |= (T.conn[i] == conn && gone[i] != 0);
            if (!__any(freed)) bad |= QOT_TOPO_PLACE_OCCUPIED;
        }
    }
    if (bad) atomicOr(&bad_all, bad);
    __syncthreads();
    if (bad_all) {                                                 // block-uniform
        topo_status_refuse(a, bad_all, orow, st.links + k);
        return;
    }

    // ---- step 4: the pair contest over the survivors and the candidate (slot < 0: n < 256, slot n is free) ----
    if (tid == 0) T.conn[slot < 0 ? n : slot] = conn_a;
    __syncthreads();                                               // (bad_all is written again below)
    bad = sg::topo_winners(d, LQ, st.src_row, st.dst_row, T, n, mat, eu, ev, v, gone, slot);   // (ends with a barrier)
    if (bad) atomicOr(&bad_all, bad);
    __syncthreads();
    if (bad_all) {                                                 // block-uniform
        topo_status_refuse(a, topo_status_bits(bad_all), orow, st.links + k);
        return;
    }
    topo_status_forward<H, D>(a, lds, mat, part, rec,
                              InferStatusEdges{rec, T.first, d, st.cols, st.P, LQ, v, slot < 0 ? n : slot}, orow, st.links + k);
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_place_release(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                                   const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E,
                                                   int64_t K, int n_max, int max_e, const float* t4, int ld4, const float* M,
                                                   int ldm, const float* P, int V, const float* w_edge, const float* w1,
                                                   const float* b1, const float* wcat, const float* bias2, const float* w0,
                                                   const float* b0, const float* w3, const float* b3, float slope_conv,
                                                   float slope_head, float* out, int H, int D, int O, int32_t* status,
                                                   int64_t* links, const double* data, const int64_t* samples, int64_t S,
                                                   int rows_p, int64_t L, int64_t Q, int conn_row, int src_row, int dst_row,
                                                   const double* cols, int ncol, const double* values, const int64_t* cells,
                                                   const int64_t* cell_ptr, int64_t n_cells, const int64_t* release,
                                                   const int64_t* release_ptr, int64_t R, qot_stream_t stream_) {
    size_t image;
    const int rc = topo_status_envelope(edge_index, edge_attr, node_ptr, edge_ptr, N, E, K, n_max, max_e, V, H, D, O, S, rows_p,
                                        L, Q, conn_row, src_row, dst_row, ncol, image);
    if (rc != QOT_OK) return rc;
    if (image + kTopoStatusStatic + kTopoReleaseStatic > kInferLdsMax) return QOT_ERR_UNSUPPORTED;
    if (n_cells < 0 || R < 0) return QOT_ERR_BADARG;
    if (K == 0) return QOT_OK;
    if (ld4 < 4 * H || (ld4 & 3) || ldm < V) return QOT_ERR_BADARG;
    const InferArgs a = topo_status_infer_args(node_ids, N, K, n_max, max_e, t4, ld4, M, ldm, P, V, w_edge, w1, b1, wcat, bias2,
                                               w0, b0, w3, b3, slope_conv, slope_head, out, O, status);
    if (!topo_weights_present(a) || !out || !links || !data || !cols || S == 0 || !samples || !values || !cell_ptr ||
        (n_cells > 0 && !cells) || !release_ptr || (R > 0 && !release))
        return QOT_ERR_BADARG;
    const TopoStatusArgs st{data, samples, S, rows_p, (int)L, (int)Q, conn_row, src_row, dst_row, cols, links};
    const sg::PlaceArgs pl{values, cells, cell_ptr, n_cells};
    const sg::ReleaseArgs rl{release, release_ptr, R};
    QOT_INFER_DISPATCH(topological_infer_place_release_kernel, H, D, dim3((unsigned)K), image, (hipStream_t)stream_, a, st, pl, rl)
}
