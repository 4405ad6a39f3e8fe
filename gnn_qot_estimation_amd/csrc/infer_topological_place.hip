// TopologicalPredictor.place: the eval-mode TopologicalGNN row of K CANDIDATE lightpaths, each placed into a network-status
// sample data[S, P, L, Q] (fp64) that does not hold it yet, in ONE launch -- no edited sample, no graph, nothing read back
// (DESIGN.md 4.23).  Candidate k is the raw lp_feat vector values[k, P] written into the channels cells[:, cell_ptr[k] :
// cell_ptr[k + 1]] (link index, frequency index) of sample samples[k].  out[k] / links[k] are, bit for bit, what
// qot_topological_infer_status gives for that edited sample.  The kernel never builds it: the candidate fills free
// channels only, so the sample's lightpaths keep their conn, end nodes and features, and the candidate joins
// topo_winners' pair contest as one more lightpath -- table slot n = T.n, thread n, end nodes and features from values[k].
// Its place in the edited sample's first-seen order is not reproduced and need not be: the forward sums the links in
// canonical (source, target) order, whatever a lightpath's number.  The cells do not enter the graph; they decide only
// whether the placement is legal.
//
// One workgroup (256 threads) per candidate:
//   1  block-uniform checks of the candidate's own arguments: sample number, cell_ptr slice, conn_id.
//   2  discover() on the unedited sample; T.conn[t] == the candidate's conn flags a taken conn, n >= 256 too many.
//   3  wave w takes the cells lo + w, lo + w + 4, ...: range check first, then the channel must be free.
//   4  topo_winners over the n + 1 lightpaths, then infer_topological_status_dev.hpp's topo_status_forward: the walk, the
//      link words and the forward behind InferStatusEdges, which reads the candidate's links from values[k].
// Cost: O(L Q) for discover plus O(cells), per candidate; candidates of one sample do not share the scan.  The LDS image
// and the static part are from_status's.  No workspace, no global scratch.  Nothing read from data or values is used as an
// index before it is checked: a conn is only compared, the end nodes pass the 1 .. 75 test first, the cell indices come
// from `cells` and are range-checked first.  All global writes are ordinary vector stores (the status word: one atomicOr).
//
// On the device, since nothing is read back (the candidate's row is NaN, its links 0, the other rows are untouched): a
// sample number outside [0, S) (QOT_TOPO_STATUS_BAD_SAMPLE); a cell_ptr slice that is empty, descending or beyond M, a link
// or frequency index outside [0, L) / [0, Q) (QOT_TOPO_PLACE_BAD_CELL); a cell whose channel is occupied
// (QOT_TOPO_PLACE_OCCUPIED); a candidate conn_id that is not finite or beyond +-2^53, or such a value in the sample
// (QOT_TOPO_STATUS_BAD_CONN); a conn_id the sample holds already (QOT_TOPO_PLACE_CONN_TAKEN); a sample of 256 or more
// lightpaths -- the edited one would hold 257 (QOT_TOPO_STATUS_TOO_MANY); a src_id / dst_id, the candidate's or one of the
// sample's, that is no integer in 1 .. 75 (QOT_TOPO_STATUS_BAD_ENDPOINT).
#include "infer_topological_status_dev.hpp"

namespace qot {

template <int H, int D>
__global__ __launch_bounds__(kInferThreads) void topological_infer_place_kernel(const InferArgs a, const TopoStatusArgs st,
                                                                                const sg::PlaceArgs pl) {
    static_assert(kInferThreads == sg::kThreads, "the scan and the forward share one workgroup");
    extern __shared__ float4 infer_place_lds_raw[];
    float* lds = reinterpret_cast<float*>(infer_place_lds_raw);
    __shared__ sg::Table T;
    __shared__ int16_t mat[sg::kCells];
    __shared__ uint8_t eu[sg::kCap], ev[sg::kCap];
    __shared__ int part[sg::kWaves + 1];
    __shared__ uint32_t rec[kTopoStatusLinks];
    __shared__ int bad_all;
    const int tid = threadIdx.x, w = tid >> 6;
    const int64_t k = blockIdx.x;
    float* orow = a.out + k * a.O;
    const double* v = pl.values + k * (int64_t)st.P;

    // ---- step 1: what the candidate's own arguments say (every value is uniform over the block) ----
    bool ok;
    const int64_t s = sg::sample_of(st.samples, k, st.S, ok);
    const int64_t lo = pl.cell_ptr[k], hi = pl.cell_ptr[k + 1];
    int64_t conn_a = 0;
    int early = ok ? 0 : QOT_TOPO_STATUS_BAD_SAMPLE;
    if (lo < 0 || hi <= lo || hi > pl.M) early |= QOT_TOPO_PLACE_BAD_CELL;
    if (!sg::sg_conn(v[st.conn_row], conn_a)) early |= QOT_TOPO_STATUS_BAD_CONN;
    if (early) {                                                   // block-uniform
        topo_status_refuse(a, early, orow, st.links + k);
        return;
    }
    const int LQ = st.L * st.Q;
    const double* d = st.data + s * (int64_t)st.P * LQ;
    for (int c = tid; c < sg::kCells; c += sg::kThreads) mat[c] = -1;
    if (tid == 0) bad_all = 0;

    // ---- step 2: the lightpaths of the unedited sample, the candidate's conn among them ----
    int bad = topo_status_bits(sg::discover(d, st.P, LQ, st.conn_row, T, nullptr));      // (begins and ends with a barrier)
    const int n = T.n;
    if (tid < n && T.conn[tid] == conn_a) bad |= QOT_TOPO_PLACE_CONN_TAKEN;
    if (tid == 0 && n >= sg::kCap) bad |= QOT_TOPO_STATUS_TOO_MANY;           // the edited sample would hold n + 1

    // ---- step 3: the candidate's cells, a wave each ----
    for (int64_t c = lo + w; c < hi; c += sg::kWaves) {            // (wave-uniform)
        const int64_t l = pl.cells[c], q = pl.cells[pl.M + c];
        int64_t conn;
        if (l < 0 || l >= st.L || q < 0 || q >= st.Q) bad |= QOT_TOPO_PLACE_BAD_CELL;
        else if (sg::channel_conn(d, st.P, LQ, st.conn_row, (int)l * st.Q + (int)q, conn)) bad |= QOT_TOPO_PLACE_OCCUPIED;
    }
    if (bad) atomicOr(&bad_all, bad);
    __syncthreads();
    if (bad_all) {                                                 // block-uniform
        topo_status_refuse(a, bad_all, orow, st.links + k);
        return;
    }

    // ---- step 4: the pair contest over n + 1 lightpaths (n < 256: slot n is free), the links, the forward ----
    if (tid == 0) T.conn[n] = conn_a;
    __syncthreads();                                               // (bad_all is written again below)
    bad = sg::topo_winners(d, LQ, st.src_row, st.dst_row, T, n, mat, eu, ev, v);         // (ends with a barrier)
    if (bad) atomicOr(&bad_all, bad);
    __syncthreads();
    if (bad_all) {                                                 // block-uniform
        topo_status_refuse(a, topo_status_bits(bad_all), orow, st.links + k);
        return;
    }
    topo_status_forward<H, D>(a, lds, mat, part, rec, InferStatusEdges{rec, T.first, d, st.cols, st.P, LQ, v, n}, orow,
                              st.links + k);
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_place(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                           const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t K,
                                           int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm,
                                           const float* P, int V, const float* w_edge, const float* w1, const float* b1,
                                           const float* wcat, const float* bias2, const float* w0, const float* b0,
                                           const float* w3, const float* b3, float slope_conv, float slope_head, float* out,
                                           int H, int D, int O, int32_t* status, int64_t* links, const double* data,
                                           const int64_t* samples, int64_t S, int rows_p, int64_t L, int64_t Q, int conn_row,
                                           int src_row, int dst_row, const double* cols, int ncol, const double* values,
                                           const int64_t* cells, const int64_t* cell_ptr, int64_t n_cells,
                                           qot_stream_t stream_) {
    size_t image;
    const int rc = topo_status_envelope(edge_index, edge_attr, node_ptr, edge_ptr, N, E, K, n_max, max_e, V, H, D, O, S, rows_p,
                                        L, Q, conn_row, src_row, dst_row, ncol, image);
    if (rc != QOT_OK) return rc;
    if (n_cells < 0) return QOT_ERR_BADARG;
    if (K == 0) return QOT_OK;
    if (ld4 < 4 * H || (ld4 & 3) || ldm < V) return QOT_ERR_BADARG;
    const InferArgs a = topo_status_infer_args(node_ids, N, K, n_max, max_e, t4, ld4, M, ldm, P, V, w_edge, w1, b1, wcat, bias2,
                                               w0, b0, w3, b3, slope_conv, slope_head, out, O, status);
    if (!topo_weights_present(a) || !out || !links || !data || !cols || S == 0 || !samples || !values || !cell_ptr ||
        (n_cells > 0 && !cells))
        return QOT_ERR_BADARG;
    const TopoStatusArgs st{data, samples, S, rows_p, (int)L, (int)Q, conn_row, src_row, dst_row, cols, links};
    const sg::PlaceArgs pl{values, cells, cell_ptr, n_cells};
    QOT_INFER_DISPATCH(topological_infer_place_kernel, H, D, dim3((unsigned)K), image, (hipStream_t)stream_, a, st, pl)
}
