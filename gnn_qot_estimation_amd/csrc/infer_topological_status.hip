// TopologicalPredictor.from_status: the eval-mode TopologicalGNN row of every network-status sample, straight from
// data[S, P, L, Q] (fp64) in ONE launch -- no graph in between, nothing read back.  out[g] / links[g]
// are, bit for bit, what qot_topological_infer gives for the graph the device builder (status_graph.hip) makes of sample
// samples[g], and that graph's directed link count: the sample's lightpaths are status_scan_dev.hpp's discover() table,
// the links the builder's own pair contest (topo_winners) and row-major walk (topo_run), the link features its scaled(),
// and the forward is infer_dev.hpp's infer_phases12 behind a third edge source, InferStatusEdges, then infer_phases34 --
// the same sums in the same order (the walk numbers the links ascending by (source, target), the builder's canonical
// order, and phase 1 sorts every destination row's slots by link number).
//
// One workgroup (256 threads) per sample:
//   1  discover(): the first-seen table (conn, first channel) in LDS; thread t reads lightpath t's end nodes on its first
//      channel; among the lightpaths of one unordered node pair the largest conn wins the pair's cells of the 75 x 75
//      int16 matrix.
//   2  every thread counts the links of its run of cells; a block exclusive scan numbers them; link e gets one LDS word
//      (source << 24 | target << 16 | lightpath).  links[g] = the total, at most 2 x 256 = kTopoStatusLinks.
//   3  infer_phases12<H, D, InferStatusEdges> over nodes 0 .. 74 (node_ids: the caller's arange(75)) and the m links --
//      the source reads a link's ends from its word and column k of its features as scaled(d[r_k, first[lightpath]]) --
//      then infer_phases34 into out[g].
// Steps 2 and 3, the edge source and the entry's envelope are infer_topological_status_dev.hpp's, shared with
// infer_topological_place.hip.  The LDS image is infer_lds(75, 512, H, D) as dynamic LDS; the table, the matrix and the link words are static beside it
// (kTopoStatusStatic bytes, which the entry point adds when it checks the budget).  No workspace, no global scratch.
// Nothing read from data is used as an index before it is checked: a conn is only compared, the end nodes pass the
// 1 .. 75 test first, the channel numbers come from the loop counters.  All global writes are ordinary vector stores
// (the status word: one atomicOr).
//
// On the device: a conn_id that is not finite or beyond +-2^53 (QOT_TOPO_STATUS_BAD_CONN), more than 256 lightpaths
// (QOT_TOPO_STATUS_TOO_MANY), a sample number outside [0, S) (QOT_TOPO_STATUS_BAD_SAMPLE), a src_id / dst_id that is no
// integer in 1 .. 75 (QOT_TOPO_STATUS_BAD_ENDPOINT): the sample's row is NaN, its link count 0.
#include "infer_topological_status_dev.hpp"

namespace qot {

template <int H, int D>
__global__ __launch_bounds__(kInferThreads) void topological_infer_status_kernel(const InferArgs a, const TopoStatusArgs st) {
    static_assert(kInferThreads == sg::kThreads, "the scan and the forward share one workgroup");
    extern __shared__ float4 infer_status_lds_raw[];
    float* lds = reinterpret_cast<float*>(infer_status_lds_raw);
    __shared__ sg::Table T;
    __shared__ int16_t mat[sg::kCells];
    __shared__ uint8_t eu[sg::kCap], ev[sg::kCap];
    __shared__ int part[sg::kWaves + 1];
    __shared__ uint32_t rec[kTopoStatusLinks];
    __shared__ int bad_all;
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    float* orow = a.out + g * a.O;
    bool ok;
    const int64_t s = sg::sample_of(st.samples, g, st.S, ok);
    if (!ok) {                                                     // block-uniform
        if (tid == 0) st.links[g] = 0;
        infer_refuse(a, QOT_TOPO_STATUS_BAD_SAMPLE, orow);
        return;
    }
    const int LQ = st.L * st.Q;
    const double* d = st.data + s * (int64_t)st.P * LQ;
    for (int k = tid; k < sg::kCells; k += sg::kThreads) mat[k] = -1;
    if (tid == 0) bad_all = 0;

    // ---- step 1: the lightpaths of the sample, the winner of every node pair ----
    int bad = sg::discover(d, st.P, LQ, st.conn_row, T, nullptr);             // (begins and ends with a barrier)
    bad |= sg::topo_winners(d, LQ, st.src_row, st.dst_row, T, T.n, mat, eu, ev);   // (ends with a barrier)
    if (bad) atomicOr(&bad_all, bad);
    __syncthreads();
    if (bad_all) {                                                 // block-uniform
        if (tid == 0) st.links[g] = 0;
        infer_refuse(a, topo_status_bits(bad_all), orow);
        return;
    }

    // ---- steps 2 and 3: the directed links in canonical order, the forward over nodes 0 .. 74 and the links ----
    topo_status_forward<H, D>(a, lds, mat, part, rec, InferStatusEdges{rec, T.first, d, st.cols, st.P, LQ}, orow, st.links + g);
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_status(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                            const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t G,
                                            int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm,
                                            const float* P, int V, const float* w_edge, const float* w1, const float* b1,
                                            const float* wcat, const float* bias2, const float* w0, const float* b0,
                                            const float* w3, const float* b3, float slope_conv, float slope_head, float* out,
                                            int H, int D, int O, int32_t* status, int64_t* links, const double* data,
                                            const int64_t* samples, int64_t S, int rows_p, int64_t L, int64_t Q, int conn_row,
                                            int src_row, int dst_row, const double* cols, int ncol, qot_stream_t stream_) {
    size_t image;
    const int rc = topo_status_envelope(edge_index, edge_attr, node_ptr, edge_ptr, N, E, G, n_max, max_e, V, H, D, O, S, rows_p,
                                        L, Q, conn_row, src_row, dst_row, ncol, image);
    if (rc != QOT_OK) return rc;
    if (G == 0) return QOT_OK;
    if (ld4 < 4 * H || (ld4 & 3) || ldm < V) return QOT_ERR_BADARG;
    const InferArgs a = topo_status_infer_args(node_ids, N, G, n_max, max_e, t4, ld4, M, ldm, P, V, w_edge, w1, b1, wcat, bias2,
                                               w0, b0, w3, b3, slope_conv, slope_head, out, O, status);
    if (!topo_weights_present(a) || !out || !links || !data || !cols || S == 0) return QOT_ERR_BADARG;
    const TopoStatusArgs st{data, samples, S, rows_p, (int)L, (int)Q, conn_row, src_row, dst_row, cols, links};
    QOT_INFER_DISPATCH(topological_infer_status_kernel, H, D, dim3((unsigned)G), image, (hipStream_t)stream_, a, st)
}
