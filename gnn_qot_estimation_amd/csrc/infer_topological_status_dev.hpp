// What the two kernels that take a TopologicalGNN row straight from a network-status sample share beyond the sample scan
// (status_scan_dev.hpp) and the forward (infer_dev.hpp): infer_topological_status.hip (from_status, DESIGN.md 4.21: the
// graph of the sample as it is) and infer_topological_place.hip (place, DESIGN.md 4.23: the graph of the sample plus one
// candidate lightpath that it does not hold).  Stated once here for both: the sample's arguments, the static LDS beside
// the forward's image, the mapping of the scan's status bits, the links of a sample as an edge source (InferStatusEdges)
// and everything behind the pair contest (topo_status_forward): the row-major walk of the winner matrix, the link words
// and the forward -- so which links a winner matrix gives, their order and the sums over them are the same code in both.
// infer_topological_place_release.hip (place(release=...)) is the third user.  The three entries share
// their envelope, the weight test and the InferArgs of a call without a batch (the host inlines at the end); the
// candidate's and the release's arguments are status_scan_dev.hpp's, shared with the lightpath kernels.
#pragma once
#include "infer_dev.hpp"
#include "status_scan_dev.hpp"

namespace qot {

constexpr int kTopoStatusLinks = 2 * sg::kCap;        // 512: the image's edge cap, a constant of these kernels
// the static LDS beside the image: table, matrix, end nodes, scan parts, link words, the flag word
constexpr size_t kTopoStatusStatic = sizeof(sg::Table) + (size_t)((sg::kCells * 2 + 15) / 16 * 16) + 2 * sg::kCap +
                                     (sg::kWaves + 1) * 4 + (size_t)kTopoStatusLinks * 4 + 16;

struct TopoStatusArgs {
    const double* data; const int64_t* samples;
    int64_t S;
    int P, L, Q;
    int conn_row, src_row, dst_row;
    const double* cols;                 // [D, 4]: lp_feat row, min, max - min, has_range
    int64_t* links;
};

// the links of one sample as an edge source: see InferBaseEdges (infer_dev.hpp) for what a source states.  A link of
// lightpath cand_lp (place's candidate; -1: there is none) reads its raw values from the vector cand [P], every other link
// from the sample on its lightpath's first channel: the doubles a channel holding cand would give, into the same scaled().
struct InferStatusEdges {
    const uint32_t* rec;                // LDS: source << 24 | target << 16 | lightpath, canonical order
    const int32_t* first;               // LDS: the first channel of every lightpath
    const double* d;                    // the sample [P, LQ]
    const double* cols;
    int P, LQ;
    const double* cand = nullptr;
    int cand_lp = -1;

    __device__ __forceinline__ float attr(const InferArgs&, int64_t, int c, int D) const {
        const int e = c / D;
        const double* col = cols + 4 * (c - e * D);
        const int r = (int)col[0];
        if (!(r >= 0 && r < P)) return 0.0f;
        const int lp = (int)(rec[e] & 0xFFFFu);
        return sg::scaled(lp == cand_lp ? cand[r] : d[(int64_t)r * LQ + first[lp]], col);
    }
    __device__ __forceinline__ bool skips(int) const { return false; }
    __device__ __forceinline__ bool ends_of(const InferArgs&, int64_t, int64_t, int, int e, int& j, int& i) const {
        const uint32_t w = rec[e];
        j = (int)(w >> 24);
        i = (int)((w >> 16) & 0xFFu);
        return true;
    }
    __device__ __forceinline__ int slots(int m, const int*, int) const { return m; }
};

__device__ __forceinline__ int topo_status_bits(int sg_bits) {
    return ((sg_bits & QOT_SG_BAD_CONN) ? QOT_TOPO_STATUS_BAD_CONN : 0) |
           ((sg_bits & QOT_SG_TOO_MANY) ? QOT_TOPO_STATUS_TOO_MANY : 0) |
           ((sg_bits & QOT_SG_BAD_SAMPLE) ? QOT_TOPO_STATUS_BAD_SAMPLE : 0) |
           ((sg_bits & QOT_SG_BAD_ENDPOINT) ? QOT_TOPO_STATUS_BAD_ENDPOINT : 0);
}

// a refused row: NaN, no links, the bits in the launch's status word (the whole workgroup calls it, then returns)
__device__ __forceinline__ void topo_status_refuse(const InferArgs& a, int bits, float* orow, int64_t* links_g) {
    if (threadIdx.x == 0) *links_g = 0;
    infer_refuse(a, bits, orow);
}

// Behind topo_winners' barrier, the whole workgroup: the directed links of the winner matrix mat in canonical order -> rec
// (src.rec), their count -> *links_g, then the forward over nodes 0 .. 74 and those links -> orow.  part: kWaves + 1 ints.
template <int H, int D>
__device__ __forceinline__ void topo_status_forward(const InferArgs& a, float* lds, const int16_t* mat, int* part,
                                                    uint32_t* rec, const InferStatusEdges& src, float* orow, int64_t* links_g) {
    // ---- the directed links in canonical order ----
    int k0, k1;
    const int cnt = sg::topo_run(mat, k0, k1);
    int m;
    int e = sg::block_exscan(cnt, part, m);
    if (m > kTopoStatusLinks) {                                    // (256 lightpaths win 256 pairs at most: never; uniform)
        topo_status_refuse(a, 2, orow, links_g);
        return;
    }
    for (int k = k0; k < k1; ++k) {
        const int i = mat[k];
        if (i < 0) continue;
        rec[e++] = ((uint32_t)(k / sg::kTopo) << 24) | ((uint32_t)(k % sg::kTopo) << 16) | (uint32_t)i;
    }
    __syncthreads();

    // ---- the forward over nodes 0 .. 74 and the m links ----
    const int bad = infer_phases12<H, D, InferStatusEdges>(a, lds, infer_lds(a.cap_n, a.cap_m, H, D), 0, 0, sg::kTopo, m, src);
    if (bad) {
        topo_status_refuse(a, bad, orow, links_g);
        return;
    }
    if (threadIdx.x == 0) *links_g = m;
    const InferLds L = infer_lds(a.cap_n, a.cap_m, H, D);           // (restated, as in infer.hip)
    infer_phases34<H, D, false>(a, lds, L, sg::kTopo, lds + L.x1, orow, InferDrop{});
}

// What both entry points check of the arguments they share (before any launch; G rows are asked for).  image: the
// dynamic LDS of the launch.
inline int topo_status_envelope(const void* edge_index, const void* edge_attr, const void* node_ptr, const void* edge_ptr,
                                int64_t N, int64_t E, int64_t G, int n_max, int max_e, int V, int H, int D, int O, int64_t S,
                                int rows_p, int64_t L, int64_t Q, int conn_row, int src_row, int dst_row, int ncol,
                                size_t& image) {
    if (!infer_sizes_ok(N, E, G, n_max, max_e, V)) return QOT_ERR_BADARG;
    // there is no graph: the batch arguments of the common prefix must be empty, the nodes the 75 of the topology
    if (edge_index || edge_attr || node_ptr || edge_ptr || E != 0 || N != sg::kTopo || n_max != sg::kTopo ||
        max_e != kTopoStatusLinks)
        return QOT_ERR_BADARG;
    if (S < 0 || rows_p < 1 || L < 1 || Q < 1) return QOT_ERR_BADARG;
    image = infer_lds_bytes(kInferEval, n_max, max_e, H, D);
    if (!infer_supported(kInferEval, n_max, max_e, H, D, O) || image + kTopoStatusStatic > kInferLdsMax)
        return QOT_ERR_UNSUPPORTED;
    if (Q > QOT_SG_MAX_FREQS || L * Q >= (int64_t)1 << 31 || G >= (int64_t)1 << 31) return QOT_ERR_UNSUPPORTED;
    if (ncol != D) return QOT_ERR_BADARG;
    if (conn_row < 0 || conn_row >= rows_p || src_row < 0 || src_row >= rows_p || dst_row < 0 || dst_row >= rows_p)
        return QOT_ERR_BADARG;
    return QOT_OK;
}

// the InferArgs of a call without a batch: G rows of out over the N nodes of the topology, no graph arguments
inline InferArgs topo_status_infer_args(const int64_t* node_ids, int64_t N, int64_t G, int n_max, int max_e, const float* t4,
                                        int ld4, const float* M, int ldm, const float* P, int V, const float* w_edge,
                                        const float* w1, const float* b1, const float* wcat, const float* bias2,
                                        const float* w0, const float* b0, const float* w3, const float* b3, float slope_conv,
                                        float slope_head, float* out, int O, int32_t* status) {
    return InferArgs{node_ids, nullptr, nullptr, nullptr, nullptr, N, 0, G, n_max, max_e, t4, ld4, M, ldm, P, V,
                     w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, out, O, status};
}

// node_ids and all twelve weights of the model are present
inline bool topo_weights_present(const InferArgs& a) {
    return a.node_ids && a.t4 && a.M && a.P && a.w_edge && a.w1 && a.b1 && a.wcat && a.bias2 && a.w0 && a.b0 && a.w3 && a.b3;
}

}  // namespace qot
