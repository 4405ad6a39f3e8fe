// "What if" in one launch: the eval-mode TopologicalGNN forward of K EDITS of a batch's graphs (DESIGN.md 4.18,
// TopologicalPredictor.what_if).  Candidate k names one base graph, removes some of that graph's edges (positions in the
// batch's edge_index) and appends edges of its own; out[k] is qot_topological_infer's row of the edited graph -- the base
// graph's nodes, its surviving edges in their order, the added edges behind them -- bit for bit.
//
// Grid (K), 256 threads, the eval kernel's LDS image sized for max_e + max_add edges.  A workgroup
//   1  reads its graph's slices through graph[k], its own slices of the add and drop lists, and checks them
//   2  runs phase 1 of infer_dev.hpp over the edge numbers 0 .. m_base + adds: number e < m_base is position e0 + e of the
//      batch unless it is dropped, number m_base + x is added edge x.  A dropped number is skipped: not staged, not
//      counted, in no slot.  Phase 1 sorts every destination row by edge number, and the numbers of the survivors and the
//      additions rise exactly as their positions in the materialised graph do, so the slot order -- and with it every sum
//      of phases 2 - 4, which are the eval kernel's code -- is that graph's.
//   3  phases 2 - 4, unchanged.
// The membership test: before phase 1 the workgroup clears the `ends` word of every edge number and then writes a mark no
// edge can have (local ids are below 2^16 each; the mark is all ones) into the words of the dropped numbers -- plain LDS
// stores of one value, so the order of the list and repeats in it do not matter.  Phase 1 asks that word: one LDS read
// per edge, whatever the length of the list.  Plain fp32 FMA, no atomics beside phase 1's LDS histogram.
#include "infer_dev.hpp"

namespace qot {

constexpr int kWhatIfMaxDrop = 32;           // (one thread per dropped position marks it)

struct InferEditArgs {
    const int64_t* add_ei;              // [2, A] batch node numbering
    const float* add_attr;              // [A, D]
    const int64_t* add_ptr;             // [K + 1]
    int64_t A;
    const int64_t* drop;                // [R] positions in the batch's edge_index; null: no removals
    const int64_t* drop_ptr;            // [K + 1]
    int64_t R;
    const int64_t* graph;               // [K]; null: graph 0
};

constexpr unsigned int kWhatIfDropped = 0xFFFFFFFFu;

// the edges of one candidate: see InferBaseEdges (infer_dev.hpp) for what a source states
struct InferEditedEdges {
    const int64_t* add_src; const int64_t* add_dst; const float* add_attr;     // the candidate's own additions
    int mb;                             // edges of the base graph: numbers below are base positions, the rest additions
    const unsigned int* ends;           // LDS: kWhatIfDropped at the dropped numbers (an added edge is never marked)

    __device__ __forceinline__ float attr(const InferArgs& a, int64_t e0, int c, int D) const {
        return c < mb * D ? a.edge_attr[e0 * D + c] : add_attr[c - mb * D];
    }
    __device__ __forceinline__ bool skips(int e) const { return ends[e] == kWhatIfDropped; }
    __device__ __forceinline__ bool ends_of(const InferArgs& a, int64_t n0, int64_t e0, int n, int e, int& j, int& i) const {
        if (skips(e)) return false;
        if (e < mb) {
            j = (int)(a.ei[e0 + e] - n0);
            i = (int)(a.ei[a.E + e0 + e] - n0);
            return true;
        }
        // an added edge: compared in 64 bits, an endpoint outside the graph becomes -1 (phase 1 flags bit 0)
        const int64_t jj = add_src[e - mb] - n0, ii = add_dst[e - mb] - n0;
        j = jj >= 0 && jj < n ? (int)jj : -1;
        i = ii >= 0 && ii < n ? (int)ii : -1;
        return true;
    }
    __device__ __forceinline__ int slots(int m, const int* rp, int n) const { return rp[n]; }
};

template <int H, int D>
__global__ __launch_bounds__(kInferThreads) void topological_infer_whatif_kernel(const InferArgs a, const InferEditArgs ed) {
    extern __shared__ float4 infer_whatif_lds_raw[];
    float* lds = reinterpret_cast<float*>(infer_whatif_lds_raw);
    const int tid = threadIdx.x;
    const int64_t k = blockIdx.x;
    float* orow = a.out + k * a.O;

    // ---- step 1: the candidate's slices (every value below is uniform over the workgroup)
    const int64_t b = ed.graph ? ed.graph[k] : 0;
    const int64_t a0 = ed.add_ptr[k], na = ed.add_ptr[k + 1] - a0;
    const int64_t d0 = ed.drop_ptr ? ed.drop_ptr[k] : 0, nd = ed.drop_ptr ? ed.drop_ptr[k + 1] - d0 : 0;
    int bad = 0;
    if (b < 0 || b >= a.B || a0 < 0 || na < 0 || a0 + na > ed.A || d0 < 0 || nd < 0 || nd > kWhatIfMaxDrop || d0 + nd > ed.R)
        bad = 2;
    int64_t n0 = 0, e0 = 0, n = 0, mb = 0;
    if (!bad) {
        n0 = a.node_ptr[b];
        e0 = a.edge_ptr[b];
        n = a.node_ptr[b + 1] - n0;
        mb = a.edge_ptr[b + 1] - e0;
        // the base graph's slices lie inside the arrays, the edited graph inside the LDS image (removals are not credited)
        if (!infer_slices_ok(a, n0, e0, n, mb) || mb + na > a.cap_m) bad = 2;
    }
    if (bad) {
        infer_refuse(a, bad, orow);
        return;
    }

    // ---- step 2: the marks of the dropped edge numbers, then phases 1 and 2 over the numbers 0 .. mb + na
    const int m = (int)(mb + na);
    unsigned int* ends = reinterpret_cast<unsigned int*>(lds + infer_lds(a.cap_n, a.cap_m, H, D).ends);
    for (int e = tid; e < m; e += kInferThreads) ends[e] = 0;
    __syncthreads();
    int out_of_slice = 0;
    if (tid < nd) {
        const int64_t pos = ed.drop[d0 + tid] - e0;
        out_of_slice = pos < 0 || pos >= mb;
        if (!out_of_slice) ends[pos] = kWhatIfDropped;
    }
    if (__syncthreads_or(out_of_slice)) {                // a drop position outside the graph's edge slice
        infer_refuse(a, 2, orow);
        return;
    }
    const InferEditedEdges src{ed.add_ei + a0, ed.add_ei + ed.A + a0, ed.add_attr + a0 * D, (int)mb, ends};
    bad = infer_phases12<H, D, InferEditedEdges>(a, lds, infer_lds(a.cap_n, a.cap_m, H, D), n0, e0, (int)n, m, src);
    if (bad) {
        infer_refuse(a, bad, orow);
        return;
    }

    // ---- step 3 (the layout restated, as in infer.hip: fewer scalar registers live across phases 1 and 2)
    const InferLds L = infer_lds(a.cap_n, a.cap_m, H, D);
    infer_phases34<H, D, false>(a, lds, L, (int)n, lds + L.x1, orow, InferDrop{});
}

}  // namespace qot

using namespace qot;

extern "C" int qot_topological_infer_whatif_supported(int n_max, int max_e, int H, int D, int O) {
    return infer_supported(kInferEval, n_max, max_e, H, D, O);
}

extern "C" int qot_topological_infer_whatif_max_edges(int n_max, int H, int D) {
    return infer_max_edges(kInferEval, n_max, H, D);
}

extern "C" int qot_topological_infer_whatif(const int64_t* node_ids, const int64_t* edge_index, const float* edge_attr,
                                            const int64_t* node_ptr, const int64_t* edge_ptr, int64_t N, int64_t E, int64_t B,
                                            int n_max, int max_e, const float* t4, int ld4, const float* M, int ldm,
                                            const float* P, int V, const float* w_edge, const float* w1, const float* b1,
                                            const float* wcat, const float* bias2, const float* w0, const float* b0,
                                            const float* w3, const float* b3, float slope_conv, float slope_head, float* out,
                                            int H, int D, int O, int32_t* status, const int64_t* add_edge_index,
                                            const float* add_edge_attr, const int64_t* add_ptr, int64_t A,
                                            const int64_t* drop, const int64_t* drop_ptr, int64_t R, const int64_t* graph,
                                            int64_t K, int max_add, qot_stream_t stream_) {
    if (!infer_sizes_ok(N, E, B, n_max, max_e, V) || A < 0 || R < 0 || K < 0 || max_add < 0 || max_add > A)
        return QOT_ERR_BADARG;
    if ((R > 0 && (!drop || !drop_ptr)) || (!graph && B != 1 && K > 0)) return QOT_ERR_BADARG;
    if (max_add > (1 << 20) || !infer_supported(kInferEval, n_max, max_e, H, D, O) ||
        !infer_supported(kInferEval, n_max, max_e + max_add, H, D, O))
        return QOT_ERR_UNSUPPORTED;
    if (K == 0) return QOT_OK;
    if (K > 0x7fffffff) return QOT_ERR_UNSUPPORTED;
    if (B == 0) return QOT_ERR_BADARG;                 // (candidates of no graph)
    InferArgs a;
    const int rc = infer_make_args(&a, node_ids, edge_index, edge_attr, node_ptr, edge_ptr, N, E, B, n_max, max_e, t4, ld4, M,
                                   ldm, P, V, w_edge, w1, b1, wcat, bias2, w0, b0, w3, b3, slope_conv, slope_head, out, H, O,
                                   status);
    if (rc != QOT_OK) return rc;
    if (!add_ptr || (A > 0 && (!add_edge_index || !add_edge_attr))) return QOT_ERR_BADARG;
    a.cap_m = max_e + max_add;                         // the image holds the base graph's edges and the additions
    const InferEditArgs ed{add_edge_index, add_edge_attr, add_ptr, A, drop, drop_ptr, R, graph};
    QOT_INFER_DISPATCH(topological_infer_whatif_kernel, H, D, dim3((unsigned)K),
                       infer_lds_bytes(kInferEval, n_max, max_e + max_add, H, D), (hipStream_t)stream_, a, ed)
}
