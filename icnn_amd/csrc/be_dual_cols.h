// Dual step, device helpers: the butterfly reductions over the rows that hold the multipliers and the column loop a = A^T lam.
// Included by be_dual_dev.h; everything is in an anonymous namespace.
#pragma once
#include "be_dual_cut.h"

namespace icnn_be {

namespace {

// Butterfly reduction over the first 16 lanes (the row that holds a bundle of up to 16 multipliers):
// quad permutes, row_half_mirror, row_mirror -- 4 DPP steps, every lane of the row ends up with the
// result (lane 0 is read back as the wave-uniform value).  Replaces k-step v_readlane scans.
template <typename Op>
__device__ __forceinline__ double row16_reduce(double v, Op op) {
    v = op(v, dpp_move<0xB1>(v));
    v = op(v, dpp_move<0x4E>(v));
    v = op(v, dpp_move<0x141>(v));
    v = op(v, dpp_move<0x140>(v));
    return uni(v);
}

// The same for bundles of up to 32 cuts (the 32-slot kernels): the rows of lanes 0..15 and 16..31 are reduced
// side by side, then combined.  `v` must be the operation's neutral element outside the bundle; k <= 16 (wave-uniform)
// takes the single-row result, so the 32-slot kernels run the 16-slot kernels' instruction sequence on small bundles.
template <int KT, typename Op>
__device__ __forceinline__ double rows_reduce(double v, int k, Op op) {
    v = op(v, dpp_move<0xB1>(v));
    v = op(v, dpp_move<0x4E>(v));
    v = op(v, dpp_move<0x141>(v));
    v = op(v, dpp_move<0x140>(v));
    if (KT == 16 || k <= 16) return uni(v);
    return op(bcast(v, 0), bcast(v, 16));
}

// a_j = sum_i lam_i A[i][j] for the columns j = tid + c * nt owned by this thread, NC of them in
// statically indexed registers: the LDS reads of several rows and all NC columns are in flight together
// and the NC transcendental chains that follow (exp, divide) interleave instead of running one after the
// other.  `fin(j, valid, a_j)` must do its arithmetic unconditionally and only guard its stores.
// Accumulation order over i is the plain sequential one (same bits as the scalar loop).
template <typename CutT, int NC, typename F>
__device__ __forceinline__ void columns_nc(const CutT *As, int ldA, int k, int zrow, int n_pad, int nt, int tid,
                                           double lam, F &&fin) {
    double acc[NC];
    int jc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int j = tid + c * nt;
        jc[c] = j < n_pad ? j : n_pad - 1;
        acc[c] = 0.0;
    }
    // rows in groups of four (4 * NC LDS reads in flight), then the remainder one by one -- the order of
    // the accumulation is the plain i = 0..k-1 one
    int i0 = 0;
    for (; i0 + 4 <= k; i0 += 4) {
        CutT av[4][NC];
        double li[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            li[d] = bcast(lam, i0 + d);
#pragma unroll
            for (int c = 0; c < NC; ++c) av[d][c] = As[(i0 + d) * ldA + jc[c]];
        }
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += li[d] * (double)av[d][c];
    }
    for (; i0 < k; ++i0) {
        const double li = bcast(lam, i0);
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += li * (double)As[i0 * ldA + jc[c]];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) fin(tid + c * nt, tid + c * nt < n_pad, acc[c]);
}
template <typename CutT, typename F>
__device__ __forceinline__ void for_columns(const CutT *As, int ldA, int k, int zrow, int n_pad, int nt, int tid,
                                            double lam, F &&fin) {
    const int per_thread = (n_pad + nt - 1) / nt;
    if (per_thread == 3) columns_nc<CutT, 3>(As, ldA, k, zrow, n_pad, nt, tid, lam, fin);
    else if (per_thread <= 2) columns_nc<CutT, 2>(As, ldA, k, zrow, n_pad, nt, tid, lam, fin);
    else if (per_thread == 4) columns_nc<CutT, 4>(As, ldA, k, zrow, n_pad, nt, tid, lam, fin);
    else
        for (int j0 = 0; j0 < n_pad; j0 += 4 * nt)       // wide rows: four columns per thread at a time
            columns_nc<CutT, 4>(As + j0, ldA, k, zrow, n_pad - j0, nt, tid, lam,
                                [&](int j, bool valid, double aj) { fin(j0 + j, valid, aj); });
}

}  // namespace
}  // namespace icnn_be
