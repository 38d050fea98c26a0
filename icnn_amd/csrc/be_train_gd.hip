// The feed of the back-optimisation training step (synthetic-cls/icnn.py:117-139, multi-label-cls/icnn-back.py;
// include/icnn_be.h icnn_be_gd_feed): everything between the unrolled GD solve and the surrogate gradient,
// which a caller otherwise composes from six elementwise launches.
//
//   gd_feed_kernel   one workgroup per sample j: d = float32(y_K) - t and ybar = (d * 2) * scale in float32, the K rows
//                    v[j K + k] = coef[k] * ybar of the sample (consecutive in memory: one coalesced sweep), c = 0 for
//                    them, row_offset[j] = K j, the sample's sum of d^2 in double (every product exact) and, when asked,
//                    its F1 tallies.  The last workgroup to take a ticket adds the per-sample sums, scales by 1 / (B n) in
//                    double and rounds once to float32.  Every sum has one fixed order: the same bits on every call.
//   gd_feed_px_kernel  the same feed for the loss mean((px (y_K - t))^2) of completion/icnn.back.py:149 (icnn_be_gd_feed_px;
//                    DESIGN.md §17) on a two-dimensional grid: workgroup (j, c) writes chunk c of the S contiguous chunks of
//                    sample j's [K][n] block, and workgroup (j, 0) alone forms the sample's sum, in gd_feed_kernel's order
//                    and tree, and takes the ticket -- no output bit depends on S.  Without rows (the test phase) the grid
//                    is B x 1 and only the loss is formed.
#include <hip/hip_runtime.h>

#include <climits>

#include "be_api_check.h"
#include "be_kernels.h"
#include "be_train_gd_dev.h"

namespace icnn_be {

namespace {

constexpr int GT = GD_FEED_THREADS;

// the arguments of icnn_be_gd_feed
struct GdFeedLaunch {
    const double *yK;             // [B][n] y_K (float32 values)
    const float *t;               // [B][n] targets
    const double *coef;           // [K] step coefficients
    int B, n, K;
    float scale;                  // float32(1) / float32(B n)
    double *v_rows, *c_rows;      // [B K][n], [B K]
    int *row_offset;              // [B + 1]
    float *loss;
    int *tallies;                 // [B][3] tp / fp / fn (may be NULL)
    void *work;                   // gd_feed_work_bytes(B)
};

struct GdFeedArgs {
    GdFeedLaunch l;
    double *partial;     // [B]
    int *ticket;
};

__global__ __launch_bounds__(GT) void gd_feed_kernel(GdFeedArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[GT];
    __shared__ int ired[GT];
    __shared__ int s_last;
    const GdFeedLaunch &l = a.l;
    const int tid = threadIdx.x, j = blockIdx.x, n = l.n, K = l.K, B = l.B;
    const double *y_row = l.yK + (size_t)j * n;
    const float *t_row = l.t + (size_t)j * n;
    // ---- this sample's squared error and tallies (be_train_gd_dev.h) ----
    const double s = gd_sample_sqerr(y_row, t_row, n, red);
    if (l.tallies) gd_sample_tallies(y_row, t_row, n, ired, l.tallies + 3 * (size_t)j);
    // ---- its K rows: element e = k n + i of the sample's [K][n] block ----
    double *v_blk = l.v_rows + (size_t)j * K * n;
    const size_t total = (size_t)K * n;
    int k = tid / n, i = tid - k * n;           // advanced by GT per pass without a division
    const int dk = GT / n, di = GT - dk * n;
    for (size_t e = tid; e < total; e += GT) {
        const float d = (float)y_row[i] - t_row[i];
        const float ybar = (d * 2.0f) * l.scale;
        v_blk[e] = l.coef[k] * (double)ybar;
        k += dk;
        i += di;
        if (i >= n) { i -= n; ++k; }
    }
    for (int r = tid; r < K; r += GT) l.c_rows[(size_t)j * K + r] = 0.0;
    if (tid == 0) {
        l.row_offset[j] = K * j;
        if (j == B - 1) l.row_offset[B] = K * B;
    }
    // ---- the loss, formed by the last workgroup to take a ticket ----
    gd_loss_behind_ticket(a.partial, a.ticket, j, s, B, n, l.loss, red, &s_last);
}

// the same feed for the loss mean((px (y_K - t))^2), on a grid of B x S workgroups; v_rows, c_rows, row_offset (and coef)
// NULL together: the loss alone
struct GdFeedPxLaunch {
    const double *yK;
    const float *t;
    const double *coef;
    int B, n, K;
    float scale, px;
    double *v_rows, *c_rows;
    int *row_offset;
    float *loss;
    void *work;                   // gd_feed_work_bytes(B)
};
#ifndef ICNN_BE_GD_FEED_PX_CHUNK
#define ICNN_BE_GD_FEED_PX_CHUNK 8192         // an experiment builds another value (tools/conv_gd_step_time.py --alt-lib)
#endif
constexpr int GD_FEED_PX_CHUNK = ICNN_BE_GD_FEED_PX_CHUNK;   // elements of a sample's [K][n] block per workgroup, at most
constexpr int GD_FEED_PX_MAX_CHUNKS = 65535; // gridDim.y

struct GdFeedPxArgs {
    GdFeedPxLaunch l;
    double *partial;     // [B]
    int *ticket;
    unsigned chunk;      // elements of a sample's [K][n] block per workgroup: ceil(K n / gridDim.y)
};

__global__ __launch_bounds__(GT) void gd_feed_px_kernel(GdFeedPxArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[GT];
    __shared__ int s_last;
    const GdFeedPxLaunch &l = a.l;
    const int tid = threadIdx.x, j = blockIdx.x, n = l.n, K = l.K, B = l.B;
    const double *y_row = l.yK + (size_t)j * n;
    const float *t_row = l.t + (size_t)j * n;
    if (l.v_rows) {
        // ---- chunk blockIdx.y of the sample's K rows: elements e = k n + i in [lo, hi) ----
        double *v_blk = l.v_rows + (size_t)j * K * n;
        const size_t total = (size_t)K * n, lo = (size_t)blockIdx.y * a.chunk;
        const size_t hi = lo + a.chunk < total ? lo + a.chunk : total;
        const size_t e0 = lo + tid;
        int k = (int)(e0 / (size_t)n), i = (int)(e0 - (size_t)k * n);    // one division, then advanced by GT per pass
        const int dk = GT / n, di = GT - dk * n;
        for (size_t e = e0; e < hi; e += GT) {
            const float d = (float)y_row[i] - t_row[i];
            const float u = l.px * d;
            const float ybar = ((u * 2.0f) * l.scale) * l.px;
            v_blk[e] = l.coef[k] * (double)ybar;
            k += dk;
            i += di;
            if (i >= n) { i -= n; ++k; }
        }
    }
    if (blockIdx.y != 0) return;
    // ---- workgroup (j, 0): c, row_offset and this sample's squared error ----
    if (l.v_rows) {
        for (int r = tid; r < K; r += GT) l.c_rows[(size_t)j * K + r] = 0.0;
        if (tid == 0) {
            l.row_offset[j] = K * j;
            if (j == B - 1) l.row_offset[B] = K * B;
        }
    }
    double s = 0.0;
    for (int i = tid; i < n; i += GT) {
        const float u = l.px * ((float)y_row[i] - t_row[i]);
        s = s + (double)u * (double)u;
    }
    s = block_tree_sum<GT>(s, red);
    // ---- one ticket per sample, whatever gridDim.y; the last of them forms the loss, as gd_feed_kernel does ----
    gd_loss_behind_ticket(a.partial, a.ticket, j, s, B, n, l.loss, red, &s_last);
}

// S of the 2-D grid: ceil(K n / GD_FEED_PX_CHUNK) workgroups per sample (DESIGN.md §17 has the measurement behind the chunk)
long long gd_feed_px_chunks(int n, int K) {
    return ((long long)K * n + GD_FEED_PX_CHUNK - 1) / GD_FEED_PX_CHUNK;
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

size_t icnn_be_gd_feed_work_bytes(int B) { return B < 0 ? 0 : gd_feed_work_bytes(B); }

int icnn_be_gd_feed(const double *yK, const float *t, const double *coef, int B, int n, int K, float scale, double *v_rows,
                    double *c_rows, int *row_offset, float *loss, int *f1_tallies, void *work, void *stream) {
    if (B < 1 || n < 1 || K < 1) return ICNN_BE_EINVAL;
    if (!yK || !t || !coef || !v_rows || !c_rows || !row_offset || !loss || !work) return ICNN_BE_EINVAL;
    if ((long long)B * K > INT_MAX) return ICNN_BE_ELIMIT;
    GdFeedArgs a{};
    a.l = GdFeedLaunch{yK, t, coef, B, n, K, scale, v_rows, c_rows, row_offset, loss, f1_tallies, work};
    a.partial = gd_feed_partial(work);
    a.ticket = gd_feed_ticket(work, B);
    return api_done(launch_kernel(gd_feed_kernel, dim3(B), dim3(GT), 0, static_cast<hipStream_t>(stream), a));
}

size_t icnn_be_gd_feed_px_work_bytes(int B, int n, int K) { return (B < 1 || n < 1 || K < 1) ? 0 : gd_feed_work_bytes(B); }

int icnn_be_gd_feed_px(const double *yK, const float *t, const double *coef, int B, int n, int K, float scale, float px,
                       double *v_rows, double *c_rows, int *row_offset, float *loss, void *work, void *stream) {
    if (B < 1 || n < 1 || K < 1) return ICNN_BE_EINVAL;
    if (!yK || !t || !loss || !work) return ICNN_BE_EINVAL;
    const int rows = (v_rows != nullptr) + (c_rows != nullptr) + (row_offset != nullptr);
    if (rows != 0 && rows != 3) return ICNN_BE_EINVAL;
    if (rows == 3 && !coef) return ICNN_BE_EINVAL;
    if ((long long)B * K > INT_MAX) return ICNN_BE_ELIMIT;
    const long long total = (long long)K * n, S = rows == 3 ? gd_feed_px_chunks(n, K) : 1;
    if (S > GD_FEED_PX_MAX_CHUNKS) return ICNN_BE_ELIMIT;
    GdFeedPxArgs a{};
    a.l = GdFeedPxLaunch{yK, t, coef, B, n, K, scale, px, v_rows, c_rows, row_offset, loss, work};
    a.partial = gd_feed_partial(work);
    a.ticket = gd_feed_ticket(work, B);
    a.chunk = (unsigned)((total + S - 1) / S);
    return api_done(launch_kernel(gd_feed_px_kernel, dim3(B, (unsigned)S), dim3(GT), 0, static_cast<hipStream_t>(stream), a));
}

}  // extern "C"
