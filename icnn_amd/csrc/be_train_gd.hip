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

#include "be_kernels.h"
#include "be_train_gd_dev.h"

namespace icnn_be {

namespace {

constexpr int GT = GD_FEED_THREADS;

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

}  // namespace

// the per-sample sums (8-byte aligned) and the ticket
size_t gd_feed_work_bytes(int batch) { return sizeof(double) * (size_t)(batch > 0 ? batch : 1) + 16; }

hipError_t launch_gd_feed(const GdFeedLaunch &l, hipStream_t stream) {
    GdFeedArgs a{};
    a.l = l;
    a.partial = gd_feed_partial(l.work);
    a.ticket = gd_feed_ticket(l.work, l.B);
    return launch_kernel(gd_feed_kernel, dim3(l.B), dim3(GT), 0, stream, a);
}

// S of the 2-D grid: ceil(K n / GD_FEED_PX_CHUNK) workgroups per sample (DESIGN.md §17 has the measurement behind the chunk)
long long gd_feed_px_chunks(int n, int K) {
    return ((long long)K * n + GD_FEED_PX_CHUNK - 1) / GD_FEED_PX_CHUNK;
}

hipError_t launch_gd_feed_px(const GdFeedPxLaunch &l, hipStream_t stream) {
    GdFeedPxArgs a{};
    a.l = l;
    a.partial = gd_feed_partial(l.work);
    a.ticket = gd_feed_ticket(l.work, l.B);
    const long long total = (long long)l.K * l.n;
    const long long S = l.v_rows ? gd_feed_px_chunks(l.n, l.K) : 1;
    a.chunk = (unsigned)((total + S - 1) / S);
    return launch_kernel(gd_feed_px_kernel, dim3(l.B, (unsigned)S), dim3(GT), 0, stream, a);
}

}  // namespace icnn_be
