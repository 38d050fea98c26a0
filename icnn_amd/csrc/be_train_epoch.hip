// What the training scripts do once per epoch around their step, on the device (include/icnn_be.h icnn_be_gd_eval,
// icnn_be_macro_f1, icnn_be_keep_best): the test phase of the FC back-optimisation trainer
// (multi-label-cls/icnn-back.py:208-216), util.macroF1 and the scripts' "keep the model when the score is better"
// (multi-label-cls/icnn_ebundle.py:274-277, synthetic-cls/icnn.py:206-209).
//
//   gd_eval_kernel    the loss-only form of gd_feed_kernel (be_train_gd.hip): one workgroup per sample forms the sample's sum
//                     of d^2 and, when asked, its F1 tallies, and the last workgroup to take a ticket forms the loss -- through
//                     the device functions of be_train_gd_dev.h that gd_feed_kernel itself runs, so the bits are the feed's.
//   macro_f1_kernel   one workgroup: mean over the examples of 2 tp / (2 tp + fp + fn), 0 where the denominator is 0, in
//                     float64 with IEEE divisions; each thread its examples in index order, then the fixed tree.
//   keep_best_kernel  one thread: go = the score is strictly better than *best (a NaN never is), the offer counters, and
//                     *best = score when it goes.  go is the word icnn_be_gated_copy takes, which makes the snapshot.
#include <hip/hip_runtime.h>

#include "be_api_check.h"
#include "be_kernels.h"
#include "be_train_gd_dev.h"

namespace icnn_be {

namespace {

constexpr int GT = GD_FEED_THREADS;

// the loss-only form of the feed of be_train_gd.hip: loss [1] and, unless NULL, tallies [B][3]; nothing else is written
struct GdEvalLaunch {
    const double *yK;             // [B][n] y_K (float32 values)
    const float *t;               // [B][n] targets
    int B, n;
    float *loss;
    int *tallies;                 // [B][3] tp / fp / fn (may be NULL)
    void *work;                   // gd_feed_work_bytes(B)
};

struct GdEvalArgs {
    GdEvalLaunch l;
    double *partial;     // [B]
    int *ticket;
};

__global__ __launch_bounds__(GT) void gd_eval_kernel(GdEvalArgs a) {
    __shared__ double red[GT];
    __shared__ int ired[GT];
    __shared__ int s_last;
    const GdEvalLaunch &l = a.l;
    const int j = blockIdx.x, n = l.n;
    const double *y_row = l.yK + (size_t)j * n;
    const float *t_row = l.t + (size_t)j * n;
    const double s = gd_sample_sqerr(y_row, t_row, n, red);
    if (l.tallies) gd_sample_tallies(y_row, t_row, n, ired, l.tallies + 3 * (size_t)j);
    gd_loss_behind_ticket(a.partial, a.ticket, j, s, l.B, n, l.loss, red, &s_last);
}

constexpr int F1T = 256;

__global__ __launch_bounds__(F1T) void macro_f1_kernel(const int *tallies, int B, double *f1) {
#pragma clang fp contract(off)
    __shared__ double red[F1T];
    double tot = 0.0;
    for (int b = threadIdx.x; b < B; b += F1T) {
        const int *row = tallies + 3 * (size_t)b;
        const double tp2 = 2.0 * (double)row[0];
        const double den = tp2 + (double)row[1] + (double)row[2];
        tot = tot + (den > 0.0 ? tp2 / den : 0.0);
    }
    tot = block_tree_sum<F1T>(tot, red);
    if (threadIdx.x == 0) *f1 = tot / (double)B;
}

__global__ void keep_best_kernel(const void *score, int score_is_f64, int mode, double *best, int *gate) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double s = score_is_f64 ? *static_cast<const double *>(score) : (double)*static_cast<const float *>(score);
    const double b = *best;
    const int go = mode ? s > b : s < b;            // false for a NaN on either side
    gate[0] = go;
    gate[1] = gate[1] + 1;
    gate[2] = gate[2] + go;
    if (go) *best = s;
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

size_t icnn_be_gd_eval_work_bytes(int B) { return B < 1 ? 0 : gd_feed_work_bytes(B); }

int icnn_be_gd_eval(const double *yK, const float *t, int B, int n, float *loss, int *f1_tallies, void *work, void *stream) {
    if (B < 1 || n < 1) return ICNN_BE_EINVAL;
    if (!yK || !t || !loss || !work) return ICNN_BE_EINVAL;
    GdEvalArgs a{};
    a.l = GdEvalLaunch{yK, t, B, n, loss, f1_tallies, work};
    a.partial = gd_feed_partial(work);
    a.ticket = gd_feed_ticket(work, B);
    return api_done(launch_kernel(gd_eval_kernel, dim3(B), dim3(GT), 0, static_cast<hipStream_t>(stream), a));
}

int icnn_be_macro_f1(const int *tallies, int B, double *f1, void *stream) {
    if (B < 1 || !tallies || !f1) return ICNN_BE_EINVAL;
    return api_done(launch_kernel(macro_f1_kernel, dim3(1), dim3(F1T), 0, static_cast<hipStream_t>(stream), tallies, B, f1));
}

int icnn_be_keep_best(const void *score, int score_is_f64, int mode, double *best, int *gate, void *stream) {
    if (!score || !best || !gate) return ICNN_BE_EINVAL;
    if (mode != ICNN_BE_KEEP_MIN && mode != ICNN_BE_KEEP_MAX) return ICNN_BE_EINVAL;
    return api_done(launch_kernel(keep_best_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), score,
                                  (int)(score_is_f64 != 0), mode, best, gate));
}

}  // extern "C"
