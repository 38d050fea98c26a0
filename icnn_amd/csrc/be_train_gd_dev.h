// Device code that the feeds of the back-optimisation trainers share (be_train_gd.hip: gd_feed_kernel, gd_feed_px_kernel;
// be_train_epoch.hip: gd_eval_kernel): a sample's squared error and F1 tallies, and the ticket behind which the last
// workgroup forms the loss.  One copy, so that the loss-only form has the feed's bits by construction: the same float64
// products, the same per-sample tree, the same fixed order over the per-sample sums.
#pragma once
#include <hip/hip_runtime.h>

#include "be_common.h"

namespace icnn_be {

constexpr int GD_FEED_THREADS = 256;

// a feed's work area (zeroed once): the per-sample sums (8-byte aligned) and the ticket, and where it keeps them
inline size_t gd_feed_work_bytes(int B) { return sizeof(double) * (size_t)(B > 0 ? B : 1) + 16; }
__host__ __device__ inline double *gd_feed_partial(void *work) { return static_cast<double *>(work); }
__host__ __device__ inline int *gd_feed_ticket(void *work, int B) {
    return reinterpret_cast<int *>(static_cast<double *>(work) + (B > 0 ? B : 1));
}

// sum over the sample's n labels of d^2, d = float32(y) - t, every product exact in float64; valid in every thread
__device__ __forceinline__ double gd_sample_sqerr(const double *y_row, const float *t_row, int n, double *red) {
#pragma clang fp contract(off)
    constexpr int GT = GD_FEED_THREADS;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += GT) {
        const float d = (float)y_row[i] - t_row[i];
        s = s + (double)d * (double)d;
    }
    return block_tree_sum<GT>(s, red);
}

// tp, fp, fn of the sample over its labels (prediction y >= 0.5, truth (int)t != 0) into out[3]
__device__ __forceinline__ void gd_sample_tallies(const double *y_row, const float *t_row, int n, int *ired, int *out) {
    constexpr int GT = GD_FEED_THREADS;
    int tp = 0, fp = 0, fn = 0;
    for (int i = threadIdx.x; i < n; i += GT) {
        const bool pred = y_row[i] >= 0.5, truth = (int)t_row[i] != 0;
        tp += pred && truth;
        fp += pred && !truth;
        fn += !pred && truth;
    }
    tp = block_tree_sum<GT>(tp, ired);
    fp = block_tree_sum<GT>(fp, ired);
    fn = block_tree_sum<GT>(fn, ired);
    if (threadIdx.x == 0) {
        out[0] = tp;
        out[1] = fp;
        out[2] = fn;
    }
}

// Thread 0 of sample j's workgroup publishes the sample's sum s and takes a ticket; the workgroup that takes the last of the
// B tickets adds the per-sample sums (each thread its samples in index order, then the fixed tree), scales by 1 / (B n) in
// double, rounds once to float32 and re-arms the ticket for the next launch.  Called by every thread of the workgroup.
__device__ __forceinline__ void gd_loss_behind_ticket(double *partial, int *ticket, int j, double s, int B, int n, float *loss,
                                                      double *red, int *s_last) {
#pragma clang fp contract(off)
    constexpr int GT = GD_FEED_THREADS;
    const int tid = threadIdx.x;
    if (tid == 0) {
        __hip_atomic_store(partial + j, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int mine = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        *s_last = mine == B - 1;
    }
    __syncthreads();
    if (!*s_last) return;
    double tot = 0.0;
    for (int b = tid; b < B; b += GT) tot = tot + __hip_atomic_load(partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tot = block_tree_sum<GT>(tot, red);
    if (tid == 0) {
        *loss = (float)(tot * (1.0 / ((double)B * (double)n)));
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch
    }
}

}  // namespace icnn_be
