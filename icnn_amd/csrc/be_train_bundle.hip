// The host-free pieces of the bundle-entropy training step (multi-label-cls/icnn_ebundle.py:208-250,
// completion/icnn_ebundle.py; include/icnn_be.h icnn_be_feed_plan and icnn_be_feed_pad): everything the
// host used to read back between the solve and the gradient.
//
//   feed_plan_kernel   one workgroup per sample: that sample's part of the training loss in double (crossEntr, :419-421,
//                      or the squared error of completion :476-477) and, for the cross entropy, its F1 tallies tp / fp / fn
//                      with the prediction y* >= 0.5 (util.macroF1 averages over EXAMPLES).  The last workgroup to take a
//                      ticket scans the counts into row_offset, adds the per-sample losses in sample order, and reduces
//                      n_iters / finished / status to the fg evaluation count (bundle_entropy.fg_evaluations) and the OR
//                      of the status words.  Every sum has one fixed order: the same bits on every call.
//   feed_pad_kernel    rows [rows, row_cap) of a fixed-capacity feed: y = 0.5, v = 0, c = 0, sample B - 1.
//   step_gate_kernel   the skip on a solver error (completion/icnn_ebundle.py:225-237) as three words of device memory, from
//                      the plan's counts: go, the BatchNorm fold count of a step that goes, the running total of steps that
//                      did not.
#include <hip/hip_runtime.h>

#include <climits>

#include "be_api_check.h"
#include "be_kernels.h"

namespace icnn_be {

namespace {

constexpr int PT = 256;

struct PlanArgs {
    FeedPlanLaunch l;
    int n_iter;
    double *partial;     // [B]
    int *ticket;
};

__global__ __launch_bounds__(PT) void feed_plan_kernel(PlanArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[PT];
    __shared__ int ired[PT];
    __shared__ int s_last;
    const icnn_be_state &st = a.l.st;
    const int tid = threadIdx.x, u = blockIdx.x, n = st.n, B = st.batch;
    // ---- this sample's loss terms and tallies ----
    const double *y_row = st.y + (size_t)u * n, *t_row = a.l.y_true + (size_t)u * n;
    double s = 0.0;
    int tp = 0, fp = 0, fn = 0;
    for (int j = tid; j < n; j += PT) {
        const double y = y_row[j], t = t_row[j];
        if (a.l.loss == ICNN_BE_LOSS_XENT) {
            if (y > 0.0) s = s - t * log(y);
            if (y < 1.0) s = s - (1.0 - t) * log(1.0 - y);
            const bool pred = y >= 0.5, truth = (int)t != 0;
            tp += pred && truth;
            fp += pred && !truth;
            fn += !pred && truth;
        } else {
            const double d = 255.0 * (y - t);
            s = s + d * d;
        }
    }
    s = block_tree_sum<PT>(s, red);
    if (a.l.tallies && a.l.loss == ICNN_BE_LOSS_XENT) {
        tp = block_tree_sum<PT>(tp, ired);
        fp = block_tree_sum<PT>(fp, ired);
        fn = block_tree_sum<PT>(fn, ired);
        if (tid == 0) {
            a.l.tallies[3 * u] = tp;
            a.l.tallies[3 * u + 1] = fp;
            a.l.tallies[3 * u + 2] = fn;
        }
    }
    if (tid == 0) {
        __hip_atomic_store(a.partial + u, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int ticket = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    // ---- the last workgroup: row_offset = exclusive scan of the counts (each clamped to 0 .. slots) ----
    const int per = (B + PT - 1) / PT, b0 = min(tid * per, B), b1 = min(b0 + per, B);
    int mine = 0;
    for (int b = b0; b < b1; ++b) mine += min(max(st.count[b], 0), st.slots);
    ired[tid] = mine;
    __syncthreads();
    int at = 0;
    for (int i = 0; i < tid; ++i) at += ired[i];
    __syncthreads();
    for (int b = b0; b < b1; ++b) {
        a.l.row_offset[b] = at;
        at += min(max(st.count[b], 0), st.slots);
    }
    const int rows = block_tree_sum<PT>(mine, ired);
    // ---- fg evaluations (bundle_entropy.fg_evaluations), OR of the status words ----
    int all_done = 1, most = INT_MIN, bits = 0;
    for (int b = tid; b < B; b += PT) {
        all_done &= st.finished[b] != 0;
        most = max(most, st.n_iters[b]);
        bits |= st.status[b];
    }
    all_done = block_tree_reduce<PT>(all_done, ired, [](int a, int b) { return min(a, b); });
    most = block_tree_reduce<PT>(most, ired, [](int a, int b) { return max(a, b); });
    bits = block_tree_reduce<PT>(bits, ired, [](int a, int b) { return a | b; });
    // ---- the loss: per-sample parts in sample order within a thread, then the fixed tree ----
    double tot = 0.0;
    for (int b = tid; b < B; b += PT) tot = tot + __hip_atomic_load(a.partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tot = block_tree_sum<PT>(tot, red);
    if (tid == 0) {
        a.l.row_offset[B] = rows;
        a.l.counts[0] = rows;
        a.l.counts[1] = all_done ? min(a.n_iter, most + 2) : a.n_iter;
        a.l.counts[2] = bits;
        *a.l.loss_out = a.l.loss == ICNN_BE_LOSS_XENT ? tot : tot / ((double)B * (double)n);
        __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch
    }
}

__global__ void feed_pad_kernel(const int *rows, int batch, int n, int row_cap, double *fd_y, double *fd_v, double *fd_c,
                                int *fd_sample) {
    const int first = min(max(*rows, 0), row_cap);
    const size_t total = (size_t)(row_cap - first) * n;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = first + i / n, at = (size_t)first * n + i;
        fd_y[at] = 0.5;
        fd_v[at] = 0.0;
        if (i % n == 0) {
            fd_c[r] = 0.0;
            fd_sample[r] = batch - 1;
        }
    }
}

// one workgroup, one lane: gate[2] is read and written by this lane alone, launches on a stream are ordered
__global__ void step_gate_kernel(const int *counts, int mask, int *gate) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int go = (counts[2] & mask) == 0;
    gate[0] = go;
    gate[1] = go ? counts[1] : 0;
    gate[2] = gate[2] + (go ? 0 : 1);
}

}  // namespace

hipError_t launch_feed_plan(const FeedPlanLaunch &l, hipStream_t stream) {
    PlanArgs a{};
    a.l = l;
    a.n_iter = l.st.iters > 0 ? l.st.iters : l.st.slots;
    a.partial = static_cast<double *>(l.work);
    a.ticket = reinterpret_cast<int *>(a.partial + (l.st.batch > 0 ? l.st.batch : 1));
    return launch_kernel(feed_plan_kernel, dim3(l.st.batch), dim3(PT), 0, stream, a);
}

}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

// the per-sample loss parts (8-byte aligned) and the ticket
size_t icnn_be_feed_plan_work_bytes(int batch) { return batch < 0 ? 0 : sizeof(double) * (size_t)(batch > 0 ? batch : 1) + 16; }

int icnn_be_feed_pad(const int *rows, int batch, int n, int row_cap, double *fd_y, double *fd_v, double *fd_c, int *fd_sample,
                     void *stream) {
    if (!rows || !fd_y || !fd_v || !fd_c || !fd_sample || batch < 1 || n < 1 || row_cap < 0) return ICNN_BE_EINVAL;
    if (row_cap == 0) return 0;
    const size_t most = (size_t)row_cap * n;
    const int blocks = (int)((most + 255) / 256 < 2048 ? (most + 255) / 256 : 2048);
    return api_done(launch_kernel(feed_pad_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, static_cast<hipStream_t>(stream),
                                  rows, batch, n, row_cap, fd_y, fd_v, fd_c, fd_sample));
}

int icnn_be_step_gate(const int *counts, int mask, int *gate, void *stream) {
    if (!counts || !gate) return ICNN_BE_EINVAL;
    return api_done(launch_kernel(step_gate_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), counts, mask, gate));
}

}  // extern "C"
