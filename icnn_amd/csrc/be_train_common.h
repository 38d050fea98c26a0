// Host runtime of the training units (be_train_common.hip, be_train_fc.hip, be_train_conv.hip): grid size, workspace walk
// and the launch latch.  A gradient entry runs its whole step twice over the same code: a dry run (no workspace) that only
// sizes the workspace, and the real run that carves it and launches.
#pragma once
#include <hip/hip_runtime.h>

#include "be_common.h"
#include "be_kernels.h"

namespace icnn_be {

// grid-stride launches: enough workgroups for `total` items, at most 4096
inline int grid_for(size_t total, int threads = 256) {
    const size_t b = (total + threads - 1) / threads;
    return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

// Workspace carving: the same walk sizes the buffer (dry run, base == nullptr) and launches (base != nullptr)
struct Carver {
    float *base;
    size_t at = 0;
    float *take(size_t floats) {
        float *p = base ? base + at : nullptr;
        at += (floats + 63) & ~size_t(63);       // 256-byte alignment of every piece
        return p;
    }
};

// The launches of one step: the first error latches and skips everything behind it; the dry run launches nothing and
// records the most split-K partial floats any product asks for
struct Runner {
    hipStream_t stream;
    float *part;            // split-K partials (dry run: nullptr)
    size_t part_need = 0;
    hipError_t err = hipSuccess;
    bool dry() const { return part == nullptr; }
    // C[M][N] (pitch ldc) = A B through launch_tr_gemm
    void gemm(const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, int M, int N, int K,
              float *C, long long ldc, const int *rows_dev = nullptr, int m_per_row = 0, bool dev_size = false) {
        // dev_size: size the partials for a device plan (the dry run of the device-count variant has no rows_dev yet)
        const size_t need = tr_gemm_part_floats(M, N, K, dev_size || rows_dev != nullptr);
        if (need > part_need) part_need = need;
        if (err != hipSuccess || dry()) return;
        err = launch_tr_gemm(A, sam, sak, B, sbk, sbn, M, N, K, C, ldc, part, stream, rows_dev, m_per_row);
    }
    template <typename... KArgs, typename... Args>
    void launch(void (*k)(KArgs...), dim3 grid, int block, Args... args) {
        if (err != hipSuccess || dry()) return;
        err = launch_kernel(k, grid, dim3(block), 0, stream, args...);
    }
    // a launcher of another unit: f() returns its hipError_t
    template <typename F>
    void call(F f) {
        if (err != hipSuccess || dry()) return;
        err = f();
    }
};

}  // namespace icnn_be
