// Host runtime of the training units (be_train_common.hip, be_train_fc.hip, be_train_ficnn.hip, be_train_conv.hip): grid
// size, workspace walk and the launch latch.  A gradient entry runs its whole step twice over the same code: a dry run (no
// workspace) that only sizes the workspace, and the real run that carves it and launches.  The flat-vector trainers
// (be_ddpg.hip, be_naf.hip, be_ff.hip, be_fcn.hip) lay their workspace out in named pieces instead: WorkPieces.  And the one
// device accessor of the packed forward operands that the units unpack their weights with.
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

// W[k][col] of a forward MFMA operand with N output columns, as pack_operand (be_picnn_fc_dev.h) and pack_frag
// (be_picnn_conv.hip) lay it out: 16 x 16 fragments, k-block major, 64 lanes of four consecutive k each
__device__ __forceinline__ float frag_at(const float *p, int N, int k, int col) {
    const int NT = (N + 15) / 16, kb = k >> 4, kk = k & 15, lane = (kk >> 2) * 16 + (col & 15), nt = col >> 4;
    return p[((size_t)(kb * NT + nt) * 64 + lane) * 4 + (kk & 3)];
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

// A workspace that the host can query piece by piece (the ICNN_BE_*_W_* tables of include/icnn_be.h): a unit's own walk gives
// walk() the floats of every piece, and its launchers reach a piece through at()
template <int PIECES>
struct WorkPieces {
    long long off[PIECES];
    float *w;
    explicit WorkPieces(void *work) : w(static_cast<float *>(work)) {}
    float *at(int piece) const { return w + off[piece]; }
    // off[i] (off not NULL): the float offset of piece i; returns the floats of the whole workspace
    static size_t walk(const size_t (&floats)[PIECES], long long *off) {
        Carver c{nullptr};
        for (int i = 0; i < PIECES; ++i) {
            if (off) off[i] = (long long)c.at;
            c.take(floats[i]);
        }
        return c.at;
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
    // partials that a launcher called through call() asks for
    void need(size_t floats) {
        if (floats > part_need) part_need = floats;
    }
    // C[M][N] (pitch ldc) = A B through launch_tr_gemm
    void gemm(const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, int M, int N, int K,
              float *C, long long ldc, const int *rows_dev = nullptr, int m_per_row = 0, bool dev_size = false) {
        // dev_size: size the partials for a device plan (the dry run of the device-count variant has no rows_dev yet)
        need(tr_gemm_part_floats(M, N, K, dev_size || rows_dev != nullptr));
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
