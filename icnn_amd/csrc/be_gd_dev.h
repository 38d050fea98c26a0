// The one-launch momentum-GD loop of a tile model (be_gd.hip's recurrence): a persistent workgroup per TM-sample tile that
// alternates phase A (the model's energy/gradient tile) and phase B (the float32 update, one wave per sample).  Instantiated
// by gd_fc_kernel (be_gd.hip, fc_fg_tile) and ficnn_gd_kernel (be_ficnn.hip, ficnn_fg_tile); a unit that includes this needs
// -mllvm -disable-machine-licm (build.py).  The host section below is the one workspace layout and the one set of float32
// constants of every GD entry.
#pragma once
#include "be_picnn_fc_dev.h"

namespace icnn_be {

// the workspace of icnn_be_gd_workspace_bytes (byte offsets, each part 256-byte aligned) and the float32 constants of the
// recurrence, both defined in be_gd.hip
struct GdWorkspace {
    size_t v, g, f, total;
};
GdWorkspace gd_workspace(int batch, int n);
struct GdConstants {
    float lr, mu, c1;      // float32(lr), float32(mu), float32(1.0 + mu)
};
GdConstants gd_constants(double lr, double momentum);

namespace {

template <typename FA>     // FA: the arguments of the model's energy/gradient tile (FcArgs, FicnnArgs)
struct GdTileArgs {
    FA fa;                 // fa.y = y (the iterate), fa.g = per-iteration dE/dy, fa.f = f_out or scratch
    const double *y0;      // [B][n] start (float32 values after rounding on entry)
    double *y;             // [B][n] the iterate, y_K on exit (the caller's y_out)
    float *v;              // [B][n] momentum (workspace)
    double *traj;          // [B][K][n] y_0 .. y_{K-1}, or nullptr
    float *f_out;          // [B] E(y_K), or nullptr: no final evaluation
    int n_iter;
    float lr, mu, c1;      // float32(lr), float32(mu), float32(1.0 + mu)
};

// The loop fields of a launch whose a.fa the model has filled (a.fa.n): the caller's buffers, v / g / f out of the workspace,
// the constants, and the tile's y / g / f / batch / finished.  a.fa.ctx (and what else the tile reads) stays the caller's.
template <typename FA>
void gd_fill_args(GdTileArgs<FA> &a, const double *y0, double *y_out, double *traj, float *f_out, int n_iter, double lr,
                  double momentum, void *ws, int batch) {
    const GdWorkspace w = gd_workspace(batch, a.fa.n);
    const GdConstants c = gd_constants(lr, momentum);
    unsigned char *base = static_cast<unsigned char *>(ws);
    a.y0 = y0; a.y = y_out; a.traj = traj; a.f_out = f_out; a.n_iter = n_iter;
    a.v = reinterpret_cast<float *>(base + w.v);
    a.lr = c.lr; a.mu = c.mu; a.c1 = c.c1;
    a.fa.y = y_out; a.fa.batch = batch; a.fa.finished = nullptr;
    a.fa.g = reinterpret_cast<float *>(base + w.g);
    a.fa.f = f_out ? f_out : reinterpret_cast<float *>(base + w.f);
}

// One step of the recurrence for one element (shared by every path: the same float32 operations in the same order)
__device__ __forceinline__ void gd_step(float &y, float &v, float g, float lr, float mu, float c1) {
#pragma clang fp contract(off)
    const float mv = mu * v;
    const float vn = mv - lr * g;
    y = (y - mv) + c1 * vn;
    v = vn;
}

// Phase A reads its arguments from the kernel-argument segment and is inlined into the iteration loop, with the thread
// index read opaquely (thread_id) and -mllvm -disable-machine-licm for the unit: the recipe of be_fused.hip / be_adam.hip.
// Tile::run(fa, tile, lds) is the model's energy/gradient tile.
template <typename Tile, typename KArgs>
__device__ __forceinline__ void gd_phase_fg(KArgs *kp, int tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    asm volatile("" : "+s"(kp), "+s"(tile));
    Tile::run(kp->fa, tile, lds);
}

// Phase B: wave w updates sample tile * TM + w (g from phase A through global memory, y and v in global memory)
template <typename KArgs>
__device__ __forceinline__ void gd_phase_update(KArgs *kp, int tile, int k) {
#pragma clang fp contract(off)
    asm volatile("" : "+s"(kp), "+s"(tile), "+s"(k));
    const int tid = thread_id(), wave = tid >> 6, lane = tid & 63;
    const int n = kp->fa.n, u = tile * TM + wave;
    if (u >= kp->fa.batch) return;
    const size_t row = (size_t)u * n;
    double *traj = kp->traj ? kp->traj + ((size_t)u * kp->n_iter + k) * n : nullptr;
    const float lr = kp->lr, mu = kp->mu, c1 = kp->c1;
    for (int j = lane; j < n; j += 64) {
        float y = (float)kp->y[row + j], v = kp->v[row + j];
        if (traj) traj[j] = (double)y;
        gd_step(y, v, kp->fa.g[row + j], lr, mu, c1);
        kp->y[row + j] = (double)y;
        kp->v[row + j] = v;
    }
}

// The body of a __global__ __launch_bounds__(NTHREADS) kernel whose only parameter is `a`, one workgroup per tile
template <typename Tile, typename FA>
__device__ __forceinline__ void gd_tile_loop(const GdTileArgs<FA> &a) {
#pragma clang fp contract(off)
    typedef const __attribute__((address_space(4))) GdTileArgs<FA> KArgs;
    KArgs *kp = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int tile = blockIdx.x;
    {
        const int tid = thread_id(), wave = tid >> 6, lane = tid & 63;
        const int n = a.fa.n, u = tile * TM + wave;
        if (u < a.fa.batch)
            for (int j = lane; j < n; j += 64) {         // y_0 rounded to float32 like a feed
                const size_t i = (size_t)u * n + j;
                a.y[i] = (double)(float)a.y0[i];
                a.v[i] = 0.f;
            }
    }
    __syncthreads();
    const int K = a.n_iter;
    for (int k = 0; k < K; ++k) {
        gd_phase_fg<Tile>(kp, tile);
        __syncthreads();                                 // g of the tile visible to its update waves
        gd_phase_update(kp, tile, k);
        __syncthreads();                                 // y_{k+1} visible to the tile's next phase A
    }
    if (a.f_out) gd_phase_fg<Tile>(kp, tile);            // E(y_K) -> fa.f = f_out
}

}  // namespace
}  // namespace icnn_be
