// Unrolled momentum gradient descent on y -- the "back-optimisation" inference of the reference
// (multi-label-cls/icnn-back.py:120-133, completion/icnn.back.py:136-147): from v_0 = 0, for k = 0 .. K-1
//     g_k     = dE/dy(x, y_k)
//     v_{k+1} = mu v_k - lr g_k
//     y_{k+1} = (y_k - mu v_k) + (1+mu) v_{k+1}
// in float32 graph arithmetic, every operation rounded, no contraction; the constants are float32(mu), float32(lr) and
// float32(1.0 + mu) with the sum formed in double.  (At k = 0 the reference's mu*v_0 is the Python 0.0 times mu, the same
// value as mu * 0.f here, so the recurrence needs no special first step.)  No stopping rule and no coupling between samples.
// This unit is the iterate loop of be_gd_dev.h with MomentumRule, in its three forms:
//     gd_fc_kernel    gd_tile_loop around fc_fg_tile: y in the caller's y_out, v and g in the workspace (the FICNN's
//                     ficnn_gd_kernel, be_ficnn.hip, is the same loop around its own tile)
//     gd_rows_kernel  gd_rows_loop (be_gd_rows_dev.h): at most two samples per CU, context rows, y and v in LDS
//     gd_init_kernel / gd_update_kernel   the conv model's elementwise launches inside conv_gd_rounds
// Both FC paths evaluate E and dE/dy with the operations of icnn_be_fc_fg, so the three forms agree bit for bit with a loop of
// icnn_be_fc_fg plus this float32 update.  The workspace carving of both rules and the float32 constants are
// defined here.
#include <cmath>

#include "be_kernels.h"
#include "be_gd_rows_dev.h"

namespace icnn_be {

namespace {

typedef GdTileArgs<FcArgs> GdArgs;

__global__ __launch_bounds__(NTHREADS) void gd_fc_kernel(GdArgs a) { gd_tile_loop<FcTile, MomentumRule>(a); }

__global__ __launch_bounds__(RTHREADS) void gd_rows_kernel(GdRowsArgs<MomentumRule> r) { gd_rows_loop(r); }

// ---- conv model: elementwise start and update around the conv fg launches ----
__global__ void gd_init_kernel(const double *y0, double *y, float *v, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    y[i] = (double)(float)y0[i];
    v[i] = 0.f;
}

__global__ void gd_update_kernel(double *y, float *v, const float *g, double *traj, int n, int n_iter, int k, size_t count,
                                 float lr, float mu, float c1) {
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float yk = (float)y[i], vk = v[i];
    if (traj) {
        const size_t s = i / (size_t)n, j = i - s * (size_t)n;
        traj[(s * n_iter + k) * n + j] = (double)yk;
    }
    gd_step(yk, vk, g[i], lr, mu, c1);
    y[i] = (double)yk;
    v[i] = vk;
}

}  // namespace

GdWorkspace gd_workspace(int batch, int n, size_t state_bytes) {
    GdWorkspace w;
    const size_t b = (size_t)(batch > 0 ? batch : 1), bn = b * (size_t)n;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    w.v = take(bn * state_bytes); w.g = take(bn * 4); w.f = take(b * 4);
    w.total = o;
    return w;
}

GdConstants gd_constants(double lr, double momentum) { return {(float)lr, (float)momentum, (float)(1.0 + momentum)}; }

size_t gd_workspace_bytes(int batch, int n) { return gd_workspace(batch, n, MomentumRule::ws_state_bytes).total; }

bool gd_constants_ok(double lr, double momentum) {
    const GdConstants c = gd_constants(lr, momentum);
    return std::isfinite(lr) && std::isfinite(momentum) && std::isfinite(c.lr) && std::isfinite(c.mu) && std::isfinite(c.c1);
}

hipError_t launch_fc_gd(const icnn_be_fc_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                        double momentum, double *y_out, double *traj, float *f_out, void *ws, hipStream_t stream) {
    GdArgs a{};
    int lds = 0;
    if (fill_args(m, a.fa, lds) != 0) return hipErrorInvalidValue;
    gd_fill_args(a, y0, y_out, traj, f_out, n_iter, lr, momentum, ws, batch);
    a.fa.ctx = ctx; a.fa.prof = fc_profile_buffer();
    return launch_fc_gd_rule<MomentumRule>(m, a, batch, lds, gd_fc_kernel, gd_rows_kernel, stream);
}

hipError_t launch_conv_gd(const icnn_be_conv_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                          double momentum, double *y_out, double *traj, float *f_out, void *ws, hipStream_t stream) {
    const GdConstants c = gd_constants(lr, momentum);
    const int n = m.H * m.W, threads = 256;
    const GdWorkspace w = gd_workspace(batch, n, MomentumRule::ws_state_bytes);
    unsigned char *base = static_cast<unsigned char *>(ws);
    float *v = reinterpret_cast<float *>(base + w.v), *g = reinterpret_cast<float *>(base + w.g);
    float *f = f_out ? f_out : reinterpret_cast<float *>(base + w.f);
    const size_t count = (size_t)batch * n;
    const dim3 grid((unsigned)((count + threads - 1) / threads));
    return conv_gd_rounds(
        m, ctx, y_out, batch, n_iter, f, g, f_out != nullptr, stream,
        [&] { return launch_kernel(gd_init_kernel, grid, dim3(threads), 0, stream, y0, y_out, v, count); },
        [&](int k) {
            return launch_kernel(gd_update_kernel, grid, dim3(threads), 0, stream, y_out, v, (const float *)g, traj, n, n_iter, k,
                                 count, c.lr, c.mu, c.c1);
        },
        [] { return hipSuccess; });                          // E(y_K) is in f = f_out already
}

}  // namespace icnn_be
