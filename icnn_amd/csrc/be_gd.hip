// Unrolled momentum gradient descent on y -- the "back-optimisation" inference of the reference
// (multi-label-cls/icnn-back.py:120-133, completion/icnn.back.py:136-147): from v_0 = 0, for k = 0 .. K-1
//     g_k     = dE/dy(x, y_k)
//     v_{k+1} = mu v_k - lr g_k
//     y_{k+1} = (y_k - mu v_k) + (1+mu) v_{k+1}
// in float32 graph arithmetic, every operation rounded, no contraction; the constants are float32(mu), float32(lr) and
// float32(1.0 + mu) with the sum formed in double.  (At k = 0 the reference's mu*v_0 is the Python 0.0 times mu, the same
// value as mu * 0.f here, so the recurrence needs no special first step.)  No stopping rule and no coupling between samples:
//     gd_fc_kernel    a persistent workgroup per 16-sample tile alternating phase A (fc_fg_tile) and phase B (one wave per
//                     sample: the update above), y in the caller's y_out, v and g in the workspace: the tile loop of
//                     be_gd_dev.h, which the FICNN's ficnn_gd_kernel (be_ficnn.hip) instantiates as well
//     gd_rows_kernel  at most two samples per CU (the rule of launch_fc_fg): context rows, y and v in LDS for the whole loop
//     gd_init_kernel / gd_update_kernel   the conv model's form: K rounds of the conv fg launches, each followed by the
//                     elementwise update (same operations)
// Both FC paths evaluate E and dE/dy with the operations of icnn_be_fc_fg, so the three forms agree bit for bit with a loop of
// icnn_be_fc_fg plus this float32 update.  gd_step, the workspace layout and the float32 constants of every
// form, the FICNN's included, are the ones of be_gd_dev.h; the layout and the constants are defined here.
#include <cmath>

#include "be_kernels.h"
#include "be_gd_dev.h"
#include "be_picnn_fc_rows_dev.h"

namespace icnn_be {

namespace {

struct FcTile {           // phase A of gd_tile_loop
    template <typename A>
    static __device__ __forceinline__ void run(const A &fa, int tile, float *lds) { fc_fg_tile(fa, tile, lds); }
};
typedef GdTileArgs<FcArgs> GdArgs;

__global__ __launch_bounds__(NTHREADS) void gd_fc_kernel(GdArgs a) { gd_tile_loop<FcTile>(a); }

struct GdRowsArgs {
    GdArgs a;
    RowsLayout lay;
    int per_wg;
    int yv_off;            // LDS floats: per sample y[npad] | v[npad], behind the rows layout
};

__global__ __launch_bounds__(RTHREADS) void gd_rows_kernel(GdRowsArgs r) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const GdArgs &a = r.a;
    const FcArgs &fa = a.fa;
    const RowsLayout &lay = r.lay;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = fa.n, npad = pad16(n), RF = lay.row_floats;
    const int s_base = blockIdx.x * r.per_wg;
    const int batch = fa.batch - s_base < r.per_wg ? fa.batch - s_base : r.per_wg;
    float *ys = lds + r.yv_off + wave * 2 * npad, *vs = ys + npad;     // only read by waves < batch
    rows_setup(fa, lay, lds, s_base, batch, tid);
    if (wave < batch) {
        float *row = lds + wave * RF;
        for (int j = lane; j < n; j += 64) {
            const float y = (float)a.y0[(size_t)(s_base + wave) * n + j];
            ys[j] = y;
            vs[j] = 0.f;
            rows_set_input(fa, lay, row, j, y);
        }
    }
    __syncthreads();
    const float lr = a.lr, mu = a.mu, c1 = a.c1;
    for (int k = 0; k < a.n_iter; ++k) {
        rows_eval(fa, lay, lds, batch, tid, [](int) {});     // ends with a workgroup barrier
        if (wave < batch) {
            float *row = lds + wave * RF;
            double *traj = a.traj ? a.traj + ((size_t)(s_base + wave) * a.n_iter + k) * n : nullptr;
            for (int j = lane; j < n; j += 64) {
                float y = ys[j], v = vs[j];
                if (traj) traj[j] = (double)y;
                gd_step(y, v, row[lay.g_off + j], lr, mu, c1);
                ys[j] = y;
                vs[j] = v;
                rows_set_input(fa, lay, row, j, y);
            }
        }
        __syncthreads();
    }
    if (wave < batch)
        for (int j = lane; j < n; j += 64) a.y[(size_t)(s_base + wave) * n + j] = (double)ys[j];
    if (a.f_out) {
        rows_eval(fa, lay, lds, batch, tid, [](int) {});
        if (wave < batch && lane == 0) a.f_out[s_base + wave] = lds[lay.f_off + wave];
    }
}

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

GdWorkspace gd_workspace(int batch, int n) {
    GdWorkspace w;
    const size_t b = (size_t)(batch > 0 ? batch : 1), bn = b * (size_t)n;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    w.v = take(bn * 4); w.g = take(bn * 4); w.f = take(b * 4);
    w.total = o;
    return w;
}

GdConstants gd_constants(double lr, double momentum) { return {(float)lr, (float)momentum, (float)(1.0 + momentum)}; }

size_t gd_workspace_bytes(int batch, int n) { return gd_workspace(batch, n).total; }

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
    // at most two samples per CU: a workgroup per one or two samples on the VALU path (launch_fc_fg's rule)
    const int cus = device_cus();
    const int per_wg = (batch + cus - 1) / cus;
    if (per_wg <= 2) {
        GdRowsArgs r{};
        const int rows_bytes = rows_layout(m, per_wg, r.lay);
        const int yv_bytes = per_wg * 2 * pad16(m.n) * 4;
        if (rows_bytes + yv_bytes <= LDS_BYTES) {
            r.a = a;
            r.per_wg = per_wg;
            r.yv_off = rows_bytes / 4;
            return launch_kernel(gd_rows_kernel, dim3((batch + per_wg - 1) / per_wg), dim3(RTHREADS), rows_bytes + yv_bytes,
                                 stream, r);
        }
    }
    if (lds > LDS_BYTES) return hipErrorNotSupported;
    return launch_kernel(gd_fc_kernel, dim3((batch + TM - 1) / TM), dim3(NTHREADS), lds, stream, a);
}

hipError_t launch_conv_gd(const icnn_be_conv_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                          double momentum, double *y_out, double *traj, float *f_out, void *ws, hipStream_t stream) {
    const GdConstants c = gd_constants(lr, momentum);
    const int n = m.H * m.W;
    const GdWorkspace w = gd_workspace(batch, n);
    unsigned char *base = static_cast<unsigned char *>(ws);
    float *v = reinterpret_cast<float *>(base + w.v), *g = reinterpret_cast<float *>(base + w.g);
    float *f = f_out ? f_out : reinterpret_cast<float *>(base + w.f);
    const size_t count = (size_t)batch * n;
    const int threads = 256;
    const dim3 grid((unsigned)((count + threads - 1) / threads));
    if (hipError_t e = launch_kernel(gd_init_kernel, grid, dim3(threads), 0, stream, y0, y_out, v, count); e != hipSuccess)
        return e;
    for (int k = 0; k < n_iter; ++k) {
        if (hipError_t e = launch_conv_fg(m, ctx, y_out, batch, f, g, nullptr, stream); e != hipSuccess) return e;
        hipError_t e = launch_kernel(gd_update_kernel, grid, dim3(threads), 0, stream, y_out, v, (const float *)g, traj, n,
                                     n_iter, k, count, c.lr, c.mu, c.c1);
        if (e != hipSuccess) return e;
    }
    if (f_out) return launch_conv_fg(m, ctx, y_out, batch, f_out, g, nullptr, stream);
    return hipSuccess;
}

}  // namespace icnn_be
