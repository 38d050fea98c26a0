// Fully input-convex network (FICNN) of synthetic-cls/icnn.py:213-234 on the device:
//     ficnn_fg_kernel   E and dE/dy of a tile of 16 samples per workgroup: forward z-layers and backward deltas in LDS,
//                       v_mfma_f32_16x16x4_f32 against pre-packed B fragments, ReLU masks recovered from the signs of the
//                       stored activations (the design of fc_fg_tile, DESIGN.md §4, without gate or yu operands)
//     ficnn_gd_kernel   unrolled momentum GD: a persistent workgroup per tile alternating phase A (the fg tile) and phase B
//                       (the float32 update, one wave per sample), plus a final phase A for E(y_K): be_gd_dev.h's gd_tile_loop
//                       with MomentumRule around this unit's tile, set up by gd_fill_args like gd_fc_kernel (be_gd.hip)
//     the context       c_i = x Wx_i + b_i of every evaluated layer: one f32-MFMA GEMM (launch_tr_gemm) and a bias row
// Every float32 operation of the tile is written out (no contraction), so the same inputs give the same bits on every call
// and the GD loop is bit-identical to a loop of ficnn fg launches plus the update.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "be_ficnn_dev.h"
#include "be_gd_dev.h"
#include "be_train_common.h"

namespace icnn_be {

namespace {

struct FicnnArgs {
    int n, L, head, ctx_width, batch;
    int width[ICNN_BE_MAX_LAYERS], c_off[ICNN_BE_MAX_LAYERS];
    long long w_yf[ICNN_BE_MAX_LAYERS], w_yb[ICNN_BE_MAX_LAYERS], w_zf[ICNN_BE_MAX_LAYERS], w_zb[ICNN_BE_MAX_LAYERS];
    long long w_yL, w_zL;
    int z_off[ICNN_BE_MAX_LAYERS], z_ld[ICNN_BE_MAX_LAYERS];
    int ldY, ybuf_off, gbuf_off, dl_off, lds_floats;
    const float *wpack, *ctx;
    const double *y;
    float *f, *g;
    const int *finished;
};

int ficnn_fill_args(const icnn_be_ficnn_model &m, FicnnArgs &a, int &lds_bytes) {
    if (int rc = ficnn_check(m)) return rc;
    const FicnnPack po = ficnn_pack_offsets(m);
    const FicnnLds l = ficnn_lds(m);
    a = FicnnArgs{};
    a.n = m.n;
    a.L = po.L;
    a.head = m.head;
    a.ctx_width = po.ctx_width;
    for (int i = 0; i <= po.L; ++i) {
        a.width[i] = m.width[i];
        a.c_off[i] = i < po.evald ? po.c_off[i] : -1;
        if (i < po.L) {
            a.w_yf[i] = po.yf[i]; a.w_yb[i] = po.yb[i];
            a.w_zf[i] = po.zf[i]; a.w_zb[i] = po.zb[i];
            a.z_off[i] = l.z_off[i]; a.z_ld[i] = l.z_ld[i];
        }
    }
    a.w_yL = po.yL;
    a.w_zL = po.zL;
    a.ldY = l.ldY;
    a.ybuf_off = l.ybuf;
    a.gbuf_off = l.gbuf;
    a.dl_off = l.dl;
    a.lds_floats = l.floats;
    lds_bytes = l.floats * 4;
    a.wpack = m.wpack;
    return 0;
}

// One tile of TM samples, workgroup-wide (NTHREADS threads); `lds` = the dynamic shared memory of the workgroup
template <typename ArgsT>          // FicnnArgs by value, or a reference into the kernel-argument segment (ficnn_gd_kernel)
__device__ __forceinline__ void ficnn_fg_tile(const ArgsT &a, int tile, float *lds) {
#pragma clang fp contract(off)
    const int tid = thread_id(), lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const int s0 = tile * TM;
    const int rows = min(TM, a.batch - s0);
    const int n = a.n, L = a.L, C = a.ctx_width, ldY = a.ldY, npad = pad16(n);
    const bool linear = a.head == ICNN_BE_FICNN_HEAD_LINEAR;
    float *ybuf = lds + a.ybuf_off, *gbuf = lds + a.gbuf_off, *dl = lds + a.dl_off;
    const float *ctx = a.ctx + (size_t)s0 * C;

    // nothing to do when every sample of the tile has finished (uniform: every thread takes the barrier)
    if (a.finished) {
        int live = 0;
        if (tid < rows) live = a.finished[s0 + tid] == 0;
        if (!__syncthreads_or(live)) return;
    }
    // wave w prepares row w: y rounded to float32 like a feed, zero pad columns behind every GEMM operand (their packed
    // weights are zero, but 0 * stale-NaN would not be); columns below pad16(width) are written by the producing phase
    static_assert(TM == NWAVE, "one wave per row in the preparation phase");
    {
        auto zero_pad = [&](float *buf, int ld, int width) {
            for (int j = pad16(width) + lane; j < ld; j += 64) buf[wave * ld + j] = 0.f;
        };
        zero_pad(ybuf, ldY, n);
        for (int i = 0; i < L; ++i) zero_pad(lds + a.z_off[i], a.z_ld[i], a.width[i]);
        zero_pad(dl, a.z_ld[L - 1], a.width[L - 1]);
        const int r = wave;
        for (int j = lane; j < npad; j += 64) {
            const bool ok = r < rows && j < n;
            ybuf[r * ldY + j] = ok ? (float)a.y[(size_t)(s0 + r) * n + j] : 0.f;
        }
    }
    __syncthreads();

    // ---------------- forward: a_i = c_i + y Wy_i + z_{i-1} Wz_i, z_i = relu(a_i) -----------------------------
    const float *wzL = linear ? a.wpack + a.w_zL : nullptr;
    const float *wyL = linear ? a.wpack + a.w_yL : nullptr;
    for (int i = 0; i < L; ++i) {
        const int wi = a.width[i], NT = pad16(wi) / 16;
        const bool last = i == L - 1;
        float *zout = lds + a.z_off[i];
        const int ldo = a.z_ld[i];
        for (int nt = wave; nt < NT; nt += NWAVE) {
            const int col = nt * 16 + r16;
            f4 acc = {0.f, 0.f, 0.f, 0.f}, unused = {0.f, 0.f, 0.f, 0.f};
            // context operands requested before the MFMA loops (their latency hides behind them)
            float cc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                cc[r] = row < rows && col < wi ? ctx[(size_t)row * C + a.c_off[i] + col] : 0.f;
            }
            // head weight of delta_{L-1}: 1 (SUM) or Wz_L[k] (LINEAR)
            const float hw = !last ? 0.f : !linear ? 1.f : col < wi ? wzL[col] : 0.f;
            gemm_tiles(ybuf, ldY, a.wpack + a.w_yf[i], kblocks_tile(n), NT, nt, -1, acc, unused);
            if (i > 0)
                gemm_tiles(lds + a.z_off[i - 1], a.z_ld[i - 1], a.wpack + a.w_zf[i], kblocks_tile(a.width[i - 1]), NT, nt, -1,
                           acc, unused);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                float v = 0.f, d = 0.f;
                if (row < rows && col < wi) {
                    const float p = acc[r] + cc[r];
                    v = p > 0.f ? p : 0.f;
                    d = p > 0.f ? hw : 0.f;
                }
                zout[row * ldo + col] = v;
                if (last) dl[row * ldo + col] = d;
            }
        }
        __syncthreads();
    }

    // ---------------- backward: dE/dy = sum_i delta_i Wy_i^T (+ Wy_L), delta_{i-1} = (delta_i Wz_i^T) relu'(a_{i-1}) ------
    const int NTy = npad / 16;
    for (int i = L - 1; i >= 0; --i) {
        const bool first = i == L - 1;
        const float *delta = first ? dl : lds + a.z_off[i];
        const int ldd = a.z_ld[i], KB = kblocks_tile(a.width[i]);
        // the few dE/dy tiles go to the waves counted from the top when a delta product shares the phase
        const int wy = i > 0 ? NWAVE - 1 - wave : wave;
        for (int nt = wy; nt < NTy; nt += NWAVE) {
            const int col = nt * 16 + r16;
            f4 acc = {0.f, 0.f, 0.f, 0.f}, unused = {0.f, 0.f, 0.f, 0.f};
            const float gy = first && linear && col < n ? wyL[col] : 0.f;
            gemm_tiles(delta, ldd, a.wpack + a.w_yb[i], KB, NTy, nt, -1, acc, unused);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                if (row < rows && col < n) {
                    const float g_in = first ? gy : gbuf[row * ldY + col];
                    gbuf[row * ldY + col] = g_in + acc[r];
                }
            }
        }
        if (i > 0) {
            const int wp = a.width[i - 1], NTp = pad16(wp) / 16;
            float *zprev = lds + a.z_off[i - 1];
            const int ldp = a.z_ld[i - 1];
            for (int nt = wave; nt < NTp; nt += NWAVE) {
                const int col = nt * 16 + r16;
                f4 acc = {0.f, 0.f, 0.f, 0.f}, unused = {0.f, 0.f, 0.f, 0.f};
                gemm_tiles(delta, ldd, a.wpack + a.w_zb[i], KB, NTp, nt, -1, acc, unused);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * q + r;
                    float d = 0.f;
                    if (row < rows && col < wp) d = zprev[row * ldp + col] > 0.f ? acc[r] : 0.f;
                    zprev[row * ldp + col] = d;           // delta_{i-1} replaces z_{i-1} (only its sign was still needed)
                }
            }
        }
        __syncthreads();
    }

    // ---------------- energy and outputs: wave w owns row w (z_{L-1} and y are still intact) --------------------------
    if (wave < rows) {
        const int r = wave;
        if (!(a.finished && a.finished[s0 + r] != 0)) {
            const float *zl = lds + a.z_off[L - 1];
            const int ldz = a.z_ld[L - 1], wl = a.width[L - 1];
            float part = 0.f;
            if (linear) {
                for (int j = lane; j < wl; j += 64) part = __builtin_fmaf(zl[r * ldz + j], wzL[j], part);
                for (int j = lane; j < n; j += 64) part = __builtin_fmaf(ybuf[r * ldY + j], wyL[j], part);
            } else {
                for (int j = lane; j < wl; j += 64) part += zl[r * ldz + j];
            }
            float e = wave_sum_f(part);
            if (linear) e += ctx[(size_t)r * C + a.c_off[L]];
            if (lane == 0) a.f[s0 + r] = e;
            for (int j = lane; j < n; j += 64) a.g[(size_t)(s0 + r) * n + j] = gbuf[r * ldY + j];
        }
    }
}

__global__ __launch_bounds__(NTHREADS) void ficnn_fg_kernel(FicnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    ficnn_fg_tile(a, blockIdx.x, lds);
}

// ---- unrolled momentum GD: the tile loop of be_gd_dev.h around ficnn_fg_tile, under the momentum rule ----
struct FicnnTile {
    template <typename A>
    static __device__ __forceinline__ void run(const A &fa, int tile, float *lds) { ficnn_fg_tile(fa, tile, lds); }
    template <typename A>
    static __device__ __forceinline__ int rows(const A &) { return TM; }
};
typedef GdTileArgs<FicnnArgs> FicnnGdArgs;

__global__ __launch_bounds__(NTHREADS) void ficnn_gd_kernel(FicnnGdArgs a) { gd_tile_loop<FicnnTile, MomentumRule>(a); }

// ---- context: ctx = x Wx + b ----
__global__ void ficnn_bias_kernel(float *ctx, const float *b, int C, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
        ctx[i] = ctx[i] + b[i % C];
}

}  // namespace

int ficnn_check_model(const icnn_be_ficnn_model &m) { return ficnn_check(m); }

size_t ficnn_pack_floats(const icnn_be_ficnn_model &m) { return ficnn_pack_offsets(m).total; }

int ficnn_pack(const icnn_be_ficnn_model &m, const float *const *w_x, const float *const *b, const float *const *w_z, float *out) {
    const FicnnPack po = ficnn_pack_offsets(m);
    const int nf = m.n_features, n = m.n, L = po.L, C = po.ctx_width;
    std::memset(out, 0, po.total * sizeof(float));
    for (int i = 0; i < po.evald; ++i) {
        const int w = m.width[i];
        for (int k = 0; k < nf; ++k)
            for (int j = 0; j < w; ++j) out[po.wx + (size_t)k * C + po.c_off[i] + j] = w_x[i][(size_t)k * w + j];
        for (int j = 0; j < w; ++j) out[po.bx + po.c_off[i] + j] = b[i][j];
    }
    for (int i = 0; i < L; ++i) {
        const int w = m.width[i];
        const float *wy = w_x[i] + (size_t)nf * w;                  // the y rows of 'z_x{i}/W': [n][w]
        pack_operand(wy, n, w, false, out + po.yf[i]);
        pack_operand(wy, w, n, true, out + po.yb[i]);
        if (i > 0) {
            pack_operand(w_z[i], m.width[i - 1], w, false, out + po.zf[i]);
            pack_operand(w_z[i], w, m.width[i - 1], true, out + po.zb[i]);
        }
    }
    if (po.evald > L) {
        for (int j = 0; j < n; ++j) out[po.yL + j] = w_x[L][(size_t)(nf + j)];       // width[L] = 1
        for (int k = 0; k < m.width[L - 1]; ++k) out[po.zL + k] = w_z[L][k];
    }
    return 0;
}

size_t ficnn_context_work_floats(const icnn_be_ficnn_model &m, int batch) {
    const FicnnPack po = ficnn_pack_offsets(m);
    const size_t need = tr_gemm_part_floats(batch > 0 ? batch : 1, po.ctx_width, m.n_features);
    return need > 0 ? need : 1;
}

hipError_t launch_ficnn_context(const icnn_be_ficnn_model &m, const float *x, int batch, float *ctx, float *work,
                                hipStream_t stream) {
    const FicnnPack po = ficnn_pack_offsets(m);
    const int C = po.ctx_width;
    hipError_t e = launch_tr_gemm(x, m.n_features, 1, m.wpack + po.wx, C, 1, batch, C, m.n_features, ctx, C, work, stream);
    if (e != hipSuccess) return e;
    const size_t total = (size_t)batch * C;
    return launch_kernel(ficnn_bias_kernel, dim3(grid_for(total)), dim3(256), 0, stream, ctx, (const float *)(m.wpack + po.bx),
                         C, total);
}

hipError_t launch_ficnn_fg(const icnn_be_ficnn_model &m, const float *ctx, const double *y, int batch, float *f, float *g,
                           const int *finished, hipStream_t stream) {
    FicnnArgs a;
    int lds = 0;
    if (ficnn_fill_args(m, a, lds) != 0) return hipErrorInvalidValue;
    a.ctx = ctx; a.y = y; a.f = f; a.g = g; a.finished = finished; a.batch = batch;
    return launch_kernel(ficnn_fg_kernel, dim3((batch + TM - 1) / TM), dim3(NTHREADS), lds, stream, a);
}

hipError_t launch_ficnn_gd(const icnn_be_ficnn_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                           double momentum, double *y_out, double *traj, float *f_out, void *ws, hipStream_t stream) {
    FicnnGdArgs a{};
    int lds = 0;
    if (ficnn_fill_args(m, a.fa, lds) != 0) return hipErrorInvalidValue;
    gd_fill_args(a, y0, y_out, traj, f_out, n_iter, lr, momentum, ws, batch);
    a.fa.ctx = ctx;
    return launch_kernel(ficnn_gd_kernel, dim3((batch + TM - 1) / TM), dim3(NTHREADS), lds, stream, a);
}

}  // namespace icnn_be
