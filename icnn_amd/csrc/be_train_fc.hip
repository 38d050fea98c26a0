// Training step of the fully-connected PICNN on the device: the parameter gradient of the reference's surrogate
//   F = sum_r c_r E(x_s(r), y_r) + <dE/dy(x_s(r), y_r), v_r>          multi-label-cls/icnn_ebundle.py:148-156
// (v absent: the RL critic's c-weighted energy, RL/src/icnn.py:90-109) over every trainable variable.
//
// Structure (DESIGN.md "Training gradient"):
//   1. x-only forward on the B unique samples, not on the R feed rows: the stage GEMMs are the context producer's
//      (launch_fc_context_stage, be_context.hip); BatchNorm is weighted by the multiplicity m_j of each sample, which
//      equals BatchNorm over the R repeated rows the reference feeds.  The context rows, the ReLU'd u-path values and
//      x-hat / inv-std are kept for the backward pass.
//   2. y-path on the R rows, layer by layer: the primal rows and the tangent rows (direction v) are stacked into one
//      [2R][n + width_{i-1}] operand [ y*yu_i | z_{i-1}*gate_i ; v*yu_i | zdot_{i-1}*gate_i ] so that one GEMM with the
//      stacked weights [Wyu_i ; Wzu_i] gives both pre-activations.  The reverse pass runs the two adjoint columns
//      (abar seeded with c_r, adot seeded with 1) through the same masks: per layer one GEMM for the weight gradient
//      of each operand (K = 2R) and one for the adjoints / context gradient.
//   3. fixed-order segment sum of the per-row context gradient over the rows of each sample.
//   4. x-only backward on B rows: head ReLUs, dW_stage = prev^T dpre, bias sums, dprev = dpre W_stage^T, ReLU and the
//      weighted BatchNorm backward with its batch-statistics terms, down to u0.
// Every product runs through be_train_common.hip's f32-MFMA GEMM (launch_tr_gemm): split-K partials summed in a fixed
// order, no atomics anywhere -- the same bits on every run, and the whole entry can be captured in a graph.
#include <hip/hip_runtime.h>

#include <climits>

#include "be_picnn_fc_dev.h"   // the packed y-path layout (pack_offsets)
#include "be_train_common.h"

namespace icnn_be {

namespace {

// network input of row r, column j: y rounded to float32 like a TensorFlow feed, 2y-1 for the RL wrapper; its tangent
// direction v (times 2 for the wrapper, RL/src/icnn.py:148-158) -- as icnn_be_fc_fg reads y
__device__ __forceinline__ float net_y(const double *y, size_t i, int box) { return box ? (float)(2.0 * y[i] - 1.0) : (float)y[i]; }
__device__ __forceinline__ float net_v(const double *v, size_t i, int box) { return box ? 2.f * (float)v[i] : (float)v[i]; }

struct RowArgs {
    const double *y, *v, *c;
    const int *samp;
    const float *ctx;
    int R, n, C, box;
    const int *rows_dev;        // not NULL: the true row count (rows [*rows_dev, R) are padding: c = 0, v = 0)
};

// PQ_i[:, 0:n) = [ y*yu_i ; v*yu_i ]  (pitch ld)
__global__ void tr_build_p_kernel(RowArgs a, int yu_off, float *pq, int ld) {
    const int total = a.R * a.n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / a.n, j = i - r * a.n;
        const float yu = a.ctx[(size_t)a.samp[r] * a.C + yu_off + j];
        pq[(size_t)r * ld + j] = net_y(a.y, i, a.box) * yu;
        if (a.v) pq[(size_t)(a.R + r) * ld + j] = net_v(a.v, i, a.box) * yu;
    }
}

// hidden layer i: a = pre + zu_i;  z = act(a), d = act'(a), zdot = d * pre_dot;  PQ_{i+1}[:, n + k] = [z ; zdot] * gate_{i+1}
__global__ void tr_hidden_fwd_kernel(RowArgs a, const float *pre, int w, int zu_off, int gate_next_off, float alpha, float *Z,
                                     float *D, float *pq_next, int ld_next) {
    const int total = a.R * w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / w, k = i - r * w;
        const float *crow = a.ctx + (size_t)a.samp[r] * a.C;
        const float p = pre[i] + crow[zu_off + k];
        const float d = p > 0.f ? 1.f : alpha;
        const float z = p > 0.f ? p : alpha * p, g = crow[gate_next_off + k];
        Z[i] = z;
        D[i] = d;
        pq_next[(size_t)r * ld_next + a.n + k] = z * g;
        if (a.v) {
            const float zd = d * pre[(size_t)a.R * w + i];
            Z[(size_t)a.R * w + i] = zd;
            pq_next[(size_t)(a.R + r) * ld_next + a.n + k] = zd * g;
        }
    }
}

// last layer: F_r = c_r (pre_r + zu_L) + pre_dot_r; adjoint seeds abar = c_r, adot = 1
__global__ void tr_final_kernel(RowArgs a, const float *pre, int zu_off, float *F, float *adj) {
    const int live = a.rows_dev ? *a.rows_dev : a.R;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += gridDim.x * blockDim.x) {
        if (r >= live) {            // padding: no energy, no adjoint
            if (F) F[r] = 0.f;
            adj[r] = 0.f;
            if (a.v) adj[a.R + r] = 0.f;
            continue;
        }
        const float c = (float)a.c[r];
        if (F) {
            const float e = pre[r] + a.ctx[(size_t)a.samp[r] * a.C + zu_off];
            F[r] = c * e + (a.v ? pre[a.R + r] : 0.f);
        }
        adj[r] = c;
        if (a.v) adj[a.R + r] = 1.f;
    }
}

// reverse step of layer i from BD = [abar_i ; adot_i] [Wyu_i ; Wzu_i]^T ([2R][n + wprev]):
//   dyu_i = y * BD[r][0:n) + v * BD[R+r][0:n),   dzu_i = abar_i,
//   dgate_i = z_{i-1} * BD[r][n:) + zdot_{i-1} * BD[R+r][n:),   [abar ; adot]_{i-1} = act'(a_{i-1}) * gate_i * BD[.][n:)
struct BackArgs {
    const float *BD, *adj, *Zp, *Dp;
    float *adj_prev, *dctx;          // dctx: per-row context gradient [R][C]
    int w, wprev, yu_off, zu_off, gate_off;
};
__global__ void tr_back_rows_kernel(RowArgs a, BackArgs b) {
    const int cols = a.n + b.wprev + b.w, ldb = a.n + b.wprev, total = a.R * cols;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / cols, j = i - r * cols;
        float *drow = b.dctx + (size_t)r * a.C;
        if (j < a.n) {
            const size_t yi = (size_t)r * a.n + j;
            float g = net_y(a.y, yi, a.box) * b.BD[(size_t)r * ldb + j];
            if (a.v) g += net_v(a.v, yi, a.box) * b.BD[(size_t)(a.R + r) * ldb + j];
            drow[b.yu_off + j] = g;
        } else if (j < ldb) {
            const int k = j - a.n;
            const size_t zi = (size_t)r * b.wprev + k, zr = (size_t)a.R * b.wprev;
            const float bd = b.BD[(size_t)r * ldb + j];
            const float gt = a.ctx[(size_t)a.samp[r] * a.C + b.gate_off + k], dg = b.Dp[zi] * gt;
            float g = b.Zp[zi] * bd;
            b.adj_prev[zi] = dg * bd;
            if (a.v) {
                const float bdd = b.BD[(size_t)(a.R + r) * ldb + j];
                g += b.Zp[zr + zi] * bdd;
                b.adj_prev[zr + zi] = dg * bdd;
            }
            drow[b.gate_off + k] = g;
        } else {
            const int k = j - ldb;
            drow[b.zu_off + k] = b.adj[(size_t)r * b.w + k];
        }
    }
}

// Weighted batch statistics (BatchNorm in training mode over the R feed rows = over the B samples with weights m_j):
// one workgroup per 32 columns, fixed-order tree.  h (the ReLU'd stage output, pitch ld) is copied to hsave, u = gamma
// xhat + beta replaces it in place (the next stage reads it there), xhat and inv-std are kept for the backward pass, the
// mean [N] and variance [N] it normalised with go to stat_out (may be NULL) for the moving statistics.
constexpr int WBT = 256, WBC = 32, WBG = WBT / WBC;
// rows_dev (may be NULL): the normaliser M is the row count read from the device; a count of 0 gives mean 0 and variance 0
__global__ __launch_bounds__(WBT) void tr_wbn_fwd_kernel(float *u, int ld, int B, int N, const float *mult, float M,
                                                         const float *gamma, const float *beta, float eps, float *hsave,
                                                         float *xhat, float *inv_out, float *stat_out, const int *rows_dev) {
    __shared__ float red[WBG][WBC];
    __shared__ float stat[2][WBC];
    if (rows_dev) M = (float)*rows_dev;
    const int c = threadIdx.x % WBC, g = threadIdx.x / WBC, col = blockIdx.x * WBC + c;
    const bool ok = col < N;
    auto total = [&](float mine, float *out) {
        red[g][c] = mine;
        __syncthreads();
        if (g == 0) {
            float t = 0.f;
            for (int i = 0; i < WBG; ++i) t += red[i][c];
            *out = M > 0.f ? t / M : 0.f;
        }
        __syncthreads();
    };
    float s = 0.f;
    if (ok) for (int j = g; j < B; j += WBG) s += mult[j] * u[(size_t)j * ld + col];
    total(s, &stat[0][c]);
    const float mean = stat[0][c];
    s = 0.f;
    if (ok) for (int j = g; j < B; j += WBG) {
        const float d = u[(size_t)j * ld + col] - mean;
        s += mult[j] * d * d;
    }
    total(s, &stat[1][c]);
    if (!ok) return;
    const float inv = 1.f / sqrtf(stat[1][c] + eps), ga = gamma[col], be = beta[col];
    if (g == 0) {
        inv_out[col] = inv;
        if (stat_out) { stat_out[col] = mean; stat_out[N + col] = stat[1][c]; }
    }
    for (int j = g; j < B; j += WBG) {
        const float h = u[(size_t)j * ld + col], xh = (h - mean) * inv;
        hsave[(size_t)j * N + col] = h;
        xhat[(size_t)j * N + col] = xh;
        u[(size_t)j * ld + col] = ga * xh + be;
    }
}

// du (gradient at u_i, [B][N]) -> the u columns of dpre_i (pitch ld_dpre).  mode 0: linear (last u layer); 1: ReLU only
// (hidden layers without BatchNorm, and the last u layer of a context with u_last_relu), mask from u itself;
// 2: weighted BatchNorm backward then ReLU:
//   S1 = sum_j du_j, S2 = sum_j du_j xhat_j,  dh_j = gamma inv (du_j - m_j / M (S1 + xhat_j S2)),  dgamma = S2, dbeta = S1
__global__ __launch_bounds__(WBT) void tr_u_back_kernel(const float *du, int B, int N, int mode, const float *u, int ld_u,
                                                        const float *hsave, const float *xhat, const float *inv,
                                                        const float *gamma, const float *mult, float M, float *dpre,
                                                        int ld_dpre, float *dgamma, float *dbeta, const int *rows_dev) {
    __shared__ float red[WBG][WBC];
    __shared__ float stat[2][WBC];
    if (rows_dev) M = (float)*rows_dev;
    const int c = threadIdx.x % WBC, g = threadIdx.x / WBC, col = blockIdx.x * WBC + c;
    const bool ok = col < N;
    float s1 = 0.f, s2 = 0.f;
    if (mode == 2) {
        if (ok) for (int j = g; j < B; j += WBG) {
            const float d = du[(size_t)j * N + col];
            s1 += d;
            s2 += d * xhat[(size_t)j * N + col];
        }
        for (int which = 0; which < 2; ++which) {
            red[g][c] = which ? s2 : s1;
            __syncthreads();
            if (g == 0) {
                float t = 0.f;
                for (int i = 0; i < WBG; ++i) t += red[i][c];
                stat[which][c] = t;
            }
            __syncthreads();
        }
        s1 = stat[0][c];
        s2 = stat[1][c];
        if (ok && g == 0) { dgamma[col] = s2; dbeta[col] = s1; }
    }
    if (!ok) return;
    for (int j = g; j < B; j += WBG) {
        const float d = du[(size_t)j * N + col];
        float o;
        if (mode == 0) o = d;
        else if (mode == 1) o = u[(size_t)j * ld_u + col] > 0.f ? d : 0.f;
        else {
            const float xh = xhat[(size_t)j * N + col];
            const float dh = gamma[col] * inv[col] * (d - (M > 0.f ? mult[j] / M : 0.f) * (s1 + xh * s2));
            o = hsave[(size_t)j * N + col] > 0.f ? dh : 0.f;
        }
        dpre[(size_t)j * ld_dpre + col] = o;
    }
}

// head columns of dpre_i (pitch ld) from the per-sample context gradient: yu_i, zu_i as they are, gate_i through its ReLU
// (mask from the gate value in the context row); the pad columns [cols, ld) are zero
__global__ void tr_dpre_heads_kernel(const float *dctx, const float *ctx, int B, int C, int col0, int n, int w, int wprev,
                                     int yu_off, int zu_off, int gate_off, float *dpre, int ld) {
    const int span = ld - col0, total = B * span;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int j = i / span, k = i - j * span;
        const float *d = dctx + (size_t)j * C, *cr = ctx + (size_t)j * C;
        float v = 0.f;
        if (k < n) v = d[yu_off + k];
        else if (k < n + w) v = d[zu_off + k - n];
        else if (k < n + w + wprev) v = cr[gate_off + k - n - w] > 0.f ? d[gate_off + k - n - w] : 0.f;
        dpre[(size_t)j * ld + col0 + k] = v;
    }
}

struct TrainShape {
    int L, n, nf, C, B, R, R2, bn;
    int w[ICNN_BE_MAX_LAYERS];
    int yu_off[ICNN_BE_MAX_LAYERS], zu_off[ICNN_BE_MAX_LAYERS], gate_off[ICNN_BE_MAX_LAYERS];
    int K(int i) const { return i == 0 ? nf : w[i - 1]; }                                   // stage input width
    int pq_ld(int i) const { return n + (i > 0 ? w[i - 1] : 0); }
};

// offsets of the variables inside the packed gradient, in the order of include/icnn_be.h (icnn_amd.picnn.init_params)
struct GradLayout {
    size_t uW[ICNN_BE_MAX_LAYERS], ub[ICNN_BE_MAX_LAYERS], gam[ICNN_BE_MAX_LAYERS], bet[ICNN_BE_MAX_LAYERS];
    size_t zuuW[ICNN_BE_MAX_LAYERS], zuub[ICNN_BE_MAX_LAYERS], zproj[ICNN_BE_MAX_LAYERS];
    size_t yuuW[ICNN_BE_MAX_LAYERS], yuub[ICNN_BE_MAX_LAYERS], yuW[ICNN_BE_MAX_LAYERS];
    size_t zW[ICNN_BE_MAX_LAYERS], zb[ICNN_BE_MAX_LAYERS];
    size_t total;
};
GradLayout grad_layout(const TrainShape &s) {
    GradLayout g{};
    size_t at = 0;
    for (int i = 0; i < s.L; ++i) {
        g.uW[i] = at; at += (size_t)s.K(i) * s.w[i];
        g.ub[i] = at; at += s.w[i];
        if (s.bn && i < s.L - 1) {
            g.gam[i] = at; at += s.w[i];
            g.bet[i] = at; at += s.w[i];
        }
    }
    for (int i = 0; i <= s.L; ++i) {
        if (i > 0) {
            g.zuuW[i] = at; at += (size_t)s.K(i) * s.w[i - 1];
            g.zuub[i] = at; at += s.w[i - 1];
            g.zproj[i] = at; at += (size_t)s.w[i - 1] * s.w[i];
        }
        g.yuuW[i] = at; at += (size_t)s.K(i) * s.n;
        g.yuub[i] = at; at += s.n;
        g.yuW[i] = at; at += (size_t)s.n * s.w[i];
        g.zW[i] = at; at += (size_t)s.K(i) * s.w[i];
        g.zb[i] = at; at += s.w[i];
    }
    g.total = at;
    return g;
}

int make_shape(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c, int batch, int rows, bool with_v, TrainShape &s) {
    if (int rc = fc_check_model(m)) return rc;
    if (c.n != m.n || c.n_layers != m.n_layers || c.n_features < 1) return ICNN_BE_EINVAL;
    s = TrainShape{};
    s.L = m.n_layers - 1;
    s.n = m.n;
    s.nf = c.n_features;
    s.bn = c.batchnorm ? 1 : 0;
    int o = 0;
    for (int i = 0; i <= s.L; ++i) {
        if (c.width[i] != m.width[i]) return ICNN_BE_EINVAL;
        s.w[i] = m.width[i];
        s.yu_off[i] = o; o += m.n;
        s.zu_off[i] = o; o += m.width[i];
        s.gate_off[i] = i > 0 ? o : -1;
        if (i > 0) o += m.width[i - 1];
    }
    s.C = o;
    if (batch < 1 || rows < 1) return ICNN_BE_EINVAL;
    // every index of the row kernels is an int: R2 x ctx_width (which covers n + 2 widths), B x the widest stage row
    int widest = o;
    for (int i = 0; i <= s.L; ++i) {
        const int cols = ctx_stage_cols(c, i);
        if (cols + 4 > widest) widest = cols + 4;
    }
    const size_t r2 = (with_v ? 2 : 1) * (size_t)rows;
    if (r2 * (size_t)o > INT_MAX || (size_t)batch * widest > INT_MAX || (size_t)c.n_features * widest > INT_MAX)
        return ICNN_BE_ELIMIT;
    s.B = batch;
    s.R = rows;
    s.R2 = with_v ? 2 * rows : rows;
    return 0;
}

// The whole step; with work == nullptr only sizes the workspace (returned through *work_floats)
hipError_t surrogate_run(const icnn_be_fc_model &m, const icnn_be_fc_ctx &cx, const TrainShape &s, const float *x, const int *row_offset,
                  const double *y, const double *v, const double *cvec, float *grad, float *F_rows, float *work,
                  size_t *work_floats, hipStream_t stream, const icnn_be_bn_moving *mv = nullptr, int updates = 0,
                  const int *rows_dev = nullptr, bool dev_sizes = false) {
    const int L = s.L, B = s.B, R = s.R, R2 = s.R2, n = s.n, C = s.C;
    Carver cv{work};
    int *samp = reinterpret_cast<int *>(cv.take(R));
    float *mult = cv.take(B);
    float *uwork = cv.take(ctx_work_floats(cx, B));
    float *ctxb = cv.take((size_t)B * C);
    float *hsave[ICNN_BE_MAX_LAYERS] = {}, *xhat[ICNN_BE_MAX_LAYERS] = {}, *inv[ICNN_BE_MAX_LAYERS] = {};
    float *stat[ICNN_BE_MAX_LAYERS] = {};       // the weighted statistics, for the moving ones
    int bn_n[ICNN_BE_MAX_LAYERS];
    fc_bn_widths(cx, bn_n);
    for (int i = 0; i + 1 < L; ++i)
        if (bn_n[i]) {
            hsave[i] = cv.take((size_t)B * bn_n[i]);
            xhat[i] = cv.take((size_t)B * bn_n[i]);
            inv[i] = cv.take(bn_n[i]);
            stat[i] = cv.take(2 * (size_t)bn_n[i]);
        }
    float *wst[ICNN_BE_MAX_LAYERS], *pq[ICNN_BE_MAX_LAYERS], *adj[ICNN_BE_MAX_LAYERS], *Z[ICNN_BE_MAX_LAYERS] = {},
          *D[ICNN_BE_MAX_LAYERS] = {}, *dpre[ICNN_BE_MAX_LAYERS];
    int max_pq = 0, max_k = 0;
    for (int i = 0; i <= L; ++i) {
        wst[i] = cv.take((size_t)s.pq_ld(i) * s.w[i]);
        pq[i] = cv.take((size_t)R2 * s.pq_ld(i));
        adj[i] = cv.take((size_t)R2 * s.w[i]);
        if (i < L) {
            Z[i] = cv.take((size_t)R2 * s.w[i]);
            D[i] = cv.take((size_t)R * s.w[i]);
        }
        dpre[i] = cv.take((size_t)B * ctx_stage_ld(cx, i));
        if (s.pq_ld(i) > max_pq) max_pq = s.pq_ld(i);
        if (s.K(i) > max_k) max_k = s.K(i);
    }
    int max_w = 1;
    for (int i = 0; i <= L; ++i) max_w = s.w[i] > max_w ? s.w[i] : max_w;
    float *pre = cv.take((size_t)R2 * max_w);
    float *bd = cv.take((size_t)R2 * max_pq);
    float *drows = cv.take((size_t)R * C);
    float *dctx = cv.take((size_t)B * C);
    float *du = cv.take((size_t)B * max_k);
    const size_t fixed = cv.at;
    // u_i (i < L) as the context producer leaves it in uwork: the input of stage i + 1, after its BatchNorm
    float *u[ICNN_BE_MAX_LAYERS] = {};
    int u_ld[ICNN_BE_MAX_LAYERS] = {};
    for (int i = 0; i < L; ++i) u[i] = uwork ? fc_ctx_u(cx, B, uwork, i, &u_ld[i]) : nullptr;

    // the partials go last: their size is what the products below ask for (measured by the dry run)
    Runner run{stream, work ? work + fixed : nullptr};
    const PackOffsets po = pack_offsets(m);
    const GradLayout gl = grad_layout(s);
    RowArgs ra{y, v, cvec, samp, ctxb, R, n, C, m.action_box ? 1 : 0, rows_dev};

    // 1. rows and multiplicities, y-path weights
    run.call([&] { return launch_tr_rows(row_offset, B, R, samp, mult, stream); });
    for (int i = 0; i <= L; ++i)        // Wst_i [(n + w_{i-1})][w_i] = [ Wyu_i ; Wzu_i ]
        run.call([&] {
            return launch_tr_unpack(m.wpack, po.yu_f[i], po.zu_f[i], n, i > 0 ? s.w[i - 1] : 0, s.w[i], i == L, wst[i], stream);
        });
    // 2. x-only forward on the B samples (context producer's stage GEMMs), weighted BatchNorm
    for (int i = 0; i <= L; ++i) {
        run.call([&] { return launch_fc_context_stage(cx, i, x, B, ctxb, C, uwork, stream); });
        if (bn_n[i])
            run.launch(tr_wbn_fwd_kernel, (s.w[i] + WBC - 1) / WBC, WBT, u[i], u_ld[i], B, s.w[i], (const float *)mult, (float)R,
                       cx.bn_gamma[i], cx.bn_beta[i], cx.bn_eps, hsave[i], xhat[i], inv[i], updates > 0 ? stat[i] : nullptr, rows_dev);
    }
    if (s.bn && updates > 0) run.call([&] { return launch_bn_fold(*mv, stat, bn_n, L - 1, updates, stream, nullptr, rows_dev); });
    // 3. y-path forward: primal and tangent rows stacked, one GEMM per layer
    for (int i = 0; i <= L; ++i) {
        const int ld = s.pq_ld(i), w = s.w[i];
        run.launch(tr_build_p_kernel, grid_for((size_t)R * n), 256, ra, s.yu_off[i], pq[i], ld);
        run.gemm(pq[i], ld, 1, wst[i], w, 1, R2, w, ld, pre, w, rows_dev, R2 / R, dev_sizes);
        if (i < L)
            run.launch(tr_hidden_fwd_kernel, grid_for((size_t)R * w), 256, ra, (const float *)pre, w, s.zu_off[i],
                       s.gate_off[i + 1], m.alpha, Z[i], D[i], pq[i + 1], s.pq_ld(i + 1));
        else
            run.launch(tr_final_kernel, grid_for(R), 256, ra, (const float *)pre, s.zu_off[i], F_rows, adj[L]);
    }
    // 4. y-path reverse: weight gradients (K = 2R) and the per-row context gradient
    for (int i = L; i >= 0; --i) {
        const int ld = s.pq_ld(i), w = s.w[i], wp = i > 0 ? s.w[i - 1] : 0;
        run.gemm(pq[i], 1, ld, adj[i], w, 1, n, w, R2, grad + gl.yuW[i], w);                     // (y*yu)^T abar
        if (i > 0) run.gemm(pq[i] + n, 1, ld, adj[i], w, 1, wp, w, R2, grad + gl.zproj[i], w);  // (z*gate)^T abar
        run.gemm(adj[i], w, 1, wst[i], 1, w, R2, ld, w, bd, ld);                                 // abar [Wyu ; Wzu]^T
        BackArgs ba{bd, adj[i], i > 0 ? Z[i - 1] : nullptr, i > 0 ? D[i - 1] : nullptr, i > 0 ? adj[i - 1] : nullptr, drows,
                    w, wp, s.yu_off[i], s.zu_off[i], s.gate_off[i]};
        run.launch(tr_back_rows_kernel, grid_for((size_t)R * (ld + w)), 256, ra, ba);
    }
    // 5. per-sample context gradient
    run.call([&] { return launch_tr_segment_sum(drows, row_offset, B, R, C, dctx, stream); });
    // 6. x-only backward on the B samples
    for (int i = L; i >= 0; --i) {
        const int K = s.K(i), ld = ctx_stage_ld(cx, i), wp = i > 0 ? s.w[i - 1] : 0, ucols = i < L ? s.w[i] : 0;
        run.launch(tr_dpre_heads_kernel, grid_for((size_t)B * (ld - ucols)), 256, (const float *)dctx, (const float *)ctxb, B, C,
                   ucols, n, s.w[i], wp, s.yu_off[i], s.zu_off[i], s.gate_off[i], dpre[i], ld);
        if (i < L) {        // u_i columns from du = dprev_{i+1} (computed in the previous iteration)
            const int mode = i == L - 1 ? (cx.u_last_relu ? 1 : 0) : (s.bn ? 2 : 1);
            run.launch(tr_u_back_kernel, (s.w[i] + WBC - 1) / WBC, WBT, (const float *)du, B, s.w[i], mode, u[i], u_ld[i],
                       (const float *)hsave[i], (const float *)xhat[i], (const float *)inv[i], cx.bn_gamma[i],
                       (const float *)mult, (float)R, dpre[i], ld, mode == 2 ? grad + gl.gam[i] : nullptr,
                       mode == 2 ? grad + gl.bet[i] : nullptr, rows_dev);
        }
        // stage input: x, or u_{i-1} as the next stage read it (after its BatchNorm)
        const float *prev = i > 0 ? u[i - 1] : x;
        const int prev_ld = i > 0 ? u_ld[i - 1] : s.nf;
        // column segments of the stage: [ u_i | yu_u | u | zu_u ] -> their gradient variables
        struct Seg { int c0, cols; size_t wo, bo; } segs[4];
        int ns = 0, c0 = 0;
        if (i < L) { segs[ns++] = Seg{c0, s.w[i], gl.uW[i], gl.ub[i]}; c0 += s.w[i]; }
        segs[ns++] = Seg{c0, n, gl.yuuW[i], gl.yuub[i]}; c0 += n;
        segs[ns++] = Seg{c0, s.w[i], gl.zW[i], gl.zb[i]}; c0 += s.w[i];
        if (i > 0) { segs[ns++] = Seg{c0, wp, gl.zuuW[i], gl.zuub[i]}; c0 += wp; }
        for (int q = 0; q < ns; ++q) {
            run.gemm(prev, 1, prev_ld, dpre[i] + segs[q].c0, ld, 1, K, segs[q].cols, B, grad + segs[q].wo, segs[q].cols);
            run.call([&] { return launch_tr_colsum(dpre[i], ld, B, segs[q].c0, segs[q].cols, grad + segs[q].bo, stream); });
        }
        if (i > 0)          // du_{i-1} = dpre_i W_stage_i^T  [B][w_{i-1}]
            run.gemm(dpre[i], ld, 1, cx.w_stage[i], 1, ld, B, K, ctx_stage_cols(cx, i), du, K);
    }
    if (work_floats) *work_floats = fixed + run.part_need;
    return run.err;
}

}  // namespace

size_t fc_grad_floats(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c) {
    TrainShape s;
    if (make_shape(m, c, 1, 1, true, s) != 0) return 0;
    return grad_layout(s).total;
}

size_t fc_surrogate_work_floats(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c, int batch, int rows, bool dev) {
    // with and without v (2R or R stacked rows): the split-K partials need not grow with the row count, so take the larger
    size_t most = 0;
    for (int with_v = 0; with_v < 2; ++with_v) {
        TrainShape s;
        if (make_shape(m, c, batch, rows, with_v != 0, s) != 0) return 0;
        size_t need = 0;
        (void)surrogate_run(m, c, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &need, nullptr,
                            nullptr, 0, nullptr, dev);
        if (need > most) most = need;
    }
    return most;
}

int fc_surrogate_shape(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c, int batch, int rows, bool with_v) {
    TrainShape s;
    return make_shape(m, c, batch, rows, with_v, s);
}

hipError_t launch_fc_surrogate_grad(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c, const float *x, int batch,
                                    const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                    float *grad, float *F_rows, float *work, hipStream_t stream, const icnn_be_bn_moving *mv,
                                    int updates, const int *rows_dev) {
    TrainShape s;
    if (make_shape(m, c, batch, rows, v != nullptr, s) != 0) return hipErrorInvalidValue;
    return surrogate_run(m, c, s, x, row_offset, y, v, cvec, grad, F_rows, work, nullptr, stream, mv, updates, rows_dev);
}

}  // namespace icnn_be
