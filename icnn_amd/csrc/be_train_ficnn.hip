// Training gradient of the FICNN (synthetic-cls/icnn.py:133-139): the parameter gradient of
//   F = sum_r c_r E(x_s(r), y_r) + <dE/dy(x_s(r), y_r), v_r>
// over every variable, in the structure of be_train_fc.hip:
//   1. the context c_i = x Wx_i + b_i on the B unique samples (launch_ficnn_context, be_ficnn.hip)
//   2. rows forward, layer by layer: primal and tangent rows stacked into one operand P_i = [ y | z_{i-1} ; v | zdot_{i-1} ]
//      ([2R][n + width_{i-1}]), one GEMM with [Wy_i ; Wz_i] gives both pre-activations; z = relu(a), zdot = relu'(a) pre_dot
//   3. rows reverse: the two adjoint columns (abar seeded with c_r, adot with 1, through the head) run through the same
//      masks; per layer P_i^T adj_i gives the y rows of 'z_x{i}/W' and 'z_z{i}_proj/W' (K = 2R), adj_i Wz_i^T the next
//      adjoints
//   4. the context gradient abar_i of each sample summed over its rows in row order, then x^T dctx_i and the bias sums on
//      the B samples.
// Every product runs through launch_tr_gemm (split-K partials summed in a fixed order); no atomics anywhere: the same bits
// on every call, and the whole entry is capturable.  Head SUM: the head layer's variables get an exact 0.
#include <hip/hip_runtime.h>

#include "be_ficnn_dev.h"
#include "be_train_common.h"

namespace icnn_be {

namespace {

struct FRowArgs {
    const double *y, *v, *c;
    const int *samp;
    const float *ctx;
    int R, n, C;
};

// P_i[:, 0:n) = [ y ; v ] (pitch ld): y rounded to float32 like a feed
__global__ void fi_build_p_kernel(FRowArgs a, float *pq, int ld) {
    const int total = a.R * a.n;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / a.n, j = i - r * a.n;
        pq[(size_t)r * ld + j] = (float)a.y[i];
        if (a.v) pq[(size_t)(a.R + r) * ld + j] = (float)a.v[i];
    }
}

// hidden layer i: a = pre + c_i, z = relu(a), D = relu'(a), zdot = D pre_dot; P_{i+1}[:, n + k] = [ z ; zdot ] (pq_next may
// be NULL: the top hidden layer of head SUM, whose z feeds the energy only) and into Zt [2R][w] (pitch w) for the head
__global__ void fi_hidden_fwd_kernel(FRowArgs a, const float *pre, int w, int c_off, float *D, float *Zt, float *pq_next,
                                     int ld_next) {
    const int total = a.R * w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / w, k = i - r * w;
        const float p = pre[i] + a.ctx[(size_t)a.samp[r] * a.C + c_off + k];
        const float d = p > 0.f ? 1.f : 0.f;
        const float z = p > 0.f ? p : 0.f;
        D[i] = d;
        if (pq_next) pq_next[(size_t)r * ld_next + a.n + k] = z;
        if (Zt) Zt[i] = z;
        if (a.v) {
            const float zd = d * pre[(size_t)a.R * w + i];
            if (pq_next) pq_next[(size_t)(a.R + r) * ld_next + a.n + k] = zd;
            if (Zt) Zt[(size_t)a.R * w + i] = zd;
        }
    }
}

// head SUM: E = sum_k z_k, F = c E + sum_k zdot_k; seeds adj_{L-1} = [ D c ; D ]
__global__ void fi_head_sum_kernel(FRowArgs a, const float *Zt, const float *D, int w, float *F, float *adj) {
    const int total = a.R * w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / w;
        const float c = (float)a.c[r];
        adj[i] = D[i] * c;
        if (a.v) adj[(size_t)a.R * w + i] = D[i];
    }
    if (!F) return;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += gridDim.x * blockDim.x) {
        float e = 0.f, ed = 0.f;
        for (int k = 0; k < w; ++k) e += Zt[(size_t)r * w + k];
        if (a.v)
            for (int k = 0; k < w; ++k) ed += Zt[(size_t)(a.R + r) * w + k];
        F[r] = (float)a.c[r] * e + ed;
    }
}

// head LINEAR: E = pre + c_L, F = c E + pre_dot; seeds adj_L = [ c ; 1 ]
__global__ void fi_head_linear_kernel(FRowArgs a, const float *pre, int c_off, float *F, float *adj) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += gridDim.x * blockDim.x) {
        const float c = (float)a.c[r];
        if (F) {
            const float e = pre[r] + a.ctx[(size_t)a.samp[r] * a.C + c_off];
            F[r] = c * e + (a.v ? pre[a.R + r] : 0.f);
        }
        adj[r] = c;
        if (a.v) adj[a.R + r] = 1.f;
    }
}

// adj_prev [R2][wp] = D_prev (per primal row, the same mask for the tangent row) * BD
__global__ void fi_back_mask_kernel(const float *BD, const float *Dp, int R, int R2, int wp, float *adj_prev) {
    const int total = R2 * wp;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int row = i / wp, k = i - row * wp;
        const int r = row < R ? row : row - R;
        adj_prev[i] = Dp[(size_t)r * wp + k] * BD[i];
    }
}

struct FShape {
    int L, evald, n, nf, C, B, R, R2, head;
    int w[ICNN_BE_MAX_LAYERS], c_off[ICNN_BE_MAX_LAYERS];
    int pq_ld(int i) const { return n + (i > 0 ? w[i - 1] : 0); }
};

// offsets of the variables in the packed gradient (include/icnn_be.h, icnn_be_ficnn_grad_floats)
struct FGradLayout {
    size_t xW[ICNN_BE_MAX_LAYERS], xb[ICNN_BE_MAX_LAYERS], proj[ICNN_BE_MAX_LAYERS];
    size_t total;
};
FGradLayout f_grad_layout(const FShape &s) {
    FGradLayout g{};
    size_t at = 0;
    for (int i = 0; i <= s.L; ++i) {
        g.xW[i] = at; at += (size_t)(s.nf + s.n) * s.w[i];
        g.xb[i] = at; at += s.w[i];
        if (i > 0) { g.proj[i] = at; at += (size_t)s.w[i - 1] * s.w[i]; }
    }
    g.total = at;
    return g;
}

int f_make_shape(const icnn_be_ficnn_model &m, int batch, int rows, bool with_v, FShape &s) {
    if (int rc = ficnn_check(m)) return rc;
    const FicnnPack po = ficnn_pack_offsets(m);
    s = FShape{};
    s.L = po.L;
    s.evald = po.evald;
    s.n = m.n;
    s.nf = m.n_features;
    s.C = po.ctx_width;
    s.head = m.head;
    for (int i = 0; i <= s.L; ++i) {
        s.w[i] = m.width[i];
        s.c_off[i] = i < po.evald ? po.c_off[i] : -1;
    }
    if (batch < 1 || rows < 1) return ICNN_BE_EINVAL;
    int widest = s.C;
    for (int i = 0; i <= s.L; ++i)
        if (s.pq_ld(i) > widest) widest = s.pq_ld(i);
    const size_t r2 = (with_v ? 2 : 1) * (size_t)rows;
    if (r2 * (size_t)widest > INT_MAX || (size_t)batch * widest > INT_MAX) return ICNN_BE_ELIMIT;
    s.B = batch;
    s.R = rows;
    s.R2 = (int)r2;
    return 0;
}

// The whole step; with work == nullptr only sizes the workspace (returned through *work_floats)
hipError_t f_surrogate_run(const icnn_be_ficnn_model &m, const FShape &s, const float *x, const int *row_offset, const double *y,
                           const double *v, const double *cvec, float *grad, float *F_rows, float *work, size_t *work_floats,
                           hipStream_t stream) {
    const int L = s.L, E = s.evald, B = s.B, R = s.R, R2 = s.R2, n = s.n, C = s.C, nf = s.nf;
    const bool linear = s.head == ICNN_BE_FICNN_HEAD_LINEAR;
    Carver cv{work};
    int *samp = reinterpret_cast<int *>(cv.take(R));
    float *mult = cv.take(B);
    float *ctxb = cv.take((size_t)B * C);
    float *wst[ICNN_BE_MAX_LAYERS], *pq[ICNN_BE_MAX_LAYERS], *adj[ICNN_BE_MAX_LAYERS], *D[ICNN_BE_MAX_LAYERS] = {};
    int max_w = 1;
    for (int i = 0; i < E; ++i) {
        wst[i] = cv.take((size_t)s.pq_ld(i) * s.w[i]);
        pq[i] = cv.take((size_t)R2 * s.pq_ld(i));
        adj[i] = cv.take((size_t)R2 * s.w[i]);
        if (i < L) D[i] = cv.take((size_t)R * s.w[i]);
        if (s.w[i] > max_w) max_w = s.w[i];
    }
    float *zt = linear ? nullptr : cv.take((size_t)R2 * s.w[L - 1]);
    float *pre = cv.take((size_t)R2 * max_w);
    float *bd = cv.take((size_t)R2 * max_w);
    float *dctx = cv.take((size_t)B * max_w);
    const size_t fixed = cv.at;

    Runner run{stream, work ? work + fixed : nullptr};
    const FicnnPack po = ficnn_pack_offsets(m);
    const FGradLayout gl = f_grad_layout(s);
    FRowArgs ra{y, v, cvec, samp, ctxb, R, n, C};

    // 0. variables that do not reach E (head SUM)
    if (!linear) run.call([&] { return launch_tr_zero(grad + gl.xW[L], gl.total - gl.xW[L], stream); });
    // 1. rows, weights, context of the B samples
    run.call([&] { return launch_tr_rows(row_offset, B, R, samp, mult, stream); });
    for (int i = 0; i < E; ++i)         // wst_i [(n + w_{i-1})][w_i] = [ Wy_i ; Wz_i ]
        run.call([&] {
            return launch_tr_unpack(m.wpack, i < L ? po.yf[i] : po.yL, i < L ? po.zf[i] : po.zL, n, i > 0 ? s.w[i - 1] : 0, s.w[i],
                                    i == L, wst[i], stream);
        });
    run.need(ficnn_context_work_floats(m, B));
    run.call([&] { return launch_ficnn_context(m, x, B, ctxb, run.part, stream); });
    // 2. rows forward
    for (int i = 0; i < E; ++i) {
        const int ld = s.pq_ld(i), w = s.w[i];
        run.launch(fi_build_p_kernel, grid_for((size_t)R * n), 256, ra, pq[i], ld);
        run.gemm(pq[i], ld, 1, wst[i], w, 1, R2, w, ld, pre, w);
        if (i < L) {
            const bool top = i == L - 1;
            float *next = top && !linear ? nullptr : pq[i + 1];
            run.launch(fi_hidden_fwd_kernel, grid_for((size_t)R * w), 256, ra, (const float *)pre, w, s.c_off[i], D[i],
                       top && !linear ? zt : nullptr, next, next ? s.pq_ld(i + 1) : 0);
            if (top && !linear)
                run.launch(fi_head_sum_kernel, grid_for((size_t)R * w), 256, ra, (const float *)zt, (const float *)D[i], w, F_rows,
                           adj[i]);
        } else {
            run.launch(fi_head_linear_kernel, grid_for(R), 256, ra, (const float *)pre, s.c_off[i], F_rows, adj[i]);
        }
    }
    // 3. rows reverse: weight gradients (K = 2R), adjoints, and 4. the context gradient of each layer
    for (int i = E - 1; i >= 0; --i) {
        const int ld = s.pq_ld(i), w = s.w[i], wp = i > 0 ? s.w[i - 1] : 0;
        run.gemm(pq[i], 1, ld, adj[i], w, 1, n, w, R2, grad + gl.xW[i] + (size_t)nf * w, w);          // [y ; v]^T adj
        if (i > 0) {
            run.gemm(pq[i] + n, 1, ld, adj[i], w, 1, wp, w, R2, grad + gl.proj[i], w);                 // [z ; zdot]^T adj
            run.gemm(adj[i], w, 1, wst[i] + (size_t)n * w, 1, w, R2, wp, w, bd, wp);                 // adj Wz^T
            run.launch(fi_back_mask_kernel, grid_for((size_t)R2 * wp), 256, (const float *)bd, (const float *)D[i - 1], R, R2,
                       wp, adj[i - 1]);
        }
        run.call([&] { return launch_tr_segment_sum(adj[i], row_offset, B, R, w, dctx, stream); });  // primal rows only
        run.gemm(x, 1, nf, dctx, w, 1, nf, w, B, grad + gl.xW[i], w);                                // x^T dctx
        run.call([&] { return launch_tr_colsum(dctx, w, B, 0, w, grad + gl.xb[i], stream); });
    }
    if (work_floats) *work_floats = fixed + run.part_need;
    return run.err;
}

}  // namespace

size_t ficnn_grad_floats(const icnn_be_ficnn_model &m) {
    FShape s;
    if (f_make_shape(m, 1, 1, true, s) != 0) return 0;
    return f_grad_layout(s).total;
}

size_t ficnn_surrogate_work_floats(const icnn_be_ficnn_model &m, int batch, int rows) {
    size_t most = 0;
    for (int with_v = 0; with_v < 2; ++with_v) {
        FShape s;
        if (f_make_shape(m, batch, rows, with_v != 0, s) != 0) return 0;
        size_t need = 0;
        (void)f_surrogate_run(m, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &need, nullptr);
        if (need > most) most = need;
    }
    return most;
}

int ficnn_surrogate_shape(const icnn_be_ficnn_model &m, int batch, int rows, bool with_v) {
    FShape s;
    return f_make_shape(m, batch, rows, with_v, s);
}

hipError_t launch_ficnn_surrogate_grad(const icnn_be_ficnn_model &m, const float *x, int batch, const int *row_offset, int rows,
                                       const double *y, const double *v, const double *cvec, float *grad, float *F_rows,
                                       float *work, hipStream_t stream) {
    FShape s;
    if (f_make_shape(m, batch, rows, v != nullptr, s) != 0) return hipErrorInvalidValue;
    return f_surrogate_run(m, s, x, row_offset, y, v, cvec, grad, F_rows, work, nullptr, stream);
}

}  // namespace icnn_be
