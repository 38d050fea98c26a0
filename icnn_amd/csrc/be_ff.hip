// The feed-forward baseline of the multi-label experiment on the device (multi-label-cls/ff.py; include/icnn_be.h,
// icnn_be_ff_*): a ReLU / BatchNorm MLP with a sigmoid head, trained with TF-Adam on the summed cross entropy.
//
// BatchNorm crosses the samples at every hidden layer, so a workgroup cannot own a tile of samples through the whole net as
// in be_ddpg.hip.  Every cross-sample quantity of the step is a COLUMN statistic (mu, sigma^2 forward; S1, S2 backward), so
// here a workgroup owns FC columns of a layer's output for ALL rows of the batch and needs no other workgroup; every
// dependency between workgroups is a launch boundary.
//
//   ff_layer_fwd_kernel   a_i = relu(h_{i-1} W_i + b_i) for the workgroup's columns, the two-pass batch mean and variance of
//                         each column in LDS, h_i; stores a_i, h_i and (mu, sigma^2).  In moving mode it normalises with the
//                         moving pair instead and the grid runs over groups of rows too.
//   ff_head_kernel        the same product for the logits: yhat, and with targets the loss partial of the workgroup
//                         (float64), the F1 tallies (integer atomics) and d loss / d logits.  The last workgroup to finish
//                         (a ticket, nobody waits) adds the partials in index order and writes the loss.
//   ff_layer_bwd_kernel   du = delta_{i+1} W_{i+1}^T for the workgroup's columns, S1 and S2 over the batch in LDS, da, the
//                         ReLU mask from the stored a_i, dz_i; d gamma_i and d beta_i go straight into the flat gradient.
//   the weight gradients  grad_table_kernel (be_train_table.hip) over a table of the L + 1 products.
//   the update            param_sets_update_kernel (be_train_table.hip) over one parameter set without a target.
//   the fold              bn_fold_kernel (be_context.hip).
//
// The product (col_gemm), the column sums and the accumulator walk are be_col_gemm.h.
#include "be_api_check.h"
#include "be_kernels.h"
#include "be_train_common.h"
#include "be_col_gemm.h"
#include "be_train_table.h"

namespace icnn_be {

namespace {

constexpr int FROWS_MOVING = 128;        // rows per workgroup in moving mode: one tile per wave

struct FfFwdArgs {
    const float *X;                      // [B][K]
    int B, K, N, rows_per, moving, kl;
    const float *W, *b, *gamma, *beta;   // W [K][N]
    const float *mean, *var;             // the moving pair (moving mode)
    float *a, *h, *stat;                 // [B][N], [B][N], mu [N] then sigma^2 [N] (batch mode)
    float eps;
    int *zero;                           // not NULL: the first layer clears the F1 tallies of its rows, [B][3]
};

__global__ __launch_bounds__(FT) void ff_layer_fwd_kernel(FfFwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int row0 = blockIdx.y * p.rows_per, nrows = p.B - row0 < p.rows_per ? p.B - row0 : p.rows_per;
    float *xs = lds, *ws = xs + ff_stage_floats(nrows, p.kl), *smean = ws + ff_weight_floats(p.kl), *svar = smean + FC;
    const int tid = threadIdx.x, r16 = tid & 15, c0 = blockIdx.x * FC, col = c0 + r16;
    const bool vc = col < p.N;
    if (p.zero && blockIdx.x == 0)
        for (int i = tid; i < 3 * nrows; i += FT) p.zero[(size_t)row0 * 3 + i] = 0;
    Frag acc;
    col_gemm(p.X, p.K, row0, nrows, p.K, p.W, p.N, 1, c0, p.N, p.kl, xs, ws, acc);
    const float bias = vc ? p.b[col] : 0.f;
    const int pitch = pad16(nrows) + 4;
    for_rows(nrows, [&](int i, int r, int row) {
        const float v = acc.t[i][r] + bias;
        acc.t[i][r] = v > 0.f ? v : 0.f;
    });
    if (!p.moving) {
        // two passes over the column in LDS: the mean, then the mean of the squared deviations
        for_rows(nrows, [&](int i, int r, int row) { xs[r16 * pitch + row] = acc.t[i][r]; });
        __syncthreads();
        const int c = tid >> 5, l = tid & 31;
        const float mean = column_sum(xs, pitch, nrows) / (float)p.B;
        __syncthreads();
        for (int r = l; r < nrows; r += 32) {
            const float d = xs[c * pitch + r] - mean;
            xs[c * pitch + r] = d * d;
        }
        __syncthreads();
        const float var = column_sum(xs, pitch, nrows) / (float)p.B;
        if (l == 0) {
            smean[c] = mean;
            svar[c] = var;
            if (c0 + c < p.N) {
                p.stat[c0 + c] = mean;
                p.stat[p.N + c0 + c] = var;
            }
        }
        __syncthreads();
    }
    const float mean = p.moving ? (vc ? p.mean[col] : 0.f) : smean[r16], var = p.moving ? (vc ? p.var[col] : 1.f) : svar[r16];
    const float inv = 1.f / sqrtf(var + p.eps), ga = vc ? p.gamma[col] : 0.f, be = vc ? p.beta[col] : 0.f;
    if (vc)
        for_rows(nrows, [&](int i, int r, int row) {
            const size_t at = (size_t)(row0 + row) * p.N + col;
            const float a = acc.t[i][r];
            p.a[at] = a;
            p.h[at] = (a - mean) * inv * ga + be;
        });
}

struct FfHeadArgs {
    const float *X;                      // h_L [B][K]
    int B, K, N, rows_per, kl;
    const float *W, *b;
    const float *y;                      // targets [B][N]; NULL: yhat alone
    float *yhat, *dlogit;                // dlogit NULL: none
    int *tallies;                        // [B][3], zeroed by the first layer's launch; NULL: none
    double *partial;                     // one per workgroup
    int *ticket;
    float *loss;
};

__global__ __launch_bounds__(FT) void ff_head_kernel(FfHeadArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[FT];
    const int row0 = blockIdx.y * p.rows_per, nrows = p.B - row0 < p.rows_per ? p.B - row0 : p.rows_per;
    float *xs = lds, *ws = xs + ff_stage_floats(nrows, p.kl);
    const int tid = threadIdx.x, r16 = tid & 15, c0 = blockIdx.x * FC, col = c0 + r16;
    const bool vc = col < p.N;
    Frag acc;
    col_gemm(p.X, p.K, row0, nrows, p.K, p.W, p.N, 1, c0, p.N, p.kl, xs, ws, acc);
    const float bias = vc ? p.b[col] : 0.f;
    double sum = 0.0;
    for_rows(nrows, [&](int i, int r, int row) {
        const size_t at = (size_t)(row0 + row) * p.N + col;
        const float yh = 1.f / (1.f + expf(-(acc.t[i][r] + bias)));
        int counts = 0;                  // tp | fp << 8 | fn << 16 of this element
        if (vc) {
            p.yhat[at] = yh;
            if (p.y) {
                const float y = p.y[at], om = 1.f - yh;
                sum = sum + (double)(-y * logf(yh + 1e-10f) - (1.f - y) * logf(om + 1e-10f));
                if (p.dlogit) {
                    const float dy = -y / (yh + 1e-10f) + (1.f - y) / (om + 1e-10f);
                    p.dlogit[at] = dy * yh * om;
                }
                const bool pred = yh >= 0.5f, truth = (int)y != 0;
                counts = pred && truth ? 1 : pred ? 1 << 8 : truth ? 1 << 16 : 0;
            }
        }
        if (p.y && p.tallies) {
            // the 16 lanes of a row add their columns; integer sums, so the order does not matter
            for (int off = 8; off > 0; off >>= 1) counts += __shfl_xor(counts, off, 16);
            if (r16 == 0 && counts) {
                int *t = p.tallies + (size_t)(row0 + row) * 3;
                if (counts & 255) atomicAdd(t, counts & 255);
                if ((counts >> 8) & 255) atomicAdd(t + 1, (counts >> 8) & 255);
                if (counts >> 16) atomicAdd(t + 2, counts >> 16);
            }
        }
    });
    if (!p.y) return;
    sum = block_tree_sum<FT>(sum, red);
    if (tid == 0) {
        const int blocks = (int)(gridDim.x * gridDim.y), me = (int)(blockIdx.y * gridDim.x + blockIdx.x);
        __hip_atomic_store(p.partial + me, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int ticket = __hip_atomic_fetch_add(p.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == blocks - 1) {
            // the last workgroup: the partials in index order, rounded to float32 once; the ticket re-armed
            double tot = 0.0;
            for (int b = 0; b < blocks; ++b) tot = tot + __hip_atomic_load(p.partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *p.loss = (float)tot;
            __hip_atomic_store(p.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

struct FfBwdArgs {
    const float *D;                      // delta of the layer above [B][K]
    int B, K, N, kl;                     // K its width, N this layer's
    const float *W;                      // the layer above's weights [N][K]
    const float *a, *stat, *gamma;       // this layer's a [B][N], (mu, sigma^2), gamma
    float *dz, *dgamma, *dbeta;          // [B][N]; [N] each, inside the flat gradient
    float eps;
};

__global__ __launch_bounds__(FT) void ff_layer_bwd_kernel(FfBwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nrows = p.B, pitch = pad16(nrows) + 4;
    float *xs = lds, *ws = xs + ff_stage_floats(nrows, p.kl), *s1s = ws + ff_weight_floats(p.kl), *s2s = s1s + FC;
    float *b1 = xs, *b2 = xs + FC * pitch;
    const int tid = threadIdx.x, r16 = tid & 15, c0 = blockIdx.x * FC, col = c0 + r16;
    const bool vc = col < p.N;
    Frag du;
    col_gemm(p.D, p.K, 0, nrows, p.K, p.W, 1, p.K, c0, p.N, p.kl, xs, ws, du);
    const float mean = vc ? p.stat[col] : 0.f, var = vc ? p.stat[p.N + col] : 1.f, inv = 1.f / sqrtf(var + p.eps);
    Frag xh, av;
    for_rows(nrows, [&](int i, int r, int row) {
        const float a = vc ? p.a[(size_t)row * p.N + col] : 0.f;
        av.t[i][r] = a;
        xh.t[i][r] = (a - mean) * inv;
        b1[r16 * pitch + row] = du.t[i][r];
        b2[r16 * pitch + row] = du.t[i][r] * xh.t[i][r];
    });
    __syncthreads();
    const int c = tid >> 5, l = tid & 31;
    const float S1 = column_sum(b1, pitch, nrows), S2 = column_sum(b2, pitch, nrows);
    if (l == 0) {
        s1s[c] = S1;
        s2s[c] = S2;
        if (c0 + c < p.N) {
            p.dbeta[c0 + c] = S1;
            p.dgamma[c0 + c] = S2;
        }
    }
    __syncthreads();
    if (!vc) return;
    const float s1 = s1s[r16], s2 = s2s[r16], scale = p.gamma[col] * inv, fb = (float)p.B;
    for_rows(nrows, [&](int i, int r, int row) {
        const float da = scale * (du.t[i][r] - (s1 + xh.t[i][r] * s2) / fb);
        p.dz[(size_t)row * p.N + col] = av.t[i][r] > 0.f ? da : 0.f;
    });
}

int row_groups(int B, int mode) { return mode == ICNN_BE_BN_MOVING ? (B + FROWS_MOVING - 1) / FROWS_MOVING : 1; }

// the workspace, piece by piece (ICNN_BE_FF_W_*): float offsets; off may be NULL
size_t work_walk(int B, int nl, const int *width, int n_labels, long long *off) {
    const size_t b = (size_t)B;
    size_t floats[ICNN_BE_FF_WORK_PIECES] = {};
    for (int i = 0; i < nl; ++i) {
        floats[ICNN_BE_FF_W_A + i] = floats[ICNN_BE_FF_W_H + i] = floats[ICNN_BE_FF_W_DZ + i] = b * width[i];
        floats[ICNN_BE_FF_W_STAT + i] = 2 * (size_t)width[i];
    }
    floats[ICNN_BE_FF_W_DLOGIT] = b * n_labels;
    floats[ICNN_BE_FF_W_PART] = 2 * (size_t)col_blocks(n_labels) * row_groups(B, ICNN_BE_BN_MOVING);
    floats[ICNN_BE_FF_W_CTL] = 4;
    return WorkPieces<ICNN_BE_FF_WORK_PIECES>::walk(floats, off);
}

// where the variables of the flat vector begin: W_i, then b_i, gamma_i, beta_i behind it; i == n_layers: W_o, b_o
struct ThetaAt {
    long long W, b, gamma, beta;
};
ThetaAt theta_at(const icnn_be_ff_args &d, int i) {
    long long at = 0;
    int in = d.n_features;
    for (int l = 0; l < i; ++l) {
        at += (long long)(in + 3) * d.width[l];
        in = d.width[l];
    }
    const int out = i < d.n_layers ? d.width[i] : d.n_labels;
    ThetaAt t;
    t.W = at;
    t.b = at + (long long)in * out;
    t.gamma = t.b + out;
    t.beta = t.gamma + out;
    return t;
}

struct Work : WorkPieces<ICNN_BE_FF_WORK_PIECES> {
    Work(const icnn_be_ff_args &d) : WorkPieces(d.work) { work_walk(d.batch, d.n_layers, d.width, d.n_labels, off); }
};

long long ff_param_floats(int n_features, int n_labels, int n_layers, const int *width) {
    long long n = 0;
    int in = n_features;
    for (int i = 0; i < n_layers; ++i) {
        n += (long long)(in + 3) * width[i];
        in = width[i];
    }
    return n + (long long)(in + 1) * n_labels;
}

// the L layer launches and the head; with_y: loss, tallies and (batch mode) d loss / d logits too
hipError_t launch_ff_forward(const icnn_be_ff_args &d, int mode, bool with_y, hipStream_t stream) {
    const Work w(d);
    const int moving = mode == ICNN_BE_BN_MOVING, B = d.batch, groups = row_groups(B, mode);
    const int rows_per = moving ? FROWS_MOVING : pad16(B), rows = rows_per < B ? rows_per : B, kl = ff_chunk_log(rows);
    const int lds = ff_lds_bytes(rows, kl);
    const float *in = d.x;
    int K = d.n_features;
    for (int i = 0; i < d.n_layers; ++i) {
        const ThetaAt t = theta_at(d, i);
        FfFwdArgs a{};
        a.X = in; a.B = B; a.K = K; a.N = d.width[i]; a.rows_per = rows_per; a.moving = moving; a.kl = kl;
        a.W = d.theta + t.W; a.b = d.theta + t.b; a.gamma = d.theta + t.gamma; a.beta = d.theta + t.beta;
        a.mean = d.mv.mean[i]; a.var = d.mv.var[i];
        a.a = w.at(ICNN_BE_FF_W_A + i); a.h = w.at(ICNN_BE_FF_W_H + i); a.stat = w.at(ICNN_BE_FF_W_STAT + i);
        a.eps = d.bn_eps;
        a.zero = i == 0 && with_y ? d.f1_tallies : nullptr;
        if (hipError_t e = launch_kernel(ff_layer_fwd_kernel, dim3(col_blocks(a.N), groups), dim3(FT), lds, stream, a); e != hipSuccess)
            return e;
        in = a.h;
        K = a.N;
    }
    const ThetaAt t = theta_at(d, d.n_layers);
    FfHeadArgs a{};
    a.X = in; a.B = B; a.K = K; a.N = d.n_labels; a.rows_per = rows_per; a.kl = kl;
    a.W = d.theta + t.W; a.b = d.theta + t.b;
    a.y = with_y ? d.true_y : nullptr;
    a.yhat = d.yhat;
    a.dlogit = with_y && !moving ? w.at(ICNN_BE_FF_W_DLOGIT) : nullptr;
    a.tallies = with_y ? d.f1_tallies : nullptr;
    a.partial = reinterpret_cast<double *>(w.at(ICNN_BE_FF_W_PART));
    a.ticket = reinterpret_cast<int *>(w.at(ICNN_BE_FF_W_CTL));
    a.loss = d.loss;
    return launch_kernel(ff_head_kernel, dim3(col_blocks(a.N), groups), dim3(FT), lds, stream, a);
}

hipError_t launch_ff_backward(const icnn_be_ff_args &d, hipStream_t stream) {
    const Work w(d);
    const int kl = ff_chunk_log(d.batch);
    const float *delta = w.at(ICNN_BE_FF_W_DLOGIT);
    int K = d.n_labels;
    for (int i = d.n_layers - 1; i >= 0; --i) {
        const ThetaAt above = theta_at(d, i + 1), t = theta_at(d, i);
        FfBwdArgs a{};
        a.D = delta; a.B = d.batch; a.K = K; a.N = d.width[i]; a.kl = kl;
        a.W = d.theta + above.W;
        a.a = w.at(ICNN_BE_FF_W_A + i); a.stat = w.at(ICNN_BE_FF_W_STAT + i); a.gamma = d.theta + t.gamma;
        a.dz = w.at(ICNN_BE_FF_W_DZ + i); a.dgamma = d.grad + t.gamma; a.dbeta = d.grad + t.beta;
        a.eps = d.bn_eps;
        if (hipError_t e = launch_kernel(ff_layer_bwd_kernel, dim3(col_blocks(a.N)), dim3(FT), ff_lds_bytes(d.batch, kl), stream, a);
            e != hipSuccess)
            return e;
        delta = a.dz;
        K = a.N;
    }
    return hipSuccess;
}

static_assert(ICNN_BE_FF_MAX_LAYERS + 1 <= GRAD_PRODUCTS, "launch_ff_grads: GradArgs::layer does not check its index");

hipError_t launch_ff_grads(const icnn_be_ff_args &d, hipStream_t stream) {
    const Work w(d);
    GradArgs a{};
    a.B = d.batch;
    // the L + 1 products in the order of the flat gradient; gamma and beta lie between the blocks
    float *g = d.grad;
    const float *in = d.x;
    int K = d.n_features;
    for (int i = 0; i < d.n_layers; ++i) {
        a.layer(in, K, w.at(ICNN_BE_FF_W_DZ + i), d.width[i], g);
        g += 2 * d.width[i];
        in = w.at(ICNN_BE_FF_W_H + i);
        K = d.width[i];
    }
    a.layer(in, K, w.at(ICNN_BE_FF_W_DLOGIT), d.n_labels, g);
    return launch_grad_table(a, stream);
}

hipError_t launch_ff_update(const icnn_be_ff_args &d, hipStream_t stream) {
    ParamSetsArgs u{};
    const long long n = ff_param_floats(d.n_features, d.n_labels, d.n_layers, d.width);
    u.set[0] = ParamSet{d.theta, d.m, d.v, nullptr, d.grad, n, (int)param_update_blocks(n), 0, 0.f, d.lr};
    u.sets = 1;
    u.step = d.step;
    u.slots = 1;
    update_coefficients(u, d.beta1, d.beta2);
    u.eps = d.eps;
    return launch_param_sets_update(u, stream);
}

hipError_t launch_ff_fold(const icnn_be_ff_args &d, hipStream_t stream) {
    const Work w(d);
    float *stat[ICNN_BE_FF_MAX_LAYERS];
    for (int i = 0; i < d.n_layers; ++i) stat[i] = w.at(ICNN_BE_FF_W_STAT + i);
    return launch_bn_fold(d.mv, stat, d.width, d.n_layers, 1, stream);
}

bool ff_sizes_ok(int n_features, int n_labels, int n_layers, const int *width) {
    if (n_features < 1 || n_features > ICNN_BE_FF_MAX_FEATURES || n_labels < 1 || n_labels > ICNN_BE_FF_MAX_WIDTH) return false;
    if (n_layers < 1 || n_layers > ICNN_BE_FF_MAX_LAYERS || !width) return false;
    for (int i = 0; i < n_layers; ++i)
        if (width[i] < 1 || width[i] > ICNN_BE_FF_MAX_WIDTH) return false;
    return true;
}

// what an icnn_be_ff_* entry needs beyond the sizes
enum : unsigned {
    FF_TRAIN_BATCH = 1, FF_X = 2, FF_Y = 4, FF_OUT = 8, FF_MOVING = 16, FF_GRAD = 32, FF_ADAM = 64, FF_WORK = 128, FF_LOSS = 256
};
int check_ff(const icnn_be_ff_args *a, void *stream, unsigned need) {
    if (!a || !ff_sizes_ok(a->n_features, a->n_labels, a->n_layers, a->width)) return ICNN_BE_EINVAL;
    if (a->batch < 1 || ((need & FF_TRAIN_BATCH) && (a->batch < 2 || a->batch > ICNN_BE_FF_MAX_BATCH))) return ICNN_BE_EINVAL;
    if (misaligned(a->theta, 16) || !stream_ok(stream)) return ICNN_BE_EINVAL;
    if ((need & FF_WORK) && misaligned(a->work, 16)) return ICNN_BE_EINVAL;
    if ((need & FF_X) && misaligned(a->x, 4)) return ICNN_BE_EINVAL;
    if ((need & FF_Y) && misaligned(a->true_y, 4)) return ICNN_BE_EINVAL;
    if ((need & FF_OUT) && misaligned(a->yhat, 4)) return ICNN_BE_EINVAL;
    if ((need & FF_LOSS) && (misaligned(a->loss, 4) || reinterpret_cast<uintptr_t>(a->f1_tallies) % 4)) return ICNN_BE_EINVAL;
    if ((need & FF_GRAD) && misaligned(a->grad, 16)) return ICNN_BE_EINVAL;
    if (need & FF_ADAM) {
        if (misaligned(a->m, 16) || misaligned(a->v, 16) || misaligned(a->step, 4)) return ICNN_BE_EINVAL;
        if (!adam_constants_ok(a->beta1, a->beta2, a->eps) || !std::isfinite(a->lr)) return ICNN_BE_EINVAL;
    }
    if (need & FF_MOVING) {
        for (int i = 0; i < a->n_layers; ++i)
            if (misaligned(a->mv.mean[i], 4) || misaligned(a->mv.var[i], 4)) return ICNN_BE_EINVAL;
        if (!(a->mv.decay >= 0.f && a->mv.decay <= 1.f)) return ICNN_BE_EINVAL;
    }
    if (!(a->bn_eps > 0.f)) return ICNN_BE_EINVAL;
    return 0;
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_ff_param_floats(int n_features, int n_labels, int n_layers, const int *width, long long *n) {
    if (!ff_sizes_ok(n_features, n_labels, n_layers, width) || !n) return ICNN_BE_EINVAL;
    *n = ff_param_floats(n_features, n_labels, n_layers, width);
    return 0;
}

size_t icnn_be_ff_work_bytes(int batch, int n_features, int n_labels, int n_layers, const int *width) {
    if (batch < 1 || !ff_sizes_ok(n_features, n_labels, n_layers, width)) return 0;
    return work_walk(batch, n_layers, width, n_labels, nullptr) * sizeof(float);
}

int icnn_be_ff_work_offsets(int batch, int n_features, int n_labels, int n_layers, const int *width,
                            long long off[ICNN_BE_FF_WORK_PIECES]) {
    if (batch < 1 || !ff_sizes_ok(n_features, n_labels, n_layers, width) || !off) return ICNN_BE_EINVAL;
    work_walk(batch, n_layers, width, n_labels, off);
    return 0;
}

int icnn_be_ff_forward(const icnn_be_ff_args *a, int mode, void *stream) {
    if (mode != ICNN_BE_BN_BATCH && mode != ICNN_BE_BN_MOVING) return ICNN_BE_EINVAL;
    const bool with_y = a && a->true_y;
    unsigned need = FF_X | FF_OUT | FF_WORK | (with_y ? FF_Y | FF_LOSS : 0u);
    need |= mode == ICNN_BE_BN_MOVING ? FF_MOVING : FF_TRAIN_BATCH;
    if (int rc = check_ff(a, stream, need)) return rc;
    return api_done(launch_ff_forward(*a, mode, with_y, static_cast<hipStream_t>(stream)));
}

int icnn_be_ff_backward(const icnn_be_ff_args *a, void *stream) {
    if (int rc = check_ff(a, stream, FF_TRAIN_BATCH | FF_WORK | FF_GRAD)) return rc;
    return api_done(launch_ff_backward(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_ff_grads(const icnn_be_ff_args *a, void *stream) {
    if (int rc = check_ff(a, stream, FF_TRAIN_BATCH | FF_X | FF_WORK | FF_GRAD)) return rc;
    return api_done(launch_ff_grads(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_ff_update(const icnn_be_ff_args *a, void *stream) {
    if (int rc = check_ff(a, stream, FF_GRAD | FF_ADAM)) return rc;
    return api_done(launch_ff_update(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_ff_step(const icnn_be_ff_args *a, void *stream) {
    if (int rc = check_ff(a, stream, FF_TRAIN_BATCH | FF_X | FF_Y | FF_OUT | FF_LOSS | FF_MOVING | FF_GRAD | FF_ADAM | FF_WORK))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_ff_forward(*a, ICNN_BE_BN_BATCH, true, s);
    if (e == hipSuccess) e = launch_ff_backward(*a, s);
    if (e == hipSuccess) e = launch_ff_grads(*a, s);
    if (e == hipSuccess) e = launch_ff_update(*a, s);
    if (e == hipSuccess) e = launch_ff_fold(*a, s);
    return api_done(e);
}

int icnn_be_ff_eval(const icnn_be_ff_args *a, void *stream) {
    if (int rc = check_ff(a, stream, FF_X | FF_Y | FF_OUT | FF_LOSS | FF_MOVING | FF_WORK)) return rc;
    return api_done(launch_ff_forward(*a, ICNN_BE_BN_MOVING, true, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
