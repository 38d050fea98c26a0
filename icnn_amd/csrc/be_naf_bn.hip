// NAF with BatchNorm, naf_bn True (RL/src/naf_nets_dm.py:18-34, naf.py; include/icnn_be.h, icnn_be_naf_bn_*): a
// BatchNorm with a trainable beta in front of the first layer and between each hidden product and its ReLU, in all three nets.
//
// BatchNorm crosses the samples, so the hidden layers follow be_ff.hip's scheme (be_col_gemm.h): a workgroup owns FC columns
// of a layer's output for ALL rows of the batch, every cross-sample quantity is a column statistic inside it and every
// dependency between workgroups is a launch boundary.  Passes that do not depend on each other share a launch through
// blockIdx.y: the four forward passes (L, U, V at obs; the target at ob2), the three backward ones.
//
//   naf_bn_input_kernel   BN0: the column statistics of obs or ob2 and h0 = xhat + beta0 of the pass; no product
//   naf_bn_fwd_kernel     z = h W + b for the workgroup's columns, the column mean and biased variance in LDS in a fixed order
//                         (two passes, both shifted by the column's first row: a constant column has variance 0 and xhat 0
//                         exactly), xhat, relu(xhat + beta); stores the activation, xhat and (mu, var).  Moving mode: the
//                         moving pair instead, and nothing of the batch is formed
//   naf_bn_sample_kernel  what stays inside one sample, one workgroup per 16-sample tile (be_tile.h): layer 3 of the four
//                         nets, y, the head (be_naf_head.h), q, td and the tile's sum of td^2, the head's backward: layer 3's
//                         deltas.  what = 0 stops behind u, what = 1 behind q: icnn_be_naf_bn_act and _q
//   naf_bn_bwd_kernel     dout = delta_up W_up^T for the workgroup's columns, the ReLU mask from the stored activation,
//                         d beta = sum dout straight into the flat gradient, dz = inv (dout - mean(dout) - xhat mean(dout xhat))
//   naf_bn_input_bwd_kernel   d beta0 = the column sums of dz1 W1^T
//   naf_bn_fold_kernel    the moving pairs: L and U once, V twice (obs, then ob2)
//   the weight gradients  grad_table_kernel, the update param_sets_update_kernel with the betas as the exempt tail
#include "be_api_check.h"
#include "be_kernels.h"
#include "be_col_gemm.h"
#include "be_naf_head.h"
#include "be_tile.h"
#include "be_train_common.h"
#include "be_train_table.h"

namespace icnn_be {

namespace {

constexpr int PASSES = ICNN_BE_NAF_BN_PASSES;
static_assert(ICNN_BE_NAF_BN_MAX_BATCH == ICNN_BE_FF_MAX_BATCH, "col_gemm's accumulators are sized by ICNN_BE_FF_MAX_BATCH");

// mean and biased variance over the rows < nrows of column tid / 32 of buf [FC][pitch], in every lane of that group.  Both
// passes in a fixed order (column_sum's); the first is taken relative to the column's first row
__device__ __forceinline__ void column_stats(const float *buf, int pitch, int nrows, float &mean, float &var) {
    const int c = threadIdx.x >> 5, l = threadIdx.x & 31;
    const float x0 = buf[c * pitch], fb = (float)nrows;
    float s = 0.f;
    for (int r = l; r < nrows; r += 32) s += buf[c * pitch + r] - x0;
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 32);
    mean = x0 + s / fb;
    float v = 0.f;
    for (int r = l; r < nrows; r += 32) {
        const float d = buf[c * pitch + r] - mean;
        v = fmaf(d, d, v);
    }
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 32);
    var = v / fb;
}

struct BnPass {
    const float *X;                      // the layer's input [B][K]
    const float *W, *b, *beta;           // W [K][N]
    const float *mv;                     // mean [N] then var [N] of this site (moving mode)
    float *h, *xh, *stat;                // [B][N], [B][N] (NULL: not kept), mu [N] then var [N] (batch mode)
};
struct BnFwdArgs {
    BnPass p[PASSES];
    int B, K, N, kl, moving;
    float eps;
};

__global__ __launch_bounds__(FT) void naf_bn_input_kernel(BnFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const BnPass &p = a.p[blockIdx.y];
    const int nrows = a.B, N = a.N, pitch = pad16(nrows) + 4;
    float *buf = lds, *smean = buf + FC * pitch, *svar = smean + FC;
    const int tid = threadIdx.x, c0 = blockIdx.x * FC;
    for (int i = tid; i < FC * nrows; i += FT) {
        const int c = i & (FC - 1), r = i >> 4;
        buf[c * pitch + r] = c0 + c < N ? p.X[(size_t)r * N + c0 + c] : 0.f;
    }
    __syncthreads();
    const int c = tid >> 5, l = tid & 31;
    const bool vc = c0 + c < N;
    float mean, var;
    if (a.moving) {
        mean = vc ? p.mv[c0 + c] : 0.f;
        var = vc ? p.mv[N + c0 + c] : 1.f;
    } else {
        column_stats(buf, pitch, nrows, mean, var);
        if (l == 0 && vc) {
            p.stat[c0 + c] = mean;
            p.stat[N + c0 + c] = var;
        }
    }
    if (l == 0) {
        smean[c] = mean;
        svar[c] = var;
    }
    __syncthreads();
    for (int i = tid; i < FC * nrows; i += FT) {
        const int cc = i & (FC - 1), r = i >> 4;
        if (c0 + cc < N) {
            const float inv = 1.f / sqrtf(svar[cc] + a.eps);
            p.h[(size_t)r * N + c0 + cc] = (buf[cc * pitch + r] - smean[cc]) * inv + p.beta[c0 + cc];
        }
    }
}

__global__ __launch_bounds__(FT) void naf_bn_fwd_kernel(BnFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const BnPass &p = a.p[blockIdx.y];
    const int nrows = a.B, N = a.N, pitch = pad16(nrows) + 4;
    float *xs = lds, *ws = xs + ff_stage_floats(nrows, a.kl), *smean = ws + ff_weight_floats(a.kl), *svar = smean + FC;
    const int tid = threadIdx.x, r16 = tid & 15, c0 = blockIdx.x * FC, col = c0 + r16;
    const bool vc = col < N;
    Frag acc;
    col_gemm(p.X, a.K, 0, nrows, a.K, p.W, N, 1, c0, N, a.kl, xs, ws, acc);
    const float bias = vc ? p.b[col] : 0.f;
    for_rows(nrows, [&](int i, int r, int row) { acc.t[i][r] += bias; });
    if (!a.moving) {
        for_rows(nrows, [&](int i, int r, int row) { xs[r16 * pitch + row] = acc.t[i][r]; });
        __syncthreads();
        const int c = tid >> 5, l = tid & 31;
        float mean, var;
        column_stats(xs, pitch, nrows, mean, var);
        if (l == 0) {
            smean[c] = mean;
            svar[c] = var;
            if (c0 + c < N) {
                p.stat[c0 + c] = mean;
                p.stat[N + c0 + c] = var;
            }
        }
        __syncthreads();
    }
    if (!vc) return;
    const float mean = a.moving ? p.mv[col] : smean[r16], var = a.moving ? p.mv[N + col] : svar[r16];
    const float inv = 1.f / sqrtf(var + a.eps), be = p.beta[col];
    for_rows(nrows, [&](int i, int r, int row) {
        const size_t at = (size_t)row * N + col;
        const float xh = (acc.t[i][r] - mean) * inv, v = xh + be;
        if (p.xh) p.xh[at] = xh;
        p.h[at] = v > 0.f ? v : 0.f;
    });
}

struct BnBwdPass {
    const float *D, *W;                  // the delta above [B][K] and that layer's weights [N][K]
    int K;
    const float *h, *xh, *stat;          // this site's activation, xhat and (mu, var)
    float *dz, *dbeta;                   // [B][N]; [N] inside the flat gradient
};
struct BnBwdArgs {
    BnBwdPass p[PASSES - 1];
    int B, N, kl;
    float eps;
};

__global__ __launch_bounds__(FT) void naf_bn_bwd_kernel(BnBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const BnBwdPass &p = a.p[blockIdx.y];
    const int nrows = a.B, N = a.N, pitch = pad16(nrows) + 4;
    float *xs = lds, *ws = xs + ff_stage_floats(nrows, a.kl), *s1s = ws + ff_weight_floats(a.kl), *s2s = s1s + FC;
    float *b1 = xs, *b2 = xs + FC * pitch;
    const int tid = threadIdx.x, r16 = tid & 15, c0 = blockIdx.x * FC, col = c0 + r16;
    const bool vc = col < N;
    Frag du, xh;
    col_gemm(p.D, p.K, 0, nrows, p.K, p.W, 1, p.K, c0, N, a.kl, xs, ws, du);
    for_rows(nrows, [&](int i, int r, int row) {
        const size_t at = (size_t)row * N + col;
        const bool on = vc && p.h[at] > 0.f;
        xh.t[i][r] = vc ? p.xh[at] : 0.f;
        du.t[i][r] = on ? du.t[i][r] : 0.f;
        b1[r16 * pitch + row] = du.t[i][r];
        b2[r16 * pitch + row] = du.t[i][r] * xh.t[i][r];
    });
    __syncthreads();
    const int c = tid >> 5, l = tid & 31;
    const float S1 = column_sum(b1, pitch, nrows), S2 = column_sum(b2, pitch, nrows);
    if (l == 0) {
        s1s[c] = S1;
        s2s[c] = S2;
        if (c0 + c < N) p.dbeta[c0 + c] = S1;
    }
    __syncthreads();
    if (!vc) return;
    const float fb = (float)nrows, m1 = s1s[r16] / fb, m2 = s2s[r16] / fb, inv = 1.f / sqrtf(p.stat[N + col] + a.eps);
    for_rows(nrows, [&](int i, int r, int row) { p.dz[(size_t)row * N + col] = inv * (du.t[i][r] - m1 - xh.t[i][r] * m2); });
}

// d beta0: BN0's output meets no ReLU and nothing propagates further
__global__ __launch_bounds__(FT) void naf_bn_input_bwd_kernel(BnBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const BnBwdPass &p = a.p[blockIdx.y];
    const int nrows = a.B, N = a.N, pitch = pad16(nrows) + 4;
    float *xs = lds, *ws = xs + ff_stage_floats(nrows, a.kl);
    const int tid = threadIdx.x, r16 = tid & 15, c0 = blockIdx.x * FC;
    Frag du;
    col_gemm(p.D, p.K, 0, nrows, p.K, p.W, 1, p.K, c0, N, a.kl, xs, ws, du);
    for_rows(nrows, [&](int i, int r, int row) { xs[r16 * pitch + row] = du.t[i][r]; });
    __syncthreads();
    const int c = tid >> 5;
    const float S1 = column_sum(xs, pitch, nrows);
    if ((tid & 31) == 0 && c0 + c < N) p.dbeta[c0 + c] = S1;
}

struct BnSampleArgs {
    int B, dimA, l2, what;               // what: 0 u alone, 1 up to q, 2 the whole step
    const float *h2[PASSES], *W3[PASSES], *b3[PASSES];       // L, U, V, the target
    const float *rew;
    const double *act;
    const unsigned char *term;
    float discount, inv_b;
    float *y, *u, *l, *ld, *h, *adv, *q, *td, *d3l, *d3u, *d3v;      // NULL where `what` does not reach
    double *sq;
    int PA, PC, PS;
};

__global__ __launch_bounds__(DT) void naf_bn_sample_kernel(BnSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, dimA = a.dimA, l2 = a.l2, nL = dimA * dimA;
    const int PA = a.PA, PC = a.PC, PS = a.PS;
    float *bA = lds, *bC = bA + TS * PA, *sU = bC + TS * PC, *sD = sU + TS * PS, *vt = sD + TS * PS;
    Tile t;
    t.s0 = blockIdx.x * TS;
    t.rows = a.B - t.s0 < TS ? a.B - t.s0 : TS;
    const int s32 = tid >> 5, j = tid & 31;                     // the head: lane j of the group of sample s32
    const bool row = s32 < t.rows, col = j < dimA;
    const size_t gs = (size_t)(t.s0 + s32);
    // ---- the target: y from the fourth pass; its advantage is the constant 0 ----
    float y = 0.f;
    if (a.what == 2) {
        load_rows(bC, PC, 0, a.h2[3], l2, t);
        __syncthreads();
        const float q2 = tile_dot(bC, PC, l2, a.W3[3]) + a.b3[3][0];
        if (row) {
            const float r = a.rew[gs];
            y = a.term[gs] ? r : r + a.discount * q2;
            if (j == 0) a.y[gs] = y;
        }
        __syncthreads();
    }
    // ---- layer 3 of U, V, then L ----
    load_rows(bC, PC, 0, a.h2[1], l2, t);
    if (a.what) load_rows(sD, PS, 0, a.act, dimA, t);           // float64 actions, rounded to float32 once
    __syncthreads();
    tile_gemm(bC, PC, l2, a.W3[1], dimA, 1, dimA, [&](int s, int c, float acc) {
        const float v = tanhf(acc + a.b3[1][c]);
        sU[s * PS + c] = v;
        if (a.u && s < t.rows) a.u[(size_t)(t.s0 + s) * dimA + c] = v;
    });
    if (!a.what) return;
    __syncthreads();
    load_rows(bC, PC, 0, a.h2[2], l2, t);
    __syncthreads();
    const float v = tile_dot(bC, PC, l2, a.W3[2]) + a.b3[2][0];
    __syncthreads();
    load_rows(bC, PC, 0, a.h2[0], l2, t);
    __syncthreads();
    tile_gemm(bC, PC, l2, a.W3[0], nL, 1, nL, [&](int s, int c, float acc) {
        const float x = acc + a.b3[0][c];
        bA[s * PA + c] = x;
        if (a.l && s < t.rows) a.l[(size_t)(t.s0 + s) * nL + c] = x;
    });
    __syncthreads();
    // ---- the head ----
    float *lr = bA + s32 * PA;                                   // l of this sample, row-major [dimA][dimA]
    const NafHead H = naf_head_forward(lr, sU + s32 * PS, sD + s32 * PS, dimA, j);
    const float q = v + H.adv;
    if (row && j == 0) a.q[gs] = q;
    if (a.what == 1) return;
    const float td = q - y, d3 = a.inv_b * (2.f * td);
    if (row) {
        if (col) {
            a.ld[gs * dimA + j] = H.e;
            a.h[gs * dimA + j] = H.hj;
        }
        if (j == 0) {
            a.adv[gs] = H.adv;
            a.td[gs] = td;
            a.d3v[gs] = d3;
        }
    }
    if (j == 0) vt[s32] = row ? td : 0.f;
    float gh;
    const float du = naf_head_du(H, lr, dimA, j, d3, gh);
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < t.rows; ++i) s = s + (double)vt[i] * (double)vt[i];
        a.sq[blockIdx.x] = s;
    }
    if (row && col) a.d3u[gs * dimA + j] = du;
    naf_head_dl(H, nullptr, dimA, j, gh, row ? a.d3l + gs * nL : nullptr);      // the backward chains are other launches
}

struct BnFoldArgs {
    float *mv[PASSES - 1];
    const float *stat[PASSES];
    int n;
    float d;                             // 1 - decay
};

__global__ __launch_bounds__(256) void naf_bn_fold_kernel(BnFoldArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x, net = blockIdx.y;
    if (i >= a.n) return;
    float m = a.mv[net][i];
    m = m - (m - a.stat[net][i]) * a.d;
    if (net == 2) m = m - (m - a.stat[3][i]) * a.d;              // V's pairs meet the target pass too: obs first, then ob2
    a.mv[net][i] = m;
}

// where the variables of a net's flat vector begin: NAF's W1 .. b3, then beta0, beta1, beta2
struct NetAt {
    long long W[3], b[3], beta[3], plain, n;
};
NetAt net_at(int dimO, int l1, int l2, int out) {
    NetAt t;
    const int in[3] = {dimO, l1, l2}, wd[3] = {l1, l2, out};
    long long at = 0;
    for (int i = 0; i < 3; ++i) {
        t.W[i] = at;
        at += (long long)in[i] * wd[i];
        t.b[i] = at;
        at += wd[i];
    }
    t.plain = at;
    for (int i = 0; i < 3; ++i) {
        t.beta[i] = at;
        at += in[i];
    }
    t.n = at;
    return t;
}
int out_of(int which, int dimA) { return which == 0 ? dimA * dimA : which == 1 ? dimA : 1; }

// the workspace, piece by piece (ICNN_BE_NAF_BN_W_*): float offsets; off may be NULL
size_t work_walk(int B, int dimO, int dimA, int l1, int l2, long long *off) {
    const size_t b = (size_t)B, S = (size_t)dimO + l1 + l2;
    const int tiles = (B + TS - 1) / TS;
    size_t f[ICNN_BE_NAF_BN_WORK_PIECES] = {};
    f[ICNN_BE_NAF_BN_W_Y] = f[ICNN_BE_NAF_BN_W_ADV] = f[ICNN_BE_NAF_BN_W_Q] = f[ICNN_BE_NAF_BN_W_TD] = b;
    f[ICNN_BE_NAF_BN_W_U] = f[ICNN_BE_NAF_BN_W_LD] = f[ICNN_BE_NAF_BN_W_H] = b * dimA;
    f[ICNN_BE_NAF_BN_W_L] = b * dimA * dimA;
    long long upd = 0;
    for (int p = 0; p < PASSES; ++p) {
        f[ICNN_BE_NAF_BN_W_H0 + p] = b * dimO;
        f[ICNN_BE_NAF_BN_W_H1 + p] = b * l1;
        f[ICNN_BE_NAF_BN_W_H2 + p] = b * l2;
        f[ICNN_BE_NAF_BN_W_STAT + p] = 2 * S;
        if (p == PASSES - 1) break;      // the target pass has no backward
        f[ICNN_BE_NAF_BN_W_D3 + p] = b * out_of(p, dimA);
        f[ICNN_BE_NAF_BN_W_XH1 + p] = f[ICNN_BE_NAF_BN_W_D1 + p] = b * l1;
        f[ICNN_BE_NAF_BN_W_XH2 + p] = f[ICNN_BE_NAF_BN_W_D2 + p] = b * l2;
        upd += param_update_blocks(net_at(dimO, l1, l2, out_of(p, dimA)).n);
    }
    f[ICNN_BE_NAF_BN_W_SQ] = 2 * (size_t)tiles;
    f[ICNN_BE_NAF_BN_W_UPD] = 2 * (size_t)upd;
    return WorkPieces<ICNN_BE_NAF_BN_WORK_PIECES>::walk(f, off);
}

struct Work : WorkPieces<ICNN_BE_NAF_BN_WORK_PIECES> {
    Work(void *work, int B, int dimO, int dimA, int l1, int l2) : WorkPieces(work) { work_walk(B, dimO, dimA, l1, l2, off); }
    Work(const icnn_be_naf_bn_args &d) : Work(d.work, d.batch, d.dimO, d.dimA, d.l1, d.l2) {}
};

struct Pitches {
    int PA, PC, PS;
    int bytes() const { return (TS * (PA + PC + 2 * PS) + TS) * (int)sizeof(float); }
};
Pitches pitches(int dimA, int l2) { return {pitch_of(dimA * dimA), pitch_of(l2), pitch_of(dimA)}; }

// one forward pass: W and b from `theta`, the betas from `betas` (a whole net's vector), the moving pairs `mv`, into slot p
struct PassNet {
    int p;
    const float *x, *theta, *betas, *mv;
};

// BN0 and the two hidden layers of `count` passes: three launches
hipError_t forward_layers(const PassNet *nets, int count, int B, int dimO, int dimA, int l1, int l2, int moving, float eps,
                          const Work &w, hipStream_t stream) {
    const int kl = ff_chunk_log(B), lds = ff_lds_bytes(B, kl), width[3] = {dimO, l1, l2};
    const int h_piece[3] = {ICNN_BE_NAF_BN_W_H0, ICNN_BE_NAF_BN_W_H1, ICNN_BE_NAF_BN_W_H2};
    const int xh_piece[3] = {-1, ICNN_BE_NAF_BN_W_XH1, ICNN_BE_NAF_BN_W_XH2};
    long long so = 0;                    // where this site's (mu, var) lie in a [2 S] block
    for (int i = 0; i < 3; ++i) {
        BnFwdArgs a{};
        a.B = B; a.K = i ? width[i - 1] : 0; a.N = width[i]; a.kl = kl; a.moving = moving; a.eps = eps;
        for (int k = 0; k < count; ++k) {
            const PassNet &n = nets[k];
            const NetAt at = net_at(dimO, l1, l2, out_of(n.p, dimA));     // W1 .. b2 and the betas lie alike in every net
            BnPass &p = a.p[k];
            p.X = i ? w.at(h_piece[i - 1] + n.p) : n.x;
            p.W = i ? n.theta + at.W[i - 1] : nullptr;
            p.b = i ? n.theta + at.b[i - 1] : nullptr;
            p.beta = n.betas + at.beta[i];
            p.mv = n.mv + so;
            p.h = w.at(h_piece[i] + n.p);
            p.xh = i && n.p < PASSES - 1 && !moving ? w.at(xh_piece[i] + n.p) : nullptr;
            p.stat = w.at(ICNN_BE_NAF_BN_W_STAT + n.p) + so;
        }
        const hipError_t e =
            i ? launch_kernel(naf_bn_fwd_kernel, dim3(col_blocks(a.N), count), dim3(FT), lds, stream, a)
              : launch_kernel(naf_bn_input_kernel, dim3(col_blocks(a.N), count), dim3(FT),
                              (FC * (pad16(B) + 4) + 2 * FC) * (int)sizeof(float), stream, a);
        if (e != hipSuccess) return e;
        so += 2 * width[i];
    }
    return hipSuccess;
}

void sample_net(BnSampleArgs &a, int p, const float *theta, int dimO, int dimA, int l1, int l2, const Work &w) {
    const NetAt at = net_at(dimO, l1, l2, out_of(p, dimA));
    a.h2[p] = w.at(ICNN_BE_NAF_BN_W_H2 + p);
    a.W3[p] = theta + at.W[2];
    a.b3[p] = theta + at.b[2];
}

hipError_t launch_sample(const BnSampleArgs &a, hipStream_t stream) {
    return launch_kernel(naf_bn_sample_kernel, dim3((a.B + TS - 1) / TS), dim3(DT), pitches(a.dimA, a.l2).bytes(), stream, a);
}

// off[ICNN_BE_NAF_BN_VARS], the floats of the vector and of its W and b alone; each may be NULL.  which: 0 L, 1 U, 2 V
void naf_bn_layout(int dimO, int dimA, int l1, int l2, int which, long long *off, long long *n, long long *plain) {
    const NetAt at = net_at(dimO, l1, l2, out_of(which, dimA));
    if (off)
        for (int i = 0; i < 3; ++i) {
            off[2 * i] = at.W[i];
            off[2 * i + 1] = at.b[i];
            off[6 + i] = at.beta[i];
        }
    if (n) *n = at.n;
    if (plain) *plain = at.plain;
}

hipError_t launch_naf_bn_chain(const icnn_be_naf_bn_args &d, hipStream_t stream) {
    const Work w(d);
    const int B = d.batch, dimO = d.dimO, dimA = d.dimA, l1 = d.l1, l2 = d.l2;
    const float *theta[PASSES] = {d.theta_l, d.theta_u, d.theta_v, d.target_v};
    float *grad[PASSES - 1] = {d.grad_l, d.grad_u, d.grad_v};
    // the target pass: target_v's W and b with V's betas; its moving pairs (unused in batch mode) are V's
    const PassNet nets[PASSES] = {{0, d.obs, d.theta_l, d.theta_l, d.mv_l}, {1, d.obs, d.theta_u, d.theta_u, d.mv_u},
                                  {2, d.obs, d.theta_v, d.theta_v, d.mv_v}, {3, d.ob2, d.target_v, d.theta_v, d.mv_v}};
    hipError_t e = forward_layers(nets, PASSES, B, dimO, dimA, l1, l2, 0, d.bn_eps, w, stream);
    if (e != hipSuccess) return e;
    const Pitches pt = pitches(dimA, l2);
    BnSampleArgs s{};
    s.B = B; s.dimA = dimA; s.l2 = l2; s.what = 2;
    for (int p = 0; p < PASSES; ++p) sample_net(s, p, theta[p], dimO, dimA, l1, l2, w);
    s.rew = d.rew; s.act = d.act; s.term = d.term;
    s.discount = d.discount;
    s.inv_b = 1.f / (float)B;
    s.y = w.at(ICNN_BE_NAF_BN_W_Y); s.u = w.at(ICNN_BE_NAF_BN_W_U); s.l = w.at(ICNN_BE_NAF_BN_W_L);
    s.ld = w.at(ICNN_BE_NAF_BN_W_LD); s.h = w.at(ICNN_BE_NAF_BN_W_H); s.adv = w.at(ICNN_BE_NAF_BN_W_ADV);
    s.q = w.at(ICNN_BE_NAF_BN_W_Q); s.td = w.at(ICNN_BE_NAF_BN_W_TD);
    s.d3l = w.at(ICNN_BE_NAF_BN_W_D3); s.d3u = w.at(ICNN_BE_NAF_BN_W_D3 + 1); s.d3v = w.at(ICNN_BE_NAF_BN_W_D3 + 2);
    s.sq = reinterpret_cast<double *>(w.at(ICNN_BE_NAF_BN_W_SQ));
    s.PA = pt.PA; s.PC = pt.PC; s.PS = pt.PS;
    if ((e = launch_sample(s, stream)) != hipSuccess) return e;
    // ---- backward: BN2, BN1, BN0; a launch each, the three nets side by side ----
    const int kl = ff_chunk_log(B), lds = ff_lds_bytes(B, kl), width[3] = {dimO, l1, l2};
    const int h_piece[3] = {ICNN_BE_NAF_BN_W_H0, ICNN_BE_NAF_BN_W_H1, ICNN_BE_NAF_BN_W_H2};
    const int xh_piece[3] = {-1, ICNN_BE_NAF_BN_W_XH1, ICNN_BE_NAF_BN_W_XH2};
    const int dz_piece[4] = {-1, ICNN_BE_NAF_BN_W_D1, ICNN_BE_NAF_BN_W_D2, ICNN_BE_NAF_BN_W_D3};
    for (int i = 2; i >= 0; --i) {
        BnBwdArgs a{};
        a.B = B; a.N = width[i]; a.kl = kl; a.eps = d.bn_eps;
        const long long so = i == 2 ? 2LL * (dimO + l1) : i == 1 ? 2LL * dimO : 0;
        for (int p = 0; p < PASSES - 1; ++p) {
            const NetAt at = net_at(dimO, l1, l2, out_of(p, dimA));
            BnBwdPass &b = a.p[p];
            b.D = w.at(dz_piece[i + 1] + p);
            b.W = theta[p] + at.W[i];
            b.K = i == 2 ? out_of(p, dimA) : width[i + 1];
            b.dbeta = grad[p] + at.beta[i];
            if (i) {
                b.h = w.at(h_piece[i] + p);
                b.xh = w.at(xh_piece[i] + p);
                b.stat = w.at(ICNN_BE_NAF_BN_W_STAT + p) + so;
                b.dz = w.at(dz_piece[i] + p);
            }
        }
        e = i ? launch_kernel(naf_bn_bwd_kernel, dim3(col_blocks(a.N), PASSES - 1), dim3(FT), lds, stream, a)
              : launch_kernel(naf_bn_input_bwd_kernel, dim3(col_blocks(a.N), PASSES - 1), dim3(FT), lds, stream, a);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_naf_bn_grads(const icnn_be_naf_bn_args &d, hipStream_t stream) {
    const Work w(d);
    float *grad[PASSES - 1] = {d.grad_l, d.grad_u, d.grad_v};
    GradArgs a{};
    a.B = d.batch;
    // the nine layers in the order of the three flat gradients; the betas lie behind them
    for (int p = 0; p < PASSES - 1; ++p) {
        float *g = grad[p];
        a.layer(w.at(ICNN_BE_NAF_BN_W_H0 + p), d.dimO, w.at(ICNN_BE_NAF_BN_W_D1 + p), d.l1, g);
        a.layer(w.at(ICNN_BE_NAF_BN_W_H1 + p), d.l1, w.at(ICNN_BE_NAF_BN_W_D2 + p), d.l2, g);
        a.layer(w.at(ICNN_BE_NAF_BN_W_H2 + p), d.l2, w.at(ICNN_BE_NAF_BN_W_D3 + p), out_of(p, d.dimA), g);
    }
    return launch_grad_table(a, stream);
}

hipError_t launch_naf_bn_update(const icnn_be_naf_bn_args &d, bool with_loss, hipStream_t stream) {
    const Work w(d);
    ParamSetsArgs u{};
    float *theta[3] = {d.theta_l, d.theta_u, d.theta_v}, *m[3] = {d.m_l, d.m_u, d.m_v}, *v[3] = {d.v_l, d.v_u, d.v_v};
    const float *grad[3] = {d.grad_l, d.grad_u, d.grad_v};
    // one optimizer: the three sets read the one step count; only V has a target; the betas are every set's exempt tail
    for (int p = 0; p < 3; ++p) {
        const NetAt at = net_at(d.dimO, d.l1, d.l2, out_of(p, d.dimA));
        u.set[p] = ParamSet{theta[p], m[p], v[p], p == 2 ? d.target_v : nullptr, grad[p], at.n, (int)param_update_blocks(at.n), 0,
                            d.l2norm, d.rate, at.n - at.plain};
        u.reg_blocks += u.set[p].blocks;
    }
    u.sets = 3;
    u.step = d.step;
    u.slots = 1;
    update_coefficients(u, d.beta1, d.beta2);
    u.eps = d.eps;
    u.tau = d.tau;
    u.loss = with_loss ? d.loss : nullptr;
    u.sq = reinterpret_cast<const double *>(w.at(ICNN_BE_NAF_BN_W_SQ));
    u.tiles = (d.batch + TS - 1) / TS;
    u.batch = d.batch;
    u.l2norm = (double)d.l2norm;
    u.partial = reinterpret_cast<double *>(w.at(ICNN_BE_NAF_BN_W_UPD));
    return launch_param_sets_update(u, stream);
}

hipError_t launch_naf_bn_fold(const icnn_be_naf_bn_args &d, hipStream_t stream) {
    const Work w(d);
    BnFoldArgs a{};
    a.mv[0] = d.mv_l; a.mv[1] = d.mv_u; a.mv[2] = d.mv_v;
    for (int p = 0; p < PASSES; ++p) a.stat[p] = w.at(ICNN_BE_NAF_BN_W_STAT + p);
    a.n = 2 * (d.dimO + d.l1 + d.l2);
    a.d = (float)(1.0 - d.bn_decay);
    return launch_kernel(naf_bn_fold_kernel, dim3((a.n + 255) / 256, PASSES - 1), dim3(256), 0, stream, a);
}

// theta_l NULL: u(obs) into out [B][dimA]; else q(obs, act) into out [B]
hipError_t launch_naf_bn_forward(int dimO, int dimA, int l1, int l2, const float *theta_l, const float *theta_u,
                                 const float *theta_v, const float *mv_l, const float *mv_u, const float *mv_v, float bn_eps,
                                 int moving, const float *obs, const double *act, int B, float *out, void *work,
                                 hipStream_t stream) {
    const Work w(work, B, dimO, dimA, l1, l2);
    const bool with_q = theta_l != nullptr;                      // else u alone
    const PassNet nets[3] = {{1, obs, theta_u, theta_u, mv_u}, {0, obs, theta_l, theta_l, mv_l}, {2, obs, theta_v, theta_v, mv_v}};
    if (hipError_t e = forward_layers(nets, with_q ? 3 : 1, B, dimO, dimA, l1, l2, moving, bn_eps, w, stream); e != hipSuccess)
        return e;
    const Pitches pt = pitches(dimA, l2);
    BnSampleArgs s{};
    s.B = B; s.dimA = dimA; s.l2 = l2; s.what = with_q ? 1 : 0;
    sample_net(s, 1, theta_u, dimO, dimA, l1, l2, w);
    if (with_q) {
        sample_net(s, 0, theta_l, dimO, dimA, l1, l2, w);
        sample_net(s, 2, theta_v, dimO, dimA, l1, l2, w);
        s.act = act;
        s.q = out;
    } else {
        s.u = out;
    }
    s.PA = pt.PA; s.PC = pt.PC; s.PS = pt.PS;
    return launch_sample(s, stream);
}

// NAF's sizes, the batch the column kernels hold and the per-sample kernel's LDS
bool naf_bn_sizes_ok(int batch, int dimO, int dimA, int l1, int l2) {
    return batch >= 1 && batch <= ICNN_BE_NAF_BN_MAX_BATCH && naf_sizes_ok(dimO, dimA, l1, l2) &&
           pitches(dimA, l2).bytes() <= LDS_BYTES;
}

bool bn_mode_ok(int mode) { return mode == ICNN_BE_BN_BATCH || mode == ICNN_BE_BN_MOVING; }

// what every icnn_be_naf_bn_* entry that takes the descriptor refuses before any launch; need_loss: loss may not be NULL
int check_naf_bn(const icnn_be_naf_bn_args *a, void *stream, bool need_loss) {
    if (!a || !naf_bn_sizes_ok(a->batch, a->dimO, a->dimA, a->l1, a->l2)) return ICNN_BE_EINVAL;
    if (int rc = check_replay_step(*a, stream, need_loss)) return rc;
    const void *a16[] = {a->theta_l, a->theta_u, a->theta_v, a->target_v, a->m_l, a->v_l, a->m_u, a->v_u, a->m_v, a->v_v,
                         a->grad_l, a->grad_u, a->grad_v};
    for (const void *p : a16)
        if (misaligned(p, 16)) return ICNN_BE_EINVAL;
    if (misaligned(a->mv_l, 4) || misaligned(a->mv_u, 4) || misaligned(a->mv_v, 4)) return ICNN_BE_EINVAL;
    if (!(a->bn_eps > 0.f) || !(a->bn_decay >= 0.0 && a->bn_decay <= 1.0)) return ICNN_BE_EINVAL;
    return 0;
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_naf_bn_param_floats(int dimO, int dimA, int l1, int l2, long long *nl, long long *nu, long long *nv, long long *nt,
                                long long *ns) {
    if (!naf_bn_sizes_ok(1, dimO, dimA, l1, l2) || !nl || !nu || !nv || !nt || !ns) return ICNN_BE_EINVAL;
    naf_bn_layout(dimO, dimA, l1, l2, 0, nullptr, nl, nullptr);
    naf_bn_layout(dimO, dimA, l1, l2, 1, nullptr, nu, nullptr);
    naf_bn_layout(dimO, dimA, l1, l2, 2, nullptr, nv, nt);
    *ns = 2LL * (dimO + l1 + l2);
    return 0;
}

int icnn_be_naf_bn_layout(int dimO, int dimA, int l1, int l2, int which, long long off[ICNN_BE_NAF_BN_VARS]) {
    if (!naf_bn_sizes_ok(1, dimO, dimA, l1, l2) || which < 0 || which > 2 || !off) return ICNN_BE_EINVAL;
    naf_bn_layout(dimO, dimA, l1, l2, which, off, nullptr, nullptr);
    return 0;
}

size_t icnn_be_naf_bn_work_bytes(int batch, int dimO, int dimA, int l1, int l2) {
    if (!naf_bn_sizes_ok(batch, dimO, dimA, l1, l2)) return 0;
    return work_walk(batch, dimO, dimA, l1, l2, nullptr) * sizeof(float);
}

int icnn_be_naf_bn_work_offsets(int batch, int dimO, int dimA, int l1, int l2, long long off[ICNN_BE_NAF_BN_WORK_PIECES]) {
    if (!naf_bn_sizes_ok(batch, dimO, dimA, l1, l2) || !off) return ICNN_BE_EINVAL;
    work_walk(batch, dimO, dimA, l1, l2, off);
    return 0;
}

int icnn_be_naf_bn_chain(const icnn_be_naf_bn_args *a, void *stream) {
    if (int rc = check_naf_bn(a, stream, false)) return rc;
    return api_done(launch_naf_bn_chain(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_naf_bn_grads(const icnn_be_naf_bn_args *a, void *stream) {
    if (int rc = check_naf_bn(a, stream, false)) return rc;
    return api_done(launch_naf_bn_grads(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_naf_bn_update(const icnn_be_naf_bn_args *a, void *stream) {
    if (int rc = check_naf_bn(a, stream, false)) return rc;
    return api_done(launch_naf_bn_update(*a, a->loss != nullptr, static_cast<hipStream_t>(stream)));
}

int icnn_be_naf_bn_step(const icnn_be_naf_bn_args *a, void *stream) {
    if (int rc = check_naf_bn(a, stream, true)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_naf_bn_chain(*a, s);
    if (e == hipSuccess) e = launch_naf_bn_grads(*a, s);
    if (e == hipSuccess) e = launch_naf_bn_update(*a, true, s);
    if (e == hipSuccess) e = launch_naf_bn_fold(*a, s);
    return api_done(e);
}

int icnn_be_naf_bn_act(int dimO, int dimA, int l1, int l2, const float *theta_u, const float *mv_u, float bn_eps, int mode,
                       const float *obs, int batch, float *out, void *work, void *stream) {
    if (!naf_bn_sizes_ok(batch, dimO, dimA, l1, l2) || !bn_mode_ok(mode)) return ICNN_BE_EINVAL;
    if (misaligned(theta_u, 16) || misaligned(work, 16) || misaligned(mv_u, 4) || misaligned(obs, 4) || misaligned(out, 4) ||
        !stream_ok(stream) || !(bn_eps > 0.f))
        return ICNN_BE_EINVAL;
    return api_done(launch_naf_bn_forward(dimO, dimA, l1, l2, nullptr, theta_u, nullptr, nullptr, mv_u, nullptr, bn_eps,
                                          mode == ICNN_BE_BN_MOVING, obs, nullptr, batch, out, work,
                                          static_cast<hipStream_t>(stream)));
}

int icnn_be_naf_bn_q(int dimO, int dimA, int l1, int l2, const float *theta_l, const float *theta_u, const float *theta_v,
                     const float *mv_l, const float *mv_u, const float *mv_v, float bn_eps, int mode, const float *obs,
                     const double *act, int batch, float *out, void *work, void *stream) {
    if (!naf_bn_sizes_ok(batch, dimO, dimA, l1, l2) || !bn_mode_ok(mode)) return ICNN_BE_EINVAL;
    if (misaligned(theta_l, 16) || misaligned(theta_u, 16) || misaligned(theta_v, 16) || misaligned(work, 16) ||
        misaligned(mv_l, 4) || misaligned(mv_u, 4) || misaligned(mv_v, 4) || misaligned(obs, 4) || misaligned(act, 8) ||
        misaligned(out, 4) || !stream_ok(stream) || !(bn_eps > 0.f))
        return ICNN_BE_EINVAL;
    return api_done(launch_naf_bn_forward(dimO, dimA, l1, l2, theta_l, theta_u, theta_v, mv_l, mv_u, mv_v, bn_eps,
                                          mode == ICNN_BE_BN_MOVING, obs, act, batch, out, work,
                                          static_cast<hipStream_t>(stream)));
}

}  // extern "C"
