// Training step of the convolutional PICNN of the completion experiment on the device: the parameter gradient of
//   F = sum_r c_r E(x_s(r), y_r) + <dE/dy(x_s(r), y_r), v_r>          completion/icnn_ebundle.py:129-140
// over every trainable variable, with the feed of train_step_fd (:315-335).  DESIGN.md "Training gradient of the conv
// PICNN" has the maths; the structure is be_train_fc.hip's:
//   1. x-only forward on the B unique samples with the context producer's stage GEMMs (launch_conv_context_stage,
//      be_context.hip); BatchNorm weighted by each sample's row count over (samples x positions) per channel.  The ReLU'd
//      pre-BN maps, x-hat and the inverse std are kept.
//   2. y-path on the R rows: primal and tangent rows stacked.  Each conv z-layer l reads ONE input map per row whose
//      channels are [ z_{l-1} * gate_l | y_red_l * yu_l | y_red_l ] (the last one for l < 2 only) and ONE stacked weight
//      [k][k][ch][F_l + 1] whose extra output column is the y_red convolution: so one explicit im2col and one GEMM give
//      the pre-activation and y_red_{l+1}.  The im2col carries a bias column (1 on primal rows, 0 on tangent rows) that
//      holds y_red's bias: the tangent chain has none.  fc3 (flat -> fch) and fc4 follow.
//   3. reverse pass: the two adjoint columns (primal seeded with c_r, tangent with 1) through the same masks; per conv
//      layer dW = im2col^T adj, dcol = adj W^T and a col2im GATHER (every input pixel sums its (position, tap) terms in a
//      fixed order); the per-row context gradient in the context-row layout; fixed-order segment sum per sample.
//   4. x-only backward on the B samples: head ReLUs, the weighted BatchNorm backward with its batch-statistics terms,
//      stage weight and bias gradients (im2col^T dpre with a ones column: the bias row lands behind the weight, where the
//      packed gradient keeps the bias), stage input gradients by col2im, down to u0.
// Every contraction runs through be_train_common.hip's strided f32-MFMA GEMM (launch_tr_gemm): split-K partials summed in
// a fixed order, no atomics anywhere -- the same bits on every run, and no host synchronisation.
#include <hip/hip_runtime.h>

#include <climits>

#include "be_train_common.h"
#include "icnn_be.h"

namespace icnn_be {

namespace {

#define TC_LOOP(i, total) for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (total); i += (size_t)gridDim.x * blockDim.x)

// stacked weight of conv z-layer l, [Kc][N] row-major, Kc = k*k*ch + 1, N = F + has_yr:
//   (tap, c < cin, o < F) Wzu_l   (tap, cin, o < F) Wyu_l   (tap, cin + 1, F) Wyr_l   (bias row, F) byr_l   else 0
struct WyArgs {
    const float *wpack;
    long long zu_frag, yu, yr, byr;
    int kk2, cin, ch, F, has_yr;
    float *dst;
};
__global__ void tc_unpack_wy_kernel(WyArgs a) {
    const int N = a.F + a.has_yr, Kc = a.kk2 * a.ch + 1;
    TC_LOOP(i, (size_t)Kc * N) {
        const int kk = (int)(i / N), o = (int)(i - (size_t)kk * N);
        float v = 0.f;
        if (kk < a.kk2 * a.ch) {
            const int tap = kk / a.ch, c = kk - tap * a.ch;
            if (c < a.cin && o < a.F) v = frag_at(a.wpack + a.zu_frag, a.F, tap * a.cin + c, o);
            else if (c == a.cin && o < a.F) v = a.wpack[a.yu + (size_t)tap * a.F + o];
            else if (a.has_yr && c == a.cin + 1 && o == a.F) v = a.wpack[a.yr + tap];
        } else if (a.has_yr && o == a.F) {
            v = a.wpack[a.byr];
        }
        a.dst[i] = v;
    }
}

// W3 [flat][fch] out of its forward MFMA operand
__global__ void tc_unpack_fc_kernel(const float *frag, int K, int N, float *dst) {
    TC_LOOP(i, (size_t)K * N) {
        const int kk = (int)(i / N), o = (int)(i - (size_t)kk * N);
        dst[i] = frag_at(frag, N, kk, o);
    }
}

// im2col of NHWC maps [rows][IH][IW][IC] ('SAME' window KS / ST / PD, OH x OW positions): col[(row, pos)][ld], ld >=
// KS*KS*IC; with bias != 0 column KS*KS*IC holds 1 for rows < ones_rows and 0 beyond (the tangent rows)
struct ColArgs {
    const float *in;
    int rows, IH, IW, IC, KS, ST, PD, OH, OW, ld, bias, ones_rows;
    float *col;
};
__global__ void tc_im2col_kernel(ColArgs a) {
    const int P = a.OH * a.OW, Kx = a.KS * a.KS * a.IC, cols = Kx + a.bias;
    TC_LOOP(i, (size_t)a.rows * P * cols) {
        const size_t m = i / cols;
        const int k = (int)(i - m * cols), r = (int)(m / P), pos = (int)(m - (size_t)r * P);
        float v;
        if (k == Kx) {
            v = r < a.ones_rows ? 1.f : 0.f;
        } else {
            const int tap = k / a.IC, ci = k - tap * a.IC, ky = tap / a.KS, kx = tap - ky * a.KS;
            const int oy = pos / a.OW, ox = pos - oy * a.OW, iy = oy * a.ST - a.PD + ky, ix = ox * a.ST - a.PD + kx;
            v = (iy >= 0 && iy < a.IH && ix >= 0 && ix < a.IW) ? a.in[(((size_t)r * a.IH + iy) * a.IW + ix) * a.IC + ci] : 0.f;
        }
        a.col[m * a.ld + k] = v;
    }
}

// the transposed convolution as a gather: out[row][iy][ix][ci] (+)= sum over the taps (ky, kx) that reach the pixel, in tap
// order, of dcol[(row, oy, ox)][(ky, kx, ci)]
__global__ void tc_col2im_kernel(ColArgs a, const float *dcol, float *out, int accumulate) {
    const int P = a.OH * a.OW;
    TC_LOOP(i, (size_t)a.rows * a.IH * a.IW * a.IC) {
        const int ci = (int)(i % a.IC);
        const size_t px = i / a.IC;
        const int ix = (int)(px % a.IW), iy = (int)((px / a.IW) % a.IH), r = (int)(px / ((size_t)a.IW * a.IH));
        float s = 0.f;
        for (int ky = 0; ky < a.KS; ++ky) {
            const int ty = iy + a.PD - ky;
            if (ty < 0 || ty % a.ST) continue;
            const int oy = ty / a.ST;
            if (oy >= a.OH) continue;
            for (int kx = 0; kx < a.KS; ++kx) {
                const int tx = ix + a.PD - kx;
                if (tx < 0 || tx % a.ST) continue;
                const int ox = tx / a.ST;
                if (ox >= a.OW) continue;
                s += dcol[((size_t)r * P + oy * a.OW + ox) * a.ld + (ky * a.KS + kx) * a.IC + ci];
            }
        }
        out[i] = accumulate ? out[i] + s : s;
    }
}

struct RowArgs {
    const double *y, *v, *c;
    const int *samp;
    const float *ctx;      // context rows of the B samples (weighted BatchNorm)
    int R, n, C, tan;      // tan: the tangent rows R..2R-1 exist (v given)
    const int *rows_dev;   // not NULL: the true row count (rows [*rows_dev, R) are padding: c = 0, v = 0)
};

// input map of z-layer 0: [y * yu0 | y] (tangent rows [v * yu0 | v]); y rounded to float32 like a TensorFlow feed
__global__ void tc_input0_kernel(RowArgs a, int c_yu0, float *X0) {
    TC_LOOP(i, (size_t)a.R * a.n) {
        const int r = (int)(i / a.n), j = (int)(i - (size_t)r * a.n);
        const float yu = a.ctx[(size_t)a.samp[r] * a.C + c_yu0 + j], y = (float)a.y[i];
        X0[2 * i] = y * yu;
        X0[2 * i + 1] = y;
        if (a.tan) {
            const float v = (float)a.v[i];
            const size_t t = 2 * ((size_t)a.R * a.n + i);
            X0[t] = v * yu;
            X0[t + 1] = v;
        }
    }
}

// epilogue of conv z-layer l from pre [R2 P][N] (N = F + has_yr):  z = relu(pre + zu_l), zdot = [z > 0] pre_dot (Z [R2][P][F]);
// y_red_{l+1} = the yr column (Yr [R2][P]); the next layer's input map [z gate | yr yu | yr] (ch_next channels), or for the
// last conv layer X3 = flatten(z_2) * gate_3 [R2][flat]
struct EpiArgs {
    const float *pre;
    int P, F, has_yr, c_zu, c_gate_next, c_yu_next, ch_next;
    float *Z, *Yr, *Xn;
};
__global__ void tc_conv_epi_kernel(RowArgs a, EpiArgs e) {
    const int N = e.F + e.has_yr;
    TC_LOOP(i, (size_t)a.R * e.P * N) {
        const int o = (int)(i % N);
        const size_t rp = i / N;
        const int r = (int)(rp / e.P), p = (int)(rp - (size_t)r * e.P);
        const float *crow = a.ctx + (size_t)a.samp[r] * a.C;
        const size_t mt = ((size_t)a.R * e.P) + rp;          // the tangent row of (r, p)
        if (o < e.F) {
            const float pa = e.pre[rp * N + o] + crow[e.c_zu + (size_t)p * e.F + o];
            const float z = pa > 0.f ? pa : 0.f, g = crow[e.c_gate_next + (size_t)p * e.F + o];
            e.Z[rp * e.F + o] = z;
            e.Xn[rp * e.ch_next + o] = z * g;
            if (a.tan) {
                const float zt = pa > 0.f ? e.pre[mt * N + o] : 0.f;
                e.Z[mt * e.F + o] = zt;
                e.Xn[mt * e.ch_next + o] = zt * g;
            }
        } else {
            const float yu = crow[e.c_yu_next + p];
            const float yr = e.pre[rp * N + o];
            e.Yr[rp] = yr;
            e.Xn[rp * e.ch_next + e.F] = yr * yu;
            if (e.ch_next > e.F + 1) e.Xn[rp * e.ch_next + e.F + 1] = yr;
            if (a.tan) {
                const float yt = e.pre[mt * N + o];
                e.Yr[mt] = yt;
                e.Xn[mt * e.ch_next + e.F] = yt * yu;
                if (e.ch_next > e.F + 1) e.Xn[mt * e.ch_next + e.F + 1] = yt;
            }
        }
    }
}

// fc3 / fc4 and the seeds, one workgroup per row: z3 = relu(pre3 + zu3), E = (z3 gate4) . w4 + zu4, Edot = (zdot3 gate4) . w4,
// F = c E + Edot; adj3 = [z3 > 0] gate4 w4 (times c on the primal row), X4 = [z3 ; zdot3] gate4, seed = [c ; 1], and the
// per-row context gradient of zu3, gate4, zu4
constexpr int FT_ = 256;
struct FinalArgs {
    const float *pre3, *w4;
    int fch, c_zu3, c_gate4, c_zu4;
    float *adj3, *X4, *seed, *F, *drows;
};
__global__ __launch_bounds__(FT_) void tc_final_kernel(RowArgs a, FinalArgs f) {
    __shared__ float red[2][FT_];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float *crow = a.ctx + (size_t)a.samp[r] * a.C;
    float *drow = f.drows + (size_t)r * a.C;
    const bool live = !a.rows_dev || r < *a.rows_dev;          // padding: no energy, no adjoint
    const float c = live ? (float)a.c[r] : 0.f;
    const size_t rt = (size_t)a.R + r;
    float e = 0.f, et = 0.f;
    for (int k = tid; k < f.fch; k += FT_) {
        const float pa = f.pre3[(size_t)r * f.fch + k] + crow[f.c_zu3 + k];
        const bool on = pa > 0.f;
        const float z = on ? pa : 0.f, g = crow[f.c_gate4 + k], w = f.w4[k];
        const float zt = (a.tan && on) ? f.pre3[rt * f.fch + k] : 0.f;
        e += z * g * w;
        et += zt * g * w;
        const float ap = on ? c * g * w : 0.f;
        f.adj3[(size_t)r * f.fch + k] = ap;
        f.X4[(size_t)r * f.fch + k] = z * g;
        if (a.tan) {
            f.adj3[rt * f.fch + k] = (on && live) ? g * w : 0.f;
            f.X4[rt * f.fch + k] = zt * g;
        }
        drow[f.c_zu3 + k] = ap;
        drow[f.c_gate4 + k] = w * (c * z + zt);
    }
    red[0][tid] = e;
    red[1][tid] = et;
    __syncthreads();
    for (int s = FT_ / 2; s > 0; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        drow[f.c_zu4] = c;
        f.seed[r] = c;
        if (a.tan) f.seed[rt] = live ? 1.f : 0.f;
        if (f.F) f.F[r] = live ? c * (red[0][0] + crow[f.c_zu4]) + red[1][0] : 0.f;
    }
}

// reverse step through the input map of a layer from dX (d/d of the map, [R2][Pin][ch]): channel c < cin is z_{l-1} gate_l,
// channel cin is y_red_l yu_l, channel cin + 1 (has_raw) is y_red_l.  Per-row context gradient of gate_l, yu_l and of
// zu_{l-1} (the primal adjoint), and the two adjoint columns at the pre-activation of layer l-1 (adj [R2][Pin][cin + 1],
// the last column y_red_l's).  fc3 (flat input, no y_red) is the case ch = cin, Pin = 1.
struct RouteArgs {
    const float *dX, *Zp, *Yr;        // Zp: z_{l-1} [R2][Pin][cin]; Yr: y_red_l [R2][Pin]
    int Pin, cin, ch, has_yu, has_raw, c_gate, c_yu, c_zu_prev, ld_adj;
    float *adj, *drows;
};
__global__ void tc_route_kernel(RowArgs a, RouteArgs b) {
    const int per = b.cin + b.has_yu;
    TC_LOOP(i, (size_t)a.R * b.Pin * per) {
        const int c = (int)(i % per);
        const size_t rp = i / per;
        const int r = (int)(rp / b.Pin), p = (int)(rp - (size_t)r * b.Pin);
        const size_t mt = (size_t)a.R * b.Pin + rp;
        const float *crow = a.ctx + (size_t)a.samp[r] * a.C;
        float *drow = b.drows + (size_t)r * a.C;
        const float dx = b.dX[rp * b.ch + c], dxt = a.tan ? b.dX[mt * b.ch + c] : 0.f;
        if (c < b.cin) {
            const size_t zi = rp * b.cin + c, ci = (size_t)p * b.cin + c;
            const float zp = b.Zp[zi], zt = a.tan ? b.Zp[mt * b.cin + c] : 0.f, g = crow[b.c_gate + ci];
            const bool on = zp > 0.f;
            drow[b.c_gate + ci] = zp * dx + zt * dxt;
            const float ap = on ? g * dx : 0.f;
            b.adj[rp * b.ld_adj + c] = ap;
            drow[b.c_zu_prev + ci] = ap;
            if (a.tan) b.adj[mt * b.ld_adj + c] = on ? g * dxt : 0.f;
        } else {
            const float yu = crow[b.c_yu + p], yp = b.Yr[rp], yt = a.tan ? b.Yr[mt] : 0.f;
            drow[b.c_yu + p] = yp * dx + yt * dxt;
            float sp = yu * dx, st = yu * dxt;
            if (b.has_raw) {
                sp += b.dX[rp * b.ch + c + 1];
                if (a.tan) st += b.dX[mt * b.ch + c + 1];
            }
            b.adj[rp * b.ld_adj + c] = sp;
            if (a.tan) b.adj[mt * b.ld_adj + c] = st;
        }
    }
}


// z-layer 0: only yu_0 has a context gradient (d/dy is not needed): y dX[.][0] + v dXdot[.][0]
__global__ void tc_route0_kernel(RowArgs a, const float *dX, int c_yu0, float *drows) {
    TC_LOOP(i, (size_t)a.R * a.n) {
        const int r = (int)(i / a.n), j = (int)(i - (size_t)r * a.n);
        float g = (float)a.y[i] * dX[2 * i];
        if (a.tan) g += (float)a.v[i] * dX[2 * ((size_t)a.R * a.n + i)];
        drows[(size_t)r * a.C + c_yu0 + j] = g;
    }
}

// dWy [Kc][N] of conv z-layer l -> 'z{l}_zu_proj/W' [k][k][cin][F], 'z{l}_yu/W' [k][k][1][F], 'z{l}_y_red/W' [k][k][1][1],
// 'z{l}_y_red/b' (the layout of tc_unpack_wy_kernel; the other entries of dWy are products with zero weights)
struct ScatterArgs {
    const float *dW;
    int kk2, cin, ch, F, has_yr;
    float *zproj, *yu, *yr, *byr;
};
__global__ void tc_scatter_wy_kernel(ScatterArgs a) {
    const int N = a.F + a.has_yr, Kc = a.kk2 * a.ch + 1;
    TC_LOOP(i, (size_t)Kc * N) {
        const int kk = (int)(i / N), o = (int)(i - (size_t)kk * N);
        const float d = a.dW[i];
        if (kk < a.kk2 * a.ch) {
            const int tap = kk / a.ch, c = kk - tap * a.ch;
            if (c < a.cin && o < a.F) a.zproj[((size_t)tap * a.cin + c) * a.F + o] = d;
            else if (c == a.cin && o < a.F) a.yu[(size_t)tap * a.F + o] = d;
            else if (a.has_yr && c == a.cin + 1 && o == a.F) a.yr[tap] = d;
        } else if (a.has_yr && o == a.F) {
            a.byr[0] = d;
        }
    }
}

// Weighted BatchNorm of a u-map [rows][N] (pitch ld; row = (sample, position), P positions per sample), BatchNorm over the R
// feed rows = over the samples with weights m_j (Mtot = R P): grid (NCH row chunks, column blocks of 32), fixed-order sums.
//   pass 0: per-chunk weighted sums;  pass 1: per-chunk weighted squared deviations from the mean (every workgroup forms it
//   from the pass-0 partials in the same order);  pass 2: hsave = h, xhat, u = gamma xhat + beta in place, inv, and the
//   mean [N] and variance [N] it normalised with to stat (may be NULL) for the moving statistics.
constexpr int NCH = 64, WBT = 256, WBC = 32, WBG = WBT / WBC;
struct WbnArgs {
    float *u;
    int ld, rows, P, N;
    const float *mult;
    float Mtot;
    const float *gamma, *beta;
    float eps;
    float *part, *hsave, *xhat, *inv, *stat;
    const int *rows_dev;       // not NULL: Mtot = (float)*rows_dev * P, read on the device; 0 gives mean 0 and variance 0
};
__device__ __forceinline__ float wg_colsum(float (*red)[WBC], int g, int c, float mine) {
    red[g][c] = mine;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < WBG; ++i) t += red[i][c];
    __syncthreads();
    return t;
}
__device__ __forceinline__ float chunk_total(const float *part, int N, int col) {
    float t = 0.f;
    for (int b = 0; b < NCH; ++b) t += part[(size_t)b * N + col];
    return t;
}
__global__ __launch_bounds__(WBT) void tc_wbn_fwd_kernel(WbnArgs a, int pass) {
    __shared__ float red[WBG][WBC];
    const int c = threadIdx.x % WBC, g = threadIdx.x / WBC, col = blockIdx.y * WBC + c, ch = blockIdx.x;
    const bool ok = col < a.N;
    const int per = (a.rows + NCH - 1) / NCH, r0 = ch * per, r1 = min(a.rows, r0 + per);
    const float Mtot = a.rows_dev ? (float)*a.rows_dev * a.P : a.Mtot;
    const float mean = (pass > 0 && ok && Mtot > 0.f) ? chunk_total(a.part, a.N, col) / Mtot : 0.f;
    if (pass < 2) {
        float s = 0.f;
        if (ok) for (int r = r0 + g; r < r1; r += WBG) {
            const float h = a.u[(size_t)r * a.ld + col], d = pass == 0 ? h : h - mean;
            s += a.mult[r / a.P] * (pass == 0 ? d : d * d);
        }
        const float t = wg_colsum(red, g, c, s);
        if (ok && g == 0) a.part[(size_t)(pass * NCH + ch) * a.N + col] = t;
        return;
    }
    if (!ok) return;
    const float var = Mtot > 0.f ? chunk_total(a.part + (size_t)NCH * a.N, a.N, col) / Mtot : 0.f, inv = 1.f / sqrtf(var + a.eps);
    const float ga = a.gamma[col], be = a.beta[col];
    if (ch == 0 && g == 0) {
        a.inv[col] = inv;
        if (a.stat) { a.stat[col] = mean; a.stat[a.N + col] = var; }
    }
    for (int r = r0 + g; r < r1; r += WBG) {
        const float h = a.u[(size_t)r * a.ld + col], xh = (h - mean) * inv;
        a.hsave[(size_t)r * a.N + col] = h;
        a.xhat[(size_t)r * a.N + col] = xh;
        a.u[(size_t)r * a.ld + col] = ga * xh + be;
    }
}

// Its backward from du [rows][N] (gradient at the normalised u), into the u columns of the producing stage's dpre (pitch
// ld_dpre), through the ReLU in front of the BatchNorm:
//   S1 = sum du, S2 = sum du xhat,  dh = gamma inv (du - m_j / Mtot (S1 + xhat S2)),  dgamma = S2, dbeta = S1
//   pass 0: per-chunk S1, S2;  pass 1: totals in chunk order, dpre, dgamma / dbeta
struct WbnBackArgs {
    const float *du, *xhat, *hsave, *inv, *gamma, *mult;
    int rows, P, N;
    float Mtot;
    float *part, *dpre;
    int ld_dpre;
    float *dgamma, *dbeta;
    const int *rows_dev;       // as WbnArgs
};
__global__ __launch_bounds__(WBT) void tc_wbn_back_kernel(WbnBackArgs a, int pass) {
    __shared__ float red[WBG][WBC];
    const int c = threadIdx.x % WBC, g = threadIdx.x / WBC, col = blockIdx.y * WBC + c, ch = blockIdx.x;
    const bool ok = col < a.N;
    const int per = (a.rows + NCH - 1) / NCH, r0 = ch * per, r1 = min(a.rows, r0 + per);
    if (pass == 0) {
        float s1 = 0.f, s2 = 0.f;
        if (ok) for (int r = r0 + g; r < r1; r += WBG) {
            const float d = a.du[(size_t)r * a.N + col];
            s1 += d;
            s2 += d * a.xhat[(size_t)r * a.N + col];
        }
        const float t1 = wg_colsum(red, g, c, s1), t2 = wg_colsum(red, g, c, s2);
        if (ok && g == 0) {
            a.part[(size_t)ch * a.N + col] = t1;
            a.part[(size_t)(NCH + ch) * a.N + col] = t2;
        }
        return;
    }
    if (!ok) return;
    const float S1 = chunk_total(a.part, a.N, col), S2 = chunk_total(a.part + (size_t)NCH * a.N, a.N, col);
    if (ch == 0 && g == 0) { a.dgamma[col] = S2; a.dbeta[col] = S1; }
    const float gi = a.gamma[col] * a.inv[col];
    const float Mtot = a.rows_dev ? (float)*a.rows_dev * a.P : a.Mtot;
    for (int r = r0 + g; r < r1; r += WBG) {
        const float d = a.du[(size_t)r * a.N + col], xh = a.xhat[(size_t)r * a.N + col];
        const float dh = gi * (d - (Mtot > 0.f ? a.mult[r / a.P] / Mtot : 0.f) * (S1 + xh * S2));
        a.dpre[(size_t)r * a.ld_dpre + col] = a.hsave[(size_t)r * a.N + col] > 0.f ? dh : 0.f;
    }
}

// head columns [c0, N) of a stage's dpre [B P][N] from the per-sample context gradient: column col of segment s reads
// dctx[j][off_s + pos (c1_s - c0_s) + col - c0_s], through the ReLU for a gate (mask from the gate value in the context row)
struct HeadSeg { int c0, c1, off, relu; };
struct HeadArgs {
    const float *dctx, *ctx;
    int C, P, rows, c0, N, nseg;
    HeadSeg seg[4];
    float *dpre;
};
__global__ void tc_heads_kernel(HeadArgs a) {
    const int span = a.N - a.c0;
    TC_LOOP(i, (size_t)a.rows * span) {
        const size_t m = i / span;
        const int col = a.c0 + (int)(i - m * span), j = (int)(m / a.P), pos = (int)(m - (size_t)j * a.P);
        int s = 0;
        while (s + 1 < a.nseg && col >= a.seg[s].c1) ++s;
        const HeadSeg sg = a.seg[s];
        const size_t at = (size_t)j * a.C + sg.off + (size_t)pos * (sg.c1 - sg.c0) + (col - sg.c0);
        float v = a.dctx[at];
        if (sg.relu && !(a.ctx[at] > 0.f)) v = 0.f;
        a.dpre[m * a.N + col] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

// offsets of the variables inside the packed gradient, in the order of include/icnn_be.h (icnn_amd.picnn.init_conv_params)
struct ConvGradLayout {
    size_t uW[4], gam[4], bet[4], u4W;                      // u{l}/b follows u{l}/W
    size_t zuuW[5], zproj[5], yuuW[3], yuW[3], yrW[3], yrb[3], zW[5];     // z*/b follows its W
    size_t total;
};
ConvGradLayout conv_grad_layout(const ConvCtxShape &g) {
    ConvGradLayout o{};
    size_t at = 0;
    int cin = 1;
    for (int l = 0; l < 3; ++l) {
        const size_t kk = (size_t)g.K[l] * g.K[l];
        const int nf = g.F[l];
        o.uW[l] = at; at += kk * cin * nf + nf;
        o.gam[l] = at; at += nf;
        o.bet[l] = at; at += nf;
        if (l > 0) {
            o.zuuW[l] = at; at += 9 * (size_t)cin * cin + cin;
            o.zproj[l] = at; at += kk * cin * nf;
        }
        o.yuuW[l] = at; at += 9 * (size_t)cin + 1;
        o.yuW[l] = at; at += kk * nf;
        o.yrW[l] = at; at += kk;
        o.yrb[l] = at; at += 1;
        o.zW[l] = at; at += kk * cin * nf + nf;
        cin = nf;
    }
    const size_t flat = g.flat, fch = g.fch;
    o.uW[3] = at; at += flat * fch + fch;
    o.gam[3] = at; at += fch;
    o.bet[3] = at; at += fch;
    o.u4W = at; at += fch + 1;
    o.zuuW[3] = at; at += flat * flat + flat;
    o.zproj[3] = at; at += flat * fch;
    o.zW[3] = at; at += flat * fch + fch;
    o.zuuW[4] = at; at += fch * fch + fch;
    o.zproj[4] = at; at += fch;
    o.zW[4] = at; at += fch + 1;
    o.total = at;
    return o;
}

struct TrainShape {
    ConvCtxShape g;
    int B, R, R2, n, C;
    int Pin[3], cin[3], ch[3], N[3], Kc[3];       // z-layer l: input positions / channels, GEMM columns, im2col width
};

int make_shape(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c, int batch, int rows, bool with_v, TrainShape &s) {
    s = TrainShape{};
    if (int rc = conv_ctx_shape(m, s.g)) return rc;
    (void)c;
    const ConvCtxShape &g = s.g;
    if (batch < 1 || rows < 1) return ICNN_BE_EINVAL;
    s.n = g.H * g.W;
    s.C = g.ctx_width;
    for (int l = 0; l < 3; ++l) {
        s.Pin[l] = l == 0 ? s.n : g.P[l - 1];
        s.cin[l] = l == 0 ? 0 : g.F[l - 1];
        s.ch[l] = s.cin[l] + 1 + (l < 2 ? 1 : 0);
        s.N[l] = g.F[l] + (l < 2 ? 1 : 0);
        s.Kc[l] = g.K[l] * g.K[l] * s.ch[l] + 1;
    }
    // every GEMM dimension is an int, and so is the element count of every im2col / map / context-row buffer
    const size_t r2 = (with_v ? 2 : 1) * (size_t)rows;
    size_t per_row = (size_t)g.ctx_width, per_sample = (size_t)g.ctx_width;
    for (int l = 0; l < 3; ++l) {
        const size_t a = (size_t)g.P[l] * s.Kc[l], b = (size_t)s.Pin[l] * s.ch[l];
        per_row = a > per_row ? a : per_row;
        per_row = b > per_row ? b : per_row;
        const size_t xs = (size_t)g.P[l] * (9 * (size_t)g.F[l] + 1);          // the widest stage im2col reading u_l's map
        per_sample = xs > per_sample ? xs : per_sample;
    }
    per_sample = (size_t)g.P[0] * (9 * (size_t)g.F[0] + 1) > per_sample ? (size_t)g.P[0] * (9 * (size_t)g.F[0] + 1) : per_sample;
    if (r2 * per_row >= (size_t)INT_MAX || (size_t)batch * per_sample >= (size_t)INT_MAX ||
        (size_t)batch * 4 * ((size_t)g.flat + g.fch) >= (size_t)INT_MAX)
        return ICNN_BE_ELIMIT;
    s.B = batch;
    s.R = rows;
    s.R2 = (int)r2;
    return 0;
}

hipError_t surrogate_run(const icnn_be_conv_model &m, const icnn_be_conv_ctx &cx, const TrainShape &s, const float *x,
                         const int *row_offset, const double *y, const double *v, const double *cvec, float *grad, float *F_rows,
                         float *work, size_t *work_floats, hipStream_t stream, const icnn_be_bn_moving *mv = nullptr,
                         int updates = 0, const int *rows_dev = nullptr, bool dev_sizes = false) {
    const ConvCtxShape &g = s.g;
    const int B = s.B, R = s.R, R2 = s.R2, n = s.n, C = s.C, fch = g.fch, flat = g.flat;
    const int tan = v != nullptr;
    Carver cv{work};
    int *samp = reinterpret_cast<int *>(cv.take(R));
    float *mult = cv.take(B);
    float *uwork = cv.take(conv_ctx_work_floats(g, B));
    float *ctxb = cv.take((size_t)B * C);
    // x-only forward state: per u-map h (pre-BN, ReLU'd), xhat, inv
    int urows[4], uN[4], uP[4], uld[4];
    for (int l = 0; l < 4; ++l) {
        uP[l] = l < 3 ? g.P[l] : 1;
        urows[l] = B * uP[l];
        uN[l] = l < 3 ? g.F[l] : fch;
        uld[l] = l < 3 ? g.F[l] : (fch + 3) & ~3;
    }
    float *hsave[4], *xhat[4], *inv[4], *stat[4];
    for (int l = 0; l < 4; ++l) {
        hsave[l] = cv.take((size_t)urows[l] * uN[l]);
        xhat[l] = cv.take((size_t)urows[l] * uN[l]);
        inv[l] = cv.take(uN[l]);
        stat[l] = cv.take(2 * (size_t)uN[l]);        // the weighted statistics, for the moving ones
    }
    float *bnpart = cv.take(2 * (size_t)NCH * (fch > 64 ? fch : 64));      // widest u-map: u3 (fch) or 64 channels
    // y-path state
    float *Wy[3], *X[3], *Z[3], *Yr[3] = {}, *adj[3];
    for (int l = 0; l < 3; ++l) {
        Wy[l] = cv.take((size_t)s.Kc[l] * s.N[l]);
        X[l] = cv.take((size_t)R2 * s.Pin[l] * s.ch[l]);
        Z[l] = cv.take((size_t)R2 * g.P[l] * g.F[l]);
        if (l > 0) Yr[l] = cv.take((size_t)R2 * s.Pin[l]);
        adj[l] = cv.take((size_t)R2 * g.P[l] * s.N[l]);
    }
    float *W3 = cv.take((size_t)flat * fch);
    float *X3 = cv.take((size_t)R2 * flat);
    float *pre3 = cv.take((size_t)R2 * fch);
    float *adj3 = cv.take((size_t)R2 * fch);
    float *X4 = cv.take((size_t)R2 * fch);
    float *seed = cv.take(R2);
    float *dWy = cv.take((size_t)s.Kc[2] * s.N[2] > (size_t)s.Kc[1] * s.N[1] ? (size_t)s.Kc[2] * s.N[2] : (size_t)s.Kc[1] * s.N[1]);
    float *drows = cv.take((size_t)R * C);
    float *dctx = cv.take((size_t)B * C);
    // the x-only stages (include/icnn_be.h icnn_be_conv_ctx): input, window, columns
    struct XStage {
        const float *in;
        int IH, IW, IC, KS, ST, PD, OH, OW, N, ucols, ulayer, nseg;
        HeadSeg seg[4];
        size_t wo[4];
        float *din;            // gradient of the stage input (nullptr: x)
        int accumulate;
    };
    float *du[4];
    for (int l = 0; l < 4; ++l) du[l] = cv.take((size_t)urows[l] * uN[l]);
    const int F0 = g.F[0], F1 = g.F[1], F2 = g.F[2];
    const ConvGradLayout gl = conv_grad_layout(g);
    float *u_[4];
    for (int l = 0; l < 4; ++l) u_[l] = uwork ? conv_ctx_u(g, B, uwork, l) : nullptr;
    XStage st[7] = {
        {x, g.H, g.W, 1, g.K[0], g.S[0], g.pad[0], g.oh[0], g.ow[0], 2 * F0, F0, 0, 2,
         {{0, F0, 0, 0}, {F0, 2 * F0, g.c_zu[0], 0}}, {gl.uW[0], gl.zW[0]}, nullptr, 0},
        {x, g.H, g.W, 1, 3, 1, 1, g.H, g.W, 1, 0, -1, 1, {{0, 1, g.c_yu[0], 0}}, {gl.yuuW[0]}, nullptr, 0},
        {u_[0], g.oh[0], g.ow[0], F0, g.K[1], g.S[1], g.pad[1], g.oh[1], g.ow[1], 2 * F1, F1, 1, 2,
         {{0, F1, 0, 0}, {F1, 2 * F1, g.c_zu[1], 0}}, {gl.uW[1], gl.zW[1]}, du[0], 1},     // after stage 3
        {u_[0], g.oh[0], g.ow[0], F0, 3, 1, 1, g.oh[0], g.ow[0], F0 + 1, 0, -1, 2,
         {{0, F0, g.c_gate[1], 1}, {F0, F0 + 1, g.c_yu[1], 0}}, {gl.zuuW[1], gl.yuuW[1]}, du[0], 0},
        {u_[1], g.oh[1], g.ow[1], F1, g.K[2], g.S[2], g.pad[2], g.oh[2], g.ow[2], 2 * F2 + F1 + 1, F2, 2, 4,
         {{0, F2, 0, 0}, {F2, F2 + F1, g.c_gate[2], 1}, {F2 + F1, F2 + F1 + 1, g.c_yu[2], 0},
          {F2 + F1 + 1, 2 * F2 + F1 + 1, g.c_zu[2], 0}}, {gl.uW[2], gl.zuuW[2], gl.yuuW[2], gl.zW[2]}, du[1], 0},
        {u_[2], 1, 1, flat, 1, 1, 0, 1, 1, 2 * fch + flat, fch, 3, 3,
         {{0, fch, 0, 0}, {fch, fch + flat, g.c_gate[3], 1}, {fch + flat, 2 * fch + flat, g.c_zu3, 0}},
         {gl.uW[3], gl.zuuW[3], gl.zW[3]}, du[2], 0},
        {u_[3], 1, 1, (fch + 3) & ~3, 1, 1, 0, 1, 1, fch + 1, 0, -1, 2,
         {{0, fch, g.c_gate[4], 1}, {fch, fch + 1, g.c_zu4, 0}}, {gl.zuuW[4], gl.zW[4]}, du[3], 0},
    };
    // one im2col buffer serves every layer and stage (and their dcol)
    size_t col_floats = 0;
    for (int l = 0; l < 3; ++l) {
        const size_t f = (size_t)R2 * g.P[l] * s.Kc[l];
        if (f > col_floats) col_floats = f;
    }
    float *dpre[7];
    for (int q = 0; q < 7; ++q) {
        const XStage &t = st[q];
        const size_t rows = (size_t)B * t.OH * t.OW, kx = (size_t)t.KS * t.KS * t.IC + 1;
        if (rows * kx > col_floats) col_floats = rows * kx;
        dpre[q] = cv.take(rows * t.N);
    }
    float *col = cv.take(col_floats);
    const size_t fixed = cv.at;

    Runner run{stream, work ? work + fixed : nullptr};
    RowArgs ra{y, v, cvec, samp, ctxb, R, n, C, tan, rows_dev};
    ConvPackOffsets po{};
    conv_pack_offsets(m, po);

    // 1. rows, multiplicities, y-path weights
    run.call([&] { return launch_tr_rows(row_offset, B, R, samp, mult, stream); });
    for (int l = 0; l < 3; ++l) {
        WyArgs wa{m.wpack, l == 1 ? po.p_l2 : po.p_l3, po.w_yu[l], l < 2 ? po.w_yr[l] : 0, l < 2 ? po.b_yr[l] : 0,
                  g.K[l] * g.K[l], s.cin[l], s.ch[l], g.F[l], l < 2 ? 1 : 0, Wy[l]};
        run.launch(tc_unpack_wy_kernel, dim3(grid_for((size_t)s.Kc[l] * s.N[l])), 256, wa);
    }
    run.launch(tc_unpack_fc_kernel, dim3(grid_for((size_t)flat * fch)), 256, (const float *)(m.wpack + po.p_fc3), flat, fch, W3);

    // 2. x-only forward on the B samples: stage GEMMs of the context producer, weighted BatchNorm behind the u-maps
    auto wbn_fwd = [&](int l) {
        WbnArgs a{u_[l], uld[l], urows[l], uP[l], uN[l], mult, (float)R * uP[l], cx.bn_gamma[l], cx.bn_beta[l], cx.bn_eps,
                  bnpart, hsave[l], xhat[l], inv[l], updates > 0 ? stat[l] : nullptr, rows_dev};
        for (int pass = 0; pass < 3; ++pass)
            run.launch(tc_wbn_fwd_kernel, dim3(NCH, (uN[l] + WBC - 1) / WBC), WBT, a, pass);
    };
    for (int q = 0; q < 7; ++q) {
        run.call([&] { return launch_conv_context_stage(g, cx, q, x, B, ctxb, uwork, stream); });
        if (q == 1) wbn_fwd(0);
        else if (q == 3) wbn_fwd(1);
        else if (q == 4) wbn_fwd(2);
        else if (q == 5) wbn_fwd(3);
    }
    if (updates > 0) run.call([&] { return launch_bn_fold(*mv, stat, uN, 4, updates, stream, nullptr, rows_dev); });

    // 3. y-path forward, primal and tangent rows stacked
    auto colargs = [&](const float *in, int rows, int IH, int IW, int IC, int KS, int ST, int PD, int OH, int OW, int ld,
                       int bias, int ones_rows) {
        return ColArgs{in, rows, IH, IW, IC, KS, ST, PD, OH, OW, ld, bias, ones_rows, col};
    };
    auto zcol = [&](int l) {
        const int IH = l == 0 ? g.H : g.oh[l - 1], IW = l == 0 ? g.W : g.ow[l - 1];
        return colargs(X[l], R2, IH, IW, s.ch[l], g.K[l], g.S[l], g.pad[l], g.oh[l], g.ow[l], s.Kc[l], 1, R);
    };
    run.launch(tc_input0_kernel, dim3(grid_for((size_t)R * n)), 256, ra, g.c_yu[0], X[0]);
    for (int l = 0; l < 3; ++l) {
        const ColArgs ca = zcol(l);
        const int M = R2 * g.P[l];
        run.launch(tc_im2col_kernel, dim3(grid_for((size_t)M * s.Kc[l])), 256, ca);
        float *pre = adj[l];          // the adjoint buffer holds the pre-activation until the reverse pass
        run.gemm(col, s.Kc[l], 1, Wy[l], s.N[l], 1, M, s.N[l], s.Kc[l], pre, s.N[l], rows_dev, (R2 / R) * g.P[l], dev_sizes);
        EpiArgs ea{pre, g.P[l], g.F[l], l < 2 ? 1 : 0, g.c_zu[l], g.c_gate[l + 1], l < 2 ? g.c_yu[l + 1] : 0,
                   l < 2 ? s.ch[l + 1] : flat, Z[l], l < 2 ? Yr[l + 1] : nullptr, l < 2 ? X[l + 1] : X3};
        if (l == 2) {           // X3 [R2][flat]: the map index (p, o) is the flat index with "channel pitch" F2
            ea.ch_next = F2;
            ea.Xn = X3;
        }
        run.launch(tc_conv_epi_kernel, dim3(grid_for((size_t)R * g.P[l] * s.N[l])), 256, ra, ea);
    }
    run.gemm(X3, flat, 1, W3, fch, 1, R2, fch, flat, pre3, fch, rows_dev, R2 / R, dev_sizes);
    FinalArgs fa{pre3, m.wpack + po.w_fc4, fch, g.c_zu3, g.c_gate[4], g.c_zu4, adj3, X4, seed, F_rows, drows};
    run.launch(tc_final_kernel, dim3(R), FT_, ra, fa);

    // 4. reverse: fc4, fc3, then the conv z-layers
    run.gemm(X4, 1, fch, seed, 1, 0, fch, 1, R2, grad + gl.zproj[4], 1);                          // (z3 gate4)^T [c ; 1]
    run.gemm(X3, 1, flat, adj3, fch, 1, flat, fch, R2, grad + gl.zproj[3], fch);                 // X3^T adj3
    float *dX3 = col;
    run.gemm(adj3, fch, 1, W3, 1, fch, R2, flat, fch, dX3, flat);                                // adj3 W3^T
    {
        RouteArgs rb{dX3, Z[2], nullptr, 1, flat, flat, 0, 0, g.c_gate[3], 0, g.c_zu[2], flat, adj[2], drows};
        run.launch(tc_route_kernel, dim3(grid_for((size_t)R * flat)), 256, ra, rb);
    }
    for (int l = 2; l >= 0; --l) {
        const ColArgs ca = zcol(l);
        const int M = R2 * g.P[l];
        run.launch(tc_im2col_kernel, dim3(grid_for((size_t)M * s.Kc[l])), 256, ca);
        run.gemm(col, 1, s.Kc[l], adj[l], s.N[l], 1, s.Kc[l], s.N[l], M, dWy, s.N[l]);          // im2col^T adj
        ScatterArgs sa{dWy, g.K[l] * g.K[l], s.cin[l], s.ch[l], g.F[l], l < 2 ? 1 : 0, l > 0 ? grad + gl.zproj[l] : nullptr,
                       grad + gl.yuW[l], grad + gl.yrW[l], grad + gl.yrb[l]};
        run.launch(tc_scatter_wy_kernel, dim3(grid_for((size_t)s.Kc[l] * s.N[l])), 256, sa);
        run.gemm(adj[l], s.N[l], 1, Wy[l], 1, s.N[l], M, s.Kc[l] - 1, s.N[l], col, s.Kc[l]);      // dcol = adj Wy^T
        float *dX = X[l];           // the input map is not read again: its gradient takes its place
        run.launch(tc_col2im_kernel, dim3(grid_for((size_t)R2 * s.Pin[l] * s.ch[l])), 256, ca, (const float *)col, dX, 0);
        if (l > 0) {
            RouteArgs rb{dX, Z[l - 1], Yr[l], s.Pin[l], s.cin[l], s.ch[l], 1, l < 2 ? 1 : 0, g.c_gate[l], g.c_yu[l],
                         g.c_zu[l - 1], s.N[l - 1], adj[l - 1], drows};
            run.launch(tc_route_kernel, dim3(grid_for((size_t)R * s.Pin[l] * (s.cin[l] + 1))), 256, ra, rb);
        } else {
            run.launch(tc_route0_kernel, dim3(grid_for((size_t)R * n)), 256, ra, (const float *)dX, g.c_yu[0], drows);
        }
    }
    run.call([&] { return launch_tr_zero(grad + gl.yrW[2], (size_t)(g.K[2] * g.K[2] + 1), stream); });   // z2_y_red: never reaches E
    run.call([&] { return launch_tr_zero(grad + gl.u4W, (size_t)fch + 1, stream); });                    // u4: never read

    // 5. per-sample context gradient
    run.call([&] { return launch_tr_segment_sum(drows, row_offset, B, R, C, dctx, stream); });

    // 6. x-only backward on the B samples, stages in reverse order
    auto wbn_back = [&](int l, int q) {
        WbnBackArgs a{du[l], xhat[l], hsave[l], inv[l], cx.bn_gamma[l], mult, urows[l], uP[l], uN[l], (float)R * uP[l], bnpart,
                      dpre[q], st[q].N, grad + gl.gam[l], grad + gl.bet[l], rows_dev};
        for (int pass = 0; pass < 2; ++pass)
            run.launch(tc_wbn_back_kernel, dim3(NCH, (uN[l] + WBC - 1) / WBC), WBT, a, pass);
    };
    for (int q = 6; q >= 0; --q) {
        const XStage &t = st[q];
        const int P = t.OH * t.OW, rows = B * P, Kx = t.KS * t.KS * t.IC;
        HeadArgs ha{dctx, ctxb, C, P, rows, t.ucols, t.N, 0, {}, dpre[q]};
        for (int k = 0; k < t.nseg; ++k)
            if (t.seg[k].c0 >= t.ucols) ha.seg[ha.nseg++] = t.seg[k];
        run.launch(tc_heads_kernel, dim3(grid_for((size_t)rows * (t.N - t.ucols))), 256, ha);
        if (t.ulayer >= 0) wbn_back(t.ulayer, q);      // du of the u-map this stage produced: every reader came before
        const ColArgs ca{t.in, B, t.IH, t.IW, t.IC, t.KS, t.ST, t.PD, t.OH, t.OW, Kx + 1, 1, B, col};
        run.launch(tc_im2col_kernel, dim3(grid_for((size_t)rows * (Kx + 1))), 256, ca);
        for (int k = 0; k < t.nseg; ++k) {       // [dW ; db] of every variable of the stage: the bias row lands behind W
            const int cols = t.seg[k].c1 - t.seg[k].c0;
            run.gemm(col, 1, Kx + 1, dpre[q] + t.seg[k].c0, t.N, 1, Kx + 1, cols, rows, grad + t.wo[k], cols);
        }
        if (!t.din) continue;
        const int ldw = (t.N + 3) & ~3;
        if (t.KS == 1) {            // dense stage: the input gradient directly
            run.gemm(dpre[q], t.N, 1, cx.w_stage[q], 1, ldw, B, Kx, t.N, t.din, Kx);
        } else {
            run.gemm(dpre[q], t.N, 1, cx.w_stage[q], 1, ldw, rows, Kx, t.N, col, Kx + 1);
            run.launch(tc_col2im_kernel, dim3(grid_for((size_t)B * t.IH * t.IW * t.IC)), 256, ca, (const float *)col, t.din,
                       t.accumulate);
        }
    }
    if (work_floats) *work_floats = fixed + run.part_need;
    return run.err;
}

}  // namespace

size_t conv_grad_floats(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c) {
    TrainShape s;
    if (make_shape(m, c, 1, 1, true, s) != 0) return 0;
    return conv_grad_layout(s.g).total;
}

size_t conv_surrogate_work_floats(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c, int batch, int rows, bool dev) {
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

int conv_surrogate_shape(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c, int batch, int rows, bool with_v) {
    TrainShape s;
    return make_shape(m, c, batch, rows, with_v, s);
}

hipError_t launch_conv_surrogate_grad(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c, const float *x, int batch,
                                      const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                      float *grad, float *F_rows, float *work, hipStream_t stream,
                                      const icnn_be_bn_moving *mv, int updates, const int *rows_dev) {
    TrainShape s;
    if (make_shape(m, c, batch, rows, v != nullptr, s) != 0) return hipErrorInvalidValue;
    return surrogate_run(m, c, s, x, row_offset, y, v, cvec, grad, F_rows, work, nullptr, stream, mv, updates, rows_dev);
}

}  // namespace icnn_be
