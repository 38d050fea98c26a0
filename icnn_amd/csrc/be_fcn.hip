// The FCN baseline of the completion experiment on the device (completion/baseline.py; include/icnn_be.h, icnn_be_fcn_*;
// DESIGN.md §25): three dilated strided convolutions, three transposed convolutions and a 1x1 head, trained with torch's Adam
// on the mean squared pixel error.  Activations and deltas are channels last, [batch][h][w][k].
//
// All four products between k channels and k channels are ONE gather: with o an output position and t a tap,
//     out[o][co] = sum_t sum_ci in[(a o + c + d t) / s][ci] Wm[t][ci][co]   where s divides a o + c + d t and the source exists
//   conv forward           (a, c, d, s) = (2, -2,  2, 1)      its data gradient  (1, 2, -2, 2)
//   transposed forward                    (1,  1, -1, 2)      its data gradient  (2, -1, 1, 1)
// the same numbers for rows and columns, Wm an index order of the torch weight (strides).  Whether s divides depends on
// the parities of o alone, so with s = 2 the output positions are split in four parity classes and a tile of 16 positions
// never leaves a class (nor a sample): a tap is then valid or not for the whole wave, and the transposed convolution does
// its 1, 2, 2 or 4 taps, the conv's data gradient 9 or none.
//
//   fcn_conv1_kernel   conv1 (Cin = 1) on the VALU
//   fcn_gemm_kernel    the gather above on mfma_f32_16x16x4f32: a wave owns a tile of 16 positions and all k columns; the A
//                      operand (16 bytes of channels per lane) comes straight from global memory, the weights of 9 taps
//                      (k <= 32) or of 3 taps at a time are staged in LDS, [tap][co][ci + 4], once per workgroup, which then
//                      walks over its tiles.  Two accumulators per column tile take the k steps alternately.  Epilogue: bias
//                      and ReLU, or the ReLU mask of the stored activation (data gradients).
//   fcn_head_kernel    up4, the loss partial (float32 terms added in float64), d yhat and up3's delta; the last workgroup by
//                      ticket adds the partials in a fixed order, writes the loss and up4.bias's gradient, re-arms the ticket
//   fcn_wgrad_kernel   G[a][b][tap] = sum_p P[p][a] Q[2 p + c + d tap][b] over a fixed chunk of positions per workgroup (one
//                      wave: an a-tile, a tap, all b-tiles), positions on the MFMA's k axis
//   fcn_wsum_kernel    the sums over positions that have one channel axis: the biases, conv1's and up4's weights
//   fcn_reduce_kernel  adds the chunk partials in index order into the flat gradient
//   fcn_adam_kernel    torch.optim.Adam's element arithmetic with the step count on the device
#include <cmath>

#include "be_api_check.h"
#include "be_common.h"
#include "be_kernels.h"
#include "be_train_common.h"
#include "icnn_be.h"

namespace icnn_be {

namespace {

constexpr int GT = 256;                  // threads of every kernel but fcn_wgrad_kernel
constexpr int GW = GT / 64;              // tiles a workgroup of fcn_gemm_kernel works on at a time
constexpr int GEMM_MAX_BLOCKS = 512;
constexpr int HEAD_POS = 256;            // positions a workgroup of the head owns
constexpr int MAX_CHUNKS = 256;          // chunks a sum over positions is split in, at most
constexpr int MIN_CHUNK = 256;           // positions of a chunk, at least; a multiple of 16
constexpr int NLAYER = 7;

struct Geo {
    int a, c, d, s;
};
constexpr Geo CONV_FWD{2, -2, 2, 1}, CONV_DGRAD{1, 2, -2, 2}, UP_FWD{1, 1, -1, 2}, UP_DGRAD{2, -1, 1, 1};

// ---- shapes -------------------------------------------------------------------------------------------------------------
struct Shape {
    int B, H, W, k;
    int h[6], w[6];                      // of the six stored activations
    long long pos[6];                    // B h w
    long long wat[NLAYER], bat[NLAYER];  // where weight and bias of a layer begin in theta
    long long n;
    Shape(int B_, int H_, int W_, int k_) : B(B_), H(H_), W(W_), k(k_) {
        const int div[6] = {2, 4, 8, 4, 2, 1};
        for (int i = 0; i < 6; ++i) {
            h[i] = H / div[i];
            w[i] = W / div[i];
            pos[i] = (long long)B * h[i] * w[i];
        }
        long long at = 0;
        for (int l = 0; l < NLAYER; ++l) {
            const long long nw = l == 0 ? 9LL * k : l == 6 ? k : 9LL * k * k, nb = l == 6 ? 1 : k;
            wat[l] = at;
            bat[l] = at + nw;
            at += nw + nb;
        }
        n = at;
    }
};

bool sizes_ok(int H, int W, int k) {
    return k >= 16 && k <= ICNN_BE_FCN_MAX_K && k % 16 == 0 && H >= 8 && H <= ICNN_BE_FCN_MAX_HW && H % 8 == 0 && W >= 8 &&
           W <= ICNN_BE_FCN_MAX_HW && W % 8 == 0;
}

// a sum over `total` positions: chunks of MIN_CHUNK, or of as many (a multiple of 16) as make MAX_CHUNKS chunks
int chunk_len(long long total) {
    const long long per = (total + MAX_CHUNKS - 1) / MAX_CHUNKS;
    return per <= MIN_CHUNK ? MIN_CHUNK : (int)((per + 15) / 16 * 16);
}
int chunks_of(long long total) { return (int)((total + chunk_len(total) - 1) / chunk_len(total)); }

// the positions the weight gradient of layer l (1..5) runs over: the smaller of its two grids
long long wgrad_pos(const Shape &s, int l) { return l <= 2 ? s.pos[l] : s.pos[l - 1]; }

// the chunk partials, segment by segment: conv1 (weights and bias), then weight and bias of layers 1..5, then up4's weight
struct PartAt {
    long long conv1, w[6], b[6], up4, end;
};
PartAt part_at(const Shape &s) {
    PartAt p{};
    long long at = 0;
    p.conv1 = at;
    at += (long long)chunks_of(s.pos[0]) * 10 * s.k;
    for (int l = 1; l <= 5; ++l) {
        p.w[l] = at;
        at += (long long)chunks_of(wgrad_pos(s, l)) * 9 * s.k * s.k;
        p.b[l] = at;
        at += (long long)chunks_of(s.pos[l]) * s.k;
    }
    p.up4 = at;
    at += (long long)chunks_of(s.pos[5]) * s.k;
    p.end = at;
    return p;
}

int head_blocks(const Shape &s) { return (int)((s.pos[5] + HEAD_POS - 1) / HEAD_POS); }

size_t work_walk(const Shape &s, long long *off) {
    size_t floats[ICNN_BE_FCN_WORK_PIECES] = {};
    for (int i = 0; i < 6; ++i) floats[ICNN_BE_FCN_W_H + i] = floats[ICNN_BE_FCN_W_DZ + i] = (size_t)s.pos[i] * s.k;
    floats[ICNN_BE_FCN_W_DY] = (size_t)s.pos[5];
    floats[ICNN_BE_FCN_W_WPART] = (size_t)part_at(s).end;
    floats[ICNN_BE_FCN_W_LPART] = 4 * (size_t)head_blocks(s);
    floats[ICNN_BE_FCN_W_CTL] = 4;
    return WorkPieces<ICNN_BE_FCN_WORK_PIECES>::walk(floats, off);
}

struct Work : WorkPieces<ICNN_BE_FCN_WORK_PIECES> {
    Work(const icnn_be_fcn_args &d, const Shape &s) : WorkPieces(d.work) { work_walk(s, off); }
};

// ---- conv1 --------------------------------------------------------------------------------------------------------------
struct Conv1Args {
    const float *x, *w, *b;              // [B][H][W]; [k][9]; [k]
    float *out;                          // [B][H/2][W/2][k]
    int H, W, k;
    long long n;                         // B H/2 W/2 k
};

__global__ __launch_bounds__(GT) void fcn_conv1_kernel(Conv1Args p) {
    const long long idx = (long long)blockIdx.x * GT + threadIdx.x;
    if (idx >= p.n) return;
    const int c = (int)(idx % p.k), ho = p.H / 2, wo = p.W / 2;
    const long long pos = idx / p.k;
    const int ox = (int)(pos % wo), oy = (int)((pos / wo) % ho);
    const float *img = p.x + (pos / ((long long)wo * ho)) * p.H * p.W;
    float acc = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = 2 * oy - 2 + 2 * (tap / 3), ix = 2 * ox - 2 + 2 * (tap % 3);
        const float v = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W ? img[iy * p.W + ix] : 0.f;
        acc = fmaf(v, p.w[c * 9 + tap], acc);
    }
    acc += p.b[c];
    p.out[idx] = acc > 0.f ? acc : 0.f;
}

// ---- the gather product ---------------------------------------------------------------------------------------------------
struct GemmArgs {
    const float *in;                     // [B][hi][wi][k]
    float *out;                          // [B][ho][wo][k]
    const float *W;                      // element (ci, co, tap) of Wm at W[ci s_in + co s_out + tap]
    const float *bias;                   // NULL: none
    const float *mask;                   // not NULL: out = mask > 0 ? v : 0 (same shape as out); NULL: ReLU
    int s_in, s_out;
    int k, hi, wi, ho, wo;
    Geo g;
    int class_pos, class_w;              // positions and columns of a parity class: (ho / s) (wo / s), wo / s
    int tiles_class, tiles_sample, tiles;
    int tpc;                             // taps staged at a time: 9 or 3
};

template <int KT>
__global__ __launch_bounds__(GT) void fcn_gemm_kernel(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) float ws[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
    const int k = KT * 16, fp = k + 4, s = p.g.s;
    bool staged = false;
    for (int tg = blockIdx.x; tg * GW < p.tiles; tg += gridDim.x) {
        const int tile = tg * GW + wave;
        const bool active = tile < p.tiles;
        const int b = tile / p.tiles_sample, rem = tile - b * p.tiles_sample, cls = rem / p.tiles_class;
        const int py = cls / s, px = cls - py * s, j0 = (rem - cls * p.tiles_class) * 16;
        // the row of the A operand this lane loads
        const int ja = j0 + r16, jya = ja / p.class_w, oya = s * jya + py, oxa = s * (ja - jya * p.class_w) + px;
        const bool va = active && ja < p.class_pos;
        const float *inb = p.in + (size_t)b * p.hi * p.wi * k;
        f4 even[KT], odd[KT];
#pragma unroll
        for (int n = 0; n < KT; ++n) even[n] = odd[n] = f4{0.f, 0.f, 0.f, 0.f};
        for (int t0 = 0; t0 < 9; t0 += p.tpc) {
            if (p.tpc < 9 || !staged) {
                __syncthreads();
                // in the order of memory: (slow channel, fast channel, tap)
                for (int idx = tid; idx < p.tpc * k * k; idx += GT) {
                    const int ca = idx / (p.tpc * k), r = idx - ca * p.tpc * k, cb = r / p.tpc, tl = r - cb * p.tpc;
                    const int ci = p.s_in > p.s_out ? ca : cb, co = p.s_in > p.s_out ? cb : ca;
                    ws[(tl * k + co) * fp + ci] = p.W[(size_t)ca * 9 * k + cb * 9 + t0 + tl];
                }
                __syncthreads();
                staged = true;
            }
            if (!active) continue;
            // a kernel row at a time: the loads of its three taps are issued before the products of the first
            for (int tl0 = 0; tl0 < p.tpc; tl0 += 3) {
                const int ty = (t0 + tl0) / 3;
                if ((p.g.a * py + p.g.c + p.g.d * ty) & (s - 1)) continue;        // s divides for the whole class or not at all
                const int sy = (p.g.a * oya + p.g.c + p.g.d * ty) / s;
                f4 av[3][KT];
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) {
                    const int nx = p.g.a * oxa + p.g.c + p.g.d * tx, sx = nx / s;
                    const bool v = va && !(nx & (s - 1)) && sy >= 0 && sy < p.hi && sx >= 0 && sx < p.wi;
                    const float *src = inb + ((size_t)(v ? sy : 0) * p.wi + (v ? sx : 0)) * k + 4 * q;
#pragma unroll
                    for (int kk = 0; kk < KT; ++kk) av[tx][kk] = v ? *reinterpret_cast<const f4 *>(src + 16 * kk) : f4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) {
                    if ((p.g.a * px + p.g.c + p.g.d * tx) & (s - 1)) continue;
#pragma unroll
                    for (int n = 0; n < KT; ++n) {
                        const float *wrow = ws + ((tl0 + tx) * k + n * 16 + r16) * fp + 4 * q;
#pragma unroll
                        for (int kk = 0; kk < KT; ++kk) {
                            const f4 bv = *reinterpret_cast<const f4 *>(wrow + 16 * kk);
                            even[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tx][kk][0], bv[0], even[n], 0, 0, 0);
                            odd[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tx][kk][1], bv[1], odd[n], 0, 0, 0);
                            even[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tx][kk][2], bv[2], even[n], 0, 0, 0);
                            odd[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tx][kk][3], bv[3], odd[n], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (!active) continue;
        // the accumulator's rows 4 q + r, column r16
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * q + r;
            if (j >= p.class_pos) continue;
            const int jy = j / p.class_w, oy = s * jy + py, ox = s * (j - jy * p.class_w) + px;
            const size_t at = (((size_t)b * p.ho + oy) * p.wo + ox) * k + r16;
#pragma unroll
            for (int n = 0; n < KT; ++n) {
                float v = even[n][r] + odd[n][r];
                if (p.bias) v += p.bias[n * 16 + r16];
                if (p.mask)
                    v = p.mask[at + n * 16] > 0.f ? v : 0.f;
                else
                    v = v > 0.f ? v : 0.f;
                p.out[at + n * 16] = v;
            }
        }
    }
}

// ---- up4, loss, d yhat, up3's delta -----------------------------------------------------------------------------------------
struct HeadArgs {
    const float *h;                      // up3's output [n][k]
    const float *w, *b;                  // up4
    const float *t;                      // NULL: yhat alone
    float *yhat;
    float *dy, *dz;                      // NULL (both): none
    long long n;                         // B H W
    int k;
    float scale, coef;                   // pixel_scale; 2 pixel_scale / n
    double *partial;                     // [blocks][2]
    int *ticket;
    float *loss, *dbias;
};

__global__ __launch_bounds__(GT) void fcn_head_kernel(HeadArgs p) {
    __shared__ double red[GT];
    const int tid = threadIdx.x, l16 = tid & 15, grp = tid >> 4;
    const float b4 = p.b[0];
    float w4[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) w4[c] = 16 * c + l16 < p.k ? p.w[16 * c + l16] : 0.f;
    double sum = 0.0, dsum = 0.0;
    for (int i = 0; i < HEAD_POS / 16; ++i) {
        const long long pos = (long long)blockIdx.x * HEAD_POS + 16 * i + grp;
        const bool vp = pos < p.n;
        float hv[4], acc = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            hv[c] = vp && 16 * c + l16 < p.k ? p.h[(size_t)pos * p.k + 16 * c + l16] : 0.f;
            acc = fmaf(hv[c], w4[c], acc);
        }
        for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
        const float yh = acc + b4;
        if (!vp) continue;                // a whole group of 16 lanes leaves together
        if (l16 == 0) p.yhat[pos] = yh;
        if (!p.t) continue;
        const float e = p.scale * (yh - p.t[pos]), dy = e * p.coef;
        if (l16 == 0) {
            sum = sum + (double)(e * e);
            dsum = dsum + (double)dy;
            if (p.dy) p.dy[pos] = dy;
        }
        if (p.dz)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (16 * c + l16 < p.k) p.dz[(size_t)pos * p.k + 16 * c + l16] = hv[c] > 0.f ? dy * w4[c] : 0.f;
    }
    if (!p.t) return;
    sum = block_tree_sum<GT>(sum, red);
    dsum = block_tree_sum<GT>(dsum, red);
    __shared__ int last;
    const int blocks = (int)gridDim.x;
    if (tid == 0) {
        __hip_atomic_store(p.partial + 2 * blockIdx.x, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p.partial + 2 * blockIdx.x + 1, dsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = __hip_atomic_fetch_add(p.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == blocks - 1;
    }
    __syncthreads();
    if (!last) return;
    // the last workgroup: thread i adds the partials i, i + 256, ... in index order, then the fixed tree; rounded to float32
    // once; the ticket re-armed
    double tot = 0.0, dtot = 0.0;
    for (int b = tid; b < blocks; b += GT) {
        tot = tot + __hip_atomic_load(p.partial + 2 * b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dtot = dtot + __hip_atomic_load(p.partial + 2 * b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    tot = block_tree_sum<GT>(tot, red);
    dtot = block_tree_sum<GT>(dtot, red);
    if (tid == 0) {
        *p.loss = (float)(tot / (double)p.n);
        if (p.dbias) *p.dbias = (float)dtot;
        __hip_atomic_store(p.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- weight gradients of the k -> k layers ------------------------------------------------------------------------------
struct WgradJob {
    const float *P, *Q;                  // [B][hs][ws][k] (the smaller grid), [B][2 hs][2 ws][k]
    float *part;                         // [chunks][k][k][9]
    int hs, ws, c, d, chunk, chunks;
    long long total;                     // B hs ws
};
struct WgradArgs {
    WgradJob job[5];
    int k;
};

template <int KT>
__global__ __launch_bounds__(64) void fcn_wgrad_kernel(WgradArgs p) {
    const WgradJob &j = p.job[blockIdx.z];
    if ((int)blockIdx.x >= j.chunks) return;
    const int lane = threadIdx.x, r16 = lane & 15, q = lane >> 4, k = KT * 16;
    const int at = blockIdx.y / 9, tap = blockIdx.y - 9 * at, ty = tap / 3, tx = tap - 3 * ty;
    const long long p0 = (long long)blockIdx.x * j.chunk;
    const int per = j.hs * j.ws;
    f4 acc[2][KT];
#pragma unroll
    for (int n = 0; n < KT; ++n) acc[0][n] = acc[1][n] = f4{0.f, 0.f, 0.f, 0.f};
    // 16 positions at a time: their loads are issued before the first product; the two accumulators alternate
    for (int st = 0; st < j.chunk; st += 16) {
        float av[4], bv[4][KT];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const long long pos = p0 + st + 4 * g + q;
            const bool vp = pos < j.total;
            const int b = (int)(pos / per), r = (int)(pos - (long long)b * per), y = r / j.ws, x = r - y * j.ws;
            const int sy = 2 * y + j.c + j.d * ty, sx = 2 * x + j.c + j.d * tx;
            const bool vq = vp && sy >= 0 && sy < 2 * j.hs && sx >= 0 && sx < 2 * j.ws;
            av[g] = vq ? j.P[(size_t)pos * k + at * 16 + r16] : 0.f;
            const float *src = j.Q + (((size_t)(vq ? b : 0) * 2 * j.hs + (vq ? sy : 0)) * 2 * j.ws + (vq ? sx : 0)) * k + r16;
#pragma unroll
            for (int n = 0; n < KT; ++n) bv[g][n] = vq ? src[16 * n] : 0.f;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int n = 0; n < KT; ++n) acc[g & 1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g], bv[g][n], acc[g & 1][n], 0, 0, 0);
    }
    float *out = j.part + (size_t)blockIdx.x * 9 * k * k;
#pragma unroll
    for (int n = 0; n < KT; ++n)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            out[((size_t)(at * 16 + 4 * q + r) * k + n * 16 + r16) * 9 + tap] = acc[0][n][r] + acc[1][n][r];
}

// ---- sums over positions with one channel axis ------------------------------------------------------------------------------
// part[chunk][o(j, c)] = sum_p X[p][c] y_j(p):  WS_BIAS y = 1;  WS_VEC y = vec[p];  WS_CONV1 y_j = x[2 p - 2 + 2 tap_j], j < 9,
// y_9 = 1, o = c 9 + j and 9 k + c (conv1.weight, conv1.bias)
enum { WS_BIAS = 0, WS_VEC = 1, WS_CONV1 = 2 };
struct WsumJob {
    const float *X;                      // [total][k]
    const float *vec;                    // WS_VEC: [total]; WS_CONV1: x [B][2 hs][2 ws]
    float *part;
    int mode, hs, ws, chunk, chunks;
    long long total;
};
struct WsumArgs {
    WsumJob job[7];
    int k;
};

__global__ __launch_bounds__(GT) void fcn_wsum_kernel(WsumArgs p) {
    __shared__ float red[10 * GT];
    const WsumJob &j = p.job[blockIdx.y];
    if ((int)blockIdx.x >= j.chunks) return;
    const int tid = threadIdx.x, c16 = tid & 15, grp = tid >> 4, nj = j.mode == WS_CONV1 ? 10 : 1;
    const long long p0 = (long long)blockIdx.x * j.chunk;
    const int per = j.hs * j.ws;
    float *out = j.part + (size_t)blockIdx.x * nj * p.k;
    // the 16 lanes of a group take the channels of a tile, group g the positions g, g + 16, ... of the chunk in index order;
    // then the groups' sums in index order
    for (int ct = 0; ct < p.k; ct += 16) {
        float acc[10];
#pragma unroll
        for (int jj = 0; jj < 10; ++jj) acc[jj] = 0.f;
#pragma unroll 2
        for (int i = grp; i < j.chunk; i += 16) {
            const long long pos = p0 + i;
            if (pos < j.total) {
                const float xv = j.X[(size_t)pos * p.k + ct + c16];
                if (j.mode == WS_CONV1) {
                    const int b = (int)(pos / per), r = (int)(pos - (long long)b * per), yy = r / j.ws, xx = r - yy * j.ws;
                    const float *img = j.vec + (size_t)b * 4 * per;
#pragma unroll
                    for (int jj = 0; jj < 9; ++jj) {
                        const int sy = 2 * yy - 2 + 2 * (jj / 3), sx = 2 * xx - 2 + 2 * (jj % 3);
                        const float y = sy >= 0 && sy < 2 * j.hs && sx >= 0 && sx < 2 * j.ws ? img[sy * 2 * j.ws + sx] : 0.f;
                        acc[jj] = fmaf(xv, y, acc[jj]);
                    }
                    acc[9] += xv;
                } else {
                    acc[0] = fmaf(xv, j.mode == WS_VEC ? j.vec[pos] : 1.f, acc[0]);
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < 10; ++jj)
            if (jj < nj) red[jj * GT + tid] = acc[jj];
        __syncthreads();
        if (tid < 16 * nj) {
            const int jj = tid >> 4, c = ct + c16;
            float tot = 0.f;
            for (int g = 0; g < 16; ++g) tot += red[jj * GT + g * 16 + c16];
            out[j.mode == WS_CONV1 ? (jj < 9 ? c * 9 + jj : 9 * p.k + c) : c] = tot;
        }
        __syncthreads();
    }
}

// ---- the chunk partials into the flat gradient ------------------------------------------------------------------------------
struct ReduceSeg {
    const float *src;                    // [chunks][n]
    long long n, dst;                    // dst: where the segment begins in grad
    int chunks;
};
struct ReduceArgs {
    ReduceSeg seg[13];
    float *grad;
    long long total;
};

// 64 elements a workgroup; wave g adds the g-th quarter of an element's chunks in index order, then the quarters in order
__global__ __launch_bounds__(GT) void fcn_reduce_kernel(ReduceArgs p) {
    __shared__ float red[GT];
    const int tid = threadIdx.x, g = tid >> 6;
    const long long i = (long long)blockIdx.x * 64 + (tid & 63);
    float tot = 0.f;
    if (i < p.total) {
        int s = 0;
        while (s < 12 && i >= p.seg[s].dst + p.seg[s].n) ++s;     // the segments lie in the order of grad and cover it
        const ReduceSeg &sg = p.seg[s];
        const long long e = i - sg.dst;
        const int quarter = (sg.chunks + 3) / 4, end = (g + 1) * quarter < sg.chunks ? (g + 1) * quarter : sg.chunks;
        for (int c = g * quarter; c < end; ++c) tot += sg.src[(size_t)c * sg.n + e];
    }
    red[tid] = tot;
    __syncthreads();
    if (g == 0 && i < p.total) p.grad[i] = ((red[tid] + red[tid + 64]) + red[tid + 128]) + red[tid + 192];
}

// ---- torch.optim.Adam ---------------------------------------------------------------------------------------------------
struct AdamArgs {
    float *theta, *m, *v;
    const float *grad;
    long long n;
    int *step;                           // [0] the updates done, [1] the ticket
    double lr, beta1, beta2;
    float eps;
};

// t = step[0] + 1;  m += (g - m) (1 - beta1);  v = beta2 v + (1 - beta2) g g;
// theta -= (lr / (1 - beta1^t)) (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)): the two corrections in float64, rounded once
__global__ __launch_bounds__(GT) void fcn_adam_kernel(AdamArgs p) {
    __shared__ float coef[2];
    if (threadIdx.x == 0) {
        const int t = __hip_atomic_load(p.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        coef[0] = (float)(p.lr / (1.0 - pow(p.beta1, (double)t)));
        coef[1] = (float)sqrt(1.0 - pow(p.beta2, (double)t));
    }
    __syncthreads();
    const long long i = (long long)blockIdx.x * GT + threadIdx.x;
    if (i < p.n) {
        const float g = p.grad[i], w1 = (float)(1.0 - p.beta1), b2 = (float)p.beta2, w2 = (float)(1.0 - p.beta2);
        const float m = p.m[i] + (g - p.m[i]) * w1;
        const float v = b2 * p.v[i] + w2 * (g * g);
        p.m[i] = m;
        p.v[i] = v;
        const float denom = sqrtf(v) / coef[1] + p.eps;
        p.theta[i] = p.theta[i] - coef[0] * (m / denom);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // every workgroup has read step[0] before it takes its ticket; the last one advances the count and re-arms
        const int ticket = __hip_atomic_fetch_add(p.step + 1, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == (int)gridDim.x - 1) {
            __hip_atomic_store(p.step, __hip_atomic_load(p.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.step + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
hipError_t launch_gemm(const float *in, int hi, int wi, float *out, int ho, int wo, int B, int k, Geo g, const float *W, bool ci_slow,
                       const float *bias, const float *mask, hipStream_t stream) {
    GemmArgs a{};
    a.in = in; a.out = out; a.W = W; a.bias = bias; a.mask = mask;
    a.s_in = ci_slow ? 9 * k : 9;
    a.s_out = ci_slow ? 9 : 9 * k;
    a.k = k; a.hi = hi; a.wi = wi; a.ho = ho; a.wo = wo; a.g = g;
    a.class_w = wo / g.s;
    a.class_pos = (ho / g.s) * a.class_w;
    a.tiles_class = (a.class_pos + 15) / 16;
    a.tiles_sample = a.tiles_class * g.s * g.s;
    a.tiles = a.tiles_sample * B;
    a.tpc = k <= 32 ? 9 : 3;
    const int groups = (a.tiles + GW - 1) / GW, blocks = groups < GEMM_MAX_BLOCKS ? groups : GEMM_MAX_BLOCKS;
    const int lds = a.tpc * k * (k + 4) * (int)sizeof(float);
    switch (k / 16) {
    case 1: return launch_kernel(fcn_gemm_kernel<1>, dim3(blocks), dim3(GT), lds, stream, a);
    case 2: return launch_kernel(fcn_gemm_kernel<2>, dim3(blocks), dim3(GT), lds, stream, a);
    case 3: return launch_kernel(fcn_gemm_kernel<3>, dim3(blocks), dim3(GT), lds, stream, a);
    default: return launch_kernel(fcn_gemm_kernel<4>, dim3(blocks), dim3(GT), lds, stream, a);
    }
}

hipError_t launch_forward(const icnn_be_fcn_args &d, bool with_t, bool train, hipStream_t stream) {
    const Shape s(d.batch, d.H, d.W, d.k);
    const Work w(d, s);
    const int k = s.k;
    float *h[6];
    for (int i = 0; i < 6; ++i) h[i] = w.at(ICNN_BE_FCN_W_H + i);
    Conv1Args c{d.x, d.theta + s.wat[0], d.theta + s.bat[0], h[0], s.H, s.W, k, s.pos[0] * k};
    hipError_t e = launch_kernel(fcn_conv1_kernel, dim3((unsigned)((c.n + GT - 1) / GT)), dim3(GT), 0, stream, c);
    for (int l = 1; l <= 5 && e == hipSuccess; ++l)
        e = launch_gemm(h[l - 1], s.h[l - 1], s.w[l - 1], h[l], s.h[l], s.w[l], s.B, k, l <= 2 ? CONV_FWD : UP_FWD, d.theta + s.wat[l],
                        l > 2, d.theta + s.bat[l], nullptr, stream);
    if (e != hipSuccess) return e;
    HeadArgs a{};
    a.h = h[5]; a.w = d.theta + s.wat[6]; a.b = d.theta + s.bat[6];
    a.t = with_t ? d.t : nullptr;
    a.yhat = d.yhat;
    a.dy = with_t && train ? w.at(ICNN_BE_FCN_W_DY) : nullptr;
    a.dz = with_t && train ? w.at(ICNN_BE_FCN_W_DZ + 5) : nullptr;
    a.n = s.pos[5]; a.k = k;
    a.scale = d.pixel_scale;
    a.coef = (float)(2.0 * (double)d.pixel_scale / (double)s.pos[5]);
    a.partial = reinterpret_cast<double *>(w.at(ICNN_BE_FCN_W_LPART));
    a.ticket = reinterpret_cast<int *>(w.at(ICNN_BE_FCN_W_CTL));
    a.loss = d.loss;
    a.dbias = with_t && train ? w.at(ICNN_BE_FCN_W_CTL) + 1 : nullptr;
    return launch_kernel(fcn_head_kernel, dim3(head_blocks(s)), dim3(GT), 0, stream, a);
}

hipError_t launch_backward(const icnn_be_fcn_args &d, hipStream_t stream) {
    const Shape s(d.batch, d.H, d.W, d.k);
    const Work w(d, s);
    hipError_t e = hipSuccess;
    // the delta of layer l from that of layer l + 1 and its weights, masked by layer l's stored output
    for (int l = 4; l >= 0 && e == hipSuccess; --l)
        e = launch_gemm(w.at(ICNN_BE_FCN_W_DZ + l + 1), s.h[l + 1], s.w[l + 1], w.at(ICNN_BE_FCN_W_DZ + l), s.h[l], s.w[l], s.B, s.k,
                        l + 1 <= 2 ? CONV_DGRAD : UP_DGRAD, d.theta + s.wat[l + 1], l + 1 <= 2, nullptr, w.at(ICNN_BE_FCN_W_H + l), stream);
    return e;
}

hipError_t launch_grads(const icnn_be_fcn_args &d, hipStream_t stream) {
    const Shape s(d.batch, d.H, d.W, d.k);
    const Work w(d, s);
    const PartAt pa = part_at(s);
    float *part = w.at(ICNN_BE_FCN_W_WPART);
    const int k = s.k;
    auto H = [&](int i) { return w.at(ICNN_BE_FCN_W_H + i); };
    auto D = [&](int i) { return w.at(ICNN_BE_FCN_W_DZ + i); };
    WgradArgs g{};
    g.k = k;
    int most = 0;
    for (int l = 1; l <= 5; ++l) {
        WgradJob &j = g.job[l - 1];
        const bool conv = l <= 2;
        // conv: dW[co][ci][t] = sum_o dz[o][co] in[2 o - 2 + 2 t][ci];  transposed: dW[ci][co][t] = sum_i in[i][ci] dz[2 i - 1 + t][co]
        j.P = conv ? D(l) : H(l - 1);
        j.Q = conv ? H(l - 1) : D(l);
        j.part = part + pa.w[l];
        j.hs = conv ? s.h[l] : s.h[l - 1];
        j.ws = conv ? s.w[l] : s.w[l - 1];
        j.c = conv ? -2 : -1;
        j.d = conv ? 2 : 1;
        j.total = wgrad_pos(s, l);
        j.chunk = chunk_len(j.total);
        j.chunks = chunks_of(j.total);
        most = j.chunks > most ? j.chunks : most;
    }
    const dim3 grid(most, 9 * (k / 16), 5);
    hipError_t e;
    switch (k / 16) {
    case 1: e = launch_kernel(fcn_wgrad_kernel<1>, grid, dim3(64), 0, stream, g); break;
    case 2: e = launch_kernel(fcn_wgrad_kernel<2>, grid, dim3(64), 0, stream, g); break;
    case 3: e = launch_kernel(fcn_wgrad_kernel<3>, grid, dim3(64), 0, stream, g); break;
    default: e = launch_kernel(fcn_wgrad_kernel<4>, grid, dim3(64), 0, stream, g); break;
    }
    if (e != hipSuccess) return e;
    WsumArgs u{};
    u.k = k;
    most = 0;
    auto sum_job = [&](int at, const float *X, const float *vec, float *out, int mode, int hs, int ws, long long total) {
        u.job[at] = WsumJob{X, vec, out, mode, hs, ws, chunk_len(total), chunks_of(total), total};
        most = u.job[at].chunks > most ? u.job[at].chunks : most;
    };
    sum_job(0, D(0), d.x, part + pa.conv1, WS_CONV1, s.h[0], s.w[0], s.pos[0]);
    for (int l = 1; l <= 5; ++l) sum_job(l, D(l), nullptr, part + pa.b[l], WS_BIAS, s.h[l], s.w[l], s.pos[l]);
    sum_job(6, H(5), w.at(ICNN_BE_FCN_W_DY), part + pa.up4, WS_VEC, s.h[5], s.w[5], s.pos[5]);
    if (e = launch_kernel(fcn_wsum_kernel, dim3(most, 7), dim3(GT), 0, stream, u); e != hipSuccess) return e;
    ReduceArgs r{};
    r.grad = d.grad;
    r.total = s.n;
    r.seg[0] = ReduceSeg{part + pa.conv1, 10LL * k, 0, u.job[0].chunks};
    for (int l = 1; l <= 5; ++l) {
        r.seg[2 * l - 1] = ReduceSeg{part + pa.w[l], 9LL * k * k, s.wat[l], g.job[l - 1].chunks};
        r.seg[2 * l] = ReduceSeg{part + pa.b[l], k, s.bat[l], u.job[l].chunks};
    }
    r.seg[11] = ReduceSeg{part + pa.up4, k, s.wat[6], u.job[6].chunks};
    r.seg[12] = ReduceSeg{w.at(ICNN_BE_FCN_W_CTL) + 1, 1, s.bat[6], 1};
    return launch_kernel(fcn_reduce_kernel, dim3((unsigned)((s.n + 63) / 64)), dim3(GT), 0, stream, r);
}

hipError_t launch_update(const icnn_be_fcn_args &d, hipStream_t stream) {
    const Shape s(d.batch > 0 ? d.batch : 1, d.H, d.W, d.k);
    AdamArgs a{d.theta, d.m, d.v, d.grad, s.n, d.step, d.lr, d.beta1, d.beta2, d.eps};
    return launch_kernel(fcn_adam_kernel, dim3((unsigned)((s.n + GT - 1) / GT)), dim3(GT), 0, stream, a);
}

// what an entry needs beyond the sizes
enum : unsigned { N_TRAIN = 1, N_X = 2, N_T = 4, N_YHAT = 8, N_LOSS = 16, N_GRAD = 32, N_ADAM = 64, N_WORK = 128, N_THETA = 256 };

int check(const icnn_be_fcn_args *a, void *stream, unsigned need) {
    if (!a || !sizes_ok(a->H, a->W, a->k)) return ICNN_BE_EINVAL;
    if (a->batch < 1 || a->batch > ((need & N_TRAIN) ? ICNN_BE_FCN_MAX_BATCH : ICNN_BE_FCN_MAX_EVAL_BATCH)) return ICNN_BE_EINVAL;
    if (!stream_ok(stream)) return ICNN_BE_EINVAL;
    if ((need & N_THETA) && misaligned(a->theta, 16)) return ICNN_BE_EINVAL;
    if ((need & N_WORK) && misaligned(a->work, 16)) return ICNN_BE_EINVAL;
    if ((need & N_X) && misaligned(a->x, 4)) return ICNN_BE_EINVAL;
    if ((need & N_T) && misaligned(a->t, 4)) return ICNN_BE_EINVAL;
    if ((need & N_YHAT) && misaligned(a->yhat, 4)) return ICNN_BE_EINVAL;
    if ((need & N_LOSS) && (misaligned(a->loss, 4) || !(a->pixel_scale > 0.f) || !std::isfinite(a->pixel_scale))) return ICNN_BE_EINVAL;
    if ((need & N_GRAD) && misaligned(a->grad, 16)) return ICNN_BE_EINVAL;
    if (need & N_ADAM) {
        if (misaligned(a->m, 16) || misaligned(a->v, 16) || misaligned(a->step, 4)) return ICNN_BE_EINVAL;
        if (!adam_constants_ok(a->beta1, a->beta2, a->eps) || !std::isfinite(a->lr)) return ICNN_BE_EINVAL;
    }
    return 0;
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_fcn_param_floats(int H, int W, int k, long long *n) {
    if (!sizes_ok(H, W, k) || !n) return ICNN_BE_EINVAL;
    *n = Shape(1, H, W, k).n;
    return 0;
}

size_t icnn_be_fcn_work_bytes(int batch, int H, int W, int k) {
    if (batch < 1 || batch > ICNN_BE_FCN_MAX_EVAL_BATCH || !sizes_ok(H, W, k)) return 0;
    return work_walk(Shape(batch, H, W, k), nullptr) * sizeof(float);
}

int icnn_be_fcn_work_offsets(int batch, int H, int W, int k, long long off[ICNN_BE_FCN_WORK_PIECES]) {
    if (batch < 1 || batch > ICNN_BE_FCN_MAX_EVAL_BATCH || !sizes_ok(H, W, k) || !off) return ICNN_BE_EINVAL;
    work_walk(Shape(batch, H, W, k), off);
    return 0;
}

int icnn_be_fcn_forward(const icnn_be_fcn_args *a, void *stream) {
    const bool with_t = a && a->t;
    if (int rc = check(a, stream, N_THETA | N_X | N_YHAT | N_WORK | (with_t ? N_TRAIN | N_T | N_LOSS : 0u))) return rc;
    return api_done(launch_forward(*a, with_t, true, static_cast<hipStream_t>(stream)));
}

int icnn_be_fcn_backward(const icnn_be_fcn_args *a, void *stream) {
    if (int rc = check(a, stream, N_TRAIN | N_THETA | N_WORK)) return rc;
    return api_done(launch_backward(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_fcn_grads(const icnn_be_fcn_args *a, void *stream) {
    if (int rc = check(a, stream, N_TRAIN | N_X | N_WORK | N_GRAD)) return rc;
    return api_done(launch_grads(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_fcn_update(const icnn_be_fcn_args *a, void *stream) {
    if (int rc = check(a, stream, N_THETA | N_GRAD | N_ADAM)) return rc;
    return api_done(launch_update(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_fcn_step(const icnn_be_fcn_args *a, void *stream) {
    if (int rc = check(a, stream, N_TRAIN | N_THETA | N_X | N_T | N_YHAT | N_LOSS | N_GRAD | N_ADAM | N_WORK)) return rc;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_forward(*a, true, true, s);
    if (e == hipSuccess) e = launch_backward(*a, s);
    if (e == hipSuccess) e = launch_grads(*a, s);
    if (e == hipSuccess) e = launch_update(*a, s);
    return api_done(e);
}

int icnn_be_fcn_eval(const icnn_be_fcn_args *a, void *stream) {
    if (int rc = check(a, stream, N_THETA | N_X | N_T | N_YHAT | N_LOSS | N_WORK)) return rc;
    return api_done(launch_forward(*a, true, false, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
