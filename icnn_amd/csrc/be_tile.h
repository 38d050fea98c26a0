// The tile routines that the per-sample chain kernels share (be_ddpg.hip, be_naf.hip, be_naf_bn.hip): one workgroup of DT threads works on
// a tile of TS samples whose activations lie in LDS.  Device code only; each translation unit gets its own copy.
#pragma once
#include "be_kernels.h"

namespace icnn_be {

namespace {

constexpr int DT = 512;                  // 8 waves; tile_dot splits them into 16 groups of 32 lanes, one per sample
constexpr int TS = 16;                   // samples per tile
static_assert(DT == 32 * TS, "tile_dot: one group of 32 lanes per sample");

struct Net {
    const float *W1, *b1, *W2, *b2, *W3, *b3;
};
__device__ __forceinline__ Net policy_net(const float *t, int dimO, int dimA, int l1, int l2) {
    Net n;
    n.W1 = t;
    n.b1 = n.W1 + (size_t)dimO * l1;
    n.W2 = n.b1 + l1;
    n.b2 = n.W2 + (size_t)l1 * l2;
    n.W3 = n.b2 + l2;
    n.b3 = n.W3 + (size_t)l2 * dimA;
    return n;
}

// epi(s, j, sum_{k < K} in[s][k] Bm(k, j)) for the 16 rows s of the tile and j < N;  Bm(k, j) = W[k sk + j sj].
// in: LDS, row pitch pin >= K rounded up to 16.  Every wave calls it; no barrier inside.
template <typename Epi>
__device__ __forceinline__ void tile_gemm(const float *in, int pin, int K, const float *W, long long sk, long long sj, int N, Epi epi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
    const int NT = (N + 15) >> 4;
    for (int nt = 2 * wave; nt < NT; nt += 2 * (DT / 64)) {
        const int c0 = nt * 16 + r16, c1 = c0 + 16;
        const bool v0 = c0 < N, v1 = c1 < N;
        const float *w0 = W + (long long)c0 * sj, *w1 = W + (long long)c1 * sj;
        f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < K; k0 += 16) {
            const int kb = k0 + 4 * q;
            const f4 av = *reinterpret_cast<const f4 *>(in + r16 * pin + kb);
            float af[4], b0[4], b1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = kb + j;
                const bool ok = kk < K;
                af[j] = ok ? av[j] : 0.f;
                b0[j] = ok && v0 ? w0[(long long)kk * sk] : 0.f;
                b1[j] = ok && v1 ? w1[(long long)kk * sk] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b0[j], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b1[j], acc1, 0, 0, 0);
            }
        }
        // acc[r] = C[row 4 q + r][column r16 of the tile]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (v0) epi(4 * q + r, c0, acc0[r]);
            if (v1) epi(4 * q + r, c1, acc1[r]);
        }
    }
}

// sum_k in[s][k] w[k] for s = tid / 32, in every lane of that group; a fixed order
__device__ __forceinline__ float tile_dot(const float *in, int pin, int K, const float *w) {
    const int s = threadIdx.x >> 5, l = threadIdx.x & 31;
    float acc = 0.f;
    for (int k = l; k < K; k += 32) acc = fmaf(in[s * pin + k], w[k], acc);
    for (int off = 16; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// the rows of this tile: s0 the first sample, rows how many of the 16 exist
struct Tile {
    int s0, rows;
};

// dst[s][c0 + c] = src[s0 + s][c], zero in the rows past the batch
template <typename T>
__device__ __forceinline__ void load_rows(float *dst, int pitch, int c0, const T *src, int width, Tile t) {
    for (int i = threadIdx.x; i < TS * width; i += DT) {
        const int s = i / width, c = i - s * width;
        dst[s * pitch + c0 + c] = s < t.rows ? (float)src[(size_t)(t.s0 + s) * width + c] : 0.f;
    }
}

// out[s][oc0 + j] = relu(in[s] . W[:, j] + b[j]) into LDS, and into g[s0 + s][gc0 + j] (pitch gw) where g is not NULL
__device__ __forceinline__ void layer_relu(const float *in, int pin, int K, const float *W, const float *b, int N, float *out, int pout,
                                           float *g, int gw, Tile t) {
    tile_gemm(in, pin, K, W, N, 1, N, [&](int s, int j, float acc) {
        float v = acc + b[j];
        v = v > 0.f ? v : 0.f;
        out[s * pout + j] = v;
        if (g && s < t.rows) g[(size_t)(t.s0 + s) * gw + j] = v;
    });
}

// out[s][j] = tanh(in[s] . W[:, j] + b[j]), likewise
__device__ __forceinline__ void layer_tanh(const float *in, int pin, int K, const float *W, const float *b, int N, float *out, int pout,
                                           float *g, Tile t) {
    tile_gemm(in, pin, K, W, N, 1, N, [&](int s, int j, float acc) {
        const float v = tanhf(acc + b[j]);
        if (out) out[s * pout + j] = v;
        if (s < t.rows) g[(size_t)(t.s0 + s) * N + j] = v;
    });
}

// the pitch of an LDS row buffer that holds w values: a multiple of 16 for tile_gemm's reads, plus 4 against bank conflicts
inline int pitch_of(int w) { return ((w + 15) & ~15) + 4; }
inline int max2(int x, int y) { return x > y ? x : y; }

}  // namespace

}  // namespace icnn_be
