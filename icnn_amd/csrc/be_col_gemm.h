// The column-owning product of the kernels that cross the samples of a batch (be_ff.hip, be_naf_bn.hip): a
// workgroup of FT threads owns FC columns of a layer's output for ALL rows it is given, so that every cross-sample quantity is
// a column statistic inside one workgroup.  Device code only; each translation unit gets its own copy.
//
// The product (col_gemm): the wave w owns the 16-row tiles w, w + 8, ... of the workgroup's rows; K is streamed in chunks of
// 128, 64 or 32 (the longest whose rows fit 72 KB): all threads stage the rows' chunk [rows][chunk] and the weight block's
// chunk [FC][chunk] (k fastest) in LDS, so all workgroups together read W once.  The global loads of the next chunk are issued
// in front of the products of this one and written to LDS behind them.  mfma_f32_16x16x4f32 with tile_gemm's operand and
// accumulator layout; two accumulators per tile take the k steps alternately and are added at the end, so a sum's order
// depends on K alone: a row's result has the same bits wherever the row lies in whichever batch, whatever the chunk.
#pragma once
#include "be_kernels.h"

namespace icnn_be {

namespace {

constexpr int FT = 512;                  // 8 waves
constexpr int FWV = FT / 64;
constexpr int FC = 16;                   // columns a workgroup owns
constexpr int FMT = ICNN_BE_FF_MAX_BATCH / 16 / FWV;      // row tiles per wave, at most
constexpr int FSTAGE = 18432;            // floats of a staged chunk of rows, at most: [512][32 + 4]
constexpr int FXQ = FSTAGE / 4 / FT;     // float4 of that chunk per thread
constexpr int FWQ = 4;                   // weight elements of the longest chunk per thread: 16 x 128 / 512
static_assert(FC == 16, "col_gemm splits a thread index by shifts");
static_assert(FT == 32 * FC, "column sums: a group of 32 lanes per column");

// The k of a staged chunk is 1 << kl, the pitch of a staged row 4 more: 128 up to 128 rows, 64 up to 256, 32 up to 512, so
// that a chunk takes at most FSTAGE floats and the few rows of a small batch come in few, long chunks.
__host__ __device__ inline int pad16(int r) { return (r + 15) & ~15; }
inline int ff_chunk_log(int rows) {
    int kl = 7;
    while (kl > 5 && pad16(rows) * ((1 << kl) + 4) > FSTAGE) --kl;
    return kl;
}
// the LDS of one workgroup that holds `rows` rows: the staged chunk, which the epilogue reuses for two column buffers
// [FC][rows16 + 4]; the weight chunk; two floats per column
__host__ __device__ inline int ff_stage_floats(int rows, int kl) {
    const int r16 = pad16(rows), rows_chunk = r16 * ((1 << kl) + 4), columns = 2 * FC * (r16 + 4);
    return rows_chunk > columns ? rows_chunk : columns;
}
__host__ __device__ inline int ff_weight_floats(int kl) { return FC * ((1 << kl) + 4); }
inline int ff_lds_bytes(int rows, int kl) { return (ff_stage_floats(rows, kl) + ff_weight_floats(kl) + 2 * FC) * (int)sizeof(float); }
inline int col_blocks(int n) { return (n + FC - 1) / FC; }

struct Frag {
    f4 t[FMT];
};

// t[i][r] = sum_{k < K} X[row0 + 16 (wave + 8 i) + 4 q + r][k] Bm(k, c0 + r16),  Bm(k, j) = W[k sk + j sj], zero for the
// rows >= row0 + nrows and the columns >= N.  xs, ws: LDS.  Ends behind a barrier: xs is free.
// The loads of chunk c + 1 are issued in front of the products of chunk c and land in LDS behind them.
__device__ __forceinline__ void col_gemm(const float *X, int ldx, int row0, int nrows, int K, const float *W, long long sk,
                                         long long sj, int c0, int N, int kl, float *xs, float *ws, Frag &out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
    const int fk = 1 << kl, fp = fk + 4, tiles = (nrows + 15) >> 4, quads = tiles * 16 * (fk >> 2), welems = FC * fk;
    // whole float4 loads where every row of X starts on 16 bytes and K is a multiple of 4: a quad is then inside or outside
    const bool vec = (K & 3) == 0 && (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    f4 even[FMT], odd[FMT], px[FXQ];
    float pw[FWQ];
#pragma unroll
    for (int i = 0; i < FMT; ++i) even[i] = odd[i] = f4{0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < FXQ; ++s) {
            const int idx = s * FT + tid, r = idx >> (kl - 2), k = k0 + 4 * (idx & ((fk >> 2) - 1));
            f4 v = {0.f, 0.f, 0.f, 0.f};
            if (idx < quads && r < nrows) {
                const float *src = X + (size_t)(row0 + r) * ldx + k;
                if (vec) {
                    if (k < K) v = *reinterpret_cast<const f4 *>(src);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (k + j < K) v[j] = src[j];
                }
            }
            px[s] = v;
        }
#pragma unroll
        for (int s = 0; s < FWQ; ++s) {
            // k fastest in memory where sk == 1, else the column
            const int idx = s * FT + tid, n = sk == 1 ? idx >> kl : idx & (FC - 1), k = k0 + (sk == 1 ? idx & (fk - 1) : idx >> 4);
            pw[s] = idx < welems && c0 + n < N && k < K ? W[(long long)k * sk + (long long)(c0 + n) * sj] : 0.f;
        }
    };
    auto land = [&]() {
#pragma unroll
        for (int s = 0; s < FXQ; ++s) {
            const int idx = s * FT + tid;
            if (idx < quads) *reinterpret_cast<f4 *>(xs + (idx >> (kl - 2)) * fp + 4 * (idx & ((fk >> 2) - 1))) = px[s];
        }
#pragma unroll
        for (int s = 0; s < FWQ; ++s) {
            const int idx = s * FT + tid, n = sk == 1 ? idx >> kl : idx & (FC - 1), k = sk == 1 ? idx & (fk - 1) : idx >> 4;
            if (idx < welems) ws[n * fp + k] = pw[s];
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += fk) {
        land();
        __syncthreads();
        if (k0 + fk < K) fetch(k0 + fk);
        for (int kk = 0; kk < fk; kk += 16) {
            const int kb = kk + 4 * q;
            const f4 bv = *reinterpret_cast<const f4 *>(ws + r16 * fp + kb);
#pragma unroll
            for (int i = 0; i < FMT; ++i) {
                const int tile = wave + FWV * i;
                if (tile < tiles) {
                    const f4 av = *reinterpret_cast<const f4 *>(xs + (tile * 16 + r16) * fp + kb);
                    even[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[0], bv[0], even[i], 0, 0, 0);
                    odd[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[1], bv[1], odd[i], 0, 0, 0);
                    even[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[2], bv[2], even[i], 0, 0, 0);
                    odd[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[3], bv[3], odd[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < FMT; ++i) out.t[i] = even[i] + odd[i];
}

// the sum over the rows < nrows of column tid / 32 of buf [FC][pitch], in every lane of that group: each lane adds its rows
// in index order, a fixed butterfly adds the lanes
__device__ __forceinline__ float column_sum(const float *buf, int pitch, int nrows) {
    const int c = threadIdx.x >> 5, l = threadIdx.x & 31;
    float s = 0.f;
    for (int r = l; r < nrows; r += 32) s += buf[c * pitch + r];
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 32);
    return s;
}

// f(i, r, row) for the accumulator elements of this lane whose row (inside the workgroup) exists
template <typename F>
__device__ __forceinline__ void for_rows(int nrows, F f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
#pragma unroll
    for (int i = 0; i < FMT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (wave + FWV * i) * 16 + 4 * q + r;
            if (row < nrows) f(i, r, row);
        }
}

}  // namespace

}  // namespace icnn_be
