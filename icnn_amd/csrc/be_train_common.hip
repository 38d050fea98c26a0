// Kernels shared by the training gradients of the models (be_train_fc.hip, be_train_ficnn.hip, be_train_conv.hip, DESIGN.md
// §8-9): the ONE f32-MFMA GEMM on strided operands that every product of a step runs through -- split-K with a fixed-order
// second pass, no atomics, so a gradient is the same bits on every run and a whole entry can be captured in a graph -- the
// per-row bookkeeping of the feed, and the small helpers of a step: the stacked y-path weight out of its packed fragments,
// zero fill and the bias column sums.
#include <hip/hip_runtime.h>

#include "be_train_common.h"

namespace icnn_be {

namespace {

constexpr int GBM = 64, GBN = 64, GBK = 16, GT_ = 256, GPITCH = GBK + 4;

// split-K plan: enough splits that a small output still fills the device
__host__ __device__ inline void gemm_splits(int M, int N, int K, int &splits, int &kchunk) {
    const int tiles = ((M + GBM - 1) / GBM) * ((N + GBN - 1) / GBN);
    splits = 1;
    if (tiles < 256 && K > 64) {
        splits = (256 + tiles - 1) / tiles;
        const int most = (K + 63) / 64;
        if (splits > most) splits = most;
        if (splits > 32) splits = 32;
    }
    kchunk = (K + splits - 1) / splits;
    kchunk = (kchunk + GBK - 1) / GBK * GBK;
    if (kchunk < GBK) kchunk = GBK;
    splits = K > 0 ? (K + kchunk - 1) / kchunk : 1;
}
// the most splits any plan of this K has
inline int gemm_max_splits(int K) { return K > 64 ? ((K + 63) / 64 < 32 ? (K + 63) / 64 : 32) : 1; }
// The plan of a product whose row count lives on the device (rows_dev != NULL): that of the compact call, which has
// m_per_row x *rows_dev rows -- the same chunks of k summed in the same order, so the rows both calls share get the same bits
__device__ __forceinline__ void gemm_dev_plan(const int *rows_dev, int m_per_row, int M, int N, int K, int &splits, int &kchunk) {
    const long long m = (long long)m_per_row * max(*rows_dev, 0);
    gemm_splits((int)(m < 1 ? 1 : (m < M ? m : M)), N, K, splits, kchunk);
}

// C_part[split][M][N] = sum over k in split's chunk of A(m, k) B(k, n); A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn]
struct TrGemmArgs {
    const float *A, *B;
    long long sam, sak, sbk, sbn;
    int M, N, K, kchunk;
    float *part;
    const int *rows_dev;     // not NULL: gemm_dev_plan; the grid has gemm_max_splits(K) slices, the surplus ones leave
    int m_per_row;
};

__global__ __launch_bounds__(GT_) void tr_gemm_kernel(TrGemmArgs a) {
    __shared__ __attribute__((aligned(16))) float As[GBM][GPITCH];
    __shared__ __attribute__((aligned(16))) float Bt[GBN][GPITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, q = lane >> 4;
    const int m0 = blockIdx.x * GBM, n0 = blockIdx.y * GBN;
    int kchunk = a.kchunk;
    if (a.rows_dev) {
        int splits;
        gemm_dev_plan(a.rows_dev, a.m_per_row, a.M, a.N, a.K, splits, kchunk);
        if ((int)blockIdx.z >= splits) return;
    }
    const int k_beg = blockIdx.z * kchunk, k_end = min(a.K, k_beg + kchunk);
    const bool a_kfast = a.sak == 1, b_nfast = a.sbn == 1;    // walk the unit-stride index across neighbouring lanes
    f4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = k_beg; k0 < k_end; k0 += GBK) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int e = tid + GT_ * p;
            const int ar = a_kfast ? e >> 4 : e & 63, ak = a_kfast ? e & 15 : e >> 6;
            const int m = m0 + ar, k = k0 + ak;
            As[ar][ak] = (m < a.M && k < k_end) ? a.A[(size_t)m * a.sam + (size_t)k * a.sak] : 0.f;
            const int bc = b_nfast ? e & 63 : e >> 4, bk = b_nfast ? e >> 6 : e & 15;
            const int n = n0 + bc, kb = k0 + bk;
            Bt[bc][bk] = (n < a.N && kb < k_end) ? a.B[(size_t)kb * a.sbk + (size_t)n * a.sbn] : 0.f;
        }
        __syncthreads();
        const f4 af = *reinterpret_cast<const f4 *>(&As[16 * wave + r16][4 * q]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f4 bf = *reinterpret_cast<const f4 *>(&Bt[16 * t + r16][4 * q]);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af.x, bf.x, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af.y, bf.y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af.z, bf.z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af.w, bf.w, acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
    // acc[t][r] = C[m0 + 16 wave + 4 q + r][n0 + 16 t + r16]
    float *out = a.part + (size_t)blockIdx.z * a.M * a.N;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = n0 + 16 * t + r16;
        if (col >= a.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + 16 * wave + 4 * q + r;
            if (row < a.M) out[(size_t)row * a.N + col] = acc[t][r];
        }
    }
}

// second pass: C[m][n] (pitch ldc) = sum_s part[s][m][n], splits in order
__global__ void tr_gemm_reduce_kernel(const float *part, int splits, int M, int N, float *C, long long ldc, int K,
                                      const int *rows_dev, int m_per_row) {
    const size_t total = (size_t)M * N;
    if (rows_dev) {
        int kchunk;
        gemm_dev_plan(rows_dev, m_per_row, M, N, K, splits, kchunk);
    }
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float s = part[i];
        for (int sp = 1; sp < splits; ++sp) s += part[(size_t)sp * total + i];
        const size_t m = i / N, n = i - m * N;
        C[m * ldc + n] = s;
    }
}

// Row bookkeeping: samp[r] = the sample whose segment [row_offset[j], row_offset[j+1]) holds r (binary search, clamped to
// 0..B-1 whatever row_offset holds), mult[j] = its row count as a float (the BatchNorm weight)
__global__ void tr_rows_kernel(const int *row_offset, int B, int R, int *samp, float *mult) {
    const int total = R > B ? R : B;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        if (i < R) {
            int lo = 0, hi = B - 1;             // last j with row_offset[j] <= i
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (row_offset[mid] <= i) lo = mid; else hi = mid - 1;
            }
            samp[i] = lo;
        }
        if (i < B) {
            const int a = min(max(row_offset[i], 0), R), b = min(max(row_offset[i + 1], 0), R);
            mult[i] = b > a ? (float)(b - a) : 0.f;
        }
    }
}

// dctx[j][col] = sum of the rows of sample j, in row order
__global__ void tr_segment_sum_kernel(const float *rows, const int *row_offset, int B, int R, int C, float *out) {
    const size_t total = (size_t)B * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i / C), col = (int)(i - (size_t)j * C);
        const int r0 = min(max(row_offset[j], 0), R), r1 = min(max(row_offset[j + 1], 0), R);
        float s = 0.f;
        for (int r = r0; r < r1; ++r) s += rows[(size_t)r * C + col];
        out[i] = s;
    }
}

// The y-path weights of a layer out of the packed fragments (both orientations are there; the forward one is read):
// dst[(n + wprev)][w] = [ Wy ; Wz ] row-major; last: the width-1 head, whose two operands are plain vectors
struct UnpackArgs {
    const float *wpack;
    long long yf, zf;
    int n, wprev, w, last;
    float *dst;
};
__global__ void tr_unpack_kernel(UnpackArgs a) {
    const int rows = a.n + a.wprev, total = rows * a.w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int k = i / a.w, col = i - k * a.w;
        float v;
        if (a.last) v = k < a.n ? a.wpack[a.yf + k] : a.wpack[a.zf + (k - a.n)];
        else v = k < a.n ? frag_at(a.wpack + a.yf, a.w, k, col) : frag_at(a.wpack + a.zf, a.w, k - a.n, col);
        a.dst[i] = v;
    }
}

__global__ void tr_zero_kernel(float *p, size_t count) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) p[i] = 0.f;
}

// out[col] = sum_j m[j][c0 + col], rows in order
__global__ void tr_colsum_kernel(const float *m, int ld, int B, int c0, int N, float *out) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= N) return;
    float s = 0.f;
    for (int j = 0; j < B; ++j) s += m[(size_t)j * ld + c0 + col];
    out[col] = s;
}

}  // namespace

size_t tr_gemm_part_floats(int M, int N, int K, bool dev_plan) {
    if (M <= 0 || N <= 0) return 0;
    int splits, kchunk;
    gemm_splits(M, N, K, splits, kchunk);
    if (dev_plan) splits = gemm_max_splits(K);
    return (size_t)splits * M * N;
}

hipError_t launch_tr_gemm(const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, int M, int N,
                          int K, float *C, long long ldc, float *part, hipStream_t stream, const int *rows_dev, int m_per_row) {
    if (M <= 0 || N <= 0) return hipSuccess;
    int splits, kchunk;
    gemm_splits(M, N, K, splits, kchunk);
    if (rows_dev) splits = gemm_max_splits(K);
    TrGemmArgs a{A, B, sam, sak, sbk, sbn, M, N, K, kchunk, part, rows_dev, m_per_row};
    hipError_t e = launch_kernel(tr_gemm_kernel, dim3((M + GBM - 1) / GBM, (N + GBN - 1) / GBN, splits), dim3(GT_), 0, stream, a);
    if (e == hipSuccess)
        e = launch_kernel(tr_gemm_reduce_kernel, dim3(grid_for((size_t)M * N)), dim3(256), 0, stream, (const float *)part, splits,
                          M, N, C, ldc, K, rows_dev, m_per_row);
    return e;
}

hipError_t launch_tr_rows(const int *row_offset, int B, int R, int *samp, float *mult, hipStream_t stream) {
    return launch_kernel(tr_rows_kernel, dim3(grid_for(R > B ? R : B)), dim3(256), 0, stream, row_offset, B, R, samp, mult);
}

hipError_t launch_tr_segment_sum(const float *rows, const int *row_offset, int B, int R, int C, float *out, hipStream_t stream) {
    return launch_kernel(tr_segment_sum_kernel, dim3(grid_for((size_t)B * C)), dim3(256), 0, stream, rows, row_offset, B, R, C,
                         out);
}

hipError_t launch_tr_unpack(const float *wpack, long long yf, long long zf, int n, int wprev, int w, bool last, float *dst,
                            hipStream_t stream) {
    UnpackArgs a{wpack, yf, zf, n, wprev, w, last ? 1 : 0, dst};
    return launch_kernel(tr_unpack_kernel, dim3(grid_for((size_t)(n + wprev) * w)), dim3(256), 0, stream, a);
}

hipError_t launch_tr_zero(float *p, size_t count, hipStream_t stream) {
    return launch_kernel(tr_zero_kernel, dim3(grid_for(count)), dim3(256), 0, stream, p, count);
}

hipError_t launch_tr_colsum(const float *m, int ld, int B, int c0, int N, float *out, hipStream_t stream) {
    return launch_kernel(tr_colsum_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, m, ld, B, c0, N, out);
}

}  // namespace icnn_be
