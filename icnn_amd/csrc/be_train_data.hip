// The training set on the device (include/icnn_be.h, icnn_be_dataset_draw and icnn_be_log_row): the one line
// of the supervised training loops that still needed the host, `I = npr.randint(nTrain, size=batch); trainX[I], trainY[I]`
// (multi-label-cls/icnn_ebundle.py:214, icnn-back.py:190, completion/icnn_ebundle.py:210, icnn.back.py:216), and the
// per-iteration scalars they write to train.csv, so that [draw, step, log] x k is one graph with no host data in it.
//
//   dataset_draw_kernel   a minibatch in one launch, ONE WORKGROUP PER SAMPLE (a row of the multi-label set is 7.3 KB, an image
//                         4 KB: four waves keep eight 16-byte loads in flight per row pass).  The index is workgroup-uniform:
//                         the draw counter goes through readfirstlane, the sample number is the workgroup's, so the Philox word,
//                         the index and both row bases are scalar.  Rows of row_words % 4 == 0 move as 16-byte words (the API's
//                         alignment rule makes every such row 16-byte aligned), the others word by word.  Row offsets are 64
//                         bits.  The last workgroup to take a ticket advances the draw counter and re-arms the ticket: every
//                         workgroup has read the counter before it takes its ticket (replay_sample_kernel's scheme).
//   log_row_kernel        one wave: lane j < width widens scalar j to float64 into row cursor % cap, lane 0 advances the cursor.
//
// The index is umulhi(word, N) < N for every 32-bit word and a workgroup exists only for k < batch, so the gather stays inside
// the arrays whatever the control block holds.
#include "be_api_check.h"
#include "be_kernels.h"

namespace icnn_be {

namespace {

constexpr int DRAW_THREADS = 256;
constexpr int LOG_THREADS = 64;
enum { CTRL_DRAWS = 0, CTRL_STATUS = 1, CTRL_TICKET = 2 };

__device__ __forceinline__ int ctrl_load(const int *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// word 0 of Philox4x32-10 (Salmon et al., SC'11) at counter (c0, c1, c2, c3) and key (k0, k1)
__device__ __forceinline__ unsigned philox4x32_10_word0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                        unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

struct DrawArgs {
    icnn_be_dataset d;
    unsigned k0, k1;
    void *dst[ICNN_BE_DATASET_MAX_ARRAYS];
    int *idx;
};

__global__ __launch_bounds__(DRAW_THREADS) void dataset_draw_kernel(DrawArgs a) {
    const int tid = threadIdx.x;
    const unsigned k = blockIdx.x;                                 // the grid is the batch
    const unsigned draws = (unsigned)__builtin_amdgcn_readfirstlane(ctrl_load(a.d.ctrl + CTRL_DRAWS));
    const unsigned word = philox4x32_10_word0(draws, k, 0u, 1u, a.k0, a.k1);
    const long long row = (long long)__builtin_amdgcn_readfirstlane((int)__umulhi(word, (unsigned)a.d.n_rows));
    if (tid == 0) a.idx[k] = (int)row;
#pragma unroll
    for (int i = 0; i < ICNN_BE_DATASET_MAX_ARRAYS; ++i) {         // unrolled: the descriptor's arrays stay kernel arguments
        if (i >= a.d.n_arrays) break;
        const long long words = a.d.row_words[i];
        const unsigned *src = static_cast<const unsigned *>(a.d.src[i]) + row * words;
        unsigned *dst = static_cast<unsigned *>(a.dst[i]) + (long long)k * words;
        if ((words & 3) == 0) {
            const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
            uint4 *d4 = reinterpret_cast<uint4 *>(dst);
            for (long long j = tid; j < (words >> 2); j += DRAW_THREADS) d4[j] = s4[j];
        } else {
            for (long long j = tid; j < words; j += DRAW_THREADS) dst[j] = src[j];
        }
    }
    // the draw counter: the last workgroup to arrive advances it and re-arms the ticket for the next launch
    __syncthreads();
    if (tid == 0) {
        const int ticket = __hip_atomic_fetch_add(a.d.ctrl + CTRL_TICKET, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket < 0 || ticket >= (int)gridDim.x)                // never with one draw of the set in flight at a time
            __hip_atomic_fetch_or(a.d.ctrl + CTRL_STATUS, ICNN_BE_DATASET_ST_STATE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == (int)gridDim.x - 1) {
            __hip_atomic_store(a.d.ctrl + CTRL_DRAWS, (int)(draws + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.d.ctrl + CTRL_TICKET, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ __launch_bounds__(LOG_THREADS) void log_row_kernel(icnn_be_step_log L) {
    const int j = threadIdx.x;
    const unsigned cursor = (unsigned)L.ctrl[0];
    double *row = L.rows + (size_t)(cursor % (unsigned)L.cap) * L.width;
#pragma unroll
    for (int c = 0; c < ICNN_BE_LOG_MAX_COLUMNS; ++c) {            // unrolled: col and kind stay kernel arguments
        if (c != j || c >= L.width) continue;
        const int kind = L.kind[c];
        row[c] = kind == ICNN_BE_LOG_F64   ? *static_cast<const double *>(L.col[c])
                 : kind == ICNN_BE_LOG_F32 ? (double)*static_cast<const float *>(L.col[c])
                                           : (double)*static_cast<const int *>(L.col[c]);
    }
    if (j == 0) L.ctrl[0] = (int)(cursor + 1u);                    // every lane of the one wave has read the cursor
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_dataset_draw(const icnn_be_dataset *d, int batch, unsigned long long seed, void *const dst[], int *idx,
                         void *stream) {
    if (!d || !d->ctrl || !idx || !dst) return ICNN_BE_EINVAL;
    if (d->n_rows < 1 || batch < 1 || d->n_arrays < 1 || d->n_arrays > ICNN_BE_DATASET_MAX_ARRAYS) return ICNN_BE_EINVAL;
    for (int a = 0; a < d->n_arrays; ++a)
        if (misaligned(d->src[a], 16) || misaligned(dst[a], 16) || d->row_words[a] < 1) return ICNN_BE_EINVAL;
    if (misaligned(idx, 16) || misaligned(d->ctrl, 4) || !stream_ok(stream)) return ICNN_BE_EINVAL;
    DrawArgs a{};
    a.d = *d;
    a.k0 = (unsigned)(seed & 0xffffffffull);
    a.k1 = (unsigned)(seed >> 32);
    for (int i = 0; i < d->n_arrays; ++i) a.dst[i] = dst[i];
    a.idx = idx;
    return api_done(launch_kernel(dataset_draw_kernel, dim3((unsigned)batch), dim3(DRAW_THREADS), 0,
                                  static_cast<hipStream_t>(stream), a));
}

int icnn_be_log_row(const icnn_be_step_log *L, void *stream) {
    if (!L || !L->rows || !L->ctrl || L->cap < 1 || L->width < 1 || L->width > ICNN_BE_LOG_MAX_COLUMNS) return ICNN_BE_EINVAL;
    for (int j = 0; j < L->width; ++j) {
        if (L->kind[j] < ICNN_BE_LOG_F32 || L->kind[j] > ICNN_BE_LOG_I32) return ICNN_BE_EINVAL;
        if (misaligned(L->col[j], L->kind[j] == ICNN_BE_LOG_F64 ? 8 : 4)) return ICNN_BE_EINVAL;
    }
    if (misaligned(L->rows, 8) || misaligned(L->ctrl, 4) || !stream_ok(stream)) return ICNN_BE_EINVAL;
    return api_done(launch_kernel(log_row_kernel, dim3(1), dim3(LOG_THREADS), 0, static_cast<hipStream_t>(stream), *L));
}

}  // extern "C"
