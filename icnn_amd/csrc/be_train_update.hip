// Parameter update of a PICNN on the device: tf.train.AdamOptimizer's step over the flat theta, the reference's proj clamp
// and the scatter of every new weight into each copy the kernels read (the weight arena), in one launch
// (include/icnn_be.h, icnn_be_param_update).
//
// One thread per four consecutive parameters: 16-byte loads and stores on the theta / m / v / grad streams, four CSR
// offsets of the map with one more 16-byte load, then the scattered stores of the copies.  The arithmetic of one element is
// tf_adam_element with tf_adam_lr_t's step size (be_tf_adam.h), and behind it
//   theta = 0 if theta < 0 and the element is a proj weight (np.maximum(theta, 0): -0 and NaN stay)
//
// The gated form (icnn_be_param_update_gated) is the same kernel body behind one word of device memory: a
// workgroup that reads *go == 0 leaves before it loads, stores or takes a ticket, so theta, m, v, the arena and both step
// words stay as they were.  gated_copy_kernel is the gate's other consumer: dst = src when (*go != 0) == (want != 0), which
// puts the BatchNorm moving statistics of a skipped step back from their shadow.
//
// The RL critic's form (icnn_be_rl_critic_update; DESIGN.md §13, RL/src/icnn.py:56-112) is a third instantiation of that
// body.  Per element, ahead of the step above and from the pre-update theta (tests/test_rl_train.py restates it):
//   target = target - tau * (target - theta)                 update_target
//   g = g + k * theta on the decayed elements                k = l2norm * wd in float32 (TF's AddN of the two gradients)
// and every new target value is scattered into the target's arena beside the critic's.
#include "be_api_check.h"
#include "be_kernels.h"
#include "be_tf_adam.h"

namespace icnn_be {

namespace {

constexpr int UPD_THREADS = ADAM_THREADS;
constexpr int UPD_PER_THREAD = ADAM_PER_THREAD;

struct UpdArgs {
    icnn_be_rl_update_args r;   // r.adam: every form; the rest and k: the critic's alone
    float b1, c1, b2, c2, k;
    const int *go;              // the gated form's word; not read by the others
};

__device__ __forceinline__ bool in_proj(const icnn_be_param_update_args &a, long long j) {
    bool p = false;
    for (int r = 0; r < a.n_proj; ++r) p |= j >= a.proj_begin[r] && j < a.proj_end[r];
    return p;
}

template <bool GATED, bool CRITIC>
__global__ __launch_bounds__(UPD_THREADS) void param_update_kernel(UpdArgs u) {
#pragma clang fp contract(off)
    const icnn_be_param_update_args &a = u.r.adam;
    __shared__ float s_lr_t;
    __shared__ int s_t;
    if (GATED) {
        // one read per workgroup; the word is not written while this launch runs, so every workgroup sees the same value
        // and either all of them take a ticket or none does
        __shared__ int s_go;
        if (threadIdx.x == 0) s_go = *u.go;
        __syncthreads();
        if (s_go == 0) return;
    }
    if (threadIdx.x == 0) {
        // updates done so far; the last workgroup of this launch writes t back only after every workgroup has taken its
        // ticket, and every workgroup reads the count before it takes one
        const int t = __hip_atomic_load(a.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        s_t = t;
        s_lr_t = tf_adam_lr_t(a.lr, a.beta1, a.beta2, t);
    }
    __syncthreads();
    const float lr_t = s_lr_t, eps = a.eps, tau = u.r.tau;
    const long long j0 = ((long long)blockIdx.x * UPD_THREADS + threadIdx.x) * UPD_PER_THREAD;
    if (j0 < a.n) {
        const int cnt = a.n - j0 < UPD_PER_THREAD ? (int)(a.n - j0) : UPD_PER_THREAD;
        float th[UPD_PER_THREAD] = {}, m[UPD_PER_THREAD] = {}, v[UPD_PER_THREAD] = {}, g[UPD_PER_THREAD] = {};
        float tt[UPD_PER_THREAD] = {};      // the critic's target theta and decay mask; dead in the other forms
        bool dk[UPD_PER_THREAD] = {};
        int off[UPD_PER_THREAD + 1] = {};
        if (cnt == UPD_PER_THREAD) {
            load_quad(th, a.theta + j0);
            if (CRITIC) load_quad(tt, u.r.target_theta + j0);
            load_quad(m, a.m + j0);
            load_quad(v, a.v + j0);
            load_quad(g, a.grad + j0);
            const int4 o4 = *reinterpret_cast<const int4 *>(a.dest_off + j0);
            off[0] = o4.x; off[1] = o4.y; off[2] = o4.z; off[3] = o4.w;
            if (CRITIC) {
                const uchar4 d4 = *reinterpret_cast<const uchar4 *>(u.r.decay + j0);
                dk[0] = d4.x; dk[1] = d4.y; dk[2] = d4.z; dk[3] = d4.w;
            }
        } else {
            for (int k = 0; k < cnt; ++k) {
                th[k] = a.theta[j0 + k];
                if (CRITIC) tt[k] = u.r.target_theta[j0 + k];
                m[k] = a.m[j0 + k]; v[k] = a.v[j0 + k]; g[k] = a.grad[j0 + k];
                off[k] = a.dest_off[j0 + k];
                if (CRITIC) dk[k] = u.r.decay[j0 + k];
            }
        }
        off[cnt] = a.dest_off[j0 + cnt];
#pragma unroll
        for (int k = 0; k < UPD_PER_THREAD; ++k) {
            const float old = th[k];
            if (CRITIC) tt[k] = tt[k] - tau * (tt[k] - old);                  // update_target, from the pre-update theta
            const float gk = CRITIC && dk[k] ? g[k] + u.k * old : g[k];      // + d (l2norm wd |W|^2 / 2) / dW  (TF's AddN)
            th[k] = tf_adam_element(old, m[k], v[k], gk, u.b1, u.c1, u.b2, u.c2, lr_t, eps);
            if (th[k] < 0.f && in_proj(a, j0 + k)) th[k] = 0.f;
        }
        if (cnt == UPD_PER_THREAD) {
            store_quad(a.theta + j0, th);
            if (CRITIC) store_quad(u.r.target_theta + j0, tt);
            store_quad(a.m + j0, m);
            store_quad(a.v + j0, v);
        } else {
            for (int k = 0; k < cnt; ++k) {
                a.theta[j0 + k] = th[k];
                if (CRITIC) u.r.target_theta[j0 + k] = tt[k];
                a.m[j0 + k] = m[k]; a.v[j0 + k] = v[k];
            }
        }
        for (int k = 0; k < cnt; ++k)
            for (int d = off[k]; d < off[k + 1]; ++d) {
                const int at = a.dest[d];
                if (at >= 0 && at < a.arena_floats) {
                    a.arena[at] = th[k];
                    if (CRITIC) u.r.target_arena[at] = tt[k];
                }
            }
    }
    // the step count: the last workgroup to arrive stores t and re-arms the ticket for the next launch
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ticket = __hip_atomic_fetch_add(a.step + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ticket == (int)gridDim.x - 1) {
            __hip_atomic_store(a.step, s_t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.step + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

constexpr int COPY_THREADS = 256;
constexpr int COPY_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(COPY_THREADS) void gated_copy_kernel(float *dst, const float *src, long long n, const int *go,
                                                                   int want) {
    __shared__ int s_go;
    if (threadIdx.x == 0) s_go = *go;
    __syncthreads();
    if ((s_go != 0) != (want != 0)) return;
    const long long stride = (long long)gridDim.x * COPY_THREADS;
    for (long long i = (long long)blockIdx.x * COPY_THREADS + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

}  // namespace

long long param_update_blocks(long long n) {
    const long long per_block = (long long)UPD_THREADS * UPD_PER_THREAD;
    return (n + per_block - 1) / per_block;
}

namespace {

template <bool GATED, bool CRITIC>
hipError_t launch_update(UpdArgs u, hipStream_t stream) {
    const icnn_be_param_update_args &a = u.r.adam;
    u.b1 = (float)a.beta1;
    u.c1 = (float)(1.0 - a.beta1);
    u.b2 = (float)a.beta2;
    u.c2 = (float)(1.0 - a.beta2);
    return launch_kernel(param_update_kernel<GATED, CRITIC>, dim3((unsigned)param_update_blocks(a.n)), dim3(UPD_THREADS), 0,
                         stream, u);
}

// what icnn_be_param_update, its gated form and icnn_be_rl_critic_update refuse before any launch
int check_param_update(const icnn_be_param_update_args *a) {
    if (!a || a->n < 1 || !a->dest || !a->arena || !a->step) return ICNN_BE_EINVAL;
    if (misaligned(a->theta, 16) || misaligned(a->m, 16) || misaligned(a->v, 16) || misaligned(a->grad, 16) ||
        misaligned(a->dest_off, 16))
        return ICNN_BE_EINVAL;
    if (a->arena_floats < 0 || a->arena_floats > 0x7fffffffLL || param_update_blocks(a->n) > 0x7fffffffLL) return ICNN_BE_EINVAL;
    if (!adam_constants_ok(a->beta1, a->beta2, a->eps) || !(a->lr == a->lr)) return ICNN_BE_EINVAL;
    if (a->n_proj < 0 || a->n_proj > ICNN_BE_MAX_PROJ_RANGES) return ICNN_BE_EINVAL;
    for (int r = 0; r < a->n_proj; ++r)
        if (a->proj_begin[r] < 0 || a->proj_begin[r] > a->proj_end[r] || a->proj_end[r] > a->n) return ICNN_BE_EINVAL;
    return 0;
}

// go NULL: the plain update
int param_update(const icnn_be_param_update_args *a, const int *go, void *stream) {
    if (int rc = check_param_update(a)) return rc;
    UpdArgs u{};
    u.r.adam = *a;
    u.go = go;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    return api_done(go ? launch_update<true, false>(u, s) : launch_update<false, false>(u, s));
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_param_update(const icnn_be_param_update_args *a, void *stream) { return param_update(a, nullptr, stream); }

int icnn_be_param_update_gated(const icnn_be_param_update_args *a, const int *go, void *stream) {
    if (!go) return ICNN_BE_EINVAL;
    return param_update(a, go, stream);
}

int icnn_be_gated_copy(float *dst, const float *src, long long n, const int *go, int want, void *stream) {
    if (!dst || !src || !go || n < 0) return ICNN_BE_EINVAL;
    if (n == 0) return 0;
    const long long blocks = (n + COPY_THREADS - 1) / COPY_THREADS;
    return api_done(launch_kernel(gated_copy_kernel, dim3((unsigned)(blocks < COPY_MAX_BLOCKS ? blocks : COPY_MAX_BLOCKS)),
                                  dim3(COPY_THREADS), 0, static_cast<hipStream_t>(stream), dst, src, n, go, want));
}

int icnn_be_rl_critic_update(const icnn_be_rl_update_args *a, void *stream) {
    if (!a) return ICNN_BE_EINVAL;
    if (int rc = check_param_update(&a->adam)) return rc;
    if (misaligned(a->target_theta, 16) || misaligned(a->decay, 4) || misaligned(a->target_arena, 4) || !stream_ok(stream))
        return ICNN_BE_EINVAL;
    if (!(a->tau >= 0.f && a->tau <= 1.f) || !(a->l2norm >= 0.f) || !(a->wd >= 0.f) || !std::isfinite(a->l2norm) ||
        !std::isfinite(a->wd))
        return ICNN_BE_EINVAL;
    UpdArgs u{};
    u.r = *a;
    u.k = a->l2norm * a->wd;                                        // float32 product of the two float32 constants
    return api_done(launch_update<false, true>(u, static_cast<hipStream_t>(stream)));
}

}  // extern "C"
