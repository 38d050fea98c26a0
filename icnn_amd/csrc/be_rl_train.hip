// The RL agent's critic training step on the device (RL/src/icnn.py:56-112, 304-323; include/icnn_be.h,
// icnn_be_rl_td and icnn_be_rl_critic_update): the two launches that join the pieces the step already
// has (the inner Adam on the target, the critic's surrogate gradient).
//
//   rl_td_kernel             the clipped TD target, the per-sample weights c_j of the loss gradient, and the loss.  The
//                            L2 part of the loss is a sum over theta (213 k floats for the halfcheetah critic): every
//                            workgroup reduces a fixed grid-stride slice of it to one double, and the last workgroup
//                            to take a ticket does the per-sample part (a few hundred samples) and adds the partials in
//                            workgroup order -- a fixed order for a given shape, so the loss is bitwise repeatable.
//   rl_critic_update_kernel  the soft target update, the decay gradient, TF-Adam, proj and the scatter of both new
//                            weight vectors into their arenas, one thread per four consecutive parameters, with the
//                            arithmetic rules of param_update_kernel (be_train_update.hip): float32 correctly rounded
//                            at every operation, no contraction, sqrt as the float of the double root, the step count
//                            on the device.  tests/test_rl_train.py restates both in NumPy.
#include "be_kernels.h"
#include "be_rl_dev.h"

namespace icnn_be {

namespace {

constexpr int TD_THREADS = 256;
constexpr int UPD_THREADS = 256;
constexpr int UPD_PER_THREAD = 4;

struct TdArgs {
    int batch, n;
    const float *e;
    const double *act;
    const float *rew;
    const unsigned char *term;
    const float *q2;
    const double *act2;          // nullptr: q2 already holds negQ_entr
    float discount, inv_b;
    const float *theta;
    long long n_theta;
    const unsigned char *decay;
    double l2norm, wd;
    float *td;
    double *c;
    float *loss;
    double *partial;             // [ICNN_BE_RL_TD_MAX_BLOCKS]
    int *ticket;
};

// sum of one double per thread, the same tree for every call: valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = TD_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();                                               // red is reused by the next call
    return out;
}

__device__ __forceinline__ float entropy_sum(const double *a, int n) {
#pragma clang fp contract(off)
    float tot = 0.f;
    for (int i = 0; i < n; ++i) tot = tot + rl_entropy_term((float)a[i]).pen;
    return tot;
}

__global__ __launch_bounds__(TD_THREADS) void rl_td_kernel(TdArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[TD_THREADS];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    // ---- the L2 regulariser: sum of theta^2 over the decayed elements, one partial per workgroup ----
    double s = 0.0;
    const long long stride = (long long)gridDim.x * TD_THREADS;
    for (long long i = (long long)blockIdx.x * TD_THREADS + tid; i < a.n_theta; i += stride)
        if (a.decay[i]) {
            const double t = a.theta[i];
            s = s + t * t;
        }
    s = block_sum(s, red);
    if (tid == 0) {
        __hip_atomic_store(a.partial + blockIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int ticket = __hip_atomic_fetch_add(a.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    // ---- the last workgroup: TD target, c and the loss (RL/src/icnn.py:79-93) ----
    double sq = 0.0;
    for (int j = tid; j < a.batch; j += TD_THREADS) {
        const float q = -(a.e[j] + entropy_sum(a.act + (size_t)j * a.n, a.n));
        const float q2 = a.act2 ? -(a.q2[j] + entropy_sum(a.act2 + (size_t)j * a.n, a.n)) : -a.q2[j];
        float y = a.term[j] ? a.rew[j] : a.rew[j] + a.discount * q2;
        y = fmaxf(q - 1.f, y);
        y = fminf(q + 1.f, y);
        const float td = q - y;
        a.td[j] = td;
        a.c[j] = (double)(-(a.inv_b * (2.f * td)));                // TF's _MeanGrad and _SquareGrad through q = -negQ
        sq = sq + (double)td * (double)td;
    }
    sq = block_sum(sq, red);
    if (tid == 0) {
        double reg = 0.0;
        for (int b = 0; b < (int)gridDim.x; ++b)
            reg = reg + __hip_atomic_load(a.partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *a.loss = (float)(sq / (double)a.batch + a.l2norm * (a.wd * reg * 0.5));
        __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch
    }
}

struct RlUpdArgs {
    icnn_be_rl_update_args r;
    float b1, c1, b2, c2, k;
};

__device__ __forceinline__ bool in_proj(const icnn_be_param_update_args &a, long long j) {
    bool p = false;
    for (int r = 0; r < a.n_proj; ++r) p |= j >= a.proj_begin[r] && j < a.proj_end[r];
    return p;
}

__global__ __launch_bounds__(UPD_THREADS) void rl_critic_update_kernel(RlUpdArgs u) {
#pragma clang fp contract(off)
    const icnn_be_param_update_args &a = u.r.adam;
    __shared__ float s_lr_t;
    __shared__ int s_t;
    if (threadIdx.x == 0) {
        const int t = __hip_atomic_load(a.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        s_t = t;
        s_lr_t = (float)(a.lr * sqrt(1.0 - pow(a.beta2, (double)t)) / (1.0 - pow(a.beta1, (double)t)));
    }
    __syncthreads();
    const float lr_t = s_lr_t, eps = a.eps, tau = u.r.tau;
    const long long j0 = ((long long)blockIdx.x * UPD_THREADS + threadIdx.x) * UPD_PER_THREAD;
    if (j0 < a.n) {
        const int cnt = a.n - j0 < UPD_PER_THREAD ? (int)(a.n - j0) : UPD_PER_THREAD;
        float th[UPD_PER_THREAD] = {}, tt[UPD_PER_THREAD] = {}, m[UPD_PER_THREAD] = {}, v[UPD_PER_THREAD] = {},
              g[UPD_PER_THREAD] = {};
        bool dk[UPD_PER_THREAD] = {};
        int off[UPD_PER_THREAD + 1] = {};
        if (cnt == UPD_PER_THREAD) {
            const float4 t4 = *reinterpret_cast<const float4 *>(a.theta + j0);
            const float4 r4 = *reinterpret_cast<const float4 *>(u.r.target_theta + j0);
            const float4 m4 = *reinterpret_cast<const float4 *>(a.m + j0);
            const float4 v4 = *reinterpret_cast<const float4 *>(a.v + j0);
            const float4 g4 = *reinterpret_cast<const float4 *>(a.grad + j0);
            const int4 o4 = *reinterpret_cast<const int4 *>(a.dest_off + j0);
            const uchar4 d4 = *reinterpret_cast<const uchar4 *>(u.r.decay + j0);
            th[0] = t4.x; th[1] = t4.y; th[2] = t4.z; th[3] = t4.w;
            tt[0] = r4.x; tt[1] = r4.y; tt[2] = r4.z; tt[3] = r4.w;
            m[0] = m4.x; m[1] = m4.y; m[2] = m4.z; m[3] = m4.w;
            v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
            g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
            off[0] = o4.x; off[1] = o4.y; off[2] = o4.z; off[3] = o4.w;
            dk[0] = d4.x; dk[1] = d4.y; dk[2] = d4.z; dk[3] = d4.w;
        } else {
            for (int k = 0; k < cnt; ++k) {
                th[k] = a.theta[j0 + k]; tt[k] = u.r.target_theta[j0 + k]; m[k] = a.m[j0 + k]; v[k] = a.v[j0 + k];
                g[k] = a.grad[j0 + k]; off[k] = a.dest_off[j0 + k]; dk[k] = u.r.decay[j0 + k];
            }
        }
        off[cnt] = a.dest_off[j0 + cnt];
#pragma unroll
        for (int k = 0; k < UPD_PER_THREAD; ++k) {
            const float old = th[k];
            tt[k] = tt[k] - tau * (tt[k] - old);                    // update_target, from the pre-update theta
            const float gk = dk[k] ? g[k] + u.k * old : g[k];       // + d (l2norm wd |W|^2 / 2) / dW  (TF's AddN)
            m[k] = u.b1 * m[k] + u.c1 * gk;
            v[k] = u.b2 * v[k] + u.c2 * (gk * gk);
            const float root = (float)__builtin_sqrt((double)v[k]);
            th[k] = th[k] - (lr_t * m[k]) / (root + eps);
            if (th[k] < 0.f && in_proj(a, j0 + k)) th[k] = 0.f;
        }
        if (cnt == UPD_PER_THREAD) {
            *reinterpret_cast<float4 *>(a.theta + j0) = make_float4(th[0], th[1], th[2], th[3]);
            *reinterpret_cast<float4 *>(u.r.target_theta + j0) = make_float4(tt[0], tt[1], tt[2], tt[3]);
            *reinterpret_cast<float4 *>(a.m + j0) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(a.v + j0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; k < cnt; ++k) {
                a.theta[j0 + k] = th[k]; u.r.target_theta[j0 + k] = tt[k]; a.m[j0 + k] = m[k]; a.v[j0 + k] = v[k];
            }
        }
        for (int k = 0; k < cnt; ++k)
            for (int d = off[k]; d < off[k + 1]; ++d) {
                const int at = a.dest[d];
                if (at >= 0 && at < a.arena_floats) {
                    a.arena[at] = th[k];
                    u.r.target_arena[at] = tt[k];
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

}  // namespace

int rl_td_blocks(long long n_theta) {
    const long long per_block = (long long)TD_THREADS * 4;
    const long long b = (n_theta + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > ICNN_BE_RL_TD_MAX_BLOCKS ? ICNN_BE_RL_TD_MAX_BLOCKS : b);
}

hipError_t launch_rl_td(const RlTdLaunch &l, hipStream_t stream) {
    TdArgs a{};
    a.batch = l.batch;
    a.n = l.n;
    a.e = l.e_critic;
    a.act = l.act;
    a.rew = l.rew;
    a.term = l.term;
    a.q2 = l.q2_src;
    a.act2 = l.act2;
    a.discount = l.discount;
    a.inv_b = 1.f / (float)l.batch;                                // float32 1 / B, as TF's _MeanGrad divides
    a.theta = l.theta;
    a.n_theta = l.n_theta;
    a.decay = l.decay;
    a.l2norm = (double)l.l2norm;
    a.wd = (double)l.wd;
    a.td = l.td;
    a.c = l.c;
    a.loss = l.loss;
    a.partial = reinterpret_cast<double *>(static_cast<char *>(l.work) + 16);
    a.ticket = static_cast<int *>(l.work);
    return launch_kernel(rl_td_kernel, dim3((unsigned)rl_td_blocks(l.n_theta)), dim3(TD_THREADS), 0, stream, a);
}

hipError_t launch_rl_critic_update(const icnn_be_rl_update_args &r, hipStream_t stream) {
    RlUpdArgs u{};
    u.r = r;
    u.b1 = (float)r.adam.beta1;
    u.c1 = (float)(1.0 - r.adam.beta1);
    u.b2 = (float)r.adam.beta2;
    u.c2 = (float)(1.0 - r.adam.beta2);
    u.k = r.l2norm * r.wd;                                          // float32 product of the two float32 constants
    return launch_kernel(rl_critic_update_kernel, dim3((unsigned)param_update_blocks(r.adam.n)), dim3(UPD_THREADS), 0,
                         stream, u);
}

}  // namespace icnn_be
