// The RL agent's critic training step on the device (RL/src/icnn.py:56-112, 304-323; include/icnn_be.h, icnn_be_rl_td;
// DESIGN.md §13): the launch that joins the pieces the step already has (the inner Adam on the target, the critic's
// surrogate gradient) to the update.  The update itself -- soft target update, decay gradient, TF-Adam, proj and the scatter
// into both arenas (icnn_be_rl_critic_update) -- is the critic instantiation of param_update_kernel in be_train_update.hip.
//
//   rl_td_kernel             the clipped TD target, the per-sample weights c_j of the loss gradient, and the loss.  The
//                            L2 part of the loss is a sum over theta (213 k floats for the halfcheetah critic): every
//                            workgroup reduces a fixed grid-stride slice of it to one double (block_tree_sum, be_common.h),
//                            and the last workgroup to take a ticket does the per-sample part (a few hundred samples) and
//                            adds the partials in workgroup order -- a fixed order for a given shape, so the loss is
//                            bitwise repeatable.  tests/test_rl_train.py restates it in NumPy.
#include "be_api_check.h"
#include "be_kernels.h"
#include "be_rl_dev.h"

namespace icnn_be {

namespace {

constexpr int TD_THREADS = 256;

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
    s = block_tree_sum<TD_THREADS>(s, red);
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
    sq = block_tree_sum<TD_THREADS>(sq, red);
    if (tid == 0) {
        double reg = 0.0;
        for (int b = 0; b < (int)gridDim.x; ++b)
            reg = reg + __hip_atomic_load(a.partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *a.loss = (float)(sq / (double)a.batch + a.l2norm * (a.wd * reg * 0.5));
        __hip_atomic_store(a.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // re-armed for the next launch
    }
}

int rl_td_blocks(long long n_theta) {
    const long long per_block = (long long)TD_THREADS * 4;
    const long long b = (n_theta + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > ICNN_BE_RL_TD_MAX_BLOCKS ? ICNN_BE_RL_TD_MAX_BLOCKS : b);
}

}  // namespace
}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_rl_td(int batch, int n, const float *e_critic, const double *act, const float *rew, const unsigned char *term,
                  const float *q2_src, const double *act2, float discount, const float *theta, long long n_theta,
                  const unsigned char *decay, float l2norm, float wd, float *td, double *c, float *loss, void *work,
                  void *stream) {
    if (batch < 1 || n < 1 || n_theta < 1 || n_theta > 0x7fffffffLL) return ICNN_BE_EINVAL;
    if (misaligned(e_critic, 4) || misaligned(rew, 4) || misaligned(q2_src, 4) || misaligned(theta, 4) || misaligned(td, 4) ||
        misaligned(loss, 4) || !term || !decay)
        return ICNN_BE_EINVAL;
    if (misaligned(act, 8) || reinterpret_cast<uintptr_t>(act2) % 8 || misaligned(c, 8) || misaligned(work, 16) || !stream_ok(stream))
        return ICNN_BE_EINVAL;
    if (!std::isfinite(discount) || !(l2norm >= 0.f) || !(wd >= 0.f) || !std::isfinite(l2norm) || !std::isfinite(wd))
        return ICNN_BE_EINVAL;
    TdArgs a{};
    a.batch = batch;
    a.n = n;
    a.e = e_critic;
    a.act = act;
    a.rew = rew;
    a.term = term;
    a.q2 = q2_src;
    a.act2 = act2;                                                 // NULL: q2_src already holds negQ_entr
    a.discount = discount;
    a.inv_b = 1.f / (float)batch;                                  // float32 1 / B, as TF's _MeanGrad divides
    a.theta = theta;
    a.n_theta = n_theta;
    a.decay = decay;
    a.l2norm = (double)l2norm;
    a.wd = (double)wd;
    a.td = td;
    a.c = c;
    a.loss = loss;
    a.partial = reinterpret_cast<double *>(static_cast<char *>(work) + 16);
    a.ticket = static_cast<int *>(work);
    return api_done(launch_kernel(rl_td_kernel, dim3((unsigned)rl_td_blocks(n_theta)), dim3(TD_THREADS), 0,
                                  static_cast<hipStream_t>(stream), a));
}

}  // extern "C"
