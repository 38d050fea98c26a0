// The two table kernels of the flat-vector trainers (be_train_table.h): be_ddpg.hip, be_naf.hip and be_ff.hip
// fill a table each and launch these.
//
//   grad_table_kernel         dW = X^T Delta over the batch and the column sums of Delta for a table of layers in one launch: a
//                             layer's W and b are one [(in + 1)][out] block of the flat gradient, the product of [X, 1]^T and
//                             Delta; a wave owns a 16 x 32 block and runs one fma chain over the batch per element
//                             (mfma_f32_16x16x4f32, two independent accumulators).  No atomics, no split of the sum: the same
//                             bits on every run.
//   param_sets_update_kernel  a table of parameter sets in one launch: g + k theta (k = 0 leaves g as it is), TF-Adam
//                             (be_tf_adam.h), then target <- target - tau (target - theta_new), from the NEW theta (ddpg.py
//                             orders the moving average behind the assignment) for a set that has a target.  The workgroups of
//                             the leading sets also reduce sum theta_old^2, and the last workgroup by ticket forms loss_q from
//                             the chain kernel's tile partials and those, each in index order (the scheme of rl_td_kernel).
//                             The last `tail` elements of a set are exempt from the decay, the sum and the target.
#include "be_train_table.h"

#include "be_common.h"
#include "be_tf_adam.h"

namespace icnn_be {

namespace {

constexpr int GW = 4;                    // waves per workgroup; a wave owns a 16 x 32 block of one layer's [(in + 1)][out]

// G[m][j] = sum_b X1[b][m] D[b][j] with X1 = [X, 1]: the row of ones makes the bias gradient row `in` of the same product.
// One fma chain over the batch in index order per element (no split of the sum, no atomics): the same bits on every run.
__global__ __launch_bounds__(64 * GW) void grad_table_kernel(GradArgs a) {
    const int lane = threadIdx.x & 63, r16 = lane & 15, q = lane >> 4;
    const int w = blockIdx.x * GW + (threadIdx.x >> 6);
    if (w >= a.waves) return;
    GradProd p = a.p[0];
#pragma unroll
    for (int i = 1; i < GRAD_PRODUCTS; ++i)
        if (i < a.count && w >= a.p[i].wave0) p = a.p[i];
    const int local = w - p.wave0, pairs = (p.out + 31) >> 5;
    const int tm = local / pairs, tn = local - tm * pairs;
    const int m = tm * 16 + r16, c0 = tn * 32 + r16, c1 = c0 + 16;
    const bool vm = m < p.in, one = m == p.in, v0 = c0 < p.out, v1 = c1 < p.out;
    f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < a.B; k0 += 16) {
        float af[4], b0[4], b1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k0 + 4 * q + j;
            const bool ok = kk < a.B;
            af[j] = ok && vm ? p.X[(size_t)kk * p.in + m] : ok && one ? 1.f : 0.f;
            b0[j] = ok && v0 ? p.D[(size_t)kk * p.out + c0] : 0.f;
            b1[j] = ok && v1 ? p.D[(size_t)kk * p.out + c1] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b0[j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], b1[j], acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = tm * 16 + 4 * q + r;
        if (row > p.in) continue;
        if (v0) p.G[(size_t)row * p.out + c0] = acc0[r];
        if (v1) p.G[(size_t)row * p.out + c1] = acc1[r];
    }
}

constexpr int UT = ADAM_THREADS;         // a set's workgroups are param_update_blocks(n) of them
constexpr int UPT = ADAM_PER_THREAD;

__global__ __launch_bounds__(UT) void param_sets_update_kernel(ParamSetsArgs u) {
#pragma clang fp contract(off)
    __shared__ float s_lr_t;
    __shared__ double red[UT];
    __shared__ int s_last;
    int which = 0, block = (int)blockIdx.x;
    while (which + 1 < u.sets && block >= u.set[which].blocks) block -= u.set[which++].blocks;
    const ParamSet &a = u.set[which];
    const bool has_target = a.target != nullptr;
    const long long plain = a.n - a.tail;    // the elements behind it: no decay, not in sum theta^2, not in the target
    if (threadIdx.x == 0) {
        // updates done so far: the last workgroup writes the counts back only after every workgroup has taken its ticket, and
        // every workgroup reads its count before it takes one
        const int t = __hip_atomic_load(u.step + a.slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        s_lr_t = tf_adam_lr_t(a.lr, u.beta1, u.beta2, t);
    }
    __syncthreads();
    const float lr_t = s_lr_t, eps = u.eps, tau = u.tau;
    const long long j0 = ((long long)block * UT + threadIdx.x) * UPT;
    double ssq = 0.0;
    if (j0 < a.n) {
        const int cnt = a.n - j0 < UPT ? (int)(a.n - j0) : UPT;
        const int tcnt = !has_target || plain <= j0 ? 0 : plain - j0 < UPT ? (int)(plain - j0) : UPT;       // of the target
        float th[UPT] = {}, m[UPT] = {}, v[UPT] = {}, g[UPT] = {}, tt[UPT] = {};
        if (cnt == UPT) {
            load_quad(th, a.theta + j0);
            load_quad(m, a.m + j0);
            load_quad(v, a.v + j0);
            load_quad(g, a.grad + j0);
        } else {
            for (int k = 0; k < cnt; ++k) {
                th[k] = a.theta[j0 + k];
                m[k] = a.m[j0 + k]; v[k] = a.v[j0 + k]; g[k] = a.grad[j0 + k];
            }
        }
        if (tcnt == UPT) {
            load_quad(tt, a.target + j0);
        } else {
            for (int k = 0; k < tcnt; ++k) tt[k] = a.target[j0 + k];
        }
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            // the decay term in front of the step and the target rule behind it, from the new theta
            const float old = th[k];
            const bool pl = j0 + k < plain;
            if (pl) ssq = ssq + (double)old * (double)old;
            const float gk = a.k != 0.f && pl ? g[k] + a.k * old : g[k];
            th[k] = tf_adam_element(old, m[k], v[k], gk, u.b1, u.c1, u.b2, u.c2, lr_t, eps);
            tt[k] = tt[k] - tau * (tt[k] - th[k]);
        }
        if (cnt == UPT) {
            store_quad(a.theta + j0, th);
            store_quad(a.m + j0, m);
            store_quad(a.v + j0, v);
        } else {
            for (int k = 0; k < cnt; ++k) {
                a.theta[j0 + k] = th[k]; a.m[j0 + k] = m[k]; a.v[j0 + k] = v[k];
            }
        }
        if (tcnt == UPT) {
            store_quad(a.target + j0, tt);
        } else {
            for (int k = 0; k < tcnt; ++k) a.target[j0 + k] = tt[k];
        }
    }
    // loss_q's decay sum: one partial per workgroup of the sets that enter it
    if (u.loss && (int)blockIdx.x < u.reg_blocks) {
        ssq = block_tree_sum<UT>(ssq, red);
        if (threadIdx.x == 0) __hip_atomic_store(u.partial + blockIdx.x, ssq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ticket = __hip_atomic_fetch_add(u.step + u.slots, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == (int)gridDim.x - 1;
        if (s_last) {
            // the last workgroup: the step counts, the loss, and the ticket re-armed for the next launch
            for (int w = 0; w < u.slots; ++w) {
                const int t = __hip_atomic_load(u.step + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(u.step + w, t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (u.loss) {
                double sq = 0.0, reg = 0.0;
                for (int i = 0; i < u.tiles; ++i) sq = sq + u.sq[i];
                for (int b = 0; b < u.reg_blocks; ++b)
                    reg = reg + __hip_atomic_load(u.partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *u.loss = (float)(sq / (double)u.batch + u.l2norm * (0.5 * reg));
            }
            __hip_atomic_store(u.step + u.slots, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

hipError_t launch_grad_table(const GradArgs &a, hipStream_t stream) {
    return launch_kernel(grad_table_kernel, dim3((a.waves + GW - 1) / GW), dim3(64 * GW), 0, stream, a);
}

void update_coefficients(ParamSetsArgs &u, double beta1, double beta2) {
    u.beta1 = beta1;
    u.beta2 = beta2;
    u.b1 = (float)beta1;
    u.c1 = (float)(1.0 - beta1);
    u.b2 = (float)beta2;
    u.c2 = (float)(1.0 - beta2);
}

hipError_t launch_param_sets_update(const ParamSetsArgs &u, hipStream_t stream) {
    int blocks = 0;
    for (int i = 0; i < u.sets; ++i) blocks += u.set[i].blocks;
    return launch_kernel(param_sets_update_kernel, dim3((unsigned)blocks), dim3(UT), 0, stream, u);
}

}  // namespace icnn_be
