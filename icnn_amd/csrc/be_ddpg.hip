// The DDPG agent's training step and act() on the device (RL/src/ddpg.py, ddpg_nets_dm.py; include/icnn_be.h,
// icnn_be_ddpg_*).  Parameters are flat float32 vectors in the order W1, b1, W2, b2, W3, b3 with W row-major
// [in][out]; the forward products read W as it lies, the backward products read it transposed -- no packed copy.
//
//   ddpg_chain_kernel    everything of a step that stays inside one sample, one workgroup per 16-sample tile, activations in
//                        LDS: the target path (a2, q2, y), the critic at (obs, act) with td and the tile's sum of td^2, the
//                        policy and the critic at (obs, pi(obs)), and both backward chains down to the pre-activation deltas.
//                        Layer inputs and deltas go to the workspace; rows past the batch and columns past a width are
//                        predicated off.  No grid barrier: nothing in it crosses samples.
//   ddpg_grads_kernel    dW = X^T Delta over the batch and the column sums of Delta for the six layers (nine for be_naf.hip),
//                        one launch over a table: a layer's W and b are one [(in + 1)][out] block of the flat gradient, the product of
//                        [X, 1]^T and Delta; a wave owns a 16 x 32 block and runs one fma chain over the batch per element.
//                        No atomics, no split of the sum: the same bits on every run.
//   ddpg_update_kernel   a table of parameter sets (here both nets; be_naf.hip brings three) in one launch: g + k theta (k = 0 leaves g as it is), TF-Adam with the arithmetic of
//                        param_update_kernel (be_train_update.hip), then target <- target - tau (target - theta_new), from
//                        the NEW theta (ddpg.py orders the moving average behind the assignment) for a set that has a
//                        target.  The workgroups of the leading sets (here the critic's) also reduce sum theta_old^2, and the last workgroup by ticket forms loss_q from the tile partials
//                        and those, each in index order (the scheme of rl_td_kernel).
//   ddpg_act_kernel      pi(obs) for B observations, ddpg_q_kernel Q(obs, act): the layer routines of the chain kernel, so
//                        the bits of its policy output.
//
// Products: mfma_f32_16x16x4f32, a wave owning two 16-column tiles of the output at a time (two independent accumulators);
// per 16 values of k a lane takes four consecutive k (the k order inside the block is permuted alike in both operands).
#include "be_kernels.h"
#include "be_tile.h"
#include "be_train_common.h"

namespace icnn_be {

namespace {

__device__ __forceinline__ Net critic_net(const float *t, int dimO, int dimA, int l1, int l2) {
    Net n;
    n.W1 = t;
    n.b1 = n.W1 + (size_t)dimO * l1;
    n.W2 = n.b1 + l1;
    n.b2 = n.W2 + (size_t)(l1 + dimA) * l2;
    n.W3 = n.b2 + l2;
    n.b3 = n.W3 + l2;
    return n;
}

struct ChainArgs {
    int B, dimO, dimA, l1, l2;
    const float *obs, *ob2, *rew;
    const double *act;
    const unsigned char *term;
    const float *tp, *tq, *ttp, *ttq;
    float discount, inv_b;
    float *a2, *y, *q, *td, *a, *qpi, *xa, *h2q, *d3q, *d2q, *d1q, *h1p, *h2p, *h2c, *d3p, *d2p, *d1p;
    double *sq;
    int PA, PB, PC, PD, PS;
};

__global__ __launch_bounds__(DT) void ddpg_chain_kernel(ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, dimO = a.dimO, dimA = a.dimA, l1 = a.l1, l2 = a.l2;
    const int PA = a.PA, PB = a.PB, PC = a.PC, PD = a.PD, PS = a.PS;
    float *bA = lds, *bB = bA + TS * PA, *bC = bB + TS * PB, *bD = bC + TS * PC, *sA = bD + TS * PD, *sD = sA + TS * PS;
    float *vy = sD + TS * PS, *vd = vy + TS;
    Tile t;
    t.s0 = blockIdx.x * TS;
    t.rows = a.B - t.s0 < TS ? a.B - t.s0 : TS;
    const Net P = policy_net(a.tp, dimO, dimA, l1, l2), Q = critic_net(a.tq, dimO, dimA, l1, l2);
    const Net PT = policy_net(a.ttp, dimO, dimA, l1, l2), QT = critic_net(a.ttq, dimO, dimA, l1, l2);
    const int s32 = tid >> 5;

    // ---- the target: a2 = pi(ob2; target), q2 = Q(ob2, a2; target), y ----
    load_rows(bA, PA, 0, a.ob2, dimO, t);
    __syncthreads();
    layer_relu(bA, PA, dimO, PT.W1, PT.b1, l1, bC, PC, nullptr, 0, t);
    layer_relu(bA, PA, dimO, QT.W1, QT.b1, l1, bB, PB, nullptr, 0, t);
    __syncthreads();
    layer_relu(bC, PC, l1, PT.W2, PT.b2, l2, bD, PD, nullptr, 0, t);
    __syncthreads();
    layer_tanh(bD, PD, l2, PT.W3, PT.b3, dimA, bB + l1, PB, a.a2, t);
    __syncthreads();
    layer_relu(bB, PB, l1 + dimA, QT.W2, QT.b2, l2, bC, PC, nullptr, 0, t);
    __syncthreads();
    {
        const float q2 = tile_dot(bC, PC, l2, QT.W3) + QT.b3[0];
        if ((tid & 31) == 0) {
            float y = 0.f;
            if (s32 < t.rows) {
                const float r = a.rew[t.s0 + s32];
                y = a.term[t.s0 + s32] ? r : r + a.discount * q2;
                a.y[t.s0 + s32] = y;
            }
            vy[s32] = y;
        }
    }
    // ---- the first layers at obs: the critic's (shared by both of its evaluations) and the policy's ----
    load_rows(bA, PA, 0, a.obs, dimO, t);
    load_rows(bB, PB, l1, a.act, dimA, t);                       // float64 actions, rounded to float32 once
    __syncthreads();
    for (int i = tid; i < t.rows * dimA; i += DT) {
        const int s = i / dimA, c = i - s * dimA;
        a.xa[(size_t)(t.s0 + s) * (l1 + dimA) + l1 + c] = bB[s * PB + l1 + c];
    }
    layer_relu(bA, PA, dimO, Q.W1, Q.b1, l1, bB, PB, a.xa, l1 + dimA, t);
    layer_relu(bA, PA, dimO, P.W1, P.b1, l1, bC, PC, a.h1p, l1, t);
    __syncthreads();
    layer_relu(bB, PB, l1 + dimA, Q.W2, Q.b2, l2, bD, PD, a.h2q, l2, t);
    layer_relu(bC, PC, l1, P.W2, P.b2, l2, bA, PA, a.h2p, l2, t);
    __syncthreads();
    // ---- q, td, delta3 of the critic; a = pi(obs) ----
    {
        const float q = tile_dot(bD, PD, l2, Q.W3) + Q.b3[0];
        if ((tid & 31) == 0) {
            float td = 0.f, d3 = 0.f;
            if (s32 < t.rows) {
                td = q - vy[s32];
                d3 = a.inv_b * (2.f * td);
                a.q[t.s0 + s32] = q;
                a.td[t.s0 + s32] = td;
                a.d3q[t.s0 + s32] = d3;
            }
            vy[s32] = td;
            vd[s32] = d3;
        }
    }
    layer_tanh(bA, PA, l2, P.W3, P.b3, dimA, sA, PS, a.a, t);
    __syncthreads();
    // ---- the critic's backward chain; the policy's action takes the place of the minibatch's in [h1, act] ----
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < t.rows; ++i) s = s + (double)vy[i] * (double)vy[i];
        a.sq[blockIdx.x] = s;
    }
    for (int i = tid; i < TS * l2; i += DT) {
        const int s = i / l2, n = i - s * l2;
        const float d = bD[s * PD + n] > 0.f ? vd[s] * Q.W3[n] : 0.f;
        bD[s * PD + n] = d;
        if (s < t.rows) a.d2q[(size_t)(t.s0 + s) * l2 + n] = d;
    }
    for (int i = tid; i < TS * dimA; i += DT) {
        const int s = i / dimA, c = i - s * dimA;
        bB[s * PB + l1 + c] = sA[s * PS + c];
    }
    __syncthreads();
    tile_gemm(bD, PD, l2, Q.W2, 1, l2, l1, [&](int s, int j, float acc) {
        if (s < t.rows) a.d1q[(size_t)(t.s0 + s) * l1 + j] = bB[s * PB + j] > 0.f ? acc : 0.f;
    });
    __syncthreads();
    // ---- the critic at (obs, pi(obs)) and the policy's backward chain ----
    layer_relu(bB, PB, l1 + dimA, Q.W2, Q.b2, l2, bD, PD, a.h2c, l2, t);
    __syncthreads();
    {
        const float qpi = tile_dot(bD, PD, l2, Q.W3) + Q.b3[0];
        if ((tid & 31) == 0 && s32 < t.rows) a.qpi[t.s0 + s32] = qpi;
    }
    __syncthreads();
    for (int i = tid; i < TS * l2; i += DT) {                     // d(-q / B) / d(pre-activation 2)
        const int s = i / l2, n = i - s * l2;
        bD[s * PD + n] = bD[s * PD + n] > 0.f ? -a.inv_b * Q.W3[n] : 0.f;
    }
    __syncthreads();
    tile_gemm(bD, PD, l2, Q.W2 + (size_t)l1 * l2, 1, l2, dimA, [&](int s, int j, float acc) {   // through W2's action rows
        const float av = sA[s * PS + j], d = acc * (1.f - av * av);
        sD[s * PS + j] = d;
        if (s < t.rows) a.d3p[(size_t)(t.s0 + s) * dimA + j] = d;
    });
    __syncthreads();
    tile_gemm(sD, PS, dimA, P.W3, 1, dimA, l2, [&](int s, int j, float acc) {
        const float d = bA[s * PA + j] > 0.f ? acc : 0.f;
        bB[s * PB + j] = d;
        if (s < t.rows) a.d2p[(size_t)(t.s0 + s) * l2 + j] = d;
    });
    __syncthreads();
    tile_gemm(bB, PB, l2, P.W2, 1, l2, l1, [&](int s, int j, float acc) {
        if (s < t.rows) a.d1p[(size_t)(t.s0 + s) * l1 + j] = bC[s * PC + j] > 0.f ? acc : 0.f;
    });
}

struct FwdArgs {
    int B, dimO, dimA, l1, l2;
    const float *theta, *obs;
    const double *act;      // the critic's form
    float *out;
    int PA, PB, PD;
};

__global__ __launch_bounds__(DT) void ddpg_act_kernel(FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *bA = lds, *bB = bA + TS * a.PA, *bD = bB + TS * a.PB;
    Tile t;
    t.s0 = blockIdx.x * TS;
    t.rows = a.B - t.s0 < TS ? a.B - t.s0 : TS;
    const Net P = policy_net(a.theta, a.dimO, a.dimA, a.l1, a.l2);
    load_rows(bA, a.PA, 0, a.obs, a.dimO, t);
    __syncthreads();
    layer_relu(bA, a.PA, a.dimO, P.W1, P.b1, a.l1, bB, a.PB, nullptr, 0, t);
    __syncthreads();
    layer_relu(bB, a.PB, a.l1, P.W2, P.b2, a.l2, bD, a.PD, nullptr, 0, t);
    __syncthreads();
    layer_tanh(bD, a.PD, a.l2, P.W3, P.b3, a.dimA, nullptr, 0, a.out, t);
}

__global__ __launch_bounds__(DT) void ddpg_q_kernel(FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *bA = lds, *bB = bA + TS * a.PA, *bD = bB + TS * a.PB;
    Tile t;
    t.s0 = blockIdx.x * TS;
    t.rows = a.B - t.s0 < TS ? a.B - t.s0 : TS;
    const Net Q = critic_net(a.theta, a.dimO, a.dimA, a.l1, a.l2);
    load_rows(bA, a.PA, 0, a.obs, a.dimO, t);
    load_rows(bB, a.PB, a.l1, a.act, a.dimA, t);
    __syncthreads();
    layer_relu(bA, a.PA, a.dimO, Q.W1, Q.b1, a.l1, bB, a.PB, nullptr, 0, t);
    __syncthreads();
    layer_relu(bB, a.PB, a.l1 + a.dimA, Q.W2, Q.b2, a.l2, bD, a.PD, nullptr, 0, t);
    __syncthreads();
    const float q = tile_dot(bD, a.PD, a.l2, Q.W3) + Q.b3[0];
    const int s32 = threadIdx.x >> 5;
    if ((threadIdx.x & 31) == 0 && s32 < t.rows) a.out[t.s0 + s32] = q;
}

// ---- the weight and bias gradients: one launch over the table of the six layers ----

constexpr int GW = 4;                    // waves per workgroup; a wave owns a 16 x 32 block of one layer's [(in + 1)][out]

// G[m][j] = sum_b X1[b][m] D[b][j] with X1 = [X, 1]: the row of ones makes the bias gradient row `in` of the same product.
// One fma chain over the batch in index order per element (no split of the sum, no atomics): the same bits on every run.
__global__ __launch_bounds__(64 * GW) void ddpg_grads_kernel(GradArgs a) {
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

// ---- the update of a table of parameter sets and loss_q ----

constexpr int UT = 256;
constexpr int UPT = 4;

__global__ __launch_bounds__(UT) void ddpg_update_kernel(UpdArgs u) {
#pragma clang fp contract(off)
    __shared__ float s_lr_t;
    __shared__ double red[UT];
    __shared__ int s_last;
    int which = 0, block = (int)blockIdx.x;
    while (which + 1 < u.sets && block >= u.set[which].blocks) block -= u.set[which++].blocks;
    const ParamSet &a = u.set[which];
    const bool has_target = a.target != nullptr;
    if (threadIdx.x == 0) {
        // updates done so far: the last workgroup writes the counts back only after every workgroup has taken its ticket, and
        // every workgroup reads its count before it takes one
        const int t = __hip_atomic_load(u.step + a.slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
        s_lr_t = (float)(a.lr * sqrt(1.0 - pow(u.beta2, (double)t)) / (1.0 - pow(u.beta1, (double)t)));
    }
    __syncthreads();
    const float lr_t = s_lr_t, eps = u.eps, tau = u.tau;
    const long long j0 = ((long long)block * UT + threadIdx.x) * UPT;
    double ssq = 0.0;
    if (j0 < a.n) {
        const int cnt = a.n - j0 < UPT ? (int)(a.n - j0) : UPT;
        float th[UPT] = {}, m[UPT] = {}, v[UPT] = {}, g[UPT] = {}, tt[UPT] = {};
        if (cnt == UPT) {
            const float4 t4 = *reinterpret_cast<const float4 *>(a.theta + j0);
            const float4 r4 = has_target ? *reinterpret_cast<const float4 *>(a.target + j0) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 m4 = *reinterpret_cast<const float4 *>(a.m + j0);
            const float4 v4 = *reinterpret_cast<const float4 *>(a.v + j0);
            const float4 g4 = *reinterpret_cast<const float4 *>(a.grad + j0);
            th[0] = t4.x; th[1] = t4.y; th[2] = t4.z; th[3] = t4.w;
            tt[0] = r4.x; tt[1] = r4.y; tt[2] = r4.z; tt[3] = r4.w;
            m[0] = m4.x; m[1] = m4.y; m[2] = m4.z; m[3] = m4.w;
            v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
            g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
        } else {
            for (int k = 0; k < cnt; ++k) {
                th[k] = a.theta[j0 + k]; tt[k] = has_target ? a.target[j0 + k] : 0.f;
                m[k] = a.m[j0 + k]; v[k] = a.v[j0 + k]; g[k] = a.grad[j0 + k];
            }
        }
#pragma unroll
        for (int k = 0; k < UPT; ++k) {
            // the element arithmetic of param_update_kernel (plain operators under the pragma; sqrt as the float of the
            // double root), with the decay term in front and the target rule behind, from the new theta
            const float old = th[k];
            ssq = ssq + (double)old * (double)old;                  // the padding elements are zero
            const float gk = a.k != 0.f ? g[k] + a.k * old : g[k];
            m[k] = u.b1 * m[k] + u.c1 * gk;
            v[k] = u.b2 * v[k] + u.c2 * (gk * gk);
            const float root = (float)__builtin_sqrt((double)v[k]);
            th[k] = old - (lr_t * m[k]) / (root + eps);
            tt[k] = tt[k] - tau * (tt[k] - th[k]);
        }
        if (cnt == UPT) {
            *reinterpret_cast<float4 *>(a.theta + j0) = make_float4(th[0], th[1], th[2], th[3]);
            if (has_target) *reinterpret_cast<float4 *>(a.target + j0) = make_float4(tt[0], tt[1], tt[2], tt[3]);
            *reinterpret_cast<float4 *>(a.m + j0) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4 *>(a.v + j0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int k = 0; k < cnt; ++k) {
                a.theta[j0 + k] = th[k]; a.m[j0 + k] = m[k]; a.v[j0 + k] = v[k];
                if (has_target) a.target[j0 + k] = tt[k];
            }
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

struct Pitches {
    int PA, PB, PC, PD, PS;
    int chain_bytes() const { return (TS * (PA + PB + PC + PD + 2 * PS) + 2 * TS) * (int)sizeof(float); }
    int fwd_bytes() const { return TS * (PA + PB + PD) * (int)sizeof(float); }
};
Pitches pitches(int dimO, int dimA, int l1, int l2) {
    return {pitch_of(max2(dimO, l2)), pitch_of(max2(l1 + dimA, l2)), pitch_of(max2(l1, l2)), pitch_of(l2), pitch_of(dimA)};
}

// the workspace, piece by piece (ICNN_BE_DDPG_W_*): float offsets
size_t work_walk(int B, int dimO, int dimA, int l1, int l2, long long *off) {
    Carver c{nullptr};
    const size_t b = (size_t)B;
    const int tiles = (B + TS - 1) / TS;
    const size_t width[ICNN_BE_DDPG_WORK_PIECES] = {
        b * dimA, b, b, b, b * dimA, b,                                     // a2, y, q, td, a, q(obs, a)
        b * (l1 + dimA), b * l2, b, b * l2, b * l1,                         // [h1, act], h2, delta3, delta2, delta1 (critic)
        b * l1, b * l2, b * l2, b * dimA, b * l2, b * l1,                   // h1, h2 (policy), h2 at pi(obs), deltas (policy)
        2 * (size_t)tiles,                                                  // sums of td^2, float64
        2 * (size_t)param_update_blocks(ddpg_critic_floats(dimO, dimA, l1, l2))};  // the update's partials, float64
    for (int i = 0; i < ICNN_BE_DDPG_WORK_PIECES; ++i) {
        if (off) off[i] = (long long)c.at;
        c.take(width[i]);
    }
    return c.at;
}

}  // namespace

long long ddpg_policy_floats(int dimO, int dimA, int l1, int l2) {
    return (long long)dimO * l1 + l1 + (long long)l1 * l2 + l2 + (long long)l2 * dimA + dimA;
}
long long ddpg_critic_floats(int dimO, int dimA, int l1, int l2) {
    return (long long)dimO * l1 + l1 + (long long)(l1 + dimA) * l2 + l2 + l2 + 1;
}

bool ddpg_fits(int dimO, int dimA, int l1, int l2) { return pitches(dimO, dimA, l1, l2).chain_bytes() <= LDS_BYTES; }

size_t ddpg_work_floats(int B, int dimO, int dimA, int l1, int l2, long long *off) { return work_walk(B, dimO, dimA, l1, l2, off); }

hipError_t launch_ddpg_chain(const icnn_be_ddpg_args &d, hipStream_t stream) {
    long long off[ICNN_BE_DDPG_WORK_PIECES];
    work_walk(d.batch, d.dimO, d.dimA, d.l1, d.l2, off);
    float *w = static_cast<float *>(d.work);
    const Pitches p = pitches(d.dimO, d.dimA, d.l1, d.l2);
    ChainArgs a{};
    a.B = d.batch; a.dimO = d.dimO; a.dimA = d.dimA; a.l1 = d.l1; a.l2 = d.l2;
    a.obs = d.obs; a.ob2 = d.ob2; a.rew = d.rew; a.act = d.act; a.term = d.term;
    a.tp = d.theta_p; a.tq = d.theta_q; a.ttp = d.target_p; a.ttq = d.target_q;
    a.discount = d.discount;
    a.inv_b = 1.f / (float)d.batch;
    a.a2 = w + off[ICNN_BE_DDPG_W_A2]; a.y = w + off[ICNN_BE_DDPG_W_Y]; a.q = w + off[ICNN_BE_DDPG_W_Q];
    a.td = w + off[ICNN_BE_DDPG_W_TD]; a.a = w + off[ICNN_BE_DDPG_W_A]; a.qpi = w + off[ICNN_BE_DDPG_W_QPI];
    a.xa = w + off[ICNN_BE_DDPG_W_XA]; a.h2q = w + off[ICNN_BE_DDPG_W_H2Q]; a.d3q = w + off[ICNN_BE_DDPG_W_D3Q];
    a.d2q = w + off[ICNN_BE_DDPG_W_D2Q]; a.d1q = w + off[ICNN_BE_DDPG_W_D1Q]; a.h1p = w + off[ICNN_BE_DDPG_W_H1P];
    a.h2p = w + off[ICNN_BE_DDPG_W_H2P]; a.h2c = w + off[ICNN_BE_DDPG_W_H2C]; a.d3p = w + off[ICNN_BE_DDPG_W_D3P];
    a.d2p = w + off[ICNN_BE_DDPG_W_D2P]; a.d1p = w + off[ICNN_BE_DDPG_W_D1P];
    a.sq = reinterpret_cast<double *>(w + off[ICNN_BE_DDPG_W_SQ]);
    a.PA = p.PA; a.PB = p.PB; a.PC = p.PC; a.PD = p.PD; a.PS = p.PS;
    return launch_kernel(ddpg_chain_kernel, dim3((d.batch + TS - 1) / TS), dim3(DT), p.chain_bytes(), stream, a);
}

hipError_t launch_ddpg_grads(const icnn_be_ddpg_args &d, hipStream_t stream) {
    long long off[ICNN_BE_DDPG_WORK_PIECES];
    work_walk(d.batch, d.dimO, d.dimA, d.l1, d.l2, off);
    float *w = static_cast<float *>(d.work);
    const int dimO = d.dimO, dimA = d.dimA, l1 = d.l1, l2 = d.l2;
    GradArgs a{};
    a.B = d.batch;
    // the layers in the order of the flat gradients
    float *g = d.grad_q;
    a.layer(d.obs, dimO, w + off[ICNN_BE_DDPG_W_D1Q], l1, g);
    a.layer(w + off[ICNN_BE_DDPG_W_XA], l1 + dimA, w + off[ICNN_BE_DDPG_W_D2Q], l2, g);
    a.layer(w + off[ICNN_BE_DDPG_W_H2Q], l2, w + off[ICNN_BE_DDPG_W_D3Q], 1, g);
    g = d.grad_p;
    a.layer(d.obs, dimO, w + off[ICNN_BE_DDPG_W_D1P], l1, g);
    a.layer(w + off[ICNN_BE_DDPG_W_H1P], l1, w + off[ICNN_BE_DDPG_W_D2P], l2, g);
    a.layer(w + off[ICNN_BE_DDPG_W_H2P], l2, w + off[ICNN_BE_DDPG_W_D3P], dimA, g);
    return launch_grad_table(a, stream);
}

hipError_t launch_grad_table(const GradArgs &a, hipStream_t stream) {
    return launch_kernel(ddpg_grads_kernel, dim3((a.waves + GW - 1) / GW), dim3(64 * GW), 0, stream, a);
}

void update_coefficients(UpdArgs &u, double beta1, double beta2) {
    u.beta1 = beta1;
    u.beta2 = beta2;
    u.b1 = (float)beta1;
    u.c1 = (float)(1.0 - beta1);
    u.b2 = (float)beta2;
    u.c2 = (float)(1.0 - beta2);
}

hipError_t launch_param_sets_update(const UpdArgs &u, hipStream_t stream) {
    int blocks = 0;
    for (int i = 0; i < u.sets; ++i) blocks += u.set[i].blocks;
    return launch_kernel(ddpg_update_kernel, dim3((unsigned)blocks), dim3(UT), 0, stream, u);
}

hipError_t launch_ddpg_update(const icnn_be_ddpg_args &d, bool with_loss, hipStream_t stream) {
    long long off[ICNN_BE_DDPG_WORK_PIECES];
    work_walk(d.batch, d.dimO, d.dimA, d.l1, d.l2, off);
    float *w = static_cast<float *>(d.work);
    UpdArgs u{};
    const long long nq = ddpg_critic_floats(d.dimO, d.dimA, d.l1, d.l2), np = ddpg_policy_floats(d.dimO, d.dimA, d.l1, d.l2);
    // 0: the critic (step count 0), 1: the policy (step count 1); only the critic's decay sum enters loss_q
    u.set[0] = ParamSet{d.theta_q, d.m_q, d.v_q, d.target_q, d.grad_q, nq, (int)param_update_blocks(nq), 0, d.l2norm, d.rate};
    u.set[1] = ParamSet{d.theta_p, d.m_p, d.v_p, d.target_p, d.grad_p, np, (int)param_update_blocks(np), 1, d.pl2norm, d.prate};
    u.sets = 2;
    u.step = d.step;
    u.slots = 2;
    u.reg_blocks = u.set[0].blocks;
    update_coefficients(u, d.beta1, d.beta2);
    u.eps = d.eps;
    u.tau = d.tau;
    u.loss = with_loss ? d.loss : nullptr;
    u.sq = reinterpret_cast<const double *>(w + off[ICNN_BE_DDPG_W_SQ]);
    u.tiles = (d.batch + TS - 1) / TS;
    u.batch = d.batch;
    u.l2norm = (double)d.l2norm;
    u.partial = reinterpret_cast<double *>(w + off[ICNN_BE_DDPG_W_UPD]);
    return launch_param_sets_update(u, stream);
}

hipError_t launch_ddpg_forward(bool critic, int dimO, int dimA, int l1, int l2, const float *theta, const float *obs,
                               const double *act, int B, float *out, hipStream_t stream) {
    const Pitches p = pitches(dimO, dimA, l1, l2);
    FwdArgs a{B, dimO, dimA, l1, l2, theta, obs, act, out, p.PA, p.PB, p.PD};
    return launch_kernel(critic ? ddpg_q_kernel : ddpg_act_kernel, dim3((B + TS - 1) / TS), dim3(DT), p.fwd_bytes(), stream, a);
}

}  // namespace icnn_be
