// The DDPG agent's training step and act() on the device (RL/src/ddpg.py, ddpg_nets_dm.py; include/icnn_be.h,
// icnn_be_ddpg_*).  Parameters are flat float32 vectors in the order W1, b1, W2, b2, W3, b3 with W row-major
// [in][out]; the forward products read W as it lies, the backward products read it transposed -- no packed copy.
//
//   ddpg_chain_kernel    everything of a step that stays inside one sample, one workgroup per 16-sample tile, activations in
//                        LDS: the target path (a2, q2, y), the critic at (obs, act) with td and the tile's sum of td^2, the
//                        policy and the critic at (obs, pi(obs)), and both backward chains down to the pre-activation deltas.
//                        Layer inputs and deltas go to the workspace; rows past the batch and columns past a width are
//                        predicated off.  No grid barrier: nothing in it crosses samples.
//   the weight gradients  grad_table_kernel (be_train_table.hip) over a table of the six layers.
//   the update            param_sets_update_kernel (be_train_table.hip) over two parameter sets, the critic's and the
//                        policy's, each with a target and a step count of its own; only the critic's sum theta_old^2 enters
//                        loss_q.
//   ddpg_act_kernel      pi(obs) for B observations, ddpg_q_kernel Q(obs, act): the layer routines of the chain kernel, so
//                        the bits of its policy output.
//
// Products: mfma_f32_16x16x4f32, a wave owning two 16-column tiles of the output at a time (two independent accumulators);
// per 16 values of k a lane takes four consecutive k (the k order inside the block is permuted alike in both operands).
#include "be_api_check.h"
#include "be_kernels.h"
#include "be_tile.h"
#include "be_train_common.h"
#include "be_train_table.h"

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

struct Pitches {
    int PA, PB, PC, PD, PS;
    int chain_bytes() const { return (TS * (PA + PB + PC + PD + 2 * PS) + 2 * TS) * (int)sizeof(float); }
    int fwd_bytes() const { return TS * (PA + PB + PD) * (int)sizeof(float); }
};
Pitches pitches(int dimO, int dimA, int l1, int l2) {
    return {pitch_of(max2(dimO, l2)), pitch_of(max2(l1 + dimA, l2)), pitch_of(max2(l1, l2)), pitch_of(l2), pitch_of(dimA)};
}

long long ddpg_policy_floats(int dimO, int dimA, int l1, int l2) {
    return (long long)dimO * l1 + l1 + (long long)l1 * l2 + l2 + (long long)l2 * dimA + dimA;
}
long long ddpg_critic_floats(int dimO, int dimA, int l1, int l2) {
    return (long long)dimO * l1 + l1 + (long long)(l1 + dimA) * l2 + l2 + l2 + 1;
}

// the workspace, piece by piece (ICNN_BE_DDPG_W_*): float offsets; off may be NULL
size_t work_walk(int B, int dimO, int dimA, int l1, int l2, long long *off) {
    const size_t b = (size_t)B;
    const int tiles = (B + TS - 1) / TS;
    const size_t width[ICNN_BE_DDPG_WORK_PIECES] = {
        b * dimA, b, b, b, b * dimA, b,                                     // a2, y, q, td, a, q(obs, a)
        b * (l1 + dimA), b * l2, b, b * l2, b * l1,                         // [h1, act], h2, delta3, delta2, delta1 (critic)
        b * l1, b * l2, b * l2, b * dimA, b * l2, b * l1,                   // h1, h2 (policy), h2 at pi(obs), deltas (policy)
        2 * (size_t)tiles,                                                  // sums of td^2, float64
        2 * (size_t)param_update_blocks(ddpg_critic_floats(dimO, dimA, l1, l2))};  // the update's partials, float64
    return WorkPieces<ICNN_BE_DDPG_WORK_PIECES>::walk(width, off);
}

struct Work : WorkPieces<ICNN_BE_DDPG_WORK_PIECES> {
    Work(const icnn_be_ddpg_args &d) : WorkPieces(d.work) { work_walk(d.batch, d.dimO, d.dimA, d.l1, d.l2, off); }
};

hipError_t launch_ddpg_chain(const icnn_be_ddpg_args &d, hipStream_t stream) {
    const Work w(d);
    const Pitches p = pitches(d.dimO, d.dimA, d.l1, d.l2);
    ChainArgs a{};
    a.B = d.batch; a.dimO = d.dimO; a.dimA = d.dimA; a.l1 = d.l1; a.l2 = d.l2;
    a.obs = d.obs; a.ob2 = d.ob2; a.rew = d.rew; a.act = d.act; a.term = d.term;
    a.tp = d.theta_p; a.tq = d.theta_q; a.ttp = d.target_p; a.ttq = d.target_q;
    a.discount = d.discount;
    a.inv_b = 1.f / (float)d.batch;
    a.a2 = w.at(ICNN_BE_DDPG_W_A2); a.y = w.at(ICNN_BE_DDPG_W_Y); a.q = w.at(ICNN_BE_DDPG_W_Q);
    a.td = w.at(ICNN_BE_DDPG_W_TD); a.a = w.at(ICNN_BE_DDPG_W_A); a.qpi = w.at(ICNN_BE_DDPG_W_QPI);
    a.xa = w.at(ICNN_BE_DDPG_W_XA); a.h2q = w.at(ICNN_BE_DDPG_W_H2Q); a.d3q = w.at(ICNN_BE_DDPG_W_D3Q);
    a.d2q = w.at(ICNN_BE_DDPG_W_D2Q); a.d1q = w.at(ICNN_BE_DDPG_W_D1Q); a.h1p = w.at(ICNN_BE_DDPG_W_H1P);
    a.h2p = w.at(ICNN_BE_DDPG_W_H2P); a.h2c = w.at(ICNN_BE_DDPG_W_H2C); a.d3p = w.at(ICNN_BE_DDPG_W_D3P);
    a.d2p = w.at(ICNN_BE_DDPG_W_D2P); a.d1p = w.at(ICNN_BE_DDPG_W_D1P);
    a.sq = reinterpret_cast<double *>(w.at(ICNN_BE_DDPG_W_SQ));
    a.PA = p.PA; a.PB = p.PB; a.PC = p.PC; a.PD = p.PD; a.PS = p.PS;
    return launch_kernel(ddpg_chain_kernel, dim3((d.batch + TS - 1) / TS), dim3(DT), p.chain_bytes(), stream, a);
}

hipError_t launch_ddpg_grads(const icnn_be_ddpg_args &d, hipStream_t stream) {
    const Work w(d);
    const int dimO = d.dimO, dimA = d.dimA, l1 = d.l1, l2 = d.l2;
    GradArgs a{};
    a.B = d.batch;
    // the layers in the order of the flat gradients
    float *g = d.grad_q;
    a.layer(d.obs, dimO, w.at(ICNN_BE_DDPG_W_D1Q), l1, g);
    a.layer(w.at(ICNN_BE_DDPG_W_XA), l1 + dimA, w.at(ICNN_BE_DDPG_W_D2Q), l2, g);
    a.layer(w.at(ICNN_BE_DDPG_W_H2Q), l2, w.at(ICNN_BE_DDPG_W_D3Q), 1, g);
    g = d.grad_p;
    a.layer(d.obs, dimO, w.at(ICNN_BE_DDPG_W_D1P), l1, g);
    a.layer(w.at(ICNN_BE_DDPG_W_H1P), l1, w.at(ICNN_BE_DDPG_W_D2P), l2, g);
    a.layer(w.at(ICNN_BE_DDPG_W_H2P), l2, w.at(ICNN_BE_DDPG_W_D3P), dimA, g);
    return launch_grad_table(a, stream);
}

hipError_t launch_ddpg_update(const icnn_be_ddpg_args &d, bool with_loss, hipStream_t stream) {
    const Work w(d);
    ParamSetsArgs u{};
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
    u.sq = reinterpret_cast<const double *>(w.at(ICNN_BE_DDPG_W_SQ));
    u.tiles = (d.batch + TS - 1) / TS;
    u.batch = d.batch;
    u.l2norm = (double)d.l2norm;
    u.partial = reinterpret_cast<double *>(w.at(ICNN_BE_DDPG_W_UPD));
    return launch_param_sets_update(u, stream);
}

}  // namespace

// the sizes every icnn_be_ddpg_* entry accepts: the limits of include/icnn_be.h and the chain kernel's LDS
bool ddpg_sizes_ok(int dimO, int dimA, int l1, int l2) {
    return dimO >= 1 && dimO <= ICNN_BE_DDPG_MAX_OBS && dimA >= 1 && dimA <= ICNN_BE_DDPG_MAX_ACT && l1 >= 1 &&
           l1 <= ICNN_BE_DDPG_MAX_HIDDEN && l2 >= 1 && l2 <= ICNN_BE_DDPG_MAX_HIDDEN &&
           pitches(dimO, dimA, l1, l2).chain_bytes() <= LDS_BYTES;
}

hipError_t launch_ddpg_forward(bool critic, int dimO, int dimA, int l1, int l2, const float *theta, const float *obs,
                               const double *act, int B, float *out, hipStream_t stream) {
    const Pitches p = pitches(dimO, dimA, l1, l2);
    FwdArgs a{B, dimO, dimA, l1, l2, theta, obs, act, out, p.PA, p.PB, p.PD};
    return launch_kernel(critic ? ddpg_q_kernel : ddpg_act_kernel, dim3((B + TS - 1) / TS), dim3(DT), p.fwd_bytes(), stream, a);
}

namespace {
// what every icnn_be_ddpg_* entry that takes the descriptor refuses before any launch; need_loss: loss may not be NULL
int check_ddpg(const icnn_be_ddpg_args *a, void *stream, bool need_loss) {
    if (!a || !ddpg_sizes_ok(a->dimO, a->dimA, a->l1, a->l2)) return ICNN_BE_EINVAL;
    if (int rc = check_replay_step(*a, stream, need_loss)) return rc;
    const void *a16[] = {a->theta_q, a->theta_p, a->target_q, a->target_p, a->m_q, a->v_q, a->m_p, a->v_p, a->grad_q, a->grad_p};
    for (const void *p : a16)
        if (misaligned(p, 16)) return ICNN_BE_EINVAL;
    if (!(a->pl2norm >= 0.f) || !std::isfinite(a->pl2norm) || !std::isfinite(a->prate)) return ICNN_BE_EINVAL;
    return 0;
}
}  // namespace

}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_ddpg_param_floats(int dimO, int dimA, int l1, int l2, long long *np, long long *nq) {
    if (!ddpg_sizes_ok(dimO, dimA, l1, l2) || !np || !nq) return ICNN_BE_EINVAL;
    *np = ddpg_policy_floats(dimO, dimA, l1, l2);
    *nq = ddpg_critic_floats(dimO, dimA, l1, l2);
    return 0;
}

size_t icnn_be_ddpg_work_bytes(int batch, int dimO, int dimA, int l1, int l2) {
    if (batch < 1 || !ddpg_sizes_ok(dimO, dimA, l1, l2)) return 0;
    return work_walk(batch, dimO, dimA, l1, l2, nullptr) * sizeof(float);
}

int icnn_be_ddpg_work_offsets(int batch, int dimO, int dimA, int l1, int l2, long long off[ICNN_BE_DDPG_WORK_PIECES]) {
    if (batch < 1 || !ddpg_sizes_ok(dimO, dimA, l1, l2) || !off) return ICNN_BE_EINVAL;
    work_walk(batch, dimO, dimA, l1, l2, off);
    return 0;
}

int icnn_be_ddpg_chain(const icnn_be_ddpg_args *a, void *stream) {
    if (int rc = check_ddpg(a, stream, false)) return rc;
    return api_done(launch_ddpg_chain(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_ddpg_grads(const icnn_be_ddpg_args *a, void *stream) {
    if (int rc = check_ddpg(a, stream, false)) return rc;
    return api_done(launch_ddpg_grads(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_ddpg_update(const icnn_be_ddpg_args *a, void *stream) {
    if (int rc = check_ddpg(a, stream, false)) return rc;
    return api_done(launch_ddpg_update(*a, a->loss != nullptr, static_cast<hipStream_t>(stream)));
}

int icnn_be_ddpg_step(const icnn_be_ddpg_args *a, void *stream) {
    if (int rc = check_ddpg(a, stream, true)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_ddpg_chain(*a, s);
    if (e == hipSuccess) e = launch_ddpg_grads(*a, s);
    if (e == hipSuccess) e = launch_ddpg_update(*a, true, s);
    return api_done(e);
}

int icnn_be_ddpg_act(int dimO, int dimA, int l1, int l2, const float *theta_p, const float *obs, int batch, float *out,
                     void *stream) {
    if (batch < 1 || !ddpg_sizes_ok(dimO, dimA, l1, l2)) return ICNN_BE_EINVAL;
    if (misaligned(theta_p, 16) || misaligned(obs, 4) || misaligned(out, 4) || !stream_ok(stream)) return ICNN_BE_EINVAL;
    return api_done(launch_ddpg_forward(false, dimO, dimA, l1, l2, theta_p, obs, nullptr, batch, out,
                                        static_cast<hipStream_t>(stream)));
}

int icnn_be_ddpg_q(int dimO, int dimA, int l1, int l2, const float *theta_q, const float *obs, const double *act, int batch,
                   float *out, void *stream) {
    if (batch < 1 || !ddpg_sizes_ok(dimO, dimA, l1, l2)) return ICNN_BE_EINVAL;
    if (misaligned(theta_q, 16) || misaligned(obs, 4) || misaligned(act, 8) || misaligned(out, 4) || !stream_ok(stream))
        return ICNN_BE_EINVAL;
    return api_done(launch_ddpg_forward(true, dimO, dimA, l1, l2, theta_q, obs, act, batch, out,
                                        static_cast<hipStream_t>(stream)));
}

}  // extern "C"
