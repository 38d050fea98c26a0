// The NAF agent's training step and Q(obs, act) on the device (RL/src/naf.py, naf_nets_dm.py with naf_bn False;
// include/icnn_be.h, icnn_be_naf_*).  Three nets L, U, V, each a flat float32 vector in the order W1, b1, W2,
// b2, W3, b3 with W row-major [in][out] -- the layout of DDPG's policy with the last width dimA^2, dimA and 1.
//
//   naf_chain_kernel     everything of a step that stays inside one sample, one workgroup per 16-sample tile, activations in
//                        LDS: the target mlp(ob2; V target) and y, the three forwards at obs, the head (Lm, delta, h, A), q,
//                        td and the tile's sum of td^2, the head's backward and the three backward chains down to the
//                        pre-activation deltas.  Products are tile_gemm of be_tile.h; the head is per-sample VALU work, a
//                        group of 32 lanes per sample with lane j owning column j of the L matrix and every sum one fma
//                        chain in index order (be_naf_head.h, shared with be_naf_bn.hip).  full = 0 stops after q: that is
//                        icnn_be_naf_q, with the chain's bits.
//   the weight gradients  grad_table_kernel (be_train_table.hip) over a table of the nine layers.
//   the update            param_sets_update_kernel (be_train_table.hip) over three parameter sets with one step count; only V
//                        has a target; sum theta_old^2 of all three enters loss_q.
//   u for B rows          the U net is DDPG's policy: icnn_be_naf_act launches ddpg_act_kernel on theta_u.
//
// LDS: bA holds the obs rows and later, when no first layer needs them any more, the dimA^2 wide l rows (then d loss / d l in
// place); bB and bC the two hidden layers of the net at hand.  The hidden layers of U and V are not kept: their backward
// chains re-read the masks from the workspace, which this workgroup wrote.
#include "be_api_check.h"
#include "be_kernels.h"
#include "be_naf_head.h"
#include "be_tile.h"
#include "be_train_common.h"
#include "be_train_table.h"

namespace icnn_be {

namespace {

struct NafChainArgs {
    int B, dimO, dimA, l1, l2, full;
    const float *obs, *ob2, *rew;
    const double *act;
    const unsigned char *term;
    const float *tl, *tu, *tv, *ttv;
    float discount, inv_b;
    // every piece but q may be NULL where full is 0
    float *y, *u, *l, *ld, *h, *adv, *q, *td, *h1l, *h2l, *h1u, *h2u, *h1v, *h2v;
    float *d3l, *d2l, *d1l, *d3u, *d2u, *d1u, *d3v, *d2v, *d1v;
    double *sq;
    int PA, PB, PC, PS;
};

__global__ __launch_bounds__(DT) void naf_chain_kernel(NafChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, dimO = a.dimO, dimA = a.dimA, l1 = a.l1, l2 = a.l2, nL = dimA * dimA;
    const int PA = a.PA, PB = a.PB, PC = a.PC, PS = a.PS;
    float *bA = lds, *bB = bA + TS * PA, *bC = bB + TS * PB, *sU = bC + TS * PC, *sD = sU + TS * PS;
    float *vt = sD + TS * PS, *vd = vt + TS;
    Tile t;
    t.s0 = blockIdx.x * TS;
    t.rows = a.B - t.s0 < TS ? a.B - t.s0 : TS;
    const Net L = policy_net(a.tl, dimO, nL, l1, l2), U = policy_net(a.tu, dimO, dimA, l1, l2), V = policy_net(a.tv, dimO, 1, l1, l2);
    const int s32 = tid >> 5, j = tid & 31;                     // the head: lane j of the group of sample s32
    const bool row = s32 < t.rows, col = j < dimA;
    const size_t gs = (size_t)(t.s0 + s32);

    // ---- the target: y from mlp(ob2; V target); its advantage is the constant 0 ----
    float y = 0.f;
    if (a.full) {
        const Net VT = policy_net(a.ttv, dimO, 1, l1, l2);
        load_rows(bA, PA, 0, a.ob2, dimO, t);
        __syncthreads();
        layer_relu(bA, PA, dimO, VT.W1, VT.b1, l1, bB, PB, nullptr, 0, t);
        __syncthreads();
        layer_relu(bB, PB, l1, VT.W2, VT.b2, l2, bC, PC, nullptr, 0, t);
        __syncthreads();
        const float q2 = tile_dot(bC, PC, l2, VT.W3) + VT.b3[0];
        if (row) {
            const float r = a.rew[gs];
            y = a.term[gs] ? r : r + a.discount * q2;
            if (j == 0) a.y[gs] = y;
        }
        __syncthreads();
    }
    // ---- the three forwards at obs: U, V, then L, whose output takes the place of the obs rows ----
    load_rows(bA, PA, 0, a.obs, dimO, t);
    load_rows(sD, PS, 0, a.act, dimA, t);                        // float64 actions, rounded to float32 once
    __syncthreads();
    layer_relu(bA, PA, dimO, U.W1, U.b1, l1, bB, PB, a.h1u, l1, t);
    __syncthreads();
    layer_relu(bB, PB, l1, U.W2, U.b2, l2, bC, PC, a.h2u, l2, t);
    __syncthreads();
    tile_gemm(bC, PC, l2, U.W3, dimA, 1, dimA, [&](int s, int c, float acc) {       // layer_tanh's arithmetic
        const float v = tanhf(acc + U.b3[c]);
        sU[s * PS + c] = v;
        if (a.u && s < t.rows) a.u[(size_t)(t.s0 + s) * dimA + c] = v;
    });
    layer_relu(bA, PA, dimO, V.W1, V.b1, l1, bB, PB, a.h1v, l1, t);
    __syncthreads();
    layer_relu(bB, PB, l1, V.W2, V.b2, l2, bC, PC, a.h2v, l2, t);
    __syncthreads();
    const float v = tile_dot(bC, PC, l2, V.W3) + V.b3[0];
    layer_relu(bA, PA, dimO, L.W1, L.b1, l1, bB, PB, a.h1l, l1, t);
    __syncthreads();
    layer_relu(bB, PB, l1, L.W2, L.b2, l2, bC, PC, a.h2l, l2, t);
    __syncthreads();
    tile_gemm(bC, PC, l2, L.W3, nL, 1, nL, [&](int s, int c, float acc) {
        const float x = acc + L.b3[c];
        bA[s * PA + c] = x;
        if (a.l && s < t.rows) a.l[(size_t)(t.s0 + s) * nL + c] = x;
    });
    __syncthreads();
    // ---- the head: Lm, delta, h, A, q.  The loops are uniform; a lane's own part is predicated behind the shuffle ----
    float *lr = bA + s32 * PA;                                   // l of this sample, row-major [dimA][dimA]
    const NafHead H = naf_head_forward(lr, sU + s32 * PS, sD + s32 * PS, dimA, j);
    const float e = H.e, hj = H.hj, adv = H.adv, q = v + adv;
    if (row && j == 0) a.q[gs] = q;
    if (!a.full) return;
    const float td = q - y, d3 = a.inv_b * (2.f * td);
    if (row) {
        if (col) {
            a.ld[gs * dimA + j] = e;
            a.h[gs * dimA + j] = hj;
        }
        if (j == 0) {
            a.adv[gs] = adv;
            a.td[gs] = td;
            a.d3v[gs] = d3;
        }
    }
    if (j == 0) {
        vt[s32] = row ? td : 0.f;
        vd[s32] = row ? d3 : 0.f;
    }
    // ---- the head's backward: gh[j] = -d3 h[j]; lane j reads ROW j of l for u's delta before the columns are overwritten ----
    float gh;
    const float du = naf_head_du(H, lr, dimA, j, d3, gh);
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < t.rows; ++i) s = s + (double)vt[i] * (double)vt[i];
        a.sq[blockIdx.x] = s;
    }
    if (col) {
        sD[s32 * PS + j] = du;
        if (row) a.d3u[gs * dimA + j] = du;
    }
    naf_head_dl(H, lr, dimA, j, gh, row ? a.d3l + gs * nL : nullptr);       // d loss / d l, column j, in place
    __syncthreads();
    // ---- L's backward chain: its hidden layers are still in bB and bC ----
    tile_gemm(bA, PA, nL, L.W3, 1, nL, l2, [&](int s, int c, float acc) {
        const float d = bC[s * PC + c] > 0.f ? acc : 0.f;        // this element is read and written by this lane alone
        bC[s * PC + c] = d;
        if (s < t.rows) a.d2l[(size_t)(t.s0 + s) * l2 + c] = d;
    });
    __syncthreads();
    tile_gemm(bC, PC, l2, L.W2, 1, l2, l1, [&](int s, int c, float acc) {
        if (s < t.rows) a.d1l[(size_t)(t.s0 + s) * l1 + c] = bB[s * PB + c] > 0.f ? acc : 0.f;
    });
    __syncthreads();
    // ---- U's and V's: the masks from the workspace ----
    tile_gemm(sD, PS, dimA, U.W3, 1, dimA, l2, [&](int s, int c, float acc) {
        float d = 0.f;
        if (s < t.rows) {
            const size_t at = (size_t)(t.s0 + s) * l2 + c;
            d = a.h2u[at] > 0.f ? acc : 0.f;
            a.d2u[at] = d;
        }
        bC[s * PC + c] = d;
    });
    __syncthreads();
    tile_gemm(bC, PC, l2, U.W2, 1, l2, l1, [&](int s, int c, float acc) {
        if (s < t.rows) {
            const size_t at = (size_t)(t.s0 + s) * l1 + c;
            a.d1u[at] = a.h1u[at] > 0.f ? acc : 0.f;
        }
    });
    __syncthreads();
    for (int i = tid; i < TS * l2; i += DT) {
        const int s = i / l2, n = i - s * l2;
        float d = 0.f;
        if (s < t.rows) {
            const size_t at = (size_t)(t.s0 + s) * l2 + n;
            d = a.h2v[at] > 0.f ? vd[s] * V.W3[n] : 0.f;
            a.d2v[at] = d;
        }
        bC[s * PC + n] = d;
    }
    __syncthreads();
    tile_gemm(bC, PC, l2, V.W2, 1, l2, l1, [&](int s, int c, float acc) {
        if (s < t.rows) {
            const size_t at = (size_t)(t.s0 + s) * l1 + c;
            a.d1v[at] = a.h1v[at] > 0.f ? acc : 0.f;
        }
    });
}

struct Pitches {
    int PA, PB, PC, PS;
    int bytes() const { return (TS * (PA + PB + PC + 2 * PS) + 2 * TS) * (int)sizeof(float); }
};
Pitches pitches(int dimO, int dimA, int l1, int l2) {
    return {pitch_of(max2(dimO, dimA * dimA)), pitch_of(l1), pitch_of(l2), pitch_of(dimA)};
}

long long naf_net_floats(int dimO, int l1, int l2, int out) {      // out: dimA^2 (L), dimA (U), 1 (V)
    return (long long)dimO * l1 + l1 + (long long)l1 * l2 + l2 + (long long)l2 * out + out;
}

long long update_blocks(int dimO, int dimA, int l1, int l2) {
    return param_update_blocks(naf_net_floats(dimO, l1, l2, dimA * dimA)) + param_update_blocks(naf_net_floats(dimO, l1, l2, dimA)) +
           param_update_blocks(naf_net_floats(dimO, l1, l2, 1));
}

// the workspace, piece by piece (ICNN_BE_NAF_W_*): float offsets; off may be NULL
size_t work_walk(int B, int dimO, int dimA, int l1, int l2, long long *off) {
    const size_t b = (size_t)B, nL = (size_t)dimA * dimA;
    const int tiles = (B + TS - 1) / TS;
    const size_t width[ICNN_BE_NAF_WORK_PIECES] = {
        b, b * dimA, b * nL, b * dimA, b * dimA, b, b, b,                   // y, u, l, diag Lm, h, A, q, td
        b * l1, b * l2, b * l1, b * l2, b * l1, b * l2,                     // h1, h2 of L, U, V
        b * nL, b * l2, b * l1, b * dimA, b * l2, b * l1, b, b * l2, b * l1,   // the deltas of L, U, V
        2 * (size_t)tiles,                                                  // sums of td^2, float64
        2 * (size_t)update_blocks(dimO, dimA, l1, l2)};                     // the update's partials, float64
    return WorkPieces<ICNN_BE_NAF_WORK_PIECES>::walk(width, off);
}

struct Work : WorkPieces<ICNN_BE_NAF_WORK_PIECES> {
    Work(const icnn_be_naf_args &d) : WorkPieces(d.work) { work_walk(d.batch, d.dimO, d.dimA, d.l1, d.l2, off); }
};

hipError_t launch_naf_chain(const icnn_be_naf_args &d, hipStream_t stream) {
    const Work w(d);
    const Pitches p = pitches(d.dimO, d.dimA, d.l1, d.l2);
    NafChainArgs a{};
    a.B = d.batch; a.dimO = d.dimO; a.dimA = d.dimA; a.l1 = d.l1; a.l2 = d.l2; a.full = 1;
    a.obs = d.obs; a.ob2 = d.ob2; a.rew = d.rew; a.act = d.act; a.term = d.term;
    a.tl = d.theta_l; a.tu = d.theta_u; a.tv = d.theta_v; a.ttv = d.target_v;
    a.discount = d.discount;
    a.inv_b = 1.f / (float)d.batch;
    a.y = w.at(ICNN_BE_NAF_W_Y); a.u = w.at(ICNN_BE_NAF_W_U); a.l = w.at(ICNN_BE_NAF_W_L);
    a.ld = w.at(ICNN_BE_NAF_W_LD); a.h = w.at(ICNN_BE_NAF_W_H); a.adv = w.at(ICNN_BE_NAF_W_ADV);
    a.q = w.at(ICNN_BE_NAF_W_Q); a.td = w.at(ICNN_BE_NAF_W_TD);
    a.h1l = w.at(ICNN_BE_NAF_W_H1L); a.h2l = w.at(ICNN_BE_NAF_W_H2L); a.h1u = w.at(ICNN_BE_NAF_W_H1U);
    a.h2u = w.at(ICNN_BE_NAF_W_H2U); a.h1v = w.at(ICNN_BE_NAF_W_H1V); a.h2v = w.at(ICNN_BE_NAF_W_H2V);
    a.d3l = w.at(ICNN_BE_NAF_W_D3L); a.d2l = w.at(ICNN_BE_NAF_W_D2L); a.d1l = w.at(ICNN_BE_NAF_W_D1L);
    a.d3u = w.at(ICNN_BE_NAF_W_D3U); a.d2u = w.at(ICNN_BE_NAF_W_D2U); a.d1u = w.at(ICNN_BE_NAF_W_D1U);
    a.d3v = w.at(ICNN_BE_NAF_W_D3V); a.d2v = w.at(ICNN_BE_NAF_W_D2V); a.d1v = w.at(ICNN_BE_NAF_W_D1V);
    a.sq = reinterpret_cast<double *>(w.at(ICNN_BE_NAF_W_SQ));
    a.PA = p.PA; a.PB = p.PB; a.PC = p.PC; a.PS = p.PS;
    return launch_kernel(naf_chain_kernel, dim3((d.batch + TS - 1) / TS), dim3(DT), p.bytes(), stream, a);
}

hipError_t launch_naf_q(int dimO, int dimA, int l1, int l2, const float *theta_l, const float *theta_u, const float *theta_v,
                        const float *obs, const double *act, int B, float *out, hipStream_t stream) {
    const Pitches p = pitches(dimO, dimA, l1, l2);
    NafChainArgs a{};
    a.B = B; a.dimO = dimO; a.dimA = dimA; a.l1 = l1; a.l2 = l2; a.full = 0;
    a.obs = obs; a.act = act;
    a.tl = theta_l; a.tu = theta_u; a.tv = theta_v;
    a.q = out;
    a.PA = p.PA; a.PB = p.PB; a.PC = p.PC; a.PS = p.PS;
    return launch_kernel(naf_chain_kernel, dim3((B + TS - 1) / TS), dim3(DT), p.bytes(), stream, a);
}

hipError_t launch_naf_grads(const icnn_be_naf_args &d, hipStream_t stream) {
    const Work w(d);
    const int dimO = d.dimO, dimA = d.dimA, l1 = d.l1, l2 = d.l2;
    GradArgs a{};
    a.B = d.batch;
    // the nine layers in the order of the three flat gradients
    float *g = d.grad_l;
    a.layer(d.obs, dimO, w.at(ICNN_BE_NAF_W_D1L), l1, g);
    a.layer(w.at(ICNN_BE_NAF_W_H1L), l1, w.at(ICNN_BE_NAF_W_D2L), l2, g);
    a.layer(w.at(ICNN_BE_NAF_W_H2L), l2, w.at(ICNN_BE_NAF_W_D3L), dimA * dimA, g);
    g = d.grad_u;
    a.layer(d.obs, dimO, w.at(ICNN_BE_NAF_W_D1U), l1, g);
    a.layer(w.at(ICNN_BE_NAF_W_H1U), l1, w.at(ICNN_BE_NAF_W_D2U), l2, g);
    a.layer(w.at(ICNN_BE_NAF_W_H2U), l2, w.at(ICNN_BE_NAF_W_D3U), dimA, g);
    g = d.grad_v;
    a.layer(d.obs, dimO, w.at(ICNN_BE_NAF_W_D1V), l1, g);
    a.layer(w.at(ICNN_BE_NAF_W_H1V), l1, w.at(ICNN_BE_NAF_W_D2V), l2, g);
    a.layer(w.at(ICNN_BE_NAF_W_H2V), l2, w.at(ICNN_BE_NAF_W_D3V), 1, g);
    return launch_grad_table(a, stream);
}

hipError_t launch_naf_update(const icnn_be_naf_args &d, bool with_loss, hipStream_t stream) {
    const Work w(d);
    ParamSetsArgs u{};
    const long long nl = naf_net_floats(d.dimO, d.l1, d.l2, d.dimA * d.dimA), nu = naf_net_floats(d.dimO, d.l1, d.l2, d.dimA),
                    nv = naf_net_floats(d.dimO, d.l1, d.l2, 1);
    // one optimizer: the three sets read the one step count; only V has a target; all three enter loss_q's decay sum
    u.set[0] = ParamSet{d.theta_l, d.m_l, d.v_l, nullptr, d.grad_l, nl, (int)param_update_blocks(nl), 0, d.l2norm, d.rate};
    u.set[1] = ParamSet{d.theta_u, d.m_u, d.v_u, nullptr, d.grad_u, nu, (int)param_update_blocks(nu), 0, d.l2norm, d.rate};
    u.set[2] = ParamSet{d.theta_v, d.m_v, d.v_v, d.target_v, d.grad_v, nv, (int)param_update_blocks(nv), 0, d.l2norm, d.rate};
    u.sets = 3;
    u.step = d.step;
    u.slots = 1;
    u.reg_blocks = u.set[0].blocks + u.set[1].blocks + u.set[2].blocks;
    update_coefficients(u, d.beta1, d.beta2);
    u.eps = d.eps;
    u.tau = d.tau;
    u.loss = with_loss ? d.loss : nullptr;
    u.sq = reinterpret_cast<const double *>(w.at(ICNN_BE_NAF_W_SQ));
    u.tiles = (d.batch + TS - 1) / TS;
    u.batch = d.batch;
    u.l2norm = (double)d.l2norm;
    u.partial = reinterpret_cast<double *>(w.at(ICNN_BE_NAF_W_UPD));
    return launch_param_sets_update(u, stream);
}

// what every icnn_be_naf_* entry that takes the descriptor refuses before any launch; need_loss: loss may not be NULL
int check_naf(const icnn_be_naf_args *a, void *stream, bool need_loss) {
    if (!a || !naf_sizes_ok(a->dimO, a->dimA, a->l1, a->l2)) return ICNN_BE_EINVAL;
    if (int rc = check_replay_step(*a, stream, need_loss)) return rc;
    const void *a16[] = {a->theta_l, a->theta_u, a->theta_v, a->target_v, a->m_l, a->v_l, a->m_u, a->v_u, a->m_v, a->v_v,
                         a->grad_l, a->grad_u, a->grad_v};
    for (const void *p : a16)
        if (misaligned(p, 16)) return ICNN_BE_EINVAL;
    return 0;
}

}  // namespace

// the sizes every icnn_be_naf_* entry accepts (and, with its own on top, every icnn_be_naf_bn_* entry): the limits of
// include/icnn_be.h and the chain kernel's LDS
bool naf_sizes_ok(int dimO, int dimA, int l1, int l2) {
    return dimO >= 1 && dimO <= ICNN_BE_NAF_MAX_OBS && dimA >= 1 && dimA <= ICNN_BE_NAF_MAX_ACT && l1 >= 1 &&
           l1 <= ICNN_BE_NAF_MAX_HIDDEN && l2 >= 1 && l2 <= ICNN_BE_NAF_MAX_HIDDEN &&
           pitches(dimO, dimA, l1, l2).bytes() <= LDS_BYTES;
}

}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_naf_param_floats(int dimO, int dimA, int l1, int l2, long long *nl, long long *nu, long long *nv) {
    if (!naf_sizes_ok(dimO, dimA, l1, l2) || !nl || !nu || !nv) return ICNN_BE_EINVAL;
    *nl = naf_net_floats(dimO, l1, l2, dimA * dimA);
    *nu = naf_net_floats(dimO, l1, l2, dimA);
    *nv = naf_net_floats(dimO, l1, l2, 1);
    return 0;
}

size_t icnn_be_naf_work_bytes(int batch, int dimO, int dimA, int l1, int l2) {
    if (batch < 1 || !naf_sizes_ok(dimO, dimA, l1, l2)) return 0;
    return work_walk(batch, dimO, dimA, l1, l2, nullptr) * sizeof(float);
}

int icnn_be_naf_work_offsets(int batch, int dimO, int dimA, int l1, int l2, long long off[ICNN_BE_NAF_WORK_PIECES]) {
    if (batch < 1 || !naf_sizes_ok(dimO, dimA, l1, l2) || !off) return ICNN_BE_EINVAL;
    work_walk(batch, dimO, dimA, l1, l2, off);
    return 0;
}

int icnn_be_naf_chain(const icnn_be_naf_args *a, void *stream) {
    if (int rc = check_naf(a, stream, false)) return rc;
    return api_done(launch_naf_chain(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_naf_grads(const icnn_be_naf_args *a, void *stream) {
    if (int rc = check_naf(a, stream, false)) return rc;
    return api_done(launch_naf_grads(*a, static_cast<hipStream_t>(stream)));
}

int icnn_be_naf_update(const icnn_be_naf_args *a, void *stream) {
    if (int rc = check_naf(a, stream, false)) return rc;
    return api_done(launch_naf_update(*a, a->loss != nullptr, static_cast<hipStream_t>(stream)));
}

int icnn_be_naf_step(const icnn_be_naf_args *a, void *stream) {
    if (int rc = check_naf(a, stream, true)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch_naf_chain(*a, s);
    if (e == hipSuccess) e = launch_naf_grads(*a, s);
    if (e == hipSuccess) e = launch_naf_update(*a, true, s);
    return api_done(e);
}

int icnn_be_naf_act(int dimO, int dimA, int l1, int l2, const float *theta_u, const float *obs, int batch, float *out,
                    void *stream) {
    // the U net is DDPG's policy; its launch needs DDPG's LDS plan, which holds wherever NAF's does
    if (batch < 1 || !naf_sizes_ok(dimO, dimA, l1, l2) || !ddpg_sizes_ok(dimO, dimA, l1, l2)) return ICNN_BE_EINVAL;
    if (misaligned(theta_u, 16) || misaligned(obs, 4) || misaligned(out, 4) || !stream_ok(stream)) return ICNN_BE_EINVAL;
    return api_done(launch_ddpg_forward(false, dimO, dimA, l1, l2, theta_u, obs, nullptr, batch, out,
                                        static_cast<hipStream_t>(stream)));
}

int icnn_be_naf_q(int dimO, int dimA, int l1, int l2, const float *theta_l, const float *theta_u, const float *theta_v,
                  const float *obs, const double *act, int batch, float *out, void *stream) {
    if (batch < 1 || !naf_sizes_ok(dimO, dimA, l1, l2)) return ICNN_BE_EINVAL;
    if (misaligned(theta_l, 16) || misaligned(theta_u, 16) || misaligned(theta_v, 16) || misaligned(obs, 4) || misaligned(act, 8) ||
        misaligned(out, 4) || !stream_ok(stream))
        return ICNN_BE_EINVAL;
    return api_done(launch_naf_q(dimO, dimA, l1, l2, theta_l, theta_u, theta_v, obs, act, batch, out,
                                 static_cast<hipStream_t>(stream)));
}

}  // extern "C"
