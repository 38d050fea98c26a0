// NAF's L-matrix head for one sample (be_naf.hip, be_naf_bn.hip): per-sample VALU work, a group of 32 lanes per
// sample with lane j owning column j of the L matrix and every sum one fma chain in index order.  The loops are uniform; a
// lane's own part is predicated behind the shuffle.  lr: the sample's l in LDS, row-major [dimA][dimA].  Device code only.
#pragma once
#include "be_kernels.h"

namespace icnn_be {

namespace {

struct NafHead {
    float uj, dl, e, hj, adv;            // u[j], delta[j], Lm[j][j], h[j] of lane j < dimA (0 beyond); A in every lane
};

// Lm, delta, h and A from u (su) and the float32 action (sd) of this sample
__device__ __forceinline__ NafHead naf_head_forward(const float *lr, const float *su, const float *sd, int dimA, int j) {
    const bool col = j < dimA;
    NafHead H;
    H.uj = col ? su[j] : 0.f;
    H.dl = col ? sd[j] - H.uj : 0.f;                             // delta[j]
    H.e = col ? expf(lr[j * dimA + j]) : 0.f;                    // Lm[j][j]
    float hj = 0.f;
    for (int i = 0; i < dimA; ++i) {
        const float di = __shfl(H.dl, i, 32);
        if (col && i >= j) hj = fmaf(di, i == j ? H.e : lr[i * dimA + j], hj);
    }
    float ss = 0.f;
    for (int c = 0; c < dimA; ++c) {
        const float hc = __shfl(hj, c, 32);
        ss = fmaf(hc, hc, ss);
    }
    H.hj = hj;
    H.adv = -0.5f * ss;
    return H;
}

// gh[j] = -d3 h[j] and u's delta before the tanh; lane j reads ROW j of l, so a barrier stands between this and naf_head_dl
__device__ __forceinline__ float naf_head_du(const NafHead &H, const float *lr, int dimA, int j, float d3, float &gh) {
    const bool col = j < dimA;
    gh = -d3 * H.hj;
    float acc_u = 0.f;
    for (int c = 0; c < dimA; ++c) {
        const float g = __shfl(gh, c, 32);
        if (col && c <= j) acc_u = fmaf(g, c == j ? H.e : lr[j * dimA + c], acc_u);
    }
    return -acc_u * (1.f - H.uj * H.uj);
}

// d loss / d l, column j: over l in LDS (lr_out, the sample's lr; NULL where no later phase of the kernel reads it) and into
// the sample's row g of the workspace where g is not NULL
__device__ __forceinline__ void naf_head_dl(const NafHead &H, float *lr_out, int dimA, int j, float gh, float *g) {
    const bool col = j < dimA;
    for (int i = 0; i < dimA; ++i) {
        const float di = __shfl(H.dl, i, 32);
        if (col) {
            const float v = i < j ? 0.f : i == j ? (di * gh) * H.e : di * gh;
            if (lr_out) lr_out[i * dimA + j] = v;
            if (g) g[i * dimA + j] = v;
        }
    }
}

}  // namespace

}  // namespace icnn_be
