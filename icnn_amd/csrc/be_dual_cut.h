// Dual step, device helpers: the cut types (float32 / float64 rows and their NumPy-exact sigmoid), the LDS carve-up that host
// and device share, and the wave-uniform / opaque-value helpers.  Included by be_dual_dev.h; everything is in an anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "be_common.h"
#include "icnn_be.h"

namespace icnn_be {

namespace {

template <typename T> struct Cut;
// NumPy's float32 exp is not correctly rounded (39 % of results are 1-2 ulp off); the
// reference computes the k = 1 update y = 1/(1+exp(g)) with it in float32 (dual :168), and
// that y is the point of the next cut.  To start from bit-identical iterates the device
// evaluates the same operation sequence as numpy/_core/src/umath/
// loops_exponent_log.dispatch.c.src (simd_exp_FLOAT, AVX512F/AVX2 paths): Cody-Waite
// reduction by round(x log2e) with fused multiply-adds, a (5,2) rational minimax, scalef.
// Every operation is a single IEEE float32 rounding, so the result is bit-identical
// (checked against np.exp on the GPU box by tests/test_gpu_parity.py).
__device__ __noinline__ float numpy_expf(float x) {
#pragma clang fp contract(off)
    if (x != x) return x;
    if (x >= 88.72283935546875f) return __builtin_inff();
    if (x <= -103.97208404541015625f) return 0.0f;
    float q = x * 1.44269504088896341f;
    q = q + 12582912.0f;                       // 0x1.8p23: round to nearest integer
    q = q - 12582912.0f;
    float r = __builtin_fmaf(q, -6.93145752e-1f, x);
    r = __builtin_fmaf(q, -1.42860677e-6f, r);
    float num = __builtin_fmaf(5.082762527590693718096e-04f, r, 6.757896990527504603057e-03f);
    num = __builtin_fmaf(num, r, 5.114512081637298353406e-02f);
    num = __builtin_fmaf(num, r, 2.473615434895520810817e-01f);
    num = __builtin_fmaf(num, r, 7.257664613233124478488e-01f);
    num = __builtin_fmaf(num, r, 9.999999999980870924916e-01f);
    float den = __builtin_fmaf(2.159509375685829852307e-02f, r, -2.742335390411667452936e-01f);
    den = __builtin_fmaf(den, r, 1.0f);
    const float poly = num / den;
    return ldexpf(poly, (int)q);
}

template <> struct Cut<float> {
    static constexpr double eps = 1.1920928955078125e-07;
    static __device__ __forceinline__ float sigmoid_neg(float g) {
#pragma clang fp contract(off)
        const float e = numpy_expf(g);
        const float d = 1.0f + e;
        return 1.0f / d;
    }
};
template <> struct Cut<double> {
    static constexpr double eps = 2.220446049250313e-16;
    static __device__ __forceinline__ double sigmoid_neg(double g) { return 1.0 / (1.0 + exp(g)); }
};

__device__ __forceinline__ double softplus_stable(double v) {   // dual :6-12
    return v > 1.0 ? log1p(exp(-v)) + v : log1p(exp(v));
}

// LDS carve-up shared by host (size query) and device.  The pairwise-sum scratch aliases the
// Hm region (they are never live together).
struct Carve {
    int As, zs, ws, sp, yv, dv, Hm, Hp, ints, total;
};
constexpr int IPM_KMAX_WAVES = 20; // most cuts ipm_solve_waves (be_ipm_dev.h, 256-register kernels) takes
// rl: variant RL keeps the softplus terms in a column buffer of its own; ipm: the interior-point variant needs that
// buffer (residual ry) and two more (y, dy)
__host__ __device__ inline Carve carve(int KT, int rows, int ldA, int n_pad, int cut_bytes, int n_leaves,
                                       bool rl, int nw = 1, bool own_const_rows = true, bool ipm = false,
                                       bool glb = false) {
    Carve c;
    int o = 0;
    auto take = [&](int bytes) { int at = o; o += (bytes + 15) & ~15; return at; };
    // + a row of zeros and a row of ones (contract_mfma) unless shared; glb: the rows live in device memory (st.scratch)
    c.As = take(glb ? 0 : (rows + (own_const_rows ? 2 : 0)) * ldA * cut_bytes);
    c.zs = take(n_pad * 8);
    c.ws = take(n_pad * 8);
    c.sp = (rl || ipm) ? take(n_pad * 8) : c.ws;
    c.yv = ipm ? take(n_pad * 8) : c.zs;
    c.dv = ipm ? take(n_pad * 8) : c.zs;
    const int hp = (rows + 1) | 1;
    int hm = rows * hp * 8;
    const int scratch = (KT * n_leaves + 2 * KT) * 8;
    if (scratch > hm) hm = scratch;
    c.Hm = take(hm);
    // per-wave partial contractions (the rank test's Gram matrix of ALL rows in both variants, the Newton system of variant
    // dual) / each wave's own copy of the k x (k + 1) system (interior point on several waves).  Where this does not fit next to
    // the column buffers the launcher takes the one-wave instance (launch_dual_step: interior point at n_pad = 3072 from 23 rows)
    c.Hp = nw > 1 ? take(nw * rows * hp * 8) : c.Hm;
    c.ints = take(KT * 4);
    c.total = o;
    return c;
}

// wave-uniform source lane -> value of that lane in every lane (v_readlane_b32 x2, no LDS)
__device__ __forceinline__ double bcast(double x, int src_lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), src_lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), src_lane);
    return __hiloint2double(hi, lo);
}

// Arguments of a non-inlined device function arrive in VGPRs and pointers as generic addresses: the
// compiler then treats every branch on them as divergent (exec-mask juggling) and every LDS access
// as a FLAT access.  These helpers restore what the caller knows: wave-uniform scalars, LDS pointers.
typedef const __attribute__((address_space(3))) double lds_cdouble;
// Opaque use of a value: the compiler must materialise it here (stops it from sinking loads into branches).
__device__ __forceinline__ void pin(double &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void pin(float &v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long uni(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double uni(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                            __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

}  // namespace
}  // namespace icnn_be
