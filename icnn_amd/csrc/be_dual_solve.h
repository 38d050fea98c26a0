// Dual step, device helpers: the reduced Newton solves and the inertia counts of the rank test, register resident, in their
// one-row-per-lane, DPP-row (be_dual_dpp_rows.h) and whole-wave forms, and the dispatch by bundle size.  Included by be_dual_dev.h;
// everything is in an anonymous namespace.
#pragma once
#include <type_traits>

#include "be_dual_cut.h"
#include "be_dual_math.h"

namespace icnn_be {

namespace {

// ---------------------------------------------------------------------------------------------
// Small dense algebra, register resident: lane i holds row i of the (<= KT x KT) system in
// statically indexed registers, pivot rows are broadcast with v_readlane -- no LDS, no barriers.
// ---------------------------------------------------------------------------------------------

// Unpivoted LDL^T inertia: number of eigenvalues of S (k x k, in Hm) that are not above mu.
// Rows and columns >= k are identity, so the elimination needs no per-column bound checks.
template <int KT>
__device__ __noinline__ int inertia_not_above_ks(const double *Hm_, int HP, int k, double mu) {
    const int lane = lane_id();
    lds_cdouble *Hm = (lds_cdouble *)Hm_;
    HP = uni(HP); k = uni(k); mu = uni(mu);
    double M[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) M[j] = Hm[(lane < k ? lane : 0) * HP + (j < k ? j : 0)];
#pragma unroll
    for (int j = 0; j < KT; ++j) pin(M[j]);                       // unconditional loads, all in flight
#pragma unroll
    for (int j = 0; j < KT; ++j)
        M[j] = (lane < k && j < k) ? M[j] - (j == lane ? mu : 0.0) : (j == lane ? 1.0 : 0.0);
    int neg = 0;
#pragma unroll
    for (int p = 0; p < KT; ++p) {
        if (p < k) {
            const double d = bcast(M[p], p);
            if (!(d > 0.0)) {
                ++neg;
                if (d == 0.0) return neg + (k - p - 1);
            }
            const double f = lane > p ? M[p] * rcp_nr(d) : 0.0;
#pragma unroll
            for (int j = p + 1; j < KT; ++j) M[j] -= f * bcast(M[j], p);
        }
    }
    return neg;
}

// Cyclic Jacobi eigenvalues of the symmetric k x k matrix in Hm (destroyed), lane 0 only.
// Rare path of the rank test.  Eigenvalues end up on the diagonal.
template <int KT, int NW>
__device__ void jacobi_lane0(double *Ms, int HP, int k, int tid) {
    if (tid == 0) {
        for (int sweep = 0; sweep < 30; ++sweep) {
            double off = 0.0, tr = 0.0;
            for (int p = 0; p < k; ++p) tr += Ms[p * HP + p];
            for (int p = 0; p < k - 1; ++p)
                for (int q = p + 1; q < k; ++q) {
                    const double apq = Ms[p * HP + q];
                    off += apq * apq;
                    if (apq == 0.0) continue;
                    const double theta = (Ms[q * HP + q] - Ms[p * HP + p]) / (2.0 * apq);
                    const double t = theta != 0.0
                        ? copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0)) : 1.0;
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    for (int j = 0; j < k; ++j) {
                        const double rp = Ms[p * HP + j], rq = Ms[q * HP + j];
                        Ms[p * HP + j] = c * rp - s * rq;
                        Ms[q * HP + j] = s * rp + c * rq;
                    }
                    for (int i = 0; i < k; ++i) {
                        const double cp = Ms[i * HP + p], cq = Ms[i * HP + q];
                        Ms[i * HP + p] = c * cp - s * cq;
                        Ms[i * HP + q] = s * cp + c * cq;
                    }
                }
            const double lim = 1e-22 * tr;
            if (off <= 1e-60 || off <= lim * lim) break;
        }
    }
    sample_sync<NW>();
}

// Solve the reduced Newton system H0[free,free] d = -g0[free] (dual :45,:53-55).  Lane i builds row
// i of the masked full-size system (identity on bound rows, so the free block is untouched),
// Gaussian elimination in natural order: the reduced Hessian is symmetric positive semi-definite,
// no pivoting is needed and the result equals LAPACK's up to rounding.  Returns false on an exactly
// zero pivot -- what LAPACK reports as singular: variant DUAL raises there (dual :56-63), variant RL
// keeps lam and leaves the Newton loop (rl :55-62).  With duplicate cuts (the RL variant has no rank
// test) the MFMA-built Hessian has bit-identical rows, so the exact zero is the normal outcome there;
// see DESIGN.md "RL variant and degenerate bundles" for what the reference's own LAPACK does on them.
// Result in registers: an output reference of a non-inlined function would live in scratch memory
// (a round trip through the vector memory path on every Newton update).
struct StepResult {
    double step;
    int ok;
};
template <int KT>
__device__ __noinline__ StepResult newton_step_ks(const double *Hm_, int HP, int k, int piv, unsigned long long fmask,
                                                  bool is_free, double g0) {
    const int lane = lane_id();
    lds_cdouble *Hm = (lds_cdouble *)Hm_;
    HP = uni(HP); k = uni(k); piv = uni(piv); fmask = uni(fmask);
    double M[KT + 1];
    // unconditional (clamped) LDS reads + selects: no exec-mask branches around the loads.  Eight columns at a time:
    // two KT-sized operand arrays next to M made the 32-slot kernels need 241 VGPRs (two waves per SIMD); the
    // arithmetic per entry is unchanged
    const int rl = lane < k ? lane : 0;
    double h_ip = Hm[rl * HP + piv], h_pp = Hm[piv * HP + piv];
    pin(h_ip);
    pin(h_pp);
    static_assert(KT % 4 == 0, "columns are loaded four at a time");
#pragma unroll
    for (int j0 = 0; j0 < KT; j0 += 4) {
        double h_ij[4], h_jp[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = j0 + jj, jc = j < k ? j : 0;
            h_ij[jj] = Hm[rl * HP + jc];
            h_jp[jj] = Hm[jc * HP + piv];
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) { pin(h_ij[jj]); pin(h_jp[jj]); }   // the four pairs in flight, none sunk into a branch
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const int j = j0 + jj;
            // H0[i][j] = ((H[i][j] - keep_i H[j][piv]) - H[i][piv] keep_j) + H[piv][piv] keep_i keep_j
            const double hv = ((h_ij[jj] - h_jp[jj]) - h_ip) + h_pp;
            const bool use = j < k && is_free && ((fmask >> j) & 1ull);
            M[j] = use ? hv : (j == lane ? 1.0 : 0.0);
        }
    }
    M[KT] = is_free ? -g0 : 0.0;
    // Rows/columns that are bound or >= k are identity: pivots there are skipped (scalar branch), and
    // columns need no bound checks.  Lane p keeps 1/pivot_p for the back substitution.
    double rinv = 1.0;
#pragma unroll
    for (int p = 0; p < KT; ++p) {
        if (p < k && ((fmask >> p) & 1ull)) {
            const double d = bcast(M[p], p);
            if (!(d != 0.0)) return StepResult{0.0, 0};           // exact zero (or NaN): singular for LAPACK
            const double inv = rcp_nr(d);
            rinv = lane == p ? inv : rinv;
            const double f = lane > p ? M[p] * inv : 0.0;
#pragma unroll
            for (int j = p + 1; j < KT; ++j) M[j] -= f * bcast(M[j], p);
            M[KT] -= f * bcast(M[KT], p);
        }
    }
#pragma unroll
    for (int p = KT - 1; p >= 0; --p) {
        if (p < k && ((fmask >> p) & 1ull)) {
            const double x = bcast(M[KT] * rinv, p);
            M[KT] = lane == p ? x : (lane < p ? M[KT] - M[p] * x : M[KT]);
        }
    }
    return StepResult{is_free ? M[KT] : 0.0, 1};
}

// ---- KS <= 16: the same eliminations with DPP64 row broadcasts ---------------------------------
// gfx90a+ can broadcast one lane of every 16-lane row to the whole row in a single 64-bit DPP move
// (v_mov_b64_dpp row_newbcast:P).  With the system in lanes 0..15 this replaces the two v_readlane +
// hazard nop of the SGPR route, keeps everything in VGPRs and lets the elimination be straight-line
// code: identity rows (bound, or >= k) have pivot 1 and multiplier -0, so they are processed like any
// other row instead of being branched around.  Lanes 16..63 compute on garbage and are ignored.
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
template <int P>
__device__ __forceinline__ double row_bcast(double v) {
    return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + P, 0xf, 0xf, true);   // bound_ctrl: no "old" value to set up
}

#define DPP_ROWS_ATTR __noinline__
#define DPP_ROWS_NAME(f) f
#include "be_dual_dpp_rows.h"
#undef DPP_ROWS_ATTR
#undef DPP_ROWS_NAME
#define DPP_ROWS_ATTR __forceinline__
#define DPP_ROWS_NAME(f) f##_inl
#include "be_dual_dpp_rows.h"
#undef DPP_ROWS_ATTR
#undef DPP_ROWS_NAME

// ---- KS > 16 (round 6): the same eliminations spread over the WHOLE wave ---------------------------------------------------
// Bundles of 17 .. 32 cuts used to fall back to one row per lane with `v_readlane` broadcasts (newton_step_ks: 12.4 k cycles
// at 17 cuts against 6.7 k for the DPP form at 16; inertia 10 k against 3.8 k -- tools/probes/dual_update_probe.hip), with 20 to 32
// of the 64 lanes holding a row of 20 .. 32 entries each.  Here the system is dealt over the four 16-lane DPP rows ("quarters"):
//   lane 16 q + r holds, of matrix rows r and 16 + r, the columns j = 4 s + q (slot s): KS / 4 entries per row instead of KS,
// so a pivot step is one row broadcast + one or two fused multiply-adds per SLOT (not per column), all four quarters working.
// What crosses the quarters is the multiplier column -(M[i][p] / d) -- formed by the quarter that owns column p, handed to the
// others by v_permlane16_swap + v_permlane32_swap (gfx950) -- and, in the back substitution, the four columns of a slot at a time.
// The right-hand side is kept in every quarter.  Every entry sees exactly the operations of newton_step_dpp / newton_step_ks in the
// same order (fma(-(M[i][p] inv), M[p][j], M[i][j]) per pivot, identity rows with multiplier -0), so the result is bit-identical.
__device__ __forceinline__ void swap16(double &x, double &y) {      // x = [x0 y0 x2 y2], y = [x1 y1 x3 y3] (quarters of the wave)
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    x = __hiloint2double((int)hi[0], (int)lo[0]);
    y = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void swap32(double &x, double &y) {      // x = [x0 x1 y0 y1], y = [x2 x3 y2 y3]
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    x = __hiloint2double((int)hi[0], (int)lo[0]);
    y = __hiloint2double((int)hi[1], (int)lo[1]);
}
// every lane gets what lane 16 Q + (lane & 15) holds
template <int Q>
__device__ __forceinline__ double quarter_bcast(double v) {
    double a = v, b = v;
    swap16(a, b);                                    // a = [v0 v0 v2 v2], b = [v1 v1 v3 v3]
    double c = (Q & 1) ? b : a, d = c;
    swap32(c, d);                                    // c = lower half twice, d = upper half twice
    return Q < 2 ? c : d;
}
// the four quarters' values of v, in every lane: out[q] = what lane 16 q + (lane & 15) holds
__device__ __forceinline__ void quarter_gather(double v, double (&out)[4]) {
    double a = v, b = v;
    swap16(a, b);
    double a2 = a, b2 = b;
    swap32(a, a2);                                   // a = [v0 v0 v0 v0], a2 = [v2 ...]
    swap32(b, b2);                                   // b = [v1 ...],      b2 = [v3 ...]
    out[0] = a; out[1] = b; out[2] = a2; out[3] = b2;
}

template <int KS>
__device__ __noinline__ StepResult newton_step_2d(const double *Hm_, int HP, int k, int piv, unsigned long long fmask,
                                                  bool is_free, double g0) {
    static_assert(KS > 16 && KS <= 32 && KS % 4 == 0, "two matrix rows per lane, four columns per slot");
    constexpr int NS = KS / 4;
    const int lane = lane_id(), q = lane >> 4, r = lane & 15;
    lds_cdouble *Hm = (lds_cdouble *)Hm_;
    HP = uni(HP); k = uni(k); piv = uni(piv); fmask = uni(fmask);
    const int i0 = r, i1 = 16 + r;                       // the two matrix rows of this lane
    const int rl0 = i0 < k ? i0 : 0, rl1 = i1 < k ? i1 : 0;
    // -g0 of the lane's two rows: row layout (lane i = row i) -> quarters 0 and 1 hold them
    const double gm = is_free ? -g0 : 0.0;
    double b0 = quarter_bcast<0>(gm), b1 = quarter_bcast<1>(gm);
    const bool free0 = (fmask >> i0) & 1ull, free1 = (fmask >> i1) & 1ull;
    double h_ip0 = Hm[rl0 * HP + piv], h_ip1 = Hm[rl1 * HP + piv], h_pp = Hm[piv * HP + piv];
    double M0[NS], M1[NS], hc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int j = 4 * s + q, jc = j < k ? j : 0;
        M0[s] = Hm[rl0 * HP + jc];
        M1[s] = Hm[rl1 * HP + jc];
        hc[s] = Hm[jc * HP + piv];
    }
    pin(h_ip0); pin(h_ip1); pin(h_pp);
#pragma unroll
    for (int s = 0; s < NS; ++s) { pin(M0[s]); pin(M1[s]); pin(hc[s]); }      // all loads in flight, none sunk into a branch
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        // H0[i][j] = ((H[i][j] - keep_i H[j][piv]) - H[i][piv] keep_j) + H[piv][piv] keep_i keep_j
        const int j = 4 * s + q;
        const bool fj = j < k && ((fmask >> j) & 1ull);
        double hv0 = ((M0[s] - hc[s]) - h_ip0) + h_pp, hv1 = ((M1[s] - hc[s]) - h_ip1) + h_pp;
        pin(hv0); pin(hv1);
        M0[s] = (fj && free0) ? hv0 : (j == i0 ? 1.0 : 0.0);
        M1[s] = (fj && free1) ? hv1 : (j == i1 ? 1.0 : 0.0);
    }
    double rinv0 = 1.0, rinv1 = 1.0;                     // lane (p & 3, p & 15) keeps 1 / pivot p
    bool bad = false;
    static_for<0, KS>([&](auto P) {
        constexpr int p = decltype(P)::value, qp = p & 3, sp = p >> 2, rp = p & 15;
        constexpr bool upper = p >= 16;                  // the pivot row is one of the rows 16 + r
        const double d = row_bcast<rp>(upper ? M1[sp] : M0[sp]);          // (meaningful in quarter qp)
        bad |= q == qp && !(d != 0.0);                   // exact zero (or NaN): singular for LAPACK
        const double inv = rcp_nr(d);
        double nf0 = 0.0, nf1;
        if constexpr (!upper) {
            rinv0 = i0 == p ? inv : rinv0;
            nf0 = quarter_bcast<qp>(i0 > p ? -(M0[sp] * inv) : 0.0);
            nf1 = quarter_bcast<qp>(-(M1[sp] * inv));
        } else {
            rinv1 = i1 == p ? inv : rinv1;
            nf1 = quarter_bcast<qp>(i1 > p ? -(M1[sp] * inv) : 0.0);
        }
        static_for<sp, NS>([&](auto S) {                 // (columns <= p of slot sp take part: they are never read again)
            constexpr int s = decltype(S)::value;
            const double pr = row_bcast<rp>(upper ? M1[s] : M0[s]);
            if constexpr (!upper) M0[s] = __builtin_fma(nf0, pr, M0[s]);
            M1[s] = __builtin_fma(nf1, pr, M1[s]);
        });
        const double pb = row_bcast<rp>(upper ? b1 : b0);
        if constexpr (!upper) b0 = __builtin_fma(nf0, pb, b0);
        b1 = __builtin_fma(nf1, pb, b1);
        __builtin_amdgcn_sched_barrier(0);     // keep the broadcasts of later pivots from being hoisted (registers)
    });
    if (__ballot(bad)) return StepResult{0.0, 0};
    // back substitution, a slot (four columns, one per quarter) at a time: every quarter gets the slot's columns of its rows
    static_for<0, NS>([&](auto S) {
        constexpr int s = NS - 1 - decltype(S)::value;
        double u0[4], u1[4];
        quarter_gather(M0[s], u0);
        if constexpr (4 * s + 3 > 16) quarter_gather(M1[s], u1);
        static_for<0, 4>([&](auto C) {
            constexpr int qp = 3 - decltype(C)::value, p = 4 * s + qp, rp = p & 15;
            constexpr bool upper = p >= 16;
            const double x = bcast((upper ? b1 : b0) * (upper ? rinv1 : rinv0), 16 * qp + rp);
            b0 = i0 == p ? x : (i0 < p ? __builtin_fma(-u0[qp], x, b0) : b0);
            if constexpr (p >= 16) b1 = i1 == p ? x : (i1 < p ? __builtin_fma(-u1[qp], x, b1) : b1);
        });
    });
    // back to the row layout: lane i < 16 has its step in b0 (quarter 0), lane 16 + r in b1 -- which quarter 1 holds as well
    const double step = q == 0 ? b0 : (q == 1 ? b1 : 0.0);
    return StepResult{is_free ? step : 0.0, 1};
}

// Unpivoted LDL^T inertia in the same layout (cf. inertia_not_above_dpp): no right-hand side, no back substitution
template <int KS>
__device__ __noinline__ int inertia_not_above_2d(const double *Hm_, int HP, int k, double mu) {
    static_assert(KS > 16 && KS <= 32 && KS % 4 == 0, "two matrix rows per lane, four columns per slot");
    constexpr int NS = KS / 4;
    const int lane = lane_id(), q = lane >> 4, r = lane & 15;
    lds_cdouble *Hm = (lds_cdouble *)Hm_;
    HP = uni(HP); k = uni(k); mu = uni(mu);
    const int i0 = r, i1 = 16 + r;
    double M0[NS], M1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int j = 4 * s + q, jc = j < k ? j : 0;
        M0[s] = Hm[(i0 < k ? i0 : 0) * HP + jc];
        M1[s] = Hm[(i1 < k ? i1 : 0) * HP + jc];
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) { pin(M0[s]); pin(M1[s]); }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int j = 4 * s + q;
        M0[s] = (i0 < k && j < k) ? M0[s] - (j == i0 ? mu : 0.0) : (j == i0 ? 1.0 : 0.0);
        M1[s] = (i1 < k && j < k) ? M1[s] - (j == i1 ? mu : 0.0) : (j == i1 ? 1.0 : 0.0);
    }
    double dp0 = 1.0, dp1 = 1.0;                         // lane (p & 3, p & 15) keeps pivot p
    static_for<0, KS>([&](auto P) {
        constexpr int p = decltype(P)::value, qp = p & 3, sp = p >> 2, rp = p & 15;
        constexpr bool upper = p >= 16;
        const double d = row_bcast<rp>(upper ? M1[sp] : M0[sp]);
        const double inv = rcp_nr(d);
        double nf0 = 0.0, nf1;
        if constexpr (!upper) {
            dp0 = (q == qp && i0 == p) ? d : dp0;
            nf0 = quarter_bcast<qp>(i0 > p ? -(M0[sp] * inv) : 0.0);
            nf1 = quarter_bcast<qp>(-(M1[sp] * inv));
        } else {
            dp1 = (q == qp && i1 == p) ? d : dp1;
            nf1 = quarter_bcast<qp>(i1 > p ? -(M1[sp] * inv) : 0.0);
        }
        static_for<sp, NS>([&](auto S) {
            constexpr int s = decltype(S)::value;
            const double pr = row_bcast<rp>(upper ? M1[s] : M0[s]);
            if constexpr (!upper) M0[s] = __builtin_fma(nf0, pr, M0[s]);
            M1[s] = __builtin_fma(nf1, pr, M1[s]);
        });
        __builtin_amdgcn_sched_barrier(0);
    });
    // pivot p sits in lane 16 (p & 3) + (p & 15) as dp0 (p < 16) or dp1: ballots per pivot class, in pivot order
    // of every group of lanes r, 16 + r, 32 + r, 48 + r exactly one -- quarter r & 3 -- owns pivots r and 16 + r
    const bool own = (r & 3) == q;
    auto fold = [](unsigned long long m) -> unsigned { return (unsigned)((m | (m >> 16) | (m >> 32) | (m >> 48)) & 0xffffull); };
    unsigned nonpos = fold(__ballot(own && !(dp0 > 0.0))) | (fold(__ballot(own && !(dp1 > 0.0))) << 16);
    unsigned zero = fold(__ballot(own && dp0 == 0.0)) | (fold(__ballot(own && dp1 == 0.0)) << 16);
    const unsigned live = k >= 32 ? 0xffffffffu : ((1u << k) - 1u);
    nonpos &= live; zero &= live;
    // pivots up to the first exact zero count individually; behind it everything counts as suspect
    if (zero) {
        const int p0 = __builtin_ctz(zero);
        return __popc(nonpos & ((2u << p0) - 1u)) + (k - p0 - 1);
    }
    return __popc(nonpos);
}

// The statically unrolled routines above cost O(KS^2) predicated steps whatever k is, so they are
// instantiated for several sizes and the smallest one that holds the bundle is used.
// KCAP > 0 (dual_step_body): k <= KCAP <= 8, and the instance today's dispatch picks for k is inlined instead of called.
template <int KT, int KCAP = 0>
__device__ __forceinline__ int inertia_not_above(const double *Hm, int HP, int k, double mu) {
    if constexpr (KCAP > 0) {
        static_assert(KCAP <= 8, "capped bodies hold bundles of up to eight cuts");
        if (KCAP <= 4 || k <= 4) return inertia_not_above_dpp_inl<4>(Hm, HP, k, mu);
        if (KCAP <= 6 || k <= 6) return inertia_not_above_dpp_inl<6>(Hm, HP, k, mu);
        return inertia_not_above_dpp_inl<8>(Hm, HP, k, mu);
    }
    if (k <= 4) return inertia_not_above_dpp<4>(Hm, HP, k, mu);
    if (k <= 6) return inertia_not_above_dpp<6>(Hm, HP, k, mu);
    if (k <= 8) return inertia_not_above_dpp<8>(Hm, HP, k, mu);
    if (k <= 10) return inertia_not_above_dpp<10>(Hm, HP, k, mu);
    if (k <= 12) return inertia_not_above_dpp<12>(Hm, HP, k, mu);
    if (KT == 16 || k <= 16) return inertia_not_above_dpp<16>(Hm, HP, k, mu);
    if constexpr (KT > 16) {                             // (round 6: the system dealt over the whole wave, above)
        if (k <= 20) return inertia_not_above_2d<20>(Hm, HP, k, mu);
        if (k <= 24) return inertia_not_above_2d<24>(Hm, HP, k, mu);
        return inertia_not_above_2d<32>(Hm, HP, k, mu);
    }
    return 0;
}
// (one-wave samples on the fused VALU pass: bundles of up to HV_K1MAX = 8 cuts, system in the pass's packed triangle)
template <int KCAP = 0>
__device__ __forceinline__ StepResult newton_step_tri(const double *P, int k, int piv, unsigned long long fmask, bool is_free,
                                                      double g0) {
    if constexpr (KCAP > 0) {                            // the same choice by k, inlined
        if (KCAP <= 4 || k <= 4) return newton_step_dpp_inl<4, true>(P, 0, k, piv, fmask, is_free, g0);
        if (KCAP <= 6 || k <= 6) return newton_step_dpp_inl<6, true>(P, 0, k, piv, fmask, is_free, g0);
        return newton_step_dpp_inl<8, true>(P, 0, k, piv, fmask, is_free, g0);
    }
    if (k <= 4) return newton_step_dpp<4, true>(P, 0, k, piv, fmask, is_free, g0);
    if (k <= 6) return newton_step_dpp<6, true>(P, 0, k, piv, fmask, is_free, g0);
    return newton_step_dpp<8, true>(P, 0, k, piv, fmask, is_free, g0);
}
template <int KT>
__device__ __forceinline__ StepResult newton_step(const double *Hm, int HP, int k, int piv, unsigned long long fmask,
                                                  bool is_free, double g0) {
    if (k <= 4) return newton_step_dpp<4>(Hm, HP, k, piv, fmask, is_free, g0);
    if (k <= 6) return newton_step_dpp<6>(Hm, HP, k, piv, fmask, is_free, g0);
    if (k <= 8) return newton_step_dpp<8>(Hm, HP, k, piv, fmask, is_free, g0);
    if (k <= 10) return newton_step_dpp<10>(Hm, HP, k, piv, fmask, is_free, g0);
    if (k <= 12) return newton_step_dpp<12>(Hm, HP, k, piv, fmask, is_free, g0);
    if (KT == 16 || k <= 16) return newton_step_dpp<16>(Hm, HP, k, piv, fmask, is_free, g0);
    if constexpr (KT > 16) {                             // (round 6: the system dealt over the whole wave, above)
        if (k <= 20) return newton_step_2d<20>(Hm, HP, k, piv, fmask, is_free, g0);
        if (k <= 24) return newton_step_2d<24>(Hm, HP, k, piv, fmask, is_free, g0);
        return newton_step_2d<32>(Hm, HP, k, piv, fmask, is_free, g0);
    }
    return StepResult{0.0, 0};
}

}  // namespace
}  // namespace icnn_be
