// Device code of the dual step (included by be_dual.hip and be_fused.hip): the body's config (DualCfg), dual_step_body and the
// two kernels that are nothing but the body.  The helpers live in headers by subject, included below.  Everything is in an
// anonymous namespace.
#pragma once
// Dual step of the bundle-entropy method: one wave64 = one sample.
//
// For outer iteration t and every unfinished sample u (one workgroup of 64 lanes):
//   1. append the cut (g_t, h_t = f_t - <g_t, y>) to slot t            dual :143,:151-153
//   2. stage the active bundle rows A[k][n] in LDS
//   3. rank test on A (variant DUAL)                                   dual :155-161
//   4. projected Newton on the simplex for lam                         dual :15-85 / rl :14-83
//   5. y <- 1/(1+exp(A^T lam)), clip/stall test (RL), prune lam == 0   dual :165-174 / rl :117-131
//
// Layouts inside the wave
//   column layout: lane l owns columns l, l+64, ... of the bundle (a = A^T lam, z, w, y)
//   row layout:    lane i < k owns bundle row i (lam_i, c_i, g_i, step_i)
// The k x k contractions A diag(w) A^T and A z go through v_mfma_f64_16x16x4_f64 with
// both operands gathered from the LDS-resident bundle; the (k-1) x (k-1) Newton system
// is solved in LDS by Gaussian elimination with partial pivoting, lane = matrix row.
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

#include "be_common.h"
#include "be_kernels.h"
#include "icnn_be.h"

#include "be_dual_cut.h"     // cut types, the LDS carve-up, wave-uniform and opaque values
#include "be_dual_mfma.h"    // the float64 MFMA contractions
#include "be_dual_math.h"    // rcp_nr, fast_exp, fast_log, softplus_fast, sigmoid_fast
#include "be_dual_solve.h"   // reduced Newton solves and inertia counts (with be_dual_dpp_rows.h)
#include "be_dual_cols.h"    // row reductions and the column loop

namespace icnn_be {

namespace {

constexpr double BOUND_EPS = 1e-12;    // dual :21
constexpr double ARMIJO_ALPHA = 1e-5;  // dual :22
constexpr double GRAD_TOL = 1e-10;     // dual :50
constexpr double TINY = 1e-10;         // dual :79
constexpr double CYCLE_TOL = 1e-13;    // DESIGN.md "limit-cycle shortcut"
// A limit cycle whose own rounding jitter is ABOVE CYCLE_TOL never passes the repeat test (ill-conditioned Newton systems: the
// iterates repeat to 1e-12, not 1e-13) and ran the full cap of 100 updates -- the same sample, in every outer iteration; a third
// of all cycling solves of the benchmark batch (tools: /DESIGN.md section 6c), and THE straggler of every long solve.  Noise-floor
// rule (variant dual): from NOISE_T0 updates on, period p is also accepted when max|lam_t - lam_{t-p}| is below NOISE_TOL and has
// STOPPED SHRINKING -- not below its value an update cycle earlier: a converging sequence shrinks geometrically, a cycle at its
// rounding floor fluctuates.  What is returned is the iterate of the right phase, as for exact repeats; it differs from the
// reference's lam_100 by the cycle's own jitter (max 2.5e-11 on 10 243 recorded solves, against 4.1e-11 without the rule).
constexpr double NOISE_TOL = 1e-10;
constexpr int NOISE_T0 = 12;
constexpr int ACCEL_T0 = 24;           // extrapolation of slow 2-cycles: not before this many updates,
constexpr int ACCEL_GAP = 6;           // this many updates apart,
constexpr double ACCEL_NEG_RESID = 1e-10;  // oscillating subsequences (negative ratio): see the extrapolation in dual_step_body
constexpr double ACCEL_D2MAX = 1e-3;   // only once lam_t - lam_{t-2} is this small
constexpr double ACCEL_RMAX = 0.98;    // and the contraction ratio is below this

#include "be_dual_valu_dev.h"
#include "be_ipm_dev.h"

// What dual_step_body is compiled for.  The body works on sample `u` with the 64 NW threads whose index is `tid`, in the LDS
// region `smem`; `round` and `rows` (the most bundle rows any sample can hold in this round) come from the caller; `crow` points
// at shared constant rows (zeros, ones) or is null, in which case the sample keeps its own behind its bundle.  Stand-alone
// kernel below: one workgroup per sample.  be_fused.hip: one single-wave sample per wave of a 16-wave workgroup (NW = 1, so
// nothing in there synchronises beyond the wave).  ArgsT, the body's other template parameter: DualArgs as the kernel's by-value
// parameter, or a reference into the kernel-argument segment (address space 4) when the caller is a non-inlined phase function
// of be_fused.hip.
template <typename Shape, int KCAP>
constexpr bool dual_cap_on_valu_pass() {               // (DualCfg::KCAP; a shape policy without constants has no capped body)
    if constexpr (KCAP > 0) return KCAP <= HV_K1MAX && Shape::FIXED && Shape::N_PAD <= 192 && hv_pitch(KCAP) <= Shape::N_PAD;
    else return true;
}
template <typename CutT_, int KT_, int NW_, bool RL_, bool IPM_ = false, bool GLB_ = false, int LR_ = 0, bool SLICED_ = true,
          typename Shape_ = DynShape, int KCAP_ = 0>
struct DualCfg {
    using CutT = CutT_;                // dtype of the cuts: float or double
    static constexpr int KT = KT_;     // bundle slots the register-resident algebra is sized for: 16 or 32
    // Waves per sample.  NW = 1: one wave64 owns the sample (n up to a few hundred).  NW > 1 (large n, e.g. the 2048-pixel
    // completion model): the columns are split over NW waves -- column phase, MFMA sweep (per-wave partial results summed through
    // LDS) and y update scale with NW -- while every wave runs the small row-layout algebra redundantly on identical data, so
    // no multiplier ever has to be exchanged.
    static constexpr int NW = NW_;
    // The variant of RL/src/bundle_entropy.py: its Armijo line search, softplus sums and pivot regularisation are compiled out
    // of the dual-variant kernels.
    static constexpr bool RL = RL_;
    // The interior-point variant (lib/bundle_entropy.py): same cut bookkeeping and rank test, then y AND the multipliers come
    // from pdipm_pc (be_ipm_dev.h) and multipliers <= 1e-8 are pruned (:234-237).
    static constexpr bool IPM = IPM_;
    // The staged bundle (rows + the two constant rows) lives in the sample's slice of st.scratch instead of LDS -- the rounds of
    // a wide-row solve whose bundle no longer fits the workgroup's 160 KB.  Same code, same arithmetic.
    static constexpr bool GLB = GLB_;
    // LR > 0 (with GLB; dual_step_wide_kernel): split staging -- the LR oldest rows of the bundle are ALSO copied into LDS behind
    // the carve-up, for the fused VALU pass of be_dual_valu_dev.h (everything else reads the device-memory copy as in any GLB round).
    static constexpr int LR = LR_;
    // SLICED = false: the caller never parks a sample (no update budget, state fresh from icnn_be_state_init: the persistent
    // tile kernel in its default form) -- the park / resume paths and their live values are compiled out (headline solve 1.024 ->
    // 1.016 ms on one box; cf. ICNN_BE_PROF, be_common.h).
    static constexpr bool SLICED = SLICED_;
    // (be_kernels.h): n, n_pad, ldA and the pairwise plan from the arguments (DynShape), or as constants (FixedDual: the fixed
    // instances of the persistent tile kernel).
    using Shape = Shape_;
    // KCAP > 0: the caller guarantees rows_cap <= KCAP <= HV_K1MAX and that the fused VALU pass is what every bundle of two and
    // more cuts takes (one-wave float32 rows of up to 192 columns, no ICNN_BE_FLAG_MFMA_CONTRACTION: the round classes of the
    // persistent tile kernel, be_fused.hip).  The pass, the reduced Newton solve and the inertia count are then inlined in the
    // instance today's dispatch picks for k, the MFMA sweep is not compiled in, and no function is called in the Newton loop.
    // Same instances, same arithmetic, same bits.  KCAP = 0: the body as it always was.
    static constexpr int KCAP = KCAP_;

    static_assert(!IPM || !RL, "interior point is a variant of its own");
    static_assert(LR == 0 || GLB, "split staging belongs to the device-memory rounds");
    static_assert(KCAP == 0 || (NW == 1 && KT == 16 && !RL && !IPM && !GLB && LR == 0 && sizeof(CutT) == 4),
                  "capped bodies: one-wave dual variant");
    static_assert(dual_cap_on_valu_pass<Shape, KCAP>(), "every bundle of a capped body takes the fused VALU pass");
};
// The config of a one-wave body inside a persistent tile kernel: C with the three things such a caller decides, so that the
// call site names only what differs from the defaults above.
template <typename C, bool SLICED, typename Shape, int KCAP = 0>
using DualCfgTile = DualCfg<typename C::CutT, C::KT, C::NW, C::RL, C::IPM, C::GLB, C::LR, SLICED, Shape, KCAP>;

// One round of one sample.  Cfg: a DualCfg; the arguments are described there.  (Why this is still one function with the
// Newton history kept by hand: profiles/dual_body_split_ab.md.)
template <typename Cfg, typename ArgsT>
__device__ __forceinline__ void dual_step_body(const ArgsT &a, int u, int tid, unsigned char *smem, int round,
                                               int rows_cap, const typename Cfg::CutT *crow_shared) {
    using CutT = typename Cfg::CutT;
    using Shape = typename Cfg::Shape;
    constexpr int KT = Cfg::KT, NW = Cfg::NW, LR = Cfg::LR, KCAP = Cfg::KCAP;
    constexpr bool RL = Cfg::RL, IPM = Cfg::IPM, GLB = Cfg::GLB, SLICED = Cfg::SLICED;
    constexpr int NT = 64 * NW;
    const auto &st = a.st;
    const int lane = tid & 63, wave = tid >> 6;
    const bool w0 = wave == 0;                 // the wave that writes per-sample results
    auto wg_any = [&](bool p) -> bool { return NW == 1 ? (bool)__any(p) : (bool)__syncthreads_or(p); };
    // reduce the per-wave partial contractions into Hm (no-op for a single wave)
    auto combine = [&](double *Hm_, const double *Hp_, int HP_, int k_, int ncols) {
        if (NW == 1) return;
        sample_sync<NW>();
        for (int e = tid; e < k_ * ncols; e += NT) {
            const int r = e / ncols, c = e - r * ncols;
            double acc = 0.0;
            for (int w = 0; w < NW; ++w) acc += Hp_[(w * rows_cap + r) * HP_ + c];
            Hm_[r * HP_ + c] = acc;
        }
    };
    long long tick = ICNN_BE_PROF_ON(a.prof) ? (long long)__builtin_readcyclecounter() : 0;
    const int T = st.slots;                               // bundle slots
    const int TI = st.iters > 0 ? st.iters : T;           // outer iterations (more than slots: slots are recycled, below)
    // The per-sample control words, the active-slot list and this thread's part of the new cut are requested
    // before the first branch: read one after the other behind the early exits they cost four dependent
    // memory round trips at the head of every launch.
    const int finished_u = st.finished[u], t_raw = st.t_next[u], phase_u = st.phase[u], cnt_raw = st.count[u];
    const int slot_pre = tid < T ? st.active[(size_t)u * T + tid] : 0;
    const int slot_lane = NW == 1 ? slot_pre : (lane < T ? st.active[(size_t)u * T + lane] : 0);   // per wave
    if (finished_u) return;
    // every sample carries its own outer-iteration counter: samples are independent, so one that
    // was parked mid-Newton simply lags behind the others (icnn_be.h, icnn_be_solve_fc)
    const int t = __builtin_amdgcn_readfirstlane(t_raw);
    if (t >= TI) return;
    const bool resume = SLICED && __builtin_amdgcn_readfirstlane(phase_u) != 0;

    const int n = Shape::n(a), n_pad = Shape::n_pad(a), ldA = Shape::ldA(a);
    const auto &plan = Shape::plan(a);
    const int HP = (rows_cap + 1) | 1;     // odd pitch of the (k x k+1) matrix H | A z in LDS
    // RL (variant of RL/src/bundle_entropy.py) is a template parameter: its Armijo line search, softplus
    // sums and pivot regularisation are compiled out of the dual-variant kernels.
    // a bundle cannot hold more cuts than outer iterations have been started: rows <= round + 1
    const Carve cv = carve(KT, rows_cap, ldA, n_pad, (int)sizeof(CutT), plan.n_leaves, RL, NW, crow_shared == nullptr, IPM, GLB);
    // this wave's share of the columns (multiple of 16)
    const int cchunk = NW == 1 ? n_pad : (((n_pad / 16 + NW - 1) / NW) * 16);
    const int cbeg = wave * cchunk < n_pad ? wave * cchunk : n_pad;
    const int cend = cbeg + cchunk < n_pad ? cbeg + cchunk : n_pad;
    CutT *As = GLB ? static_cast<CutT *>(st.scratch) + (size_t)u * (st.slots + 2) * ldA : reinterpret_cast<CutT *>(smem + cv.As);
    CutT *AsL = reinterpret_cast<CutT *>(smem + ((cv.total + 15) & ~15));          // LR > 0: [LR][ldA], the oldest rows
    const bool mirror = LR > 0 && rows_cap <= HV_KMAX;     // split staging: the LR oldest rows also in LDS (there is room up to
                                                           // the carve-up of a HV_KMAX-cut bundle, dual_step_wide_kernel)
    double *zs = reinterpret_cast<double *>(smem + cv.zs);
    double *ws = reinterpret_cast<double *>(smem + cv.ws);
    double *sp = reinterpret_cast<double *>(smem + cv.sp);     // == ws unless RL
    double *Hm = reinterpret_cast<double *>(smem + cv.Hm);
    double *Hp = reinterpret_cast<double *>(smem + cv.Hp) + (NW == 1 ? 0 : wave * rows_cap * HP);   // my partial
    double *Hp0 = reinterpret_cast<double *>(smem + cv.Hp);
    double *leaf = Hm;                                        // pairwise-sum scratch aliases Hm
    double *psum = Hm + KT * plan.n_leaves;                 // [2*KT] results of pairwise sums
    int *slots = reinterpret_cast<int *>(smem + cv.ints);

    const CutT *g_row = static_cast<const CutT *>(a.g) + (size_t)u * n;
    // energy of the new cut: cut dtype, or float64 when the caller's fg returns it so (ICNN_BE_FLAG_F64_ENERGY)
    const double f_u = (sizeof(CutT) == 4 && (st.flags & ICNN_BE_FLAG_F64_ENERGY))
                           ? static_cast<const double *>(a.f)[u] : (double)static_cast<const CutT *>(a.f)[u];
    double *y_row = st.y + (size_t)u * n;
    CutT *G_u = static_cast<CutT *>(st.G) + (size_t)u * T * n;
    double *ys_u = st.ys + (size_t)u * T * n;
    double *h_u = st.h + (size_t)u * T;

    const int cnt = __builtin_amdgcn_readfirstlane(cnt_raw);
    const int k = cnt + 1;
    if (k > rows_cap) {                 // the active bundle no longer fits the staging area (wide rows only: the launch
        if (tid == 0) {                 // sizes it for min(round + 1, slots, what 160 KB hold)): stop at this iterate
            st.status[u] |= ICNN_BE_ST_OVERFLOW;
            st.finished[u] = 1;
            st.skip_fg[u] = 1;
        }
        return;
    }
    auto lap = [&](int phase) {                     // diagnostic only: cycles per phase, per sample
        if (ICNN_BE_PROF_ON(a.prof)) {
            const long long now = (long long)__builtin_readcyclecounter();
            // no-return atomic: fire and forget (a read-modify-write would bill its memory round trip
            // to the next phase)
            if (tid == 0)
                atomicAdd(reinterpret_cast<unsigned long long *>(a.prof) + (size_t)u * DUAL_PROF_PHASES + phase,
                          (unsigned long long)(now - tick));
            tick = now;
        }
    };
    lap(12);                                        // the control words have arrived
    // Slot of the new cut: slot t while there are as many slots as iterations (the layout the host's per-iteration views
    // rely on).  With more iterations than slots (nIter > ICNN_BE_MAX_SLOTS: the reference has no cap, dual :129) a cut
    // takes the lowest slot that is not in the active list -- pruned cuts (dual :171-174) give their slots back; the
    // active list is only rewritten when an iteration completes, so a parked solve finds the same slot again.
    int slot_new = t;
    if (TI > T) {
        unsigned used = 0;
        for (int i = 0; i < cnt; ++i) used |= 1u << __builtin_amdgcn_readlane(slot_lane, i);
        slot_new = __builtin_ctz(~used);
    }
    if (tid < cnt) slots[tid] = slot_pre;
    if (tid == cnt) slots[tid] = slot_new;
    const double h_old = lane < cnt ? h_u[slot_lane] : 0.0;   // offsets of the older cuts, requested with the new cut's rows
    if (NW > 1) sample_sync<NW>();                    // other waves read the slot list

    // ---- 1. the new cut: slot t <- (g, h, y); 2. stage the older active rows -----------------
    // The global reads of both steps are issued back to back (new cut into registers, then the older
    // rows) so that their memory round trips overlap; the h reduction follows.
    const int per_row = (n_pad + NT - 1) / NT;                            // workgroup-wide chunks per row
    constexpr int MAXC = 4;
    auto stage_older = [&]() {
        if constexpr (NW == 1 && !GLB && LR == 0 && sizeof(CutT) == 4) {
            // Round 6: the older rows go from device memory STRAIGHT into LDS (global_load_lds_dword: lane l of a 64-column chunk
            // lands at chunk base + 4 l; M0 carries the chunk's LDS address), every chunk of every row requested back to back and
            // awaited once -- through registers, four rows per batch, a bundle of nine rows cost three memory round trips and
            // sixteen registers, seventeen rows five.  Columns n .. n_pad - 1 (no lane loads them) are zeroed by hand: the
            // region held another phase's data, and 0 x garbage must stay 0 in the sweeps.
            if (per_row <= MAXC) {
                for (int r = 0; r < cnt; ++r) {
                    const CutT *src = G_u + (size_t)uni(slots[r]) * n;
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) {
                        const int j = tid + c * 64;
                        if (c < per_row && j < n)
                            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + j),
                                                             (__attribute__((address_space(3))) void *)(As + r * ldA + c * 64), 4, 0, 0);
                    }
                }
                for (int j = n + tid; j < n_pad; j += 64)
                    for (int r = 0; r < cnt; ++r) As[r * ldA + j] = (CutT)0;
                __builtin_amdgcn_s_waitcnt(0x0f70);                // vmcnt(0): the rows are in LDS
                return;
            }
        }
        if (per_row <= MAXC) {
            // four rows per batch, all their loads in flight before the first LDS store: a bundle of nine rows costs
            // three memory round trips (one chunk at a time with a 4-deep unroll it cost seven; eight rows per batch measured slower)
            constexpr int RB = 4;
            for (int r0 = 0; r0 < cnt; r0 += RB) {
                CutT v[RB][MAXC];
#pragma unroll
                for (int rr = 0; rr < RB; ++rr) {
                    const bool rok = r0 + rr < cnt;
                    const CutT *src = G_u + (size_t)(rok ? slots[r0 + rr] : 0) * n;
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) {
                        const int j = tid + c * NT;
                        v[rr][c] = rok && c < per_row && j < n ? src[j] : (CutT)0;
                    }
                }
#pragma unroll
                for (int rr = 0; rr < RB; ++rr)
#pragma unroll
                    for (int c = 0; c < MAXC; ++c) {
                        const int j = tid + c * NT;
                        if (r0 + rr < cnt && c < per_row && j < n_pad) {
                            As[(r0 + rr) * ldA + j] = v[rr][c];
                            if (LR > 0 && mirror && r0 + rr < LR) AsL[(r0 + rr) * ldA + j] = v[rr][c];
                        }
                    }
            }
            return;
        }
        const int chunks = cnt * per_row;
#pragma unroll 4
        for (int c = 0; c < chunks; ++c) {
            const int r = c / per_row, j = (c - r * per_row) * NT + tid;
            if (j < n_pad) {
                const CutT v = j < n ? G_u[(size_t)slots[r] * n + j] : (CutT)0;
                As[r * ldA + j] = v;
                if (LR > 0 && mirror && r < LR) AsL[r * ldA + j] = v;
            }
        }
    };
    double h_new;
    if (!resume) {
        bool bad = !isfinite(f_u);
        if (per_row <= MAXC) {
            CutT gr[MAXC];
            double yr[MAXC];
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int j = tid + c * NT;
                gr[c] = j < n ? g_row[j] : (CutT)0;
                yr[c] = j < n ? y_row[j] : 0.0;
            }
            stage_older();
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int j = tid + c * NT;
                if (j < n) {
                    G_u[(size_t)slot_new * n + j] = gr[c];
                    ys_u[(size_t)slot_new * n + j] = yr[c];
                    bad |= !isfinite((double)gr[c]);
                }
                if (j < n_pad) {
                    As[cnt * ldA + j] = gr[c];
                    if (LR > 0 && mirror && cnt < LR) AsL[cnt * ldA + j] = gr[c];
                    sp[j] = (double)gr[c] * yr[c];                // dual :143  gi * x in float64 (0 for j >= n)
                }
            }
        } else {
            for (int j = tid; j < n_pad; j += NT) {
                double prod = 0.0;
                if (j < n) {
                    const CutT gj = g_row[j];
                    const double yj = y_row[j];
                    G_u[(size_t)slot_new * n + j] = gj;
                    ys_u[(size_t)slot_new * n + j] = yj;
                    prod = (double)gj * yj;                       // dual :143  gi * x in float64
                    bad |= !isfinite((double)gj);
                    As[cnt * ldA + j] = gj;
                    if (LR > 0 && mirror && cnt < LR) AsL[cnt * ldA + j] = gj;
                } else {
                    As[cnt * ldA + j] = (CutT)0;
                    if (LR > 0 && mirror && cnt < LR) AsL[cnt * ldA + j] = (CutT)0;
                }
                sp[j] = prod;
            }
            stage_older();
        }
        sample_sync<NW>();
        lap(13);
        np_pairwise_rows<NW, double>(plan, 1, [&](int, int j) { return sp[j]; }, leaf, psum, tid);
        h_new = f_u - psum[0];                        // fi - np.sum(gi * x)
        if (tid == 0) {
            h_u[slot_new] = h_new;
            if (st.fvals) st.fvals[(size_t)u * T + slot_new] = f_u;          // energy of the cut (callback replay, host)
        }
        if (wg_any(bad)) {
            if (tid == 0) { st.status[u] |= ICNN_BE_ST_NONFINITE; st.finished[u] = 1; st.skip_fg[u] = 1; }
            return;
        }
    } else {                                                  // parked solve: the cut is already in slot t
        for (int j = tid; j < n_pad; j += NT) {
            const CutT v = j < n ? G_u[(size_t)slot_new * n + j] : (CutT)0;
            As[cnt * ldA + j] = v;
            if (LR > 0 && mirror && cnt < LR) AsL[cnt * ldA + j] = v;
        }
        h_new = h_u[slot_new];
        stage_older();
    }
    lap(0);
    const CutT *crow = crow_shared ? crow_shared : As + rows_cap * ldA;
    if (!crow_shared)
        for (int j = tid; j < ldA; j += NT) { As[rows_cap * ldA + j] = (CutT)0; As[(rows_cap + 1) * ldA + j] = (CutT)1; }
    const double h_i = lane < cnt ? h_old : h_new;                // row layout (lane < k)
    // Wide rows, small bundle: column phase and contraction fused on the VALU (be_dual_valu_dev.h).  The per-wave partial
    // sums live where z would (two buffers, alternating by update: one barrier per update instead of four).
    const bool hv_on = !(st.flags & ICNN_BE_FLAG_MFMA_CONTRACTION);
    const int hv_p = hv_pitch(k);                          // partial sums per wave (two buffers of NW rows where z and w would live)
    // Round 4: one-wave samples with rows of up to 192 columns (float32 cuts) take the same pass -- three columns per lane,
    // the k (k + 3) / 2 sums through the transposing butterfly, H | A z written by the lanes that end up with them: no z / w
    // round trip through LDS, no operand gathers (the MFMA sweep reads ten times the bundle per update and is what the CU's
    // LDS bandwidth bounds when sixteen samples share it).  Every kernel that runs dual_step_body takes the same decision,
    // so the dispatch paths stay bit-identical; ICNN_BE_FLAG_MFMA_CONTRACTION keeps the sweep everywhere.
    // Up to HV_K1MAX = 8 cuts: the pass costs k (k + 3) / 2 sums per column and their reduction, the sweep a fixed number of
    // MFMAs -- measured crossover on the long solves (4096 x 30: sweep only 6.65 ms, pass up to 8 cuts 6.50, up to 16 7.24;
    // 4096 x 15: 1.97 / 1.76 / 1.78).
    const bool valu = KCAP > 0 ? k >= 2 : hv_on && (NW > 1 || (n_pad <= 192 && sizeof(CutT) == 4 && k <= HV_K1MAX)) && !RL && !IPM && k >= 2 &&
                      k <= HV_KMAX && (LR == 0 || mirror) && n_pad <= 256 * NW && NW * hv_p <= n_pad;
    double *hv_part = zs;
    const HvEntry hv_first = hv_entry<true>(lane, k, HP);  // this lane's first entry of the per-update gather
    sample_sync<NW>();

    lap(1);
    // ---- 3. rank test (variant DUAL only) -----------------------------------------------
    if (!RL && !resume) {
        bool deficient = false;
        const double cfac = (double)(k > n ? k : n) * Cut<CutT>::eps;   // max(M.shape) * eps
        if (k == 1) {
            bool nz = false;
            for (int j = tid; j < n; j += NT) nz |= As[j] != (CutT)0;
            deficient = !wg_any(nz);
        } else if (sizeof(CutT) == 8 && NW == 1) {
            // float64 cuts: one-sided Jacobi on the rows (in place; restaged afterwards)
            for (int sweep = 0; sweep < 30; ++sweep) {
                bool rotated = false;
                for (int p = 0; p < k - 1; ++p)
                    for (int q = p + 1; q < k; ++q) {
                        double al = 0, be = 0, ga = 0;
                        for (int j = lane; j < n; j += 64) {
                            const double vp = (double)As[p * ldA + j], vq = (double)As[q * ldA + j];
                            al += vp * vp; be += vq * vq; ga += vp * vq;
                        }
                        al = wave_sum(al); be = wave_sum(be); ga = wave_sum(ga);
                        if (ga == 0.0 || fabs(ga) <= 2.3e-16 * sqrt(al * be)) continue;
                        rotated = true;
                        const double zeta = (be - al) / (2.0 * ga);
                        const double tt = zeta != 0.0
                            ? copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta)) : 1.0;
                        const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
                        for (int j = lane; j < n; j += 64) {
                            const double vp = (double)As[p * ldA + j], vq = (double)As[q * ldA + j];
                            As[p * ldA + j] = (CutT)(c * vp - s * vq);
                            As[q * ldA + j] = (CutT)(s * vp + c * vq);
                        }
                    }
                if (!rotated) break;
            }
            double sv = 0.0, smax = 0.0;
            for (int r = 0; r < k; ++r) {
                double ss = 0;
                for (int j = lane; j < n; j += 64) { const double v = (double)As[r * ldA + j]; ss += v * v; }
                ss = sqrt(wave_sum(ss));
                if (lane == r) sv = ss;
                smax = fmax(smax, ss);
            }
            deficient = __popcll(__ballot(lane < k && sv > smax * cfac)) < k;
            sample_sync<NW>();
            for (int r = 0; r < k; ++r) {                 // restage
                const CutT *src = r < cnt ? G_u + (size_t)slots[r] * n : g_row;
                for (int j = lane; j < n_pad; j += 64) As[r * ldA + j] = j < n ? src[j] : (CutT)0;
            }
            sample_sync<NW>();
        } else {
            if (KCAP > 0 || valu) {                        // (be_dual_valu_dev.h)
                hv_column_pass_k<CutT, NW, false, LR, GLB, (NW == 1 && KT > 16), KCAP>(As, AsL, ldA, k, rows_cap, n, n_pad, tid, 0.0, hv_part + wave * hv_p);
                sample_sync<NW>();
                hv_gather<NW, false>(hv_part, hv_p, Hm, HP, k, tid, NT, hv_entry<false>(tid, k, HP));   // the whole sample: the shared copy
            } else {
                contract_mfma<CutT, KT, false>(As, ldA, k, crow, cbeg, cend, ws, zs, Hp, HP);
                combine(Hm, Hp0, HP, k, k);
            }
            sample_sync<NW>();
            // brackets lo <= lambda_max <= hi, replicated in every lane
            double trace = 0, total = 0, dmax = 0, rmax = 0;
            {
                double diag = 0, rsum = 0, rabs = 0;
                if (lane < k) {
                    diag = Hm[lane * HP + lane];
                    for (int c = 0; c < k; ++c) { const double v = Hm[lane * HP + c]; rsum += v; rabs += fabs(v); }
                }
                for (int i = 0; i < k; ++i) {
                    const double di = bcast(diag, i);
                    trace += di; dmax = fmax(dmax, di);
                    total += bcast(rsum, i); rmax = fmax(rmax, bcast(rabs, i));
                }
            }
            const double lo = fmax(dmax, total / (double)k);     // Rayleigh quotients <= lambda_max
            const double hi = fmin(trace, rmax);                 // trace, Gershgorin  >= lambda_max
            const double c2 = cfac * cfac;
            if (inertia_not_above<KT, KCAP>(Hm, HP, k, c2 * hi) == 0) {
                deficient = false;
            } else if (inertia_not_above<KT, KCAP>(Hm, HP, k, c2 * lo) > 0) {
                deficient = true;
            } else {
                jacobi_lane0<KT, NW>(Hm, HP, k, tid);
                const double ev = lane < k ? fmax(Hm[lane * HP + lane], 0.0) : 0.0;
                const double svv = sqrt(ev), smax = wave_max(svv);
                deficient = __popcll(__ballot(lane < k && svv > smax * cfac)) < k;
            }
            sample_sync<NW>();
        }
        if (deficient) {                                   // dual :156-161
            if (tid == 0) { st.finished[u] = 1; st.n_iters[u] = t - 1; st.skip_fg[u] = 1; }
            return;
        }
    }

    lap(2);
    // ---- 4. multipliers (row layout: lane i < k holds lam_i) -----------------------------------
    double lam = 0.0;
    int updates = 0, updates_before = 0;
    if constexpr (IPM) {
        int ipm_status = 0;
        if constexpr (NW > 1) {
            // wide rows (round 5): the columns over the NW waves (ipm_solve_waves; GLB: bundle rows from device memory); what it
            // does not cover -- more than IPM_KMAX_WAVES cuts -- runs the one-wave solve on wave 0 while the others wait
            const int kp = k < 2 ? 2 : hv_padded(k);
            const bool waves_ok = sizeof(CutT) == 4 && k <= IPM_KMAX_WAVES && NW * ((ipm_nv(kp) + 3) & ~3) <= n_pad;
            if (waves_ok) {
                lam = ipm_solve_waves<CutT, KT, NW, GLB>(As, ldA, k, n, n_pad, ws, zs, sp, reinterpret_cast<double *>(smem + cv.yv),
                                                    reinterpret_cast<double *>(smem + cv.dv), Hp, HP, h_i, tid, &ipm_status, lap);
            } else {
                if (w0) {
                    lam = ipm_solve<CutT, KT, GLB>(As, ldA, k, crow, n, n_pad, ws, zs, sp, reinterpret_cast<double *>(smem + cv.yv),
                                                   reinterpret_cast<double *>(smem + cv.dv), Hm, HP, h_i, lane, &ipm_status, lap);
                    if (lane == 0) slots[KT - 1] = ipm_status;      // (slot list: at most KT - 1 entries)
                }
                sample_sync<NW>();
                ipm_status = slots[KT - 1];
            }
        } else
        lam = ipm_solve<CutT, KT, GLB>(As, ldA, k, crow, n, n_pad, ws, zs, sp, reinterpret_cast<double *>(smem + cv.yv),
                                  reinterpret_cast<double *>(smem + cv.dv), Hm, HP, h_i, lane, &ipm_status, lap);
        if (ipm_status) {                                  // numpy.linalg.cholesky raises (:42): the caller sees LinAlgError
            if (tid == 0) { st.status[u] |= ICNN_BE_ST_SINGULAR; st.finished[u] = 1; st.skip_fg[u] = 1; }
            return;
        }
    } else if (k == 1) {
        lam = lane == 0 ? 1.0 : 0.0;                       // dual :167
    } else {
        // c = np.sum(A, axis=1) + b with the row sum in the cut dtype (dual :18)
        CutT *rowsum = reinterpret_cast<CutT *>(psum);
        np_pairwise_rows<NW, CutT>(plan, k, [&](int r, int j) { return As[r * ldA + j]; },
                                   reinterpret_cast<CutT *>(leaf), rowsum, tid);
        const double c_i = lane < k ? (double)rowsum[lane] + h_i : 0.0;
        sample_sync<NW>();
        lap(3);
        const int cap = RL ? 20 : 100;                     // rl :29 / dual :30
        const int backoff_cap = RL ? 10 : 50;              // rl :65 / dual :67
        const bool shortcut = !(st.flags & ICNN_BE_FLAG_NO_CYCLE_SHORTCUT);
        lam = lane < k ? 1.0 / (double)k : 0.0;            // dual :26
        double prev1 = 0.0, prev2 = 0.0, prev3 = 0.0, prev4 = 0.0;
        int hist = 0, last_jump = -1000;                   // valid previous iterates (<= 4); update of the last jump
        double d4_prev = -1.0;                             // max|lam_{t-1} - lam_{t-5}| of the previous update; -1: not available
        bool abort_sample = false, parked = false;
        int upd0 = 0;                                      // updates done in earlier rounds
        double *park = st.park + (size_t)u * (5 * T + 4);
        if (resume) {
            updates = upd0 = updates_before = uni((int)park[5 * T]);
            hist = uni((int)park[5 * T + 1]);
            last_jump = uni((int)park[5 * T + 2]);
            d4_prev = uni(park[5 * T + 3]);
            if (lane < k) {
                lam = park[lane]; prev1 = park[T + lane]; prev2 = park[2 * T + lane]; prev3 = park[3 * T + lane];
                prev4 = park[4 * T + lane];
            }
        }
        int budget = a.budget > 0 ? a.budget : cap;

        while (updates < cap) {
            if (SLICED && budget-- <= 0) { parked = true; break; }
            // a = A^T lam, z = sigmoid(a), w = z (1 - z)                     dual :32-33
            if (KCAP > 0 || valu) {
                double *part = hv_part + (updates & 1) * (NW * hv_p);
                hv_column_pass_k<CutT, NW, true, LR, GLB, (NW == 1 && KT > 16), KCAP>(As, AsL, ldA, k, rows_cap, n, n_pad, tid, lam, part + wave * hv_p);
                sample_sync<NW>();
                lap(4);
                if (NW > 1) hv_gather<NW, true>(part, hv_p, Hp, HP, k, lane, 64, hv_first);  // this wave's own copy of H | A z
                lap(5);
            } else {
                for_columns<CutT>(As, ldA, k, rows_cap, n_pad, NT, tid, lam, [&](int j, bool valid, double aj) {
                    double z = sigmoid_fast(aj);
                    double w = z * (1.0 - z);
                    if (j >= n) { z = 0.0; w = 0.0; }
                    if (valid) {
                        zs[j] = z;
                        ws[j] = w;
                        if (RL) sp[j] = j < n ? softplus_fast(aj) : 0.0;
                    }
                });
                sample_sync<NW>();
                lap(4);
                contract_mfma<CutT, KT, true>(As, ldA, k, crow, cbeg, cend, ws, zs, Hp, HP, lap);
                combine(Hm, Hp0, HP, k, k + 1);
                sample_sync<NW>();
                lap(5);
            }
            const double *Hq = valu ? Hp : Hm;                                 // the system this wave reads
            // one wave per sample on the pass: there is no other wave's share to add, the sums are read where the pass left
            // them -- the packed upper triangle (k <= 8: the instance's size is the bundle's), A z behind it
            static_assert(HV_K1MAX <= 8 && hv_padded(HV_K1MAX) == HV_K1MAX, "the packed triangle of a k-cut bundle is the k-cut instance's");
            const bool tri = KCAP > 0 || (NW == 1 && valu);
            const int hvT = k * (k + 1) / 2;

            const double grad = lane < k ? -c_i + (tri ? hv_part[(updates & 1) * (NW * hv_p) + hvT + lane] : Hq[lane * HP + k]) : 0.0;     // dual :35
            // first maximum of lam (:39), replicated scan
            int piv_v = 0;
            {
                const double mx = rows_reduce<KT>(lane < k ? lam : -1e300, k, [](double x, double y) { return fmax(x, y); });
                const unsigned long long at = __ballot(lane < k && lam == mx);
                piv_v = at ? __builtin_ctzll(at) : 0;
            }
            const int piv = __builtin_amdgcn_readfirstlane(piv_v);
            const bool is_piv = lane == piv;
            const double red = is_piv ? 1.0 : lam;                               // :40-41
            const double keep = is_piv ? 0.0 : 1.0;                              // :42
            const double g0 = grad - keep * bcast(grad, piv);                    // :44
            const bool bound = is_piv || (red <= BOUND_EPS && g0 > 0.0);         // :48-49
            const bool is_free = lane < k && !bound;
            const unsigned long long fmask = __ballot(is_free);
            const double nrm2 = rows_reduce<KT>(is_free ? g0 * g0 : 0.0, k, [](double x, double y) { return x + y; });
            if (sqrt(nrm2) < GRAD_TOL) break;                                    // :50 -> return lam

            lap(8);
            const StepResult sr = tri ? newton_step_tri<KCAP>(hv_part + (updates & 1) * (NW * hv_p), k, piv, fmask, is_free, g0)
                                      : newton_step<KT>(Hq, HP, k, piv, fmask, is_free, g0);
            const double step = sr.step;
            if (!__builtin_amdgcn_readfirstlane(sr.ok)) {
                if (tid == 0) st.status[u] |= ICNN_BE_ST_SINGULAR;
                if (!RL) abort_sample = true;              // dual :63 raises
                break;                                     // rl :62 keeps lam
            }

            lap(9);
            double tt = 1.0;                                                     // dual :66
            double fval = 0.0, slope = 0.0;
            if (RL) {
                double dmax = 0.0;
                for (int i = 0; i < k; ++i) dmax = fmax(dmax, fabs(bcast(step, i)));
                tt = fmin(1.0 / dmax, 1.0);                                      // rl :64
                sample_sync<NW>();
                np_pairwise_rows<NW, double>(plan, 1, [&](int, int j) { return sp[j]; }, leaf, psum, tid);
                double cl = 0.0;
                for (int i = 0; i < k; ++i) { cl += bcast(c_i * lam, i); slope += bcast(step * g0, i); }
                fval = -cl + psum[0];                                            // :34
                sample_sync<NW>();
            }
            double lam_new = lam;
            bool returned = false;
            for (int bt = 0; bt < backoff_cap; ++bt) {
                const double trial = is_piv ? 1.0 : fmax(red + tt * step, 0.0);  // :68-69
                const double s = rows_reduce<KT>((lane < k && !is_piv) ? trial : 0.0, k,              // e.dot(y_n)
                                                 [](double x, double y) { return x + y; });
                const double lam_p = 1.0 - s;                                    // :71
                lam_new = lane < k ? (is_piv ? lam_p : trial) : 0.0;
                bool accept = false;
                if (lam_p >= 0.0) {
                    if (RL) {                                                    // rl :71-74
                        for (int j = tid; j < n_pad; j += NT) {
                            double aj = 0.0;
                            for (int i = 0; i < k; ++i) aj += bcast(lam_new, i) * (double)As[i * ldA + j];
                            sp[j] = j < n ? softplus_fast(aj) : 0.0;
                        }
                        sample_sync<NW>();
                        np_pairwise_rows<NW, double>(plan, 1, [&](int, int j) { return sp[j]; }, leaf, psum, tid);
                        double cl = 0.0;
                        for (int i = 0; i < k; ++i) cl += bcast(c_i * lam_new, i);
                        const double f_new = -cl + psum[0];
                        sample_sync<NW>();
                        accept = f_new < fval + tt * ARMIJO_ALPHA * slope;
                    } else {
                        accept = true;
                    }
                }
                if (accept) break;
                if (RL) {
                    double mv = 0.0;
                    for (int i = 0; i < k; ++i) mv = fmax(mv, tt * fabs(bcast(step, i)));
                    if (mv < TINY) { returned = true; break; }                   // rl :77
                } else if (tt < TINY) { returned = true; break; }                // dual :79
                tt *= 0.5;
            }
            ++updates;
            if (returned) { lam = lam_new; break; }
            if (shortcut && hist >= 1) {
                if (!__any(fabs(lam_new - prev1) > CYCLE_TOL)) { lam = lam_new; break; }
                if (hist >= 2 && !__any(fabs(lam_new - prev2) > CYCLE_TOL)) {
                    lam = ((cap - updates) & 1) ? prev1 : lam_new;
                    break;
                }
                // period 3: lam_cap = lam_{updates + r}, r = (cap - updates) mod 3, and lam_{t+1} = lam_{t-2}
                if (hist >= 3 && !__any(fabs(lam_new - prev3) > CYCLE_TOL)) {
                    const int r = (cap - updates) % 3;
                    lam = r == 0 ? lam_new : (r == 1 ? prev2 : prev1);
                    break;
                }
                // period 4: lam_{t+1} = lam_{t-3}
                if (hist >= 4 && !__any(fabs(lam_new - prev4) > CYCLE_TOL)) {
                    const int r = (cap - updates) & 3;
                    lam = r == 0 ? lam_new : (r == 1 ? prev3 : (r == 2 ? prev2 : prev1));
                    break;
                }
                // the same periods at their rounding floor (NOISE_TOL above).  Stateless but for one scalar: "an update cycle
                // earlier" is formed from the four stored iterates (period 3 compares with ONE update earlier, lam_{t-1} -
                // lam_{t-4}; period 4 with its own value of the previous update, which is parked with the iterates).
                if (!RL && updates >= NOISE_T0 && hist >= 2) {
                    const bool in = lane < k;
                    const auto mx = [](double x, double y) { return fmax(x, y); };
                    const double d1 = rows_reduce<KT>(in ? fabs(lam_new - prev1) : 0.0, k, mx);
                    if (d1 <= NOISE_TOL && d1 >= rows_reduce<KT>(in ? fabs(prev1 - prev2) : 0.0, k, mx)) { lam = lam_new; break; }
                    if (hist >= 4) {
                        const double d2 = rows_reduce<KT>(in ? fabs(lam_new - prev2) : 0.0, k, mx);
                        if (d2 <= NOISE_TOL && d2 >= rows_reduce<KT>(in ? fabs(prev2 - prev4) : 0.0, k, mx)) {
                            lam = ((cap - updates) & 1) ? prev1 : lam_new;
                            break;
                        }
                        const double d3 = rows_reduce<KT>(in ? fabs(lam_new - prev3) : 0.0, k, mx);
                        if (d3 <= NOISE_TOL && d3 >= rows_reduce<KT>(in ? fabs(prev1 - prev4) : 0.0, k, mx)) {
                            const int r = (cap - updates) % 3;
                            lam = r == 0 ? lam_new : (r == 1 ? prev2 : prev1);
                            break;
                        }
                        const double d4 = rows_reduce<KT>(in ? fabs(lam_new - prev4) : 0.0, k, mx);
                        if (d4 <= NOISE_TOL && d4_prev >= 0.0 && d4 >= d4_prev) {
                            const int r = (cap - updates) & 3;
                            lam = r == 0 ? lam_new : (r == 1 ? prev3 : (r == 2 ? prev2 : prev1));
                            break;
                        }
                        d4_prev = d4;
                    } else {
                        d4_prev = -1.0;
                    }
                }
            }
            // Slow 2-cycles (contraction 0.6-0.7 per update: 35-85 updates until lam_t - lam_{t-2} <= 1e-13; a
            // handful per 40 000 solves, each of which holds its whole tile or launch): once the even and the
            // odd subsequence converge geometrically, both are extrapolated to their limits (one step of the
            // vector Aitken / Anderson-1 formula with a common ratio) and the iteration goes on from there.  The
            // stopping rule above is unchanged, so what is returned is still an iterate that repeats within
            // 1e-13 after two updates, i.e. a point of the limit cycle the reference's 100 updates end on.
            bool jumped = false;
            if (shortcut && hist >= 4 && updates >= ACCEL_T0 && updates - last_jump >= ACCEL_GAP) {
                const bool in = lane < k;
                const double d_t = in ? lam_new - prev2 : 0.0, d_p = in ? prev2 - prev4 : 0.0;
                const auto mx = [](double x, double y) { return fmax(x, y); };
                const auto ad = [](double x, double y) { return x + y; };
                const double n1 = rows_reduce<KT>(fabs(d_t), k, mx), n0 = rows_reduce<KT>(fabs(d_p), k, mx);
                if (n1 > 0.0 && n1 < ACCEL_D2MAX && n1 < n0) {
                    const double ratio = rows_reduce<KT>(d_t * d_p, k, ad) / rows_reduce<KT>(d_p * d_p, k, ad);
                    // ratio < 0 (each subsequence oscillates around its limit): only where the reference's own remaining
                    // updates would close the gap anyway, |lam_cap - limit| ~ n1 |ratio|^((cap - t) / 2) <= ACCEL_NEG_RESID
                    bool take = ratio > 0.0 && ratio < ACCEL_RMAX;
                    if (ratio < 0.0 && -ratio < ACCEL_RMAX) {
                        double left = n1;
                        for (int m = (cap - updates) / 2; m > 0; --m) left *= -ratio;
                        take = left <= ACCEL_NEG_RESID;
                    }
                    if (take) {
                        const double gain = ratio / (1.0 - ratio);
                        const double xe = lam_new + d_t * gain;                       // limit of lam_t, lam_{t+-2}, ..
                        const double xo = in ? prev1 + (prev1 - prev3) * gain : 0.0;  // limit of lam_{t-1}, ..
                        if (!__any(in && (xe < 0.0 || xo < 0.0))) {
                            lam_new = xe;                // lam_t := xe, lam_{t-1} := xo; older history is void
                            prev1 = xe;
                            prev2 = xo;
                            hist = 2;
                            d4_prev = -1.0;
                            last_jump = updates;
                            jumped = true;
                        }
                    }
                }
            }
            if (!jumped) {
                prev4 = prev3;
                prev3 = prev2;
                prev2 = prev1;
                prev1 = lam_new;
                hist = hist < 4 ? hist + 1 : 4;
            }
            lam = lam_new;                                                       // :84
            if (!valu) sample_sync<NW>();       // Hm / zs / ws are rewritten by the next iteration
            lap(6);
        }
        if (abort_sample) {
            if (tid == 0) { st.finished[u] = 1; st.skip_fg[u] = 1; }
            return;
        }
        if (parked) {                                      // continue in the next round
            if (w0 && lane < k) {
                park[lane] = lam; park[T + lane] = prev1; park[2 * T + lane] = prev2; park[3 * T + lane] = prev3;
                park[4 * T + lane] = prev4;
            }
            if (tid == 0) {
                park[5 * T] = (double)updates;
                park[5 * T + 1] = (double)hist;
                park[5 * T + 2] = (double)last_jump;
                park[5 * T + 3] = d4_prev;
                st.newton_iters[u] += updates - upd0;
                st.phase[u] = 1;
                st.skip_fg[u] = 1;
                st.pending[round] = 1;   // plain store: only "any work left" is needed, and a
                                           // same-address atomic per sample costs ~13 ns each (50 us per launch)
            }
            return;
        }
    }

    lap(6);
    // The bookkeeping below re-reads its pointers from the kernel-argument segment through an opaque
    // pointer: otherwise a dozen 64-bit pointers stay live in SGPRs across the whole Newton loop, whose
    // scalar registers then spill (v_readlane/v_writelane traffic on the critical path).
    typedef const __attribute__((address_space(4))) DualArgs KernArgs;   // the by-value argument, in place
    KernArgs *ea;
    if constexpr (std::is_same<ArgsT, DualArgs>::value) ea = (KernArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    else ea = (KernArgs *)uni((unsigned long long)&a);    // already a reference into the kernel-argument segment
    asm volatile("" : "+s"(ea));
    KernArgs &eargs = *ea;
    const auto &es = eargs.st;
    // ---- 5. y <- sigmoid(-A^T lam), bookkeeping ---------------------------------------
    double *ey_row = es.y + (size_t)u * n;
    double move = 0.0;
    bool nonfinite = false;
    auto commit = [&](int j, double ynew) {
        if (RL) {
            ynew = fmin(fmax(ynew, 0.03), 0.97);                   // rl :118,:123
            move = fmax(move, fabs(ey_row[j] - ynew));
        }
        nonfinite |= !isfinite(ynew);
        ey_row[j] = ynew;
    };
    if constexpr (IPM) {
        const double *yv = reinterpret_cast<const double *>(smem + cv.yv);
        for (int j = tid; j < n; j += NT) commit(j, yv[j]);         // lib/bundle_entropy.py:225: x[u] = y of pdipm_pc
    } else if (k == 1) {
        for (int j = tid; j < n; j += NT)
            commit(j, (double)Cut<CutT>::sigmoid_neg(As[j]));      // dual :168, cut-dtype arithmetic
    } else {
        for_columns<CutT>(As, ldA, k, rows_cap, n_pad, NT, tid, lam, [&](int j, bool, double aj) {
            const double ynew = 1.0 / (1.0 + exp(aj));             // dual :165
            if (j < n) commit(j, ynew);
        });
    }
    bool fin = false;
    if (RL && wave_max(move) < 1e-6) fin = true;                        // rl :125-126 (NW == 1 only)
    if (wg_any(nonfinite)) { fin = true; if (tid == 0) es.status[u] |= ICNN_BE_ST_NONFINITE; }

    const bool pos = lane < k && lam > (IPM ? 1e-8 : 0.0);           // dual :171-174; lib/bundle_entropy.py:234-237
    const unsigned long long pmask = __ballot(pos);
    if (pos && w0) {
        const int at = __popcll(pmask & ((1ull << lane) - 1ull));
        es.active[(size_t)u * T + at] = slots[lane];
        es.lam[(size_t)u * T + at] = lam;
    }
    if (tid == 0) {
        es.count[u] = __popcll(pmask);
        es.newton_iters[u] += updates - updates_before;
        if (fin) es.finished[u] = 1;
        const bool more = !fin && t + 1 < TI;
        es.t_next[u] = t + 1;
        es.phase[u] = 0;
        es.skip_fg[u] = more ? 0 : 1;
        if (more) es.pending[round] = 1;   // plain store: only "any work left" is needed, and a
                                           // same-address atomic per sample costs ~13 ns each (50 us per launch)
    }
    lap(7);
}

// Wide rows past the LDS capacity (n = 2048: 12 cuts), the rounds in which a bundle could outgrow it: the bundle is staged in
// device memory as in any GLB round, and -- split staging -- its WIDE_LR oldest rows are mirrored in LDS for the fused VALU pass,
// which re-reads them there and keeps the few younger rows in registers: per Newton update a sample with 15 cuts streams 3 rows
// from L2 instead of 15 (256 samples x 123 KB do not fit the L2s, the GLB rounds were bound by that traffic).  The mirror fits
// next to the carve-up of a bundle of up to HV_KMAX cuts; a sample beyond that (rows_cap = every row the round allows) runs the
// plain GLB body: no mirror, MFMA sweep.  Same arithmetic whichever way a sample is staged: no bit of its result changes.
constexpr int WIDE_LR = 12;
__global__ __launch_bounds__(512, 1) void dual_step_wide_kernel(DualArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int k = __builtin_amdgcn_readfirstlane(a.st.count[blockIdx.x]) + 1;
    const int mid = a.rows < HV_KMAX ? a.rows : HV_KMAX;
    dual_step_body<DualCfg<float, 32, 8, false, false, /* GLB */ true, /* LR */ WIDE_LR>>(a, blockIdx.x, threadIdx.x, smem, a.round, k <= mid ? mid : a.rows, nullptr);
}

template <typename CutT, int KT, int NW, bool RL, bool IPM = false, bool GLB = false>
__global__ __launch_bounds__(64 * NW, NW == 1 ? (RL && KT > 16 ? 2 : 4) : 1) void dual_step_kernel(DualArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    dual_step_body<DualCfg<CutT, KT, NW, RL, IPM, GLB>>(a, blockIdx.x, threadIdx.x, smem, a.round, a.rows, nullptr);
}


}  // namespace
}  // namespace icnn_be
