// Adam inner optimiser of the RL agent (RL/src/icnn.py:160-215 `adam(func, obs)` with func = `_fg_entr`, :59-63,131):
// projected Adam on negQ(obs, act) - H((act+1)/2) over act in [-1+1e-8, 1-1e-8]^n from act = 0, best iterate per
// sample, batch-level stopping rule -- up to 1000 evaluations of the PICNN and its action gradient per call.  The
// reference pays one sess.run per evaluation; here the WHOLE loop is one launch: a persistent workgroup per tile of
// 16 states alternates
//     phase A  fc_fg_tile (be_picnn_fc_dev.h: negQ and d negQ / d act of the tile on the f32 MFMA chain)
//     phase B  one wave per state: entropy term, best-iterate bookkeeping, moment update, clipped step (float64)
// and the only cross-workgroup traffic is the stopping rule's mean displacement of the best iterates: one double
// per tile and iteration through a grid barrier (none at all for batch <= 16, the agent's act() shape).
//
// Arithmetic contract (oracle/adam_oracle.py reproduces it bit for bit): entropy per element from the float32
// action with float64 logs rounded to float32, summed sequentially in float32; the moment products (1-b1) g and
// (1-b2) g g in float32 as NumPy forms them, everything else float64 with IEEE division and square root, no
// contraction; the step divides by sqrt(v) (not vhat) as the reference does.
#include "be_dual_dev.h"
#include "be_picnn_fc_dev.h"
#include "be_picnn_fc_rows_dev.h"
#include "be_rl_dev.h"

namespace icnn_be {

namespace {

struct AdamArgs {
    FcArgs fa;            // fa.y = act, fa.f / fa.g = per-iteration energies / gradients, fa.finished = nullptr
    double *act, *m, *v;  // [B][n] iterate and moments (workspace; initialised by the kernel)
    double *act_best;     // [B][n] out
    float *f_best;        // [B] out
    double *partial;      // [2][tiles] per-tile sums of ||best_t - best_{t-1}||, double-buffered by iteration parity
    unsigned *arrive;     // [tiles] iteration number each workgroup has published, zero at launch
    int *iters;           // out: iterations run (== max_iter when the rule never fired)
    int max_iter, tiles, red_off;   // red_off: float offset of the reduction scratch behind fc_fg_tile's LDS
};

__device__ __forceinline__ float lane_value(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Sum of one double per workgroup over all workgroups of the (cooperative) launch, the same value (same order) in
// every workgroup; called by all lanes of ONE wave per workgroup.  Flag-based, no read-modify-write: a counter
// that 256 workgroups increment serialises at the device's coherence point (0.15 us per arrival: 40 us per
// iteration), and release/acquire semantics at agent scope would write back and INVALIDATE the whole L2 of every
// XCD each iteration, so that the read-only weights came from memory again.  Here a workgroup publishes its
// partial sum and then its iteration number (both agent-scope atomic stores, the second after the first has been
// acknowledged), and every workgroup polls all iteration numbers, 64 per round across the lanes, and then reads
// the partial sums: everything the workgroups exchange goes through agent-scope atomics, nothing else needs
// ordering.  `partial` is double-buffered by iteration parity (a slot is rewritten only after everybody has passed
// the next exchange).
__device__ __forceinline__ double grid_sum(double *partial, unsigned *seq, int tiles, int it, int me, double mine,
                                           int lane) {
    double *slot = partial + (size_t)(it & 1) * tiles;
    if (lane == 0) {
        __hip_atomic_store(slot + me, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(seq + me, (unsigned)it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (;;) {
        bool ready = true;
        for (int t = lane; t < tiles; t += 64)
            ready &= __hip_atomic_load(seq + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)it;
        if (__all(ready)) break;
        __builtin_amdgcn_s_sleep(4);
    }
    asm volatile("" ::: "memory");
    double acc = 0.0;
    for (int t = lane; t < tiles; t += 64) acc += __hip_atomic_load(slot + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return wave_sum(acc);
}

// Phase A reads its arguments from the kernel-argument segment and is inlined into the iteration loop (as a function
// of its own it saved and restored 48 callee-saved VGPRs per call; see be_fused.hip for why the inlined form needs
// the opaque thread index and -mllvm -disable-machine-licm to stay at 17 spilled values).
typedef const __attribute__((address_space(4))) AdamArgs KArgs;
__device__ __forceinline__ void phase_fg(KArgs *kp, int tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    asm volatile("" : "+s"(kp), "+s"(tile));
    fc_fg_tile(kp->fa, tile, lds);
}

// EACH: the stopping rule of every state on its own (icnn_be_adam_fc_each): drift from the state's own displacement, a state
// whose rule has fired is frozen (phase A still evaluates its row, phase B leaves it alone), the workgroup leaves when none of
// its states is live.  No exchange between workgroups, a.iters is [B].
template <bool EACH>
__global__ __launch_bounds__(NTHREADS) void adam_fc_kernel(AdamArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    KArgs *kp = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    double *red = reinterpret_cast<double *>(lds + a.red_off);      // [NWAVE] per-state moves, [NWAVE] the batch sum
    const int tile = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = a.fa.n, batch = a.fa.batch;
    const int u = tile * TM + wave;
    const bool mine = u < batch;
    const size_t row = (size_t)(mine ? u : 0) * n;
    const double b1 = 0.9, b2 = 0.999, box = 1. - 1e-8;
    const float c1 = (float)(1. - b1), c2 = (float)(1. - b2);       // NumPy: weak Python scalar times a float32 array
    if (mine)
        for (int j = lane; j < n; j += 64) a.act[row + j] = a.m[row + j] = a.v[row + j] = 0.0;
    __syncthreads();
    double pow1 = 1.0, pow2 = 1.0, drift = -1.0;                    // drift < 0: not yet defined (:186)
    float best_f = 0.f;                                             // wave-uniform, written out when it improves
    int it = 0;
    bool live = mine;                                               // EACH: this wave's state has not fired yet
    int fired = a.max_iter;
    long long tick = ICNN_BE_PROF_ON(a.fa.prof) ? (long long)__builtin_readcyclecounter() : 0;
    auto lap = [&](int phase) {          // diagnostic only (tools/fc_phase_profile.py adam): slots 14/15 of phase A's table
        if (ICNN_BE_PROF_ON(a.fa.prof)) {
            const long long now = (long long)__builtin_readcyclecounter();
            if (lane == 0)
                atomicAdd(reinterpret_cast<unsigned long long *>(a.fa.prof) +
                              ((size_t)tile * NWAVE + wave) * FC_PROF_PHASES + phase,
                          (unsigned long long)(now - tick));
            tick = now;
        }
    };
    for (; it < a.max_iter; ++it) {
        phase_fg(kp, tile);
        __syncthreads();
        if (ICNN_BE_PROF_ON(a.fa.prof)) tick = (long long)__builtin_readcyclecounter();
        // ---- f = negQ + sum_j pen_j, g += d pen / d act; best iterate (:176-183) ----
        double moved = 0.0;
        if (EACH ? live : mine) {
            float tot = 0.f;
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int j = j0 + lane;
                float pen = 0.f;
                if (j < n) {
                    const EntropyTerm e = rl_entropy_term((float)a.act[row + j]);
                    pen = e.pen;
                    const float ge = a.fa.g[row + j] + e.dpen;
                    a.fa.g[row + j] = ge;                                        // read back by the same lane below
                }
                const int cnt = n - j0 < 64 ? n - j0 : 64;
                for (int l = 0; l < cnt; ++l) tot = tot + lane_value(pen, l);
            }
            const float fe = a.fa.f[u] + tot;
            const bool better = it == 0 || fe < best_f;
            if (better) {
                double d2 = 0.0;
                for (int j = lane; j < n; j += 64) {
                    const double x = a.act[row + j];
                    const double d = it == 0 ? 0.0 : x - a.act_best[row + j];
                    d2 += d * d;
                    a.act_best[row + j] = x;
                }
                best_f = fe;
                if (lane == 0) a.f_best[u] = fe;
                moved = sqrt(wave_sum(d2));
            }
        }
        // ---- stopping rule over the whole batch (:184-192), or over this state as a batch of one ----
        if constexpr (EACH) {
            if (it > 0 && live) {
                drift = drift < 0.0 ? moved : 0.5 * drift + 0.5 * moved;
                if (drift < 1e-3 && it > 5) { live = false; fired = it; }
            }
            if (it > 5) {                                           // the exit is the workgroup's: OR of `live` over the waves
                if (lane == 0) red[wave] = live ? 1.0 : 0.0;
                __syncthreads();
                double any = 0.0;
                for (int w = 0; w < NWAVE; ++w) any += red[w];
                if (any == 0.0) break;
            }
        } else if (it > 0) {
            if (lane == 0) red[wave] = moved;
            __syncthreads();
            if (wave == 0) {
                double s = 0.0;
                for (int w = 0; w < NWAVE; ++w) s += red[w];
                if (a.tiles > 1) s = grid_sum(a.partial, a.arrive, a.tiles, it, tile, s, lane);
                if (lane == 0) red[NWAVE] = s;
            }
            __syncthreads();
            const double step_mean = red[NWAVE] / (double)batch;
            drift = drift < 0.0 ? step_mean : 0.5 * drift + 0.5 * step_mean;
            if (drift < 1e-3 && it > 5) break;
        }
        lap(14);
        // ---- moments and the clipped step (:194-203) ----
        pow1 *= b1;
        pow2 *= b2;
        if (EACH ? live : mine)
            for (int j = lane; j < n; j += 64) {
                const float ge = a.fa.g[row + j];
                const double mj = b1 * a.m[row + j] + (double)(c1 * ge);
                const double vj = b2 * a.v[row + j] + (double)(c2 * (ge * ge));
                a.m[row + j] = mj;
                a.v[row + j] = vj;
                const double mhat = mj / (1. - pow1);
                double x = a.act[row + j] - (0.01 * mhat) / (sqrt(vj) + 1e-8);
                x = fmin(fmax(x, -box), box);
                a.act[row + j] = x;
            }
        __syncthreads();                                            // act visible to the tile's next phase A
        lap(15);
    }
    if constexpr (EACH) {
        if (mine && lane == 0) a.iters[u] = fired;
    } else if (tile == 0 && tid == 0) {
        *a.iters = it;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Latency path: 1-4 states per workgroup -- the agent's act() optimises ONE observation per environment step
// (RL/src/icnn.py:264-288), its training step a minibatch of 256 (one state per CU here, the stopping rule through
// the same grid barrier as above).  A 16-row MFMA tile would spend the same 31 us per evaluation on one row as on
// sixteen (the chain of k-blocks through a single matrix pipe per SIMD); here each (state, 64 columns) unit is a
// wave of its own running the k-ordered fma chain of its columns on the VALU -- the very order the MFMA
// applies (kk = 16 kb + 4 q + s, s outer; oracle/picnn_chain.c), so the two paths agree bit for bit -- with
// the packed weights read as 16-byte fragments straight from L2 and EVERYTHING else (context rows, activations,
// iterate, moments, best iterate) resident in LDS and registers for the whole loop: no global store until the end.
// ---------------------------------------------------------------------------------------------------------
struct RowsArgs {
    AdamArgs a;
    RowsLayout lay;
    int per_wg;                        // states per workgroup (<= ROWS_MAX); a.tiles = number of workgroups
    CtxRowsArgs cr;                    // cr.obs != nullptr: the context rows are computed here from the observations
};

template <bool EACH>
__global__ __launch_bounds__(RTHREADS) void adam_rows_kernel(RowsArgs r) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const FcArgs &fa = r.a.fa;
    const RowsLayout &lay = r.lay;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = fa.n, total = fa.batch, RF = lay.row_floats;
    const int s_base = blockIdx.x * r.per_wg;                         // this workgroup's states
    const int batch = total - s_base < r.per_wg ? total - s_base : r.per_wg;
    float *fbuf = lds + lay.f_off;                                    // [ROWS_MAX] energies
    double *red = reinterpret_cast<double *>(lds + lay.misc_off);     // [ROWS_MAX] moves, [1] the batch sum
    if (r.cr.obs) rows_context_from_obs(r.cr, fa, lay, lds, s_base, batch, tid);
    rows_setup(fa, lay, lds, s_base, batch, tid, r.cr.obs != nullptr);   // act = 0 (:169): all operands zero
    // Adam state of (state = wave, action component = lane) in registers
    const bool mine = wave < batch && lane < n;
    const double b1 = 0.9, b2 = 0.999, box = 1. - 1e-8;
    const float c1 = (float)(1. - b1), c2 = (float)(1. - b2);
    double x = 0.0, m1 = 0.0, m2 = 0.0, best_x = 0.0, pow1 = 1.0, pow2 = 1.0, drift = -1.0;
    float best_f = 0.f;
    int it = 0;
    bool live = wave < batch;                                         // EACH: as in adam_fc_kernel
    int fired = r.a.max_iter;
    long long tick = ICNN_BE_PROF_ON(fa.prof) ? (long long)__builtin_readcyclecounter() : 0;
    auto lap = [&](int phase) {          // diagnostic only (tools/fc_phase_profile.py adam): [wave][phase] cycle sums
        if (ICNN_BE_PROF_ON(fa.prof)) {
            const long long now = (long long)__builtin_readcyclecounter();
            if (lane == 0)
                atomicAdd(reinterpret_cast<unsigned long long *>(fa.prof) + (size_t)wave * FC_PROF_PHASES + phase,
                          (unsigned long long)(now - tick));
            tick = now;
        }
    };
    for (; it < r.a.max_iter; ++it) {
        // ================= phase A: negQ and d negQ / d act of every state (be_picnn_fc_rows_dev.h) ===============
        rows_eval(fa, lay, lds, batch, tid, lap);
        // ================= phase B: the same operations as adam_fc_kernel, state in registers =================
        double moved = 0.0;
        float ge = 0.f;
        if (EACH ? live : wave < batch) {
            const float *row = lds + wave * RF;
            float pen = 0.f;
            if (lane < n) {
                const EntropyTerm e = rl_entropy_term((float)x);
                pen = e.pen;
                ge = row[lay.g_off + lane] + e.dpen;
            }
            float tot = 0.f;
            for (int l = 0; l < n; ++l) tot = tot + lane_value(pen, l);
            const float fe = fbuf[wave] + tot;
            if (it == 0 || fe < best_f) {
                const double d = it == 0 || lane >= n ? 0.0 : x - best_x;
                best_x = x;
                best_f = fe;
                moved = sqrt(wave_sum(d * d));
            }
        }
        if constexpr (EACH) {
            if (it > 0 && live) {
                drift = drift < 0.0 ? moved : 0.5 * drift + 0.5 * moved;
                if (drift < 1e-3 && it > 5) { live = false; fired = it; }
            }
            if (it > 5) {
                if (lane == 0 && wave < ROWS_MAX) red[wave] = live ? 1.0 : 0.0;
                __syncthreads();
                double any = 0.0;
                for (int w = 0; w < batch; ++w) any += red[w];
                if (any == 0.0) break;
            }
        } else if (it > 0) {
            if (lane == 0 && wave < ROWS_MAX) red[wave] = wave < batch ? moved : 0.0;
            __syncthreads();
            double ssum = 0.0;
            for (int w = 0; w < batch; ++w) ssum += red[w];
            if (r.a.tiles > 1) {          // several workgroups: one double each, exchanged as in adam_fc_kernel
                if (wave == 0) {
                    const double tsum = grid_sum(r.a.partial, r.a.arrive, r.a.tiles, it, blockIdx.x, ssum, lane);
                    if (lane == 0) red[ROWS_MAX] = tsum;
                }
                __syncthreads();
                ssum = red[ROWS_MAX];
            }
            const double step_mean = ssum / (double)total;
            drift = drift < 0.0 ? step_mean : 0.5 * drift + 0.5 * step_mean;
            if (drift < 1e-3 && it > 5) break;
        }
        lap(14);
        pow1 *= b1;
        pow2 *= b2;
        if (EACH ? mine && live : mine) {
            m1 = b1 * m1 + (double)(c1 * ge);
            m2 = b2 * m2 + (double)(c2 * (ge * ge));
            const double mhat = m1 / (1. - pow1);
            x = x - (0.01 * mhat) / (sqrt(m2) + 1e-8);
            x = fmin(fmax(x, -box), box);
            // network input of the next evaluation, already multiplied into every layer's operand y * yu_i
            rows_set_input(fa, lay, lds + wave * RF, lane, (float)x);
        }
        __syncthreads();
        lap(15);
    }
    if (mine) r.a.act_best[(size_t)(s_base + wave) * n + lane] = best_x;
    if (wave < batch && lane == 0) r.a.f_best[s_base + wave] = best_f;
    if constexpr (EACH) {
        if (wave < batch && lane == 0) r.a.iters[s_base + wave] = fired;
    } else if (blockIdx.x == 0 && tid == 0) {
        *r.a.iters = it;
    }
}

struct Workspace {
    size_t act, m, v, g, f, partial, arrive, total;
};
Workspace workspace(int batch, int n) {
    Workspace w;
    const size_t bn = (size_t)(batch > 0 ? batch : 1) * n, tiles = (size_t)batch + 1;   // up to one workgroup per state
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    w.act = take(bn * 8); w.m = take(bn * 8); w.v = take(bn * 8);
    w.g = take(bn * 4); w.f = take((size_t)(batch > 0 ? batch : 1) * 4);
    w.partial = take(2 * tiles * 8); w.arrive = take(tiles * 4);
    w.total = o;
    return w;
}

}  // namespace

size_t adam_workspace_bytes(int batch, int n) { return workspace(batch, n).total; }

namespace {

// What launch_adam_fc does with a model and a batch, decided in ONE place (icnn_be_debug_adam_plan reports it; results are
// bit-identical whichever kernel runs).  dim(action) <= 64 with at most ROWS_MAX states per resident workgroup: the latency
// path (adam_rows_kernel, everything in LDS and registers), as few states per workgroup as keep all workgroups resident;
// otherwise 16-state MFMA tiles (adam_fc_kernel).  One workgroup is an ordinary launch, several a cooperative one: the
// stopping rule needs them all resident, and ICNN_BE_ADAM_NONE says they would not be.  With `cx` the plan also says
// whether the observations can take the place of the context rows: latency path only, a model without BatchNorm, the
// producer's scratch inside the row's operand region.  Enqueues nothing; with more than ROWS_MAX states it asks the
// runtime how many workgroups fit a CU (and raises the kernel's dynamic-LDS limit first, as the launch would).
struct AdamLaunch {
    AdamPlan plan;
    int lds;              // dynamic LDS bytes of the launch
    RowsLayout lay;       // the latency path's
};

// `each` (icnn_be_adam_fc_each): the same rule for the rows path -- 1-4 states per workgroup over as many workgroups as would be
// resident --, but nothing couples the workgroups: an ordinary launch, and any number of 16-state tiles beyond it.
hipError_t plan_adam(const icnn_be_fc_model &m, const icnn_be_fc_ctx *cx, int batch, FcArgs &fa, AdamLaunch &p,
                     bool each = false) {
    const void *rows_kernel = each ? reinterpret_cast<const void *>(adam_rows_kernel<true>)
                                   : reinterpret_cast<const void *>(adam_rows_kernel<false>);
    const void *tile_kernel = reinterpret_cast<const void *>(adam_fc_kernel<false>);
    p = AdamLaunch{};
    int lds = 0;
    if (fill_args(m, fa, lds) != 0) return hipErrorInvalidValue;
    if (m.n <= 64) {   // latency path: 1-4 states per workgroup, as many workgroups as fit
        const int rows_lds = rows_layout(m, ROWS_MAX, p.lay) + (ROWS_MAX + 1) * 8;
        int resident = 1;
        if (rows_lds <= LDS_BYTES && batch > ROWS_MAX) {      // more than one workgroup: they must all be resident
            if (hipError_t e = ensure_dynamic_lds(rows_kernel, rows_lds); e != hipSuccess) return e;
            int per_cu = 0;
            hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rows_kernel, RTHREADS, rows_lds);
            if (e != hipSuccess) return e;
            resident = per_cu * device_cus();
        }
        const int per_wg = batch <= ROWS_MAX ? batch : (batch + resident - 1) / (resident > 0 ? resident : 1);
        if (rows_lds <= LDS_BYTES && per_wg >= 1 && per_wg <= ROWS_MAX) {
            const int wgs = (batch + per_wg - 1) / per_wg;
            p.plan = {ICNN_BE_ADAM_ROWS, per_wg, wgs, wgs > 1 && !each, 0};
            p.lds = rows_lds;
            if (cx && !cx->batchnorm && cx->n == m.n && cx->n_layers == m.n_layers) {
                for (int i = 0; i < m.n_layers; ++i)           // (icnn_be_adam_fc_obs has refused these already: the stage matrices
                    if (cx->width[i] != m.width[i]) return hipErrorInvalidValue;   //  are laid out for cx's widths, read with m's)
                int wmax = cx->n_features;
                for (int i = 0; i + 1 < m.n_layers; ++i) wmax = m.width[i] > wmax ? m.width[i] : wmax;
                p.plan.obs_ok = 2 * wmax <= p.lay.ctx_off;                      // scratch = the row's operand region
            }
            return hipSuccess;
        }
    }
    const int tiles = (batch + TM - 1) / TM;
    lds = ((fa.lds_floats + 3) & ~3) * 4 + (NWAVE + 1) * 8;     // the reduction scratch behind fc_fg_tile's LDS
    if (lds > LDS_BYTES) return hipSuccess;                     // ICNN_BE_ADAM_NONE
    p.lds = lds;
    if (tiles > 1 && !each) {
        if (hipError_t e = ensure_dynamic_lds(tile_kernel, lds); e != hipSuccess) return e;
        int per_cu = 0;
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, tile_kernel, NTHREADS, lds);
        if (e != hipSuccess) return e;
        if (tiles > per_cu * device_cus()) return hipSuccess;   // ICNN_BE_ADAM_NONE
    }
    p.plan = {ICNN_BE_ADAM_TILE, TM, tiles, tiles > 1 && !each, 0};
    return hipSuccess;
}

}  // namespace

hipError_t adam_fc_plan(const icnn_be_fc_model &m, const icnn_be_fc_ctx *cx, int batch, AdamPlan &plan, bool each) {
    FcArgs fa{};
    AdamLaunch p;
    const hipError_t e = plan_adam(m, each ? nullptr : cx, batch, fa, p, each);
    plan = p.plan;
    return e;
}

// hipErrorNotSupported: more tiles than a cooperative launch can keep resident (the stopping rule needs them all)
// `cx` + `obs` instead of `ctx`: observation -> action in ONE launch (latency path only: at most ROWS_MAX states per
// workgroup, a model without BatchNorm); hipErrorNotSupported otherwise -- the caller produces the context first.
hipError_t launch_adam_fc(const icnn_be_fc_model &m, const float *ctx, int batch, int max_iter, double *act_best,
                          float *f_best, int *iters, void *ws, hipStream_t stream, const icnn_be_fc_ctx *cx,
                          const float *obs, bool each) {
    AdamArgs a{};
    AdamLaunch p;
    if (each && obs) return hipErrorInvalidValue;
    if (hipError_t e = plan_adam(m, obs ? cx : nullptr, batch, a.fa, p, each); e != hipSuccess) return e;
    if (p.plan.kernel == ICNN_BE_ADAM_NONE || (obs && !p.plan.obs_ok)) return hipErrorNotSupported;
    const Workspace w = workspace(batch, m.n);
    unsigned char *base = static_cast<unsigned char *>(ws);
    a.act = reinterpret_cast<double *>(base + w.act);
    a.m = reinterpret_cast<double *>(base + w.m);
    a.v = reinterpret_cast<double *>(base + w.v);
    a.partial = reinterpret_cast<double *>(base + w.partial);
    a.arrive = reinterpret_cast<unsigned *>(base + w.arrive);
    a.fa.ctx = ctx; a.fa.y = a.act; a.fa.batch = batch; a.fa.finished = nullptr; a.fa.prof = fc_profile_buffer();
    a.fa.g = reinterpret_cast<float *>(base + w.g);
    a.fa.f = reinterpret_cast<float *>(base + w.f);
    a.act_best = act_best; a.f_best = f_best; a.iters = iters;
    a.max_iter = max_iter;
    a.tiles = p.plan.workgroups;
    if (p.plan.cooperative)
        if (hipError_t e = hipMemsetAsync(a.arrive, 0, sizeof(unsigned) * a.tiles, stream); e != hipSuccess) return e;
    if (p.plan.kernel == ICNN_BE_ADAM_ROWS) {
        RowsArgs r{};
        r.a = a;
        r.lay = p.lay;
        r.per_wg = p.plan.per_wg;
        if (obs) {
            r.cr.obs = obs;
            r.cr.n_features = cx->n_features;
            for (int i = 0; i < m.n_layers; ++i) { r.cr.w_stage[i] = cx->w_stage[i]; r.cr.b_stage[i] = cx->b_stage[i]; }
        }
        if (each) return launch_kernel(adam_rows_kernel<true>, dim3(a.tiles), dim3(RTHREADS), p.lds, stream, r);
        if (!p.plan.cooperative) return launch_kernel(adam_rows_kernel<false>, dim3(1), dim3(RTHREADS), p.lds, stream, r);
        void *params[] = {&r};
        return hipLaunchCooperativeKernel(reinterpret_cast<const void *>(adam_rows_kernel<false>), dim3(a.tiles), dim3(RTHREADS),
                                          params, (unsigned)p.lds, stream);
    }
    a.red_off = (a.fa.lds_floats + 3) & ~3;
    if (each) return launch_kernel(adam_fc_kernel<true>, dim3(a.tiles), dim3(NTHREADS), p.lds, stream, a);
    if (!p.plan.cooperative) return launch_kernel(adam_fc_kernel<false>, dim3(1), dim3(NTHREADS), p.lds, stream, a);
    void *params[] = {&a};
    return hipLaunchCooperativeKernel(reinterpret_cast<const void *>(adam_fc_kernel<false>), dim3(a.tiles), dim3(NTHREADS), params,
                                      (unsigned)p.lds, stream);
}

}  // namespace icnn_be
