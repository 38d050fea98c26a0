// C ABI of libicnn_be.so (see include/icnn_be.h for the contract and the reference lines each entry point replaces): the
// error state, the per-device launch configuration, the solve plan, and every entry that takes an icnn_be_state, a model
// (icnn_be_fc_model, icnn_be_conv_model, icnn_be_ficnn_model) or a context descriptor (icnn_be_fc_ctx, icnn_be_conv_ctx).
// Those entries share checks across units and own the dispatch.  An entry that takes none of them concerns one unit only
// and is defined in that unit, behind its kernels (be_api_check.h has what such entries share).  Everything here only
// validates arguments and enqueues work.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>

#include <map>
#include <mutex>
#include <utility>

#include "be_api_check.h"
#include "be_kernels.h"
#include "icnn_be.h"

namespace {
thread_local hipError_t g_last = hipSuccess;

int fail(hipError_t e) {
    g_last = e;
    return e == hipErrorInvalidValue ? ICNN_BE_EINVAL : ICNN_BE_ELAUNCH;
}

int done(hipError_t e) { return e == hipSuccess ? 0 : fail(e); }
}  // namespace

// for the entries defined beside their kernels
int icnn_be::api_done(hipError_t e) { return done(e); }

namespace {

// everything about a state but its buffers
int check_shape(const icnn_be_state *st) {
    if (!st) return ICNN_BE_EINVAL;
    if (st->batch < 0 || st->n < 1) return ICNN_BE_EINVAL;
    if (st->slots < 1) return ICNN_BE_EINVAL;
    if (st->slots > ICNN_BE_MAX_SLOTS || st->iters > ICNN_BE_MAX_ITERS) return ICNN_BE_ELIMIT;
    if (st->iters != 0 && st->iters < st->slots) return ICNN_BE_EINVAL;
    if (st->cut_dtype != ICNN_BE_CUT_F32 && st->cut_dtype != ICNN_BE_CUT_F64) return ICNN_BE_EINVAL;
    if (st->variant != ICNN_BE_VARIANT_DUAL && st->variant != ICNN_BE_VARIANT_RL && st->variant != ICNN_BE_VARIANT_PDIPM)
        return ICNN_BE_EINVAL;
    /* a bundle of at least two cuts (one, for a single iteration) must fit the LDS of a workgroup */
    const int fit = icnn_be::dual_rows_fit(st->n, st->slots, st->cut_dtype, st->variant);
    if (fit < (st->slots < 2 ? st->slots : 2)) return ICNN_BE_ELIMIT;
    return 0;
}

int check_state(const icnn_be_state *st) {
    if (int rc = check_shape(st)) return rc;
    if (!st->y || !st->G || !st->h || !st->ys || !st->lam || !st->active || !st->count ||
        !st->n_iters || !st->finished || !st->status || !st->newton_iters || !st->t_next || !st->phase ||
        !st->skip_fg || !st->pending || !st->park)
        return ICNN_BE_EINVAL;
    return 0;
}

// BatchNorm mode arguments of the *_context_bn / *_surrogate_grad_bn entries (include/icnn_be.h); n[l] > 0 for the
// batch-normalised layers.  mv is only needed (and only checked) when the model normalises and the call reads or folds it.
int check_bn_mode(const icnn_be_bn_moving *mv, int mode, int updates, const int *n, int nl) {
    if (mode != ICNN_BE_BN_BATCH && mode != ICNN_BE_BN_MOVING) return ICNN_BE_EINVAL;
    if (updates < 0 || (mode == ICNN_BE_BN_MOVING && updates > 0)) return ICNN_BE_EINVAL;
    bool any = false;
    for (int l = 0; l < nl; ++l) any = any || n[l] > 0;
    if (!any || (mode == ICNN_BE_BN_BATCH && updates == 0)) return 0;
    if (!mv || !(mv->decay >= 0.f && mv->decay <= 1.f)) return ICNN_BE_EINVAL;
    for (int l = 0; l < nl; ++l)
        if (n[l] > 0 && (!mv->mean[l] || !mv->var[l])) return ICNN_BE_EINVAL;
    return 0;
}

// what the GD and PGD entries of every model refuse alike; constants_ok: gd_constants_ok / pgd_constants_ok of the call's own
template <typename Model>
int check_gd_args(const Model *model, const float *ctx, const double *y0, const double *y_out, const void *workspace, int batch,
                  int n_iter, bool constants_ok) {
    if (!model || !ctx || !y0 || !y_out || !workspace || !model->wpack) return ICNN_BE_EINVAL;
    if (batch < 0 || n_iter < 1 || !constants_ok) return ICNN_BE_EINVAL;
    return 0;
}

// what icnn_be_solve_fc requires of a model and a state beyond their buffers
int check_fc_solve(const icnn_be_fc_model *model, const icnn_be_state *st) {
    if (int rc = check_shape(st)) return rc;
    if (!model || st->cut_dtype != ICNN_BE_CUT_F32 || st->n != model->n) return ICNN_BE_EINVAL;
    if (st->flags & ICNN_BE_FLAG_F64_ENERGY) return ICNN_BE_EINVAL;        /* the fused energies are float32 */
    return icnn_be::fc_check_model(*model);
}
}  // namespace

namespace icnn_be {
namespace {
std::mutex g_cfg_mutex;
std::map<std::pair<int, const void *>, int> g_lds_limit;   // (device, kernel) -> configured dynamic LDS bytes
std::map<int, int> g_cus;                                  // device -> CU count
int current_device() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? dev : 0;
}
}  // namespace

hipError_t ensure_dynamic_lds(const void *kernel, int bytes) {
    const int dev = current_device();
    std::lock_guard<std::mutex> lock(g_cfg_mutex);
    int &have = g_lds_limit[std::make_pair(dev, kernel)];
    if (bytes <= have) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) have = bytes;
    else (void)hipGetLastError();      // do not leave the refusal behind as the "last error" of a later, successful launch
    return e;
}

int device_cus() {
    const int dev = current_device();
    std::lock_guard<std::mutex> lock(g_cfg_mutex);
    int &cus = g_cus[dev];
    if (cus == 0) {
        hipDeviceProp_t prop;
        cus = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0
                  ? prop.multiProcessorCount : 256;
    }
    return cus;
}
}  // namespace icnn_be

namespace {
constexpr int SLICE_BUDGET = 8;   /* Newton updates per sliced round before a sample is parked ("Solve dispatch") */
static_assert(ICNN_BE_MAX_ROUNDS >= 2 * ICNN_BE_MAX_ITERS, "a sliced solve's straggler rounds fit st.pending");

int outer_iters(const icnn_be_state &st) { return st.iters > 0 ? st.iters : st.slots; }

/* Sliced rounds without a finishing launch: nIter more unbudgeted rounds for the samples that are behind.  How many are
   needed -- the largest lag -- is only known on the device, and the host does NOT ask (no synchronisation anywhere in this
   library; the call stays capturable in a HIP graph); a sample cannot be behind by more than the nIter iterations it has and
   an unbudgeted round completes one of them, so nIter rounds always suffice ("Solve dispatch"). */
int sliced_extra_rounds(int T) { return T + (T < ICNN_BE_MAX_ROUNDS - T ? T : ICNN_BE_MAX_ROUNDS - T); }

// `total` rounds of { energy/gradient ; dual step }, shared by the FC and the conv entry points.  The first nIter give each
// sample `budget` Newton updates (0: lockstep, every round completes an outer iteration of every sample); the rounds beyond
// them are unbudgeted straggler rounds, closed by a launch that marks anything still behind with ICNN_BE_ST_UNFINISHED
// (a safety net: unreachable by the argument of sliced_extra_rounds).
template <typename LaunchFg>
hipError_t solve_rounds(const icnn_be_state &st, int budget, int total, float *f_work, float *g_work, hipStream_t s,
                        LaunchFg launch_fg) {
    const int T = outer_iters(st);
    for (int r = 0; r < total; ++r) {
        hipError_t e = launch_fg();
        if (e == hipSuccess) e = icnn_be::launch_dual_step(st, r, r < T ? budget : 0, f_work, g_work, s);
        if (e != hipSuccess) return e;
    }
    return total > T ? icnn_be::launch_mark_unfinished(st, s) : hipSuccess;
}

/* The round solve of the models without a persistent kernel (icnn_be_solve_conv, icnn_be_solve_ficnn); returns the rounds or
   an ICNN_BE_E* code.  Lockstep rounds at EVERY nIter (time slicing on request, ICNN_BE_FLAG_TIME_SLICE).  Slicing pays when a
   round is held up by a Newton solve that runs its 100-update cap; since limit cycles at their rounding floor are recognised
   (be_dual_dev.h, NOISE_TOL) those are one solve in a thousand, while every sliced solve pays nIter finishing rounds of
   five launches for its few laggards.  Measured on the conv model at 256 samples (tools/conv_slice_experiment.py): nIter 30
   lockstep 12.0 / 11.0 ms against 16.4 / 15.0 sliced on two instances, nIter 5 2.24 / 1.73 against 2.22 / 2.04.  No finishing
   launch: the conv evaluation couples sixteen samples in the 2048 x 512 layer, so the stragglers get nIter whole rounds. */
template <typename LaunchFg>
int solve_generic(const icnn_be_state &st, float *f_work, float *g_work, hipStream_t s, LaunchFg launch_fg) {
    const bool lockstep = (st.flags & ICNN_BE_FLAG_LOCKSTEP) || st.variant == ICNN_BE_VARIANT_PDIPM ||
                          !(st.flags & ICNN_BE_FLAG_TIME_SLICE);
    const int T = outer_iters(st), total = lockstep ? T : sliced_extra_rounds(T);
    hipError_t e = solve_rounds(st, lockstep ? 0 : SLICE_BUDGET, total, f_work, g_work, s, launch_fg);
    return e == hipSuccess ? total : fail(e);
}

struct SolvePlan {
    int path;      // ICNN_BE_PATH_*, or a negative ICNN_BE_E* code
    int per_wg;    // samples per workgroup of the persistent kernel (0: launch pairs)
    int budget;    // Newton updates per sample and round (0: unlimited)
    int rounds;    // what icnn_be_solve_fc returns
};

int env_tile_budget() {
    static const int budget = [] {         /* tuning knob (tools/tile_budget_sweep.py); default measured there */
        const char *v = std::getenv("ICNN_BE_TILE_BUDGET");
        return v ? std::atoi(v) : 0;
    }();
    return budget;
}

// The dispatch table of icnn_be_solve_fc: the first row that applies decides.  Pure host arithmetic (no HIP call, no device
// memory); every fit decision is the layout function's that the launcher uses.  The measurements behind each row are in
// DESIGN.md, "Solve dispatch".  Results are bit-identical whichever row runs.
SolvePlan plan_fc_solve(const icnn_be_fc_model &m, const icnn_be_state &st, int cus, int env_budget) {
    const int T = outer_iters(st), F = st.flags;
    const bool dual = st.variant == ICNN_BE_VARIANT_DUAL, ipm = st.variant == ICNN_BE_VARIANT_PDIPM;
    const bool two = F & ICNN_BE_FLAG_TWO_KERNELS, persistent = F & ICNN_BE_FLAG_PERSISTENT, slice = F & ICNN_BE_FLAG_TIME_SLICE;
    const bool forced = F & (ICNN_BE_FLAG_TWO_KERNELS | ICNN_BE_FLAG_PERSISTENT | ICNN_BE_FLAG_TIME_SLICE | ICNN_BE_FLAG_LOCKSTEP);
    /* lockstep rounds by default up to nIter 15; the interior-point solve (fixed cap of 20 iterations per round) at any nIter */
    const bool lockstep = (F & ICNN_BE_FLAG_LOCKSTEP) || (!slice && T <= 15);
    const int per_wg = (st.batch + cus - 1) / cus, tiles = (st.batch + 15) / 16;
    const int tile_rows = per_wg <= 4 ? 4 : per_wg <= 8 ? 8 : 16;
    icnn_be::FusedRowsLayout rows;
    icnn_be::FusedTileLayout tile;
    // up to four samples per CU: a persistent workgroup per 1-4 samples, any nIter
    if (!forced && per_wg <= 4 && icnn_be::fused_rows_layout(m, st, per_wg, false, rows))
        return {ICNN_BE_PATH_ROWS, per_wg, 0, T};
    // nIter > 15 (or forced): persistent tiles, the dual phase in groups; a per-round update budget (TIME_SLICE, or the
    // ICNN_BE_TILE_BUDGET knob) parks samples, and one launch of the per-sample kernel finishes them
    if (!lockstep && !ipm && !two && ((dual && 4 * tiles >= cus && !slice) || persistent)) {
        const int budget = slice ? SLICE_BUDGET : env_budget;
        if (icnn_be::fused_tile_layout(m, st, tile_rows, budget, tile)) {
            if (budget <= 0) return {ICNN_BE_PATH_TILE, tile_rows, budget, T};
            if (!icnn_be::fused_rows_layout(m, st, 1, true, rows)) return {ICNN_BE_ELIMIT, 0, 0, 0};
            return {ICNN_BE_PATH_TILE_BUDGETED_THEN_ROWS, tile_rows, budget, T + 1};
        }
    }
    // lockstep tiles where every CU has between a quarter of a tile and two tiles (variants dual, pdipm), any batch if forced
    const bool tile_shape = (dual || ipm) && 4 * tiles >= cus && tiles <= 2 * cus;
    if (!two && (lockstep || ipm) && (persistent || tile_shape) && icnn_be::fused_tile_layout(m, st, tile_rows, 0, tile))
        return {ICNN_BE_PATH_TILE, tile_rows, 0, T};
    // launch pairs: lockstep, or time-sliced with the stragglers finished by the per-sample kernel or by nIter more rounds
    if (lockstep || ipm) return {ICNN_BE_PATH_ROUNDS_LOCKSTEP, 0, 0, T};
    if (!two && icnn_be::fused_rows_layout(m, st, 1, true, rows))
        return {ICNN_BE_PATH_ROUNDS_SLICED_THEN_ROWS, 0, SLICE_BUDGET, T + 1};
    return {ICNN_BE_PATH_ROUNDS_SLICED_EXTRA, 0, SLICE_BUDGET, sliced_extra_rounds(T)};
}
}  // namespace

extern "C" {

int icnn_be_abi_version(void) { return ICNN_BE_ABI_VERSION; }

const char *icnn_be_last_hip_error(void) { return hipGetErrorString(g_last); }

size_t icnn_be_struct_size(int which) {
    return which == 0 ? sizeof(icnn_be_state) : which == 1 ? sizeof(icnn_be_fc_model)
         : which == 2 ? sizeof(icnn_be_fc_ctx) : which == 3 ? sizeof(icnn_be_conv_model)
         : which == 4 ? sizeof(icnn_be_conv_ctx) : which == 5 ? sizeof(icnn_be_bn_moving)
         : which == 6 ? sizeof(icnn_be_param_update_args) : which == 7 ? sizeof(icnn_be_rl_update_args)
         : which == 8 ? sizeof(icnn_be_ficnn_model) : which == 9 ? sizeof(icnn_be_replay)
         : which == 10 ? sizeof(icnn_be_dataset) : which == 11 ? sizeof(icnn_be_step_log)
         : which == 13 ? sizeof(icnn_be_ddpg_args) : which == 14 ? sizeof(icnn_be_naf_args)
         : which == 16 ? sizeof(icnn_be_ff_args) : which == 18 ? sizeof(icnn_be_fcn_args)
         : which == 20 ? sizeof(icnn_be_naf_bn_args) : which == 22 ? sizeof(icnn_be_vec_replay) : 0;
}

/* diagnostic hooks (include/icnn_be.h): per-phase cycle counters */
void icnn_be_debug_profile(long long *device_buf) { icnn_be::set_dual_profile_buffer(device_buf); }
void icnn_be_debug_profile_fc(long long *device_buf) { icnn_be::set_fc_profile_buffer(device_buf); }
void icnn_be_debug_profile_conv(long long *device_buf) { icnn_be::set_conv_profile_buffer(device_buf); }

int icnn_be_debug_fast_math(int which, const double *x, double *out, int count, void *stream) {
    if (which < 0 || which > 3 || !x || !out || count < 0) return ICNN_BE_EINVAL;
    if (count == 0) return 0;
    return done(icnn_be::launch_fast_math(which, x, out, count, static_cast<hipStream_t>(stream)));
}

int icnn_be_debug_profile_phases(void) { return icnn_be::DUAL_PROF_PHASES; }
void icnn_be_debug_trace(long long *device_buf) { icnn_be::set_dual_trace_buffer(device_buf); }

int icnn_be_bundle_capacity(int n, int slots, int cut_dtype, int variant) {
    if (n < 1 || slots < 1 || slots > ICNN_BE_MAX_SLOTS) return ICNN_BE_EINVAL;
    return icnn_be::dual_rows_fit(n, slots, cut_dtype, variant);
}

size_t icnn_be_scratch_bytes(const icnn_be_state *shape) {
    if (!shape || shape->batch < 0 || shape->n < 1 || shape->slots < 1 || shape->slots > ICNN_BE_MAX_SLOTS) return 0;
    return icnn_be::scratch_bytes(*shape);
}

int icnn_be_dual_lds_bytes(int n, int slots, int cut_dtype) {
    if (n < 1 || slots < 1 || slots > ICNN_BE_MAX_SLOTS) return ICNN_BE_EINVAL;
    return icnn_be::dual_lds_bytes(n, slots, cut_dtype, ICNN_BE_VARIANT_PDIPM);   /* the variant with the most column buffers */
}

int icnn_be_state_init(const icnn_be_state *st, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (st->batch == 0) return 0;
    return done(icnn_be::launch_state_init(*st, static_cast<hipStream_t>(stream)));
}

int icnn_be_dual_step(const icnn_be_state *st, int t, const void *f, const void *g, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (t < 0 || t >= (st->iters > 0 ? st->iters : st->slots) || !f || !g) return ICNN_BE_EINVAL;
    if (st->batch == 0) return 0;
    /* lockstep: every unfinished sample is at outer iteration t and completes it in this launch */
    return done(icnn_be::launch_dual_step(*st, t, 0, f, g, static_cast<hipStream_t>(stream)));
}

int icnn_be_debug_dual_plan(const icnn_be_state *st, int t, int out[8]) {
    if (!out) return ICNN_BE_EINVAL;
    if (int rc = check_shape(st)) return rc;
    if (t < 0 || t >= (st->iters > 0 ? st->iters : st->slots) || st->batch == 0) return ICNN_BE_EINVAL;
    icnn_be::DualStepPlan p;
    if (!icnn_be::plan_dual_step(*st, t, p)) return ICNN_BE_EINVAL;
    out[0] = p.cut; out[1] = p.kt; out[2] = p.waves; out[3] = p.variant;
    out[4] = p.staged; out[5] = p.kernel; out[6] = p.lds; out[7] = p.rows;
    return 0;
}

int icnn_be_debug_dual_step_body(const icnn_be_state *st, int t, const void *f, const void *g, int which, int rows_mode,
                                 void *stream) {
    if (int rc = check_state(st)) return rc;
    if (t < 0 || t >= (st->iters > 0 ? st->iters : st->slots) || !f || !g) return ICNN_BE_EINVAL;
    return done(icnn_be::launch_dual_body_probe(*st, t, f, g, which, rows_mode, static_cast<hipStream_t>(stream)));
}

size_t icnn_be_fc_pack_floats(const icnn_be_fc_model *shape) {
    if (!shape || icnn_be::fc_check_model(*shape) != 0) return 0;
    return icnn_be::fc_pack_floats(*shape);
}

int icnn_be_fc_tile_rows(const icnn_be_fc_model *shape) {
    if (!shape) return ICNN_BE_EINVAL;
    return icnn_be::fc_tile_rows(*shape);
}

int icnn_be_fc_pack(const icnn_be_fc_model *shape, const float *const *w_yu_host,
                    const float *const *w_zu_host, float *out_host) {
    if (!shape || !w_yu_host || !w_zu_host || !out_host) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*shape)) return rc;
    for (int i = 0; i < shape->n_layers; ++i) {
        if (!w_yu_host[i]) return ICNN_BE_EINVAL;
        if (i > 0 && !w_zu_host[i]) return ICNN_BE_EINVAL;
    }
    return icnn_be::fc_pack(*shape, w_yu_host, w_zu_host, out_host);
}

int icnn_be_fc_fg(const icnn_be_fc_model *model, const float *ctx, const double *y, int batch,
                  float *f, float *g, const int *finished, void *stream) {
    if (!model || !ctx || !y || !f || !g || batch < 0 || !model->wpack) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    if (batch == 0) return 0;
    return done(icnn_be::launch_fc_fg(*model, ctx, y, batch, f, g, finished, static_cast<hipStream_t>(stream)));
}

namespace {
/* icnn_be_solve_fc and icnn_be_solve_fc_reset.  reset.on: the solve starts from y0 / the constant and from a fresh state.  A plan
   that begins with a persistent kernel resets inside that launch (every sample has one owner there); the others -- launch
   pairs, and budgeted tiles, whose finishing launch must find the state the tiles left -- get the reset as launches of its
   own in front. */
int solve_fc(const icnn_be_fc_model *model, const float *ctx, const icnn_be_state *st, float *f_work, float *g_work,
             const icnn_be::SolveReset &reset, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (!model || !ctx || !f_work || !g_work || !model->wpack) return ICNN_BE_EINVAL;
    if (int rc = check_fc_solve(model, st)) return rc;
    if (st->batch == 0) return 0;
    const SolvePlan p = plan_fc_solve(*model, *st, icnn_be::device_cus(), env_tile_budget());
    if (p.path < 0) return p.path;
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long *prof = icnn_be::dual_profile_buffer();
    auto finish = [&] { return icnn_be::launch_fused_rows_solve(*model, ctx, *st, f_work, g_work, 1, prof, s, true); };
    auto fg = [&] { return icnn_be::launch_fc_fg(*model, ctx, st->y, st->batch, f_work, g_work, st->skip_fg, s); };
    hipError_t e = hipSuccess;
    const bool in_kernel = p.path == ICNN_BE_PATH_ROWS || p.path == ICNN_BE_PATH_TILE;
    if (reset.on && !in_kernel) {
        e = icnn_be::launch_y_reset(*st, reset, s);
        if (e == hipSuccess) e = icnn_be::launch_state_init(*st, s);
        if (e != hipSuccess) return fail(e);
    }
    switch (p.path) {
    case ICNN_BE_PATH_ROWS:
        e = icnn_be::launch_fused_rows_solve(*model, ctx, *st, f_work, g_work, p.per_wg, prof, s, false, reset);
        break;
    case ICNN_BE_PATH_TILE:
        e = icnn_be::launch_fused_fc_solve(*model, ctx, *st, f_work, g_work, prof, s, p.per_wg, p.budget, reset);
        break;
    case ICNN_BE_PATH_TILE_BUDGETED_THEN_ROWS:
        e = icnn_be::launch_fused_fc_solve(*model, ctx, *st, f_work, g_work, prof, s, p.per_wg, p.budget);
        if (e == hipSuccess) e = finish();
        break;
    case ICNN_BE_PATH_ROUNDS_SLICED_THEN_ROWS:
        e = solve_rounds(*st, p.budget, outer_iters(*st), f_work, g_work, s, fg);
        if (e == hipSuccess) e = finish();
        break;
    default:            // ICNN_BE_PATH_ROUNDS_LOCKSTEP, ICNN_BE_PATH_ROUNDS_SLICED_EXTRA
        e = solve_rounds(*st, p.budget, p.rounds, f_work, g_work, s, fg);
    }
    return e == hipSuccess ? p.rounds : fail(e);
}
}  // namespace

int icnn_be_solve_fc(const icnn_be_fc_model *model, const float *ctx, const icnn_be_state *st,
                     float *f_work, float *g_work, void *stream) {
    return solve_fc(model, ctx, st, f_work, g_work, icnn_be::SolveReset{}, stream);
}

int icnn_be_solve_fc_reset(const icnn_be_fc_model *model, const float *ctx, const icnn_be_state *st,
                           float *f_work, float *g_work, const double *y0, double y0_fill, void *stream) {
    return solve_fc(model, ctx, st, f_work, g_work, icnn_be::SolveReset{1, y0, y0_fill}, stream);
}

int icnn_be_rl_bundle_solve(const icnn_be_fc_model *model, const float *ctx, const icnn_be_state *st, float *f_work,
                            float *g_work, double y0_fill, double *act_out, float *q_out, void *stream) {
    if (!model || !ctx || !st || !f_work || !g_work || !act_out) return ICNN_BE_EINVAL;
    if (int rc = check_state(st)) return rc;
    if (!model->wpack || model->action_box == 0 || st->variant != ICNN_BE_VARIANT_RL || st->cut_dtype != ICNN_BE_CUT_F32)
        return ICNN_BE_EINVAL;
    if (!std::isfinite(y0_fill)) return ICNN_BE_EINVAL;
    if (int rc = check_fc_solve(model, st)) return rc;
    if (icnn_be::fc_narrow_model(*model)) return ICNN_BE_ELIMIT;  /* the agents' networks are small: 16-row models only */
    if (st->batch == 0) return 0;
    const SolvePlan p = plan_fc_solve(*model, *st, icnn_be::device_cus(), env_tile_budget());
    if (p.path < 0) return p.path;
    if (p.path != ICNN_BE_PATH_ROWS) return ICNN_BE_ELIMIT;      /* the epilogue lives in the per-sample kernel only */
    const icnn_be::RowsValue value{act_out, q_out};
    hipError_t e = icnn_be::launch_fused_rows_solve(*model, ctx, *st, f_work, g_work, p.per_wg, icnn_be::dual_profile_buffer(),
                                                    static_cast<hipStream_t>(stream), false,
                                                    icnn_be::SolveReset{1, nullptr, y0_fill}, &value);
    return e == hipSuccess ? p.rounds : fail(e);
}

int icnn_be_debug_solve_plan(const icnn_be_fc_model *model, const icnn_be_state *st, int cus, int out[3]) {
    if (!out) return ICNN_BE_EINVAL;
    if (int rc = check_fc_solve(model, st)) return rc;
    if (st->batch == 0) return ICNN_BE_EINVAL;
    const SolvePlan p = plan_fc_solve(*model, *st, cus > 0 ? cus : icnn_be::device_cus(), env_tile_budget());
    if (p.path < 0) return p.path;
    out[0] = p.per_wg; out[1] = p.budget; out[2] = p.rounds;
    return p.path;
}

int icnn_be_debug_fc_deal(const icnn_be_fc_model *model, int *out, int cap) {
    if (!model || cap < 0 || (cap > 0 && !out)) return ICNN_BE_EINVAL;
    return icnn_be::fc_deal_units(*model, out, cap);
}

int icnn_be_debug_shape_instance(const icnn_be_fc_model *model, const icnn_be_state *st) {
    /* float64 cuts: icnn_be_solve_fc launches nothing for them, so no instance either; everything else it refuses is refused here */
    if (model && st && st->cut_dtype == ICNN_BE_CUT_F64 && check_shape(st) == 0 && st->n == model->n && st->batch > 0 &&
        icnn_be::fc_check_model(*model) == 0)
        return ICNN_BE_SHAPE_GENERIC;
    if (int rc = check_fc_solve(model, st)) return rc;
    if (st->batch == 0) return ICNN_BE_EINVAL;
    const SolvePlan p = plan_fc_solve(*model, *st, icnn_be::device_cus(), env_tile_budget());
    if (p.path < 0) return p.path;
    if (p.path != ICNN_BE_PATH_TILE) return ICNN_BE_SHAPE_GENERIC;
    return icnn_be::fused_shape_instance(*model, *st, p.per_wg, p.budget);
}

size_t icnn_be_fc_context_work_floats(const icnn_be_fc_ctx *c, int batch) {
    if (!c || batch < 0 || icnn_be::ctx_check(*c) != 0) return 0;
    return icnn_be::ctx_work_floats(*c, batch);
}

int icnn_be_fc_context(const icnn_be_fc_ctx *c, const float *x, int batch, float *ctx, int ctx_width, float *work,
                       void *stream) {
    return icnn_be_fc_context_bn(c, nullptr, ICNN_BE_BN_BATCH, 0, x, batch, ctx, ctx_width, work, stream);
}

size_t icnn_be_fc_context_bn_work_floats(const icnn_be_fc_ctx *c, int batch) {
    if (!c || batch < 0 || icnn_be::ctx_check(*c) != 0) return 0;
    return icnn_be::ctx_bn_work_floats(*c, batch);
}

namespace {
int fc_context_bn(const icnn_be_fc_ctx *c, const icnn_be_bn_moving *mv, int mode, int updates, const int *updates_dev,
                  const float *x, int batch, float *ctx, int ctx_width, float *work, void *stream) {
    if (!c || !x || !ctx || !work || batch < 0) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ctx_check(*c)) return rc;
    int n[ICNN_BE_MAX_LAYERS];
    icnn_be::fc_bn_widths(*c, n);
    /* a device count may be anything: the arguments a fold needs are checked as for one update */
    if (int rc = check_bn_mode(mv, mode, updates_dev ? 1 : updates, n, ICNN_BE_MAX_LAYERS)) return rc;
    if (batch == 0) return 0;
    return done(icnn_be::launch_fc_context(*c, x, batch, ctx, ctx_width, work, static_cast<hipStream_t>(stream), mv, mode,
                                           updates, updates_dev));
}
}  // namespace

int icnn_be_fc_context_bn(const icnn_be_fc_ctx *c, const icnn_be_bn_moving *mv, int mode, int updates, const float *x,
                          int batch, float *ctx, int ctx_width, float *work, void *stream) {
    return fc_context_bn(c, mv, mode, updates, nullptr, x, batch, ctx, ctx_width, work, stream);
}

int icnn_be_fc_context_bn_dev(const icnn_be_fc_ctx *c, const icnn_be_bn_moving *mv, const int *updates_dev, const float *x,
                              int batch, float *ctx, int ctx_width, float *work, void *stream) {
    if (!updates_dev) return ICNN_BE_EINVAL;
    return fc_context_bn(c, mv, ICNN_BE_BN_BATCH, 0, updates_dev, x, batch, ctx, ctx_width, work, stream);
}

size_t icnn_be_fc_grad_floats(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c) {
    if (!model || !c) return 0;
    return icnn_be::fc_grad_floats(*model, *c);
}

size_t icnn_be_fc_surrogate_grad_work_floats(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, int batch, int rows) {
    if (!model || !c) return 0;
    return icnn_be::fc_surrogate_work_floats(*model, *c, batch, rows);
}

int icnn_be_fc_surrogate_grad(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, const float *x, int batch,
                              const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                              float *grad, float *F_rows, float *work, void *stream) {
    return icnn_be_fc_surrogate_grad_bn(model, c, x, batch, row_offset, rows, y, v, cvec, grad, F_rows, work, nullptr, 0, stream);
}

int icnn_be_fc_surrogate_grad_bn(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, const float *x, int batch,
                                 const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                 float *grad, float *F_rows, float *work, const icnn_be_bn_moving *mv, int updates,
                                 void *stream) {
    return icnn_be_fc_surrogate_grad_dev(model, c, x, batch, row_offset, rows, y, v, cvec, grad, F_rows, work, mv, updates,
                                         nullptr, stream);
}

int icnn_be_fc_surrogate_grad_dev(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, const float *x, int batch,
                                  const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                  float *grad, float *F_rows, float *work, const icnn_be_bn_moving *mv, int updates,
                                  const int *rows_dev, void *stream) {
    if (!model || !c || !x || !row_offset || !y || !cvec || !grad || !work || !model->wpack) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ctx_check(*c)) return rc;
    int n[ICNN_BE_MAX_LAYERS];
    icnn_be::fc_bn_widths(*c, n);
    if (int rc = check_bn_mode(mv, ICNN_BE_BN_BATCH, updates, n, ICNN_BE_MAX_LAYERS)) return rc;
    if (int rc = icnn_be::fc_surrogate_shape(*model, *c, batch, rows, v != nullptr)) return rc;
    return done(icnn_be::launch_fc_surrogate_grad(*model, *c, x, batch, row_offset, rows, y, v, cvec, grad, F_rows, work,
                                                  static_cast<hipStream_t>(stream), mv, updates, rows_dev));
}

size_t icnn_be_fc_surrogate_grad_dev_work_floats(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, int batch, int rows) {
    if (!model || !c) return 0;
    return icnn_be::fc_surrogate_work_floats(*model, *c, batch, rows, true);
}

size_t icnn_be_conv_surrogate_grad_dev_work_floats(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, int batch,
                                                   int rows) {
    if (!model || !c) return 0;
    return icnn_be::conv_surrogate_work_floats(*model, *c, batch, rows, true);
}

size_t icnn_be_conv_grad_floats(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c) {
    if (!model || !c) return 0;
    return icnn_be::conv_grad_floats(*model, *c);
}

size_t icnn_be_conv_surrogate_grad_work_floats(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, int batch, int rows) {
    if (!model || !c) return 0;
    return icnn_be::conv_surrogate_work_floats(*model, *c, batch, rows);
}

int icnn_be_conv_surrogate_grad(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, const float *x, int batch,
                                const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                float *grad, float *F_rows, float *work, void *stream) {
    return icnn_be_conv_surrogate_grad_bn(model, c, x, batch, row_offset, rows, y, v, cvec, grad, F_rows, work, nullptr, 0,
                                          stream);
}

int icnn_be_conv_surrogate_grad_bn(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, const float *x, int batch,
                                   const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                   float *grad, float *F_rows, float *work, const icnn_be_bn_moving *mv, int updates,
                                   void *stream) {
    return icnn_be_conv_surrogate_grad_dev(model, c, x, batch, row_offset, rows, y, v, cvec, grad, F_rows, work, mv, updates,
                                           nullptr, stream);
}

int icnn_be_conv_surrogate_grad_dev(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, const float *x, int batch,
                                    const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                    float *grad, float *F_rows, float *work, const icnn_be_bn_moving *mv, int updates,
                                    const int *rows_dev, void *stream) {
    if (!model || !c || !x || !row_offset || !y || !cvec || !grad || !work || !model->wpack) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::conv_ctx_check(*c)) return rc;
    icnn_be::ConvCtxShape g{};
    if (int rc = icnn_be::conv_ctx_shape(*model, g)) return rc;
    int n[4];
    icnn_be::conv_bn_widths(g, n);
    if (int rc = check_bn_mode(mv, ICNN_BE_BN_BATCH, updates, n, 4)) return rc;
    if (int rc = icnn_be::conv_surrogate_shape(*model, *c, batch, rows, v != nullptr)) return rc;
    return done(icnn_be::launch_conv_surrogate_grad(*model, *c, x, batch, row_offset, rows, y, v, cvec, grad, F_rows, work,
                                                    static_cast<hipStream_t>(stream), mv, updates, rows_dev));
}

int icnn_be_fc_context_stage(const icnn_be_fc_ctx *c, int stage, const float *x, int batch, float *ctx, int ctx_width,
                             float *work, double *stats, void *stream) {
    /* an empty shard (a rank of a data-parallel group whose batch is smaller than the group) has no rows: its zero-element
       tensors have null data pointers, and it must still take part in the all-reduce of the sums */
    if (!c || batch < 0 || (batch > 0 && (!x || !ctx || !work))) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ctx_check(*c)) return rc;
    if (stage < 0 || stage >= c->n_layers) return ICNN_BE_EINVAL;
    if (batch == 0) return stage < c->n_layers - 2 && c->batchnorm ? 1 : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = icnn_be::launch_fc_context_stage(*c, stage, x, batch, ctx, ctx_width, work, s);
    if (e != hipSuccess) return fail(e);
    if (stage >= c->n_layers - 2 || !c->batchnorm) return 0;     /* no BatchNorm behind this stage */
    if (!stats) return ICNN_BE_EINVAL;
    icnn_be::launch_fc_context_sums(*c, stage, batch, work, stats, s, e);
    return e == hipSuccess ? 1 : fail(e);
}

int icnn_be_fc_context_norm(const icnn_be_fc_ctx *c, int stage, int batch, double batch_total, const double *stats,
                            float *work, void *stream) {
    if (!c || !stats || !work || batch < 0 || !(batch_total >= 1.0)) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ctx_check(*c)) return rc;
    if (stage < 0 || stage >= c->n_layers - 2 || !c->batchnorm) return ICNN_BE_EINVAL;
    if (batch == 0) return 0;
    return done(icnn_be::launch_fc_context_norm(*c, stage, batch, batch_total, stats, work, static_cast<hipStream_t>(stream)));
}

int icnn_be_fc_clamp(const icnn_be_fc_model *model, int mode, void *stream) {
    if (!model || !model->wpack || mode < ICNN_BE_CLAMP_ABS || mode > ICNN_BE_CLAMP_ABS_HALF) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    return done(icnn_be::launch_fc_clamp(*model, mode, static_cast<hipStream_t>(stream)));
}

size_t icnn_be_adam_workspace_bytes(int batch, int n) {
    return batch < 0 || n < 1 ? 0 : icnn_be::adam_workspace_bytes(batch, n);
}

int icnn_be_adam_fc(const icnn_be_fc_model *model, const float *ctx, int batch, int max_iter, double *act_best,
                    float *f_best, int *iters, void *workspace, void *stream) {
    if (!model || !ctx || !act_best || !f_best || !iters || !workspace || !model->wpack) return ICNN_BE_EINVAL;
    if (batch < 0 || max_iter < 1 || model->action_box) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    if (icnn_be::fc_narrow_model(*model)) return ICNN_BE_ELIMIT;      /* the Adam kernels own 16-row tiles */
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (batch == 0) {
        return done(hipMemsetAsync(iters, 0, sizeof(int), s));
    }
    hipError_t e = icnn_be::launch_adam_fc(*model, ctx, batch, max_iter, act_best, f_best, iters, workspace, s);
    if (e == hipErrorNotSupported) return ICNN_BE_ELIMIT;
    return done(e);
}

int icnn_be_adam_fc_each(const icnn_be_fc_model *model, const float *ctx, int batch, int max_iter, double *act_best,
                         float *f_best, int *iters, void *workspace, void *stream) {
    if (!model || !ctx || !act_best || !f_best || !iters || !workspace || !model->wpack) return ICNN_BE_EINVAL;
    if (batch < 0 || max_iter < 1 || model->action_box) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    if (icnn_be::fc_narrow_model(*model)) return ICNN_BE_ELIMIT;      /* the Adam kernels own 16-row tiles */
    if (batch == 0) return 0;                          /* iters is [0]: nothing to write */
    hipError_t e = icnn_be::launch_adam_fc(*model, ctx, batch, max_iter, act_best, f_best, iters, workspace,
                                           static_cast<hipStream_t>(stream), nullptr, nullptr, true);
    if (e == hipErrorNotSupported) return ICNN_BE_ELIMIT;
    return done(e);
}

int icnn_be_debug_adam_each_plan(const icnn_be_fc_model *model, int batch, int out[2]) {
    if (!model || !out || batch < 1 || model->action_box) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    if (icnn_be::fc_narrow_model(*model)) return ICNN_BE_ELIMIT;
    icnn_be::AdamPlan p{};
    if (hipError_t e = icnn_be::adam_fc_plan(*model, nullptr, batch, p, true); e != hipSuccess) return fail(e);
    out[0] = p.per_wg; out[1] = p.workgroups;
    return p.kernel;
}

int icnn_be_debug_adam_plan(const icnn_be_fc_model *model, const icnn_be_fc_ctx *cx, int batch, int out[4]) {
    if (!model || !out || batch < 1 || model->action_box) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    if (icnn_be::fc_narrow_model(*model)) return ICNN_BE_ELIMIT;
    if (cx) {                                          /* what icnn_be_adam_fc_obs refuses */
        if (int rc = icnn_be::ctx_check(*cx)) return rc;
        if (cx->u_last_relu || cx->n != model->n || cx->n_layers != model->n_layers) return ICNN_BE_EINVAL;
        for (int i = 0; i < model->n_layers; ++i)
            if (cx->width[i] != model->width[i]) return ICNN_BE_EINVAL;
    }
    icnn_be::AdamPlan p{};
    if (hipError_t e = icnn_be::adam_fc_plan(*model, cx, batch, p); e != hipSuccess) return fail(e);
    out[0] = p.per_wg; out[1] = p.workgroups; out[2] = p.cooperative; out[3] = p.obs_ok;
    return p.kernel;
}

int icnn_be_adam_fc_obs(const icnn_be_fc_model *model, const icnn_be_fc_ctx *cx, const float *obs, int batch, int max_iter,
                        double *act_best, float *f_best, int *iters, void *workspace, void *stream) {
    if (!model || !cx || !obs || !act_best || !f_best || !iters || !workspace || !model->wpack) return ICNN_BE_EINVAL;
    if (batch < 0 || max_iter < 1 || model->action_box) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    if (icnn_be::fc_narrow_model(*model)) return ICNN_BE_ELIMIT;      /* the Adam kernels own 16-row tiles */
    if (int rc = icnn_be::ctx_check(*cx)) return rc;
    if (cx->u_last_relu) return ICNN_BE_EINVAL;        /* the in-kernel producer keeps the last u layer linear */
    /* the in-kernel context producer sizes its reads from the MODEL's layer widths while the stage matrices were laid out
       for cx's: both structs must describe the same network */
    if (cx->n != model->n || cx->n_layers != model->n_layers) return ICNN_BE_EINVAL;
    for (int i = 0; i < model->n_layers; ++i)
        if (cx->width[i] != model->width[i]) return ICNN_BE_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (batch == 0) {
        return done(hipMemsetAsync(iters, 0, sizeof(int), s));
    }
    hipError_t e = icnn_be::launch_adam_fc(*model, nullptr, batch, max_iter, act_best, f_best, iters, workspace, s, cx, obs);
    if (e == hipErrorNotSupported) return ICNN_BE_ELIMIT;
    return done(e);
}

int icnn_be_implicit_feed(const icnn_be_state *st, const double *y_true, int loss, const int *row_offset,
                          double *fd_y, double *fd_v, double *fd_c, int *fd_sample, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (!y_true || !row_offset || !fd_y || !fd_v || !fd_c || !fd_sample) return ICNN_BE_EINVAL;
    if (loss != ICNN_BE_LOSS_XENT && loss != ICNN_BE_LOSS_MSE) return ICNN_BE_EINVAL;
    if (st->batch == 0) return 0;
    return done(icnn_be::launch_implicit_feed(*st, y_true, loss, row_offset, fd_y, fd_v, fd_c, fd_sample,
                                              static_cast<hipStream_t>(stream)));
}

int icnn_be_feed_plan(const icnn_be_state *st, const double *y_true, int loss, int *row_offset, int *counts,
                      double *loss_out, int *tallies, void *work, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (!y_true || !row_offset || !counts || !loss_out || !work) return ICNN_BE_EINVAL;
    if (loss != ICNN_BE_LOSS_XENT && loss != ICNN_BE_LOSS_MSE) return ICNN_BE_EINVAL;
    if (st->batch == 0) return 0;
    icnn_be::FeedPlanLaunch l{*st, y_true, loss, row_offset, counts, loss_out, tallies, work};
    return done(icnn_be::launch_feed_plan(l, static_cast<hipStream_t>(stream)));
}

int icnn_be_export_active(const icnn_be_state *st, const int *row_offset, void *G_rows, double *ys_rows, double *h_rows,
                          double *lam_rows, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (!row_offset || !G_rows || !ys_rows || !h_rows || !lam_rows) return ICNN_BE_EINVAL;
    if (st->batch == 0) return 0;
    return done(icnn_be::launch_export_active(*st, row_offset, G_rows, ys_rows, h_rows, lam_rows, static_cast<hipStream_t>(stream)));
}

size_t icnn_be_conv_pack_floats(const icnn_be_conv_model *shape) {
    return shape ? icnn_be::conv_pack_floats(*shape) : 0;
}

size_t icnn_be_conv_work_floats(const icnn_be_conv_model *shape, int batch) {
    return shape ? icnn_be::conv_work_floats(*shape, batch) : 0;
}

int icnn_be_conv_pack(const icnn_be_conv_model *shape, const float *const *w_yu_host,
                      const float *const *w_yr_host, const float *const *b_yr_host,
                      const float *const *w_zu_host, const float *w_fc3_host, const float *w_fc4_host,
                      float *out_host) {
    if (!shape || !w_yu_host || !w_yr_host || !b_yr_host || !w_zu_host || !w_fc3_host || !w_fc4_host || !out_host)
        return ICNN_BE_EINVAL;
    for (int l = 0; l < 3; ++l) {
        if (!w_yu_host[l] || (l < 2 && (!w_yr_host[l] || !b_yr_host[l])) || (l > 0 && !w_zu_host[l]))
            return ICNN_BE_EINVAL;
    }
    return icnn_be::conv_pack(*shape, w_yu_host, w_yr_host, b_yr_host, w_zu_host, w_fc3_host, w_fc4_host, out_host);
}

size_t icnn_be_gd_workspace_bytes(int batch, int n) {
    return batch < 0 || n < 1 ? 0 : icnn_be::gd_workspace_bytes(batch, n);
}

int icnn_be_fc_gd(const icnn_be_fc_model *model, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                  double momentum, double *y_out, double *traj, float *f_out, void *workspace, void *stream) {
    const bool constants_ok = icnn_be::gd_constants_ok(lr, momentum);
    if (int rc = check_gd_args(model, ctx, y0, y_out, workspace, batch, n_iter, constants_ok)) return rc;
    if (model->action_box) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    if (batch == 0) return 0;
    hipError_t e = icnn_be::launch_fc_gd(*model, ctx, y0, batch, n_iter, lr, momentum, y_out, traj, f_out, workspace,
                                         static_cast<hipStream_t>(stream));
    if (e == hipErrorNotSupported) return ICNN_BE_ELIMIT;
    return done(e);
}

int icnn_be_conv_gd(const icnn_be_conv_model *model, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                    double momentum, double *y_out, double *traj, float *f_out, void *workspace, void *stream) {
    const bool constants_ok = icnn_be::gd_constants_ok(lr, momentum);
    if (int rc = check_gd_args(model, ctx, y0, y_out, workspace, batch, n_iter, constants_ok)) return rc;
    if (int rc = icnn_be::conv_check_model(*model)) return rc;
    if (batch == 0) return 0;
    if (!model->work || model->work_batch < batch) return ICNN_BE_EINVAL;
    return done(icnn_be::launch_conv_gd(*model, ctx, y0, batch, n_iter, lr, momentum, y_out, traj, f_out, workspace,
                                        static_cast<hipStream_t>(stream)));
}

size_t icnn_be_pgd_workspace_bytes(int batch, int n) {
    return batch < 0 || n < 1 ? 0 : icnn_be::pgd_workspace_bytes(batch, n);
}

int icnn_be_fc_pgd(const icnn_be_fc_model *model, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                   double lo, double hi, double *y_out, double *obj, double *obj_final, void *workspace, void *stream) {
    const bool constants_ok = icnn_be::pgd_constants_ok(lr, lo, hi);
    if (int rc = check_gd_args(model, ctx, y0, y_out, workspace, batch, n_iter, constants_ok)) return rc;
    if (model->action_box) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::fc_check_model(*model)) return rc;
    if (batch == 0) return 0;
    hipError_t e = icnn_be::launch_fc_pgd(*model, ctx, y0, batch, n_iter, lr, lo, hi, y_out, obj, obj_final, workspace,
                                          static_cast<hipStream_t>(stream));
    if (e == hipErrorNotSupported) return ICNN_BE_ELIMIT;
    return done(e);
}

int icnn_be_conv_pgd(const icnn_be_conv_model *model, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                     double lo, double hi, double *y_out, double *obj, double *obj_final, void *workspace, void *stream) {
    const bool constants_ok = icnn_be::pgd_constants_ok(lr, lo, hi);
    if (int rc = check_gd_args(model, ctx, y0, y_out, workspace, batch, n_iter, constants_ok)) return rc;
    if (int rc = icnn_be::conv_check_model(*model)) return rc;
    if (batch == 0) return 0;
    if (!model->work || model->work_batch < batch) return ICNN_BE_EINVAL;
    return done(icnn_be::launch_conv_pgd(*model, ctx, y0, batch, n_iter, lr, lo, hi, y_out, obj, obj_final, workspace,
                                         static_cast<hipStream_t>(stream)));
}

int icnn_be_bundle_trace(const icnn_be_state *st, double *obj, int *calls, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (!obj || !calls || !st->fvals) return ICNN_BE_EINVAL;
    if (st->variant == ICNN_BE_VARIANT_RL) return ICNN_BE_EINVAL;      /* its callback has no x */
    if (st->iters != 0) return ICNN_BE_ELIMIT;                         /* recycled slots hold no per-iteration history */
    if (st->batch == 0) return 0;
    return done(icnn_be::launch_bundle_trace(*st, obj, calls, static_cast<hipStream_t>(stream)));
}

int icnn_be_dual_bound(const icnn_be_state *st, double *out, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (!out) return ICNN_BE_EINVAL;
    if (st->batch == 0) return 0;
    return done(icnn_be::launch_dual_bound(*st, out, static_cast<hipStream_t>(stream)));
}

int icnn_be_conv_fg(const icnn_be_conv_model *model, const float *ctx, const double *y, int batch,
                    float *f, float *g, const int *finished, void *stream) {
    if (!model || !ctx || !y || !f || !g || batch < 0 || !model->wpack) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::conv_check_model(*model)) return rc;
    if (batch == 0) return 0;
    if (!model->work || model->work_batch < batch) return ICNN_BE_EINVAL;
    return done(icnn_be::launch_conv_fg(*model, ctx, y, batch, f, g, finished, static_cast<hipStream_t>(stream)));
}

size_t icnn_be_conv_context_work_floats(const icnn_be_conv_model *shape, int batch) {
    icnn_be::ConvCtxShape g{};
    if (!shape || batch < 0 || icnn_be::conv_ctx_shape(*shape, g) != 0) return 0;
    return icnn_be::conv_ctx_work_floats(g, batch);
}

int icnn_be_conv_context(const icnn_be_conv_model *shape, const icnn_be_conv_ctx *c, const float *x, int batch, float *ctx,
                         float *work, void *stream) {
    return icnn_be_conv_context_bn(shape, c, nullptr, ICNN_BE_BN_BATCH, 0, x, batch, ctx, work, stream);
}

size_t icnn_be_conv_context_bn_work_floats(const icnn_be_conv_model *shape, int batch) {
    icnn_be::ConvCtxShape g{};
    if (!shape || batch < 0 || icnn_be::conv_ctx_shape(*shape, g) != 0) return 0;
    return icnn_be::conv_ctx_bn_work_floats(g, batch);
}

namespace {
int conv_context_bn(const icnn_be_conv_model *shape, const icnn_be_conv_ctx *c, const icnn_be_bn_moving *mv, int mode,
                    int updates, const int *updates_dev, const float *x, int batch, float *ctx, float *work, void *stream) {
    if (!shape || !c || !x || !ctx || !work || batch < 0) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::conv_ctx_check(*c)) return rc;
    icnn_be::ConvCtxShape g{};
    if (int rc = icnn_be::conv_ctx_shape(*shape, g)) return rc;
    int n[4];
    icnn_be::conv_bn_widths(g, n);
    if (int rc = check_bn_mode(mv, mode, updates_dev ? 1 : updates, n, 4)) return rc;
    if (batch == 0) return 0;
    return done(icnn_be::launch_conv_context(g, *c, x, batch, ctx, work, static_cast<hipStream_t>(stream), mv, mode, updates,
                                             updates_dev));
}
}  // namespace

int icnn_be_conv_context_bn(const icnn_be_conv_model *shape, const icnn_be_conv_ctx *c, const icnn_be_bn_moving *mv, int mode,
                            int updates, const float *x, int batch, float *ctx, float *work, void *stream) {
    return conv_context_bn(shape, c, mv, mode, updates, nullptr, x, batch, ctx, work, stream);
}

int icnn_be_conv_context_bn_dev(const icnn_be_conv_model *shape, const icnn_be_conv_ctx *c, const icnn_be_bn_moving *mv,
                                const int *updates_dev, const float *x, int batch, float *ctx, float *work, void *stream) {
    if (!updates_dev) return ICNN_BE_EINVAL;
    return conv_context_bn(shape, c, mv, ICNN_BE_BN_BATCH, 0, updates_dev, x, batch, ctx, work, stream);
}

int icnn_be_conv_clamp(const icnn_be_conv_model *model, int mode, void *stream) {
    if (!model || !model->wpack || mode < ICNN_BE_CLAMP_ABS || mode > ICNN_BE_CLAMP_ABS_HALF) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::conv_check_model(*model)) return rc;
    return done(icnn_be::launch_conv_clamp(*model, mode, static_cast<hipStream_t>(stream)));
}

int icnn_be_solve_conv(const icnn_be_conv_model *model, const float *ctx, const icnn_be_state *st,
                       float *f_work, float *g_work, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (!model || !ctx || !f_work || !g_work || !model->wpack) return ICNN_BE_EINVAL;
    if (st->cut_dtype != ICNN_BE_CUT_F32 || st->n != model->H * model->W) return ICNN_BE_EINVAL;
    if (st->flags & ICNN_BE_FLAG_F64_ENERGY) return ICNN_BE_EINVAL;
    if (st->batch > 0 && (!model->work || model->work_batch < st->batch)) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::conv_check_model(*model)) return rc;
    if (st->batch == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return solve_generic(*st, f_work, g_work, s, [&] {
        return icnn_be::launch_conv_fg(*model, ctx, st->y, st->batch, f_work, g_work, st->skip_fg, s);
    });
}

/* ---- FICNN (be_ficnn.hip, be_train_ficnn.hip) ---- */
size_t icnn_be_ficnn_pack_floats(const icnn_be_ficnn_model *shape) {
    if (!shape || icnn_be::ficnn_check_model(*shape) != 0) return 0;
    return icnn_be::ficnn_pack_floats(*shape);
}

int icnn_be_ficnn_pack(const icnn_be_ficnn_model *shape, const float *const *w_x_host, const float *const *b_host,
                       const float *const *w_z_host, float *out_host) {
    if (!shape || !w_x_host || !b_host || !w_z_host || !out_host) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ficnn_check_model(*shape)) return rc;
    const int L = shape->n_layers - 1, top = shape->head == ICNN_BE_FICNN_HEAD_LINEAR ? L : L - 1;
    for (int i = 0; i <= top; ++i)
        if (!w_x_host[i] || !b_host[i] || (i > 0 && !w_z_host[i])) return ICNN_BE_EINVAL;
    return icnn_be::ficnn_pack(*shape, w_x_host, b_host, w_z_host, out_host);
}

size_t icnn_be_ficnn_context_work_floats(const icnn_be_ficnn_model *model, int batch) {
    if (!model || batch < 0 || icnn_be::ficnn_check_model(*model) != 0) return 0;
    return icnn_be::ficnn_context_work_floats(*model, batch);
}

int icnn_be_ficnn_context(const icnn_be_ficnn_model *model, const float *x, int batch, float *ctx, float *work, void *stream) {
    if (!model || !x || !ctx || !work || batch < 0 || !model->wpack) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ficnn_check_model(*model)) return rc;
    if (batch == 0) return 0;
    return done(icnn_be::launch_ficnn_context(*model, x, batch, ctx, work, static_cast<hipStream_t>(stream)));
}

int icnn_be_ficnn_fg(const icnn_be_ficnn_model *model, const float *ctx, const double *y, int batch, float *f, float *g,
                     const int *finished, void *stream) {
    if (!model || !ctx || !y || !f || !g || batch < 0 || !model->wpack) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ficnn_check_model(*model)) return rc;
    if (batch == 0) return 0;
    return done(icnn_be::launch_ficnn_fg(*model, ctx, y, batch, f, g, finished, static_cast<hipStream_t>(stream)));
}

int icnn_be_ficnn_gd(const icnn_be_ficnn_model *model, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                     double momentum, double *y_out, double *traj, float *f_out, void *workspace, void *stream) {
    const bool constants_ok = icnn_be::gd_constants_ok(lr, momentum);
    if (int rc = check_gd_args(model, ctx, y0, y_out, workspace, batch, n_iter, constants_ok)) return rc;
    if (int rc = icnn_be::ficnn_check_model(*model)) return rc;
    if (batch == 0) return 0;
    return done(icnn_be::launch_ficnn_gd(*model, ctx, y0, batch, n_iter, lr, momentum, y_out, traj, f_out, workspace,
                                         static_cast<hipStream_t>(stream)));
}

int icnn_be_solve_ficnn(const icnn_be_ficnn_model *model, const float *ctx, const icnn_be_state *st, float *f_work,
                        float *g_work, void *stream) {
    if (int rc = check_state(st)) return rc;
    if (!model || !ctx || !f_work || !g_work || !model->wpack) return ICNN_BE_EINVAL;
    if (st->cut_dtype != ICNN_BE_CUT_F32 || st->n != model->n) return ICNN_BE_EINVAL;
    if (st->flags & ICNN_BE_FLAG_F64_ENERGY) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ficnn_check_model(*model)) return rc;
    if (st->batch == 0) return 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return solve_generic(*st, f_work, g_work, s, [&] {
        return icnn_be::launch_ficnn_fg(*model, ctx, st->y, st->batch, f_work, g_work, st->skip_fg, s);
    });
}

size_t icnn_be_ficnn_grad_floats(const icnn_be_ficnn_model *model) {
    if (!model) return 0;
    return icnn_be::ficnn_grad_floats(*model);
}

size_t icnn_be_ficnn_surrogate_grad_work_floats(const icnn_be_ficnn_model *model, int batch, int rows) {
    if (!model) return 0;
    return icnn_be::ficnn_surrogate_work_floats(*model, batch, rows);
}

int icnn_be_ficnn_surrogate_grad(const icnn_be_ficnn_model *model, const float *x, int batch, const int *row_offset, int rows,
                                 const double *y, const double *v, const double *cvec, float *grad, float *F_rows, float *work,
                                 void *stream) {
    if (!model || !x || !row_offset || !y || !cvec || !grad || !work || !model->wpack) return ICNN_BE_EINVAL;
    if (int rc = icnn_be::ficnn_surrogate_shape(*model, batch, rows, v != nullptr)) return rc;
    return done(icnn_be::launch_ficnn_surrogate_grad(*model, x, batch, row_offset, rows, y, v, cvec, grad, F_rows, work,
                                                     static_cast<hipStream_t>(stream)));
}

}  // extern "C"
