/*
 * icnn_be.h -- C ABI of the MI355X bundle-entropy inference library (libicnn_be.so).
 *
 * The reference (locuslab/icnn) has no FFI: its solver is a Python function
 *   solveBatch(fg, initXs, nIter, callback)   lib/bundle_entropy_dual.py:129-179
 *                                             RL/src/bundle_entropy.py:85-136
 * called from multi-label-cls/icnn_ebundle.py:225, completion/icnn_ebundle.py:226 and
 * RL/src/icnn.py:155, and the energy it minimises is a TensorFlow graph evaluated with
 *   sess.run([E_, dE_dy_])                    multi-label-cls/icnn_ebundle.py:218-221.
 * The entry points below are what a binding for that path would call; every
 * comment cites the reference lines the entry point replaces.  INTEGRATION.md
 * shows the ctypes stub that turns them back into `bundle_entropy.solveBatch`.
 *
 * Conventions
 *   - every data pointer is DEVICE memory unless the name ends in _host;
 *     row-major; caller-allocated; the library never frees or keeps them.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).  All
 *     calls only enqueue work; NONE synchronises or copies to the host, so every
 *     call can be captured into a HIP graph (round 3: the time-sliced solves used
 *     to read a device counter after nIter + 4 rounds; they now enqueue a fixed
 *     number of finishing rounds whose kernels leave at once when nothing is left).
 *   - return value: 0 on success, a negative ICNN_BE_E* code for argument /
 *     launch errors.  Per-sample numerical conditions are reported in
 *     icnn_be_state.status[] (device memory), not in the return value.
 */
#ifndef ICNN_BE_H
#define ICNN_BE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define ICNN_BE_API __attribute__((visibility("default")))
#else
#define ICNN_BE_API
#endif

#define ICNN_BE_ABI_VERSION 12
#define ICNN_BE_MAX_LAYERS 8   /* z-layers of a PICNN including the final scalar one */
#define ICNN_BE_MAX_SLOTS 31   /* bundle slots (= outer iterations) per solve */
#define ICNN_BE_MAX_ITERS 64   /* outer iterations per solve (icnn_be_state.iters; beyond MAX_SLOTS the slots are recycled) */
#define ICNN_BE_MAX_ROUNDS 128 /* launch rounds of one fused solve (scheduling, see icnn_be_solve_fc) */

/* solver variants */
#define ICNN_BE_VARIANT_DUAL 0 /* lib/bundle_entropy_dual.py */
#define ICNN_BE_VARIANT_RL 1   /* RL/src/bundle_entropy.py   */
#define ICNN_BE_VARIANT_PDIPM 2 /* lib/bundle_entropy.py, solver='pc': the per-sample subproblem
                                  min t - H(y) s.t. G y + h <= t by Mehrotra's predictor-corrector
                                  interior-point method (pdipm_pc :5-78); rank test as in DUAL,
                                  multipliers <= 1e-8 pruned (:234-237).  The module the
                                  icnn_ebundle.py scripts import. */

/* dtype of the cuts (f, g) handed to the solver: whatever `fg` returns */
#define ICNN_BE_CUT_F32 0
#define ICNN_BE_CUT_F64 1

/* per-sample status bits */
#define ICNN_BE_ST_OK 0
#define ICNN_BE_ST_SINGULAR 1  /* Newton system exactly singular: the reference raises
                                  numpy.linalg.LinAlgError in variant DUAL (:56-63) and
                                  keeps the current multipliers in variant RL (:55-62);
                                  variant PDIPM: the KKT matrix is not positive definite
                                  (numpy.linalg.cholesky raises, lib/bundle_entropy.py:42) */
#define ICNN_BE_ST_NONFINITE 2 /* a non-finite value reached the bundle */
#define ICNN_BE_ST_OVERFLOW 4  /* the sample's active bundle outgrew what one workgroup can stage in LDS
                                  (icnn_be_bundle_capacity; only wide rows reach it: n = 2048 holds 13 cuts).
                                  The sample stops at its current iterate; the reference has no such limit */

#define ICNN_BE_ST_UNFINISHED 8 /* a fused solve with time-sliced rounds gives the samples that fall behind (parked Newton
                                  solves) nIter finishing rounds instead of asking the device how many are needed -- always
                                  enough: a sample has nIter iterations and a finishing round completes one --; a sample
                                  still behind after them would say so here (safety net of icnn_be_solve_conv) */

/* how icnn_be_solve_fc runs a solve (icnn_be_debug_solve_plan) */
#define ICNN_BE_PATH_ROWS 0                     /* one launch of the persistent per-sample kernel (1-4 samples per workgroup) */
#define ICNN_BE_PATH_TILE 1                     /* one launch of the persistent per-tile kernel (4, 8 or 16 samples) */
#define ICNN_BE_PATH_TILE_BUDGETED_THEN_ROWS 2  /* per-tile kernel with an update budget + one finishing per-sample launch */
#define ICNN_BE_PATH_ROUNDS_LOCKSTEP 3          /* nIter rounds of { icnn_be_fc_fg ; dual step } launches */
#define ICNN_BE_PATH_ROUNDS_SLICED_THEN_ROWS 4  /* nIter time-sliced rounds + one finishing per-sample launch */
#define ICNN_BE_PATH_ROUNDS_SLICED_EXTRA 5      /* nIter time-sliced rounds + nIter unbudgeted rounds for the stragglers */

/* which kernel icnn_be_adam_fc launches (icnn_be_debug_adam_plan) */
#define ICNN_BE_ADAM_NONE 0                     /* none: more workgroups than stay resident, or no layout fits (ICNN_BE_ELIMIT) */
#define ICNN_BE_ADAM_ROWS 1                     /* the latency path: 1-4 states per workgroup, state in LDS and registers */
#define ICNN_BE_ADAM_TILE 2                     /* 16-state MFMA tiles */

/* which kernel icnn_be_dual_step launches (icnn_be_debug_dual_plan, out[5]) */
#define ICNN_BE_DUAL_PLAN_SMALL 0               /* dual_step_small_kernel: n <= 16, variant rl, four samples per wave */
#define ICNN_BE_DUAL_PLAN_BODY 1                /* dual_step_kernel: one workgroup of 1 or 8 waves per sample */
#define ICNN_BE_DUAL_PLAN_WIDE 2                /* dual_step_wide_kernel: eight waves, bundle staged in scratch, oldest rows mirrored in LDS */

/* return codes */
#define ICNN_BE_EINVAL (-1)    /* bad argument */
#define ICNN_BE_ELIMIT (-2)    /* size beyond a compiled-in limit */
#define ICNN_BE_ELAUNCH (-3)   /* HIP launch failed (see icnn_be_last_hip_error) */

/* flags */
#define ICNN_BE_FLAG_NO_CYCLE_SHORTCUT 1 /* always run the full Newton cap (dual :30, rl :29).  Without this flag a Newton
                                          * iteration that has entered a limit cycle of period 1..4 is cut short: exact repeats
                                          * (to 1e-13) return the very iterate the cap would end on; cycles at their rounding
                                          * floor (variant dual, NOISE_TOL in be_dual_dev.h) and extrapolated slow 2-cycles
                                          * return a point of the same cycle that differs from the reference's lam_100 by the
                                          * cycle's own jitter (<= ~2.5e-11 on 10 243 recorded solves).  "The reference's
                                          * sequence of operations, bit for bit" below therefore holds with this flag set;
                                          * the default agrees with it to ~1e-11 in lam (tests/test_gpu_parity.py keeps one
                                          * parity test on each side) */
#define ICNN_BE_FLAG_TIME_SLICE 2        /* fused solve: always park Newton solves that exceed a per-round
                                            budget and resume them in later rounds (icnn_be_solve_fc) */
#define ICNN_BE_FLAG_LOCKSTEP 4          /* fused solve: never do that; exactly nIter rounds, no sync.
                                            Neither flag: time slicing when nIter > 15 (measured) */
#define ICNN_BE_FLAG_TWO_KERNELS 8       /* icnn_be_solve_fc: one launch per phase and round, never a persistent kernel */
#define ICNN_BE_FLAG_PERSISTENT 16       /* icnn_be_solve_fc: the persistent per-tile kernel (a workgroup per 4, 8 or 16
                                          * samples) wherever the shape fits it, whatever the batch size.  Without a flag
                                          * the batch size, nIter and the variant choose the path; icnn_be_debug_solve_plan
                                          * reports which.  Results are bit-identical whichever path runs. */

#define ICNN_BE_FLAG_WAVE_PER_SAMPLE 128  /* narrow rows (n <= 16, variant RL) run four samples per wave by default (one per
                                          * 16-lane DPP row, be_dual_small.hip); this flag keeps the wave-per-sample kernel.
                                          * Same operations in the same order: bit-identical results */
#define ICNN_BE_FLAG_MFMA_CONTRACTION 256  /* variant dual: keep the float64-MFMA sweep for H = A diag(w) A^T, A z instead of the
                                          * fused VALU pass (be_dual_valu_dev.h) that wide rows (several waves per sample)
                                          * take for bundles of up to 20 cuts and -- round 4 -- one-wave samples with float32
                                          * rows of up to 192 columns for bundles of up to 8 cuts.  Same sums in another
                                          * order: results agree to rounding, not bit for bit.  Whichever it is, every
                                          * dispatch path takes the same decision (bit-identical among themselves) */
#define ICNN_BE_FLAG_GLOBAL_BUNDLE 64      /* stage the bundle of EVERY round in st->scratch instead of LDS (diagnostic: the
                                          * rounds whose bundle does not fit LDS do so anyway); same arithmetic, same bits.
                                          * One exception: variant PDIPM on float32 rows of up to 192 columns with 2..12 cuts
                                          * forms its column sums (M = G Hinv G^T, G Hinv ry, G y) by the unrolled VALU
                                          * passes from LDS and by the f64-MFMA sweep / wave reductions from st->scratch
                                          * (another summation order: results agree to ~1e-13, not bit for bit;
                                          * tests/test_gpu_parity.py).  Wider float32 rows take the same column-chunked
                                          * passes from either place (same order, same bits). */
#define ICNN_BE_FLAG_GENERIC_SHAPE 512     /* icnn_be_solve_fc: the persistent tile kernel never takes an instance compiled for one
                                          * network's shape (ICNN_BE_SHAPE_*), always the generic one that reads the shape from
                                          * its arguments.  Same operations in the same order: bit-identical results (the
                                          * identity tests and same-library A/B timings use it) */
#define ICNN_BE_FLAG_NO_ROUND_CLASSES 1024 /* icnn_be_solve_fc (additive to ABI 12): the Bibsonomy instance of the persistent tile
                                          * kernel runs one dual body in every round instead of the body compiled for the
                                          * rounds whose bundles hold at most 8 cuts in rounds 0 .. 7 (be_fused.hip).  Same operations
                                          * in the same order: bit-identical results (identity tests, same-library A/B) */
#define ICNN_BE_FLAG_F64_ENERGY 32        /* icnn_be_dual_step: f is float64 [B] whatever the cut dtype (an `fg` that
                                          * returns float64 energies with float32 gradients: the reference's
                                          * bi = fi - sum(gi * x) keeps fi's precision, dual :143) */

/*
 * Bundle state of one solveBatch call, slot-addressed: the cut taken at outer
 * iteration t lives in slot t; `active[u]` lists, in order, the slots still in
 * sample u's bundle and `lam[u]` their multipliers.  This replaces the ragged
 * Python lists A, b, xs, lam of the reference (dual :131-134) one for one:
 *   A[u][i]  = G[u][active[u][i]]      b[u][i] = h[u][active[u][i]]
 *   xs[u][i] = ys[u][active[u][i]]     lam[u]  = lam[u][0:count[u]]
 */
typedef struct icnn_be_state {
    int batch;          /* B */
    int n;              /* dim(y) */
    int slots;          /* T = nIter of this call, 1..ICNN_BE_MAX_SLOTS */
    int cut_dtype;      /* ICNN_BE_CUT_* : dtype of G (and of f, g passed per step) */
    int variant;        /* ICNN_BE_VARIANT_* */
    int flags;          /* ICNN_BE_FLAG_* */
    double *y;          /* [B][n]    in: start point (initXs); out: minimiser, updated in place */
    void *G;            /* [B][T][n] cut gradients, cut dtype */
    double *h;          /* [B][T]    cut offsets  f - <g, y> */
    double *ys;         /* [B][T][n] points the cuts were taken at */
    double *lam;        /* [B][T]    multipliers of the active slots (after pruning: all > 0) */
    int *active;        /* [B][T]    ordered active slots */
    int *count;         /* [B]       len(active[u]) */
    int *n_iters;       /* [B]       reference `nIters` */
    int *finished;      /* [B]       1 once the sample left the loop (rank test / stall / error) */
    int *status;        /* [B]       ICNN_BE_ST_* bits */
    int *newton_iters;  /* [B]       total Newton updates spent on the sample (diagnostic) */
    /* scheduling state, internal to the library (caller only allocates it) */
    int *t_next;        /* [B]       next outer iteration of the sample */
    int *phase;         /* [B]       0 = needs a cut at y, 1 = Newton solve parked mid-way */
    int *skip_fg;       /* [B]       1 = the sample needs no energy/gradient in the next round */
    int *pending;       /* [ICNN_BE_MAX_ROUNDS] per round: non-zero if any sample still has work afterwards */
    double *park;       /* [B][5*T+4] parked Newton state (lam, four previous iterates, counters) */
    void *scratch;      /* icnn_be_scratch_bytes() bytes or NULL: staging area in device memory for the rounds whose
                           bundle exceeds the LDS capacity (wide rows: n = 2048 stages 12 cuts in LDS); NULL: such a
                           sample stops with ICNN_BE_ST_OVERFLOW */
    double *fvals;      /* [B][T] or NULL: energy f of the cut in each slot as fg returned it (the host replays the reference's
                           callback(t, f, y) of a fused solve from fvals and ys, lib/bundle_entropy_dual.py:144-145) */
    int iters;          /* outer iterations of this call, slots..ICNN_BE_MAX_ITERS; 0 = slots.  More iterations than slots
                           (the reference has no cap on nIter, dual :129): a new cut takes the lowest slot that is not in
                           the sample's active list -- pruned cuts give their slots back --, so only the ACTIVE bundle is
                           limited to `slots` cuts (a sample that would exceed it stops with ICNN_BE_ST_OVERFLOW); slot t
                           is then no longer iteration t, and fvals / ys hold no per-iteration history */
} icnn_be_state;

/*
 * Shape + packed weights of the y-dependent part of a fully-connected PICNN,
 *   z_i = act( (z_{i-1} * gate_i) Wzu_i  +  (y * yu_i) Wyu_i  +  zu_i ),  i = 0..L,
 * multi-label-cls/icnn_ebundle.py:349-388, RL/src/icnn.py:356-404.  width[L] = 1.
 * gate_i, yu_i, zu_i are the x-only "context", one row of `ctx_width` floats per
 * sample laid out per layer as  yu_i[n] | zu_i[width[i]] | gate_i[width[i-1]] (i>0).
 */
typedef struct icnn_be_fc_model {
    int n;                              /* dim(y) */
    int n_layers;                       /* L+1 */
    int width[ICNN_BE_MAX_LAYERS];      /* s_0 .. s_L, s_L == 1 */
    float alpha;                        /* leaky-ReLU slope of the hidden z-layers; 0 = ReLU */
    int action_box;                     /* 1: RL wrapper, network sees 2y-1 and dE/dy is doubled
                                           (RL/src/icnn.py:148-158) */
    int ctx_width;                      /* floats per context row (checked against the shape) */
    int tile_rows;                      /* samples per evaluation tile: 0 or 16 = the 16-row MFMA tile, whose activation
                                           buffers must fit 160 KB of LDS (else ICNN_BE_ELIMIT from every entry); 8 or 4 = a
                                           narrow tile, the LDS sized for that many rows (icnn_be_fc_tile_rows() picks one).
                                           Results do not depend on it bit for bit, the pack neither.  Anything else is
                                           ICNN_BE_EINVAL.  Narrow tiles: fg, solve (per-sample kernel or launch pairs), gd,
                                           pgd, context and the training entries; icnn_be_adam_fc* and
                                           icnn_be_rl_bundle_solve return ICNN_BE_ELIMIT for 8 and 4 */
    const float *wpack;                 /* packed y-path weights, icnn_be_fc_pack_floats() floats */
} icnn_be_fc_model;

/*
 * Shape + packed weights of the y-dependent part of the convolutional PICNN of the image
 * completion experiment (completion/icnn_ebundle.py:376-452): three conv z-layers
 * (reference: 32 k8 s4, 64 k4 s2, 64 k3 s1 on a 64x32x1 image) with the learned down-sampling
 * chain y_red, then fc `fc_hidden` and fc 1.  NHWC, 'SAME' padding.  Context row per sample:
 *   yu_0[H*W] | zu_0 | gate_1 | yu_1 | zu_1 | gate_2 | yu_2 | zu_2 | gate_3[flat] | zu_3 | gate_4 | zu_4[1]
 * (gate_l has the shape of z_{l-1}, yu_l of y_red_l, zu_l of z_l).
 */
typedef struct icnn_be_conv_model {
    int H, W;                /* y (and x) are H x W x 1; n = H*W */
    int filters[3], ksize[3], stride[3];
    int fc_hidden;
    int ctx_width;           /* floats per context row (checked against the shape) */
    const float *wpack;      /* packed y-path weights, icnn_be_conv_pack_floats() floats */
    float *work;             /* device scratch of icnn_be_conv_work_floats(model, work_batch) floats: the activations
                                that cross the four launches of one evaluation (ReLU masks, flatten(z_2), z_3, delta_2) */
    int work_batch;          /* batch the scratch was sized for (>= every batch passed with this model).
                                SINGLE-STREAM: `work` is written by every icnn_be_conv_fg / icnn_be_solve_conv call that names
                                this model although the struct is passed as const -- two calls that share one model struct
                                must be ordered on ONE stream (or use two structs with their own `work` and the same
                                `wpack`); the library does not synchronise them */
} icnn_be_conv_model;

ICNN_BE_API int icnn_be_abi_version(void);
ICNN_BE_API const char *icnn_be_last_hip_error(void);

/* sizeof(icnn_be_state) for which = 0, sizeof(icnn_be_fc_model) for 1, sizeof(icnn_be_fc_ctx) for 2,
 * sizeof(icnn_be_conv_model) for 3, sizeof(icnn_be_conv_ctx) for 4, sizeof(icnn_be_bn_moving) for 5,
 * sizeof(icnn_be_param_update_args) for 6, sizeof(icnn_be_rl_update_args) for 7, sizeof(icnn_be_ficnn_model) for 8, sizeof(icnn_be_replay) for 9,
 * sizeof(icnn_be_dataset) for 10, sizeof(icnn_be_step_log) for 11, 0 for 12, sizeof(icnn_be_ddpg_args) for 13,
 * sizeof(icnn_be_naf_args) for 14, 0 for 15, sizeof(icnn_be_ff_args) for 16, 0 for 17,
 * sizeof(icnn_be_fcn_args) for 18, 0 for 19, sizeof(icnn_be_naf_bn_args) for 20, 0 for 21, sizeof(icnn_be_vec_replay) for 22: lets a foreign-language binding verify its struct layout at load time. */
ICNN_BE_API size_t icnn_be_struct_size(int which);

/* bytes of dynamic LDS one workgroup of the dual-step kernel needs (diagnostic) */
ICNN_BE_API int icnn_be_dual_lds_bytes(int n, int slots, int cut_dtype);

/* Most cuts (the new one included) a sample's ACTIVE bundle may hold at once: min(slots, what fits 160 KB of LDS).
 * The number of outer iterations (slots) is not limited by it -- the reference keeps only the cuts with a positive
 * multiplier from one iteration to the next (dual :171-174) and so does the state; a sample whose active bundle would
 * exceed the capacity gets ICNN_BE_ST_OVERFLOW unless st->scratch is provided (below).  Negative: error code. */
ICNN_BE_API int icnn_be_bundle_capacity(int n, int slots, int cut_dtype, int variant);

/* Bytes of st->scratch that lift the capacity to `slots` cuts (batch, n, slots, cut_dtype, variant of *shape are read):
 * from the round on in which the bundle could outgrow the LDS, the dual step stages it in device memory instead -- same
 * kernel, same arithmetic, the sweeps then run at L2 latency.  0: not needed (everything fits LDS) or not available
 * (the RL variant, whose action vectors are narrow).  */
ICNN_BE_API size_t icnn_be_scratch_bytes(const icnn_be_state *shape);

/* Reset count/finished/status/n_iters/newton_iters for a new solve (dual :130-139). */
ICNN_BE_API int icnn_be_state_init(const icnn_be_state *st, void *stream);

/*
 * One outer bundle iteration t for the whole batch, given the batch's energies
 * f[B] and gradients g[B][n] (cut dtype) at the current st->y: append the cut,
 * rank test, projected-Newton dual solve, y <- sigmoid(-G^T lam), prune.
 * Replaces the body of the reference's `for u in range(bsize)` loop,
 * lib/bundle_entropy_dual.py:143-174 and RL/src/bundle_entropy.py:102-131
 * (proj_newton_logistic :15-85 / :14-83 and logexp1p :6-12 included).
 */
ICNN_BE_API int icnn_be_dual_step(const icnn_be_state *st, int t, const void *f, const void *g, void *stream);

/* Number of floats of the packed weight buffer for a model shape (wpack may be NULL); 0 for a shape the entries refuse.
 * The pack does not depend on shape->tile_rows: same count and contents for 16, 8 and 4. */
ICNN_BE_API size_t icnn_be_fc_pack_floats(const icnn_be_fc_model *shape);

/* The largest evaluation tile of 16, 8 or 4 rows whose activation buffers fit 160 KB of LDS for this shape (n, n_layers,
 * width, ctx_width are read; shape->tile_rows is ignored): the value to store in tile_rows.  ICNN_BE_ELIMIT: not even four
 * rows fit; ICNN_BE_EINVAL: not a network.  Host arithmetic.  The tile needs
 * 4 R (pitch(n) (L + 2) + sum_i pitch(width[i]) + pitch(width[L-1])) bytes, pitch() the LDS row pitch of a width. */
ICNN_BE_API int icnn_be_fc_tile_rows(const icnn_be_fc_model *shape);

/*
 * Pack the y-path weights for the kernels (host -> host; upload the result and
 * store the device pointer in model->wpack).  w_yu_host[i] is 'z{i}_yu/W'
 * [n][width[i]], w_zu_host[i] (i >= 1) is 'z{i}_zu_proj/W' [width[i-1]][width[i]],
 * both row-major float32 as tflearn stores them (icnn_ebundle.py:357-368).
 */
ICNN_BE_API int icnn_be_fc_pack(const icnn_be_fc_model *shape, const float *const *w_yu_host,
                    const float *const *w_zu_host, float *out_host);

/*
 * E[B] and dE/dy[B][n] (float32) of the PICNN at y (float64, rounded to float32
 * on entry like a TensorFlow feed).  Replaces sess.run([E_, dE_dy_]) --
 * multi-label-cls/icnn_ebundle.py:218-221, RL/src/icnn.py:127-131 -- for the
 * y-dependent part; ctx[B][ctx_width] is the x-only part.  Rows whose
 * finished[u] != 0 are skipped (finished may be NULL).
 */
ICNN_BE_API int icnn_be_fc_fg(const icnn_be_fc_model *model, const float *ctx, const double *y, int batch,
                  float *f, float *g, const int *finished, void *stream);

/*
 * The whole solveBatch loop on the device for a PICNN energy: nIter rounds of
 * { icnn_be_fc_fg ; dual step }, enqueued without any host synchronisation.
 *
 * With time slicing (default for nIter > 15, see the flags) the samples do not advance in lockstep: a sample whose Newton
 * solve exceeds a per-round budget (the un-line-searched iteration of the reference falls into
 * limit cycles on ~0.1 % of the solves and then runs its full 100-iteration cap) is parked and
 * resumed in the next round while all other samples move on; every sample still performs exactly
 * the same sequence of operations as in lockstep rounds (bit-identical results between the paths; against the
 * reference see ICNN_BE_FLAG_NO_CYCLE_SHORTCUT).  The samples that are behind after
 * the nIter budgeted rounds are finished without asking the host: by ONE launch of the persistent per-sample
 * kernel (FC models), or by nIter unbudgeted rounds whose kernels leave at once where nothing is left (conv
 * model, ICNN_BE_FLAG_TWO_KERNELS).  For 1024..8192 samples the budgeted rounds themselves are ONE launch of
 * the persistent per-tile kernel (dual phase in LDS groups sized by the cuts the samples hold).  Measured on
 * MI355X at batch 4096, nIter 30: 6.3-6.7 ms (24.7 ms in lockstep launch pairs, 10.3 ms as time-sliced launch
 * pairs); nIter 10: lockstep (the extra rounds cost more than the slicing saves).  Replaces
 * bundle_entropy.solveBatch(fg, y0, nIter) at multi-label-cls/icnn_ebundle.py:225-226
 * with fg = the TensorFlow closure of :218-221.  f_work[B], g_work[B][n] are scratch.
 * The state must have been reset with icnn_be_state_init; st->cut_dtype must be F32.
 * Returns the number of rounds issued (> 0) or a negative error code.
 */
ICNN_BE_API int icnn_be_solve_fc(const icnn_be_fc_model *model, const float *ctx, const icnn_be_state *st,
                     float *f_work, float *g_work, void *stream);

/*
 * icnn_be_solve_fc with the reset of the solve inside it: bit for bit
 *     st->y <- y0 ; icnn_be_state_init(st) ; icnn_be_solve_fc(model, ctx, st, f_work, g_work)
 * where row u of st->y starts from y0[u] (device, [B][n] float64; y0 may be st->y itself: the rows stay) or, with
 * y0 == NULL, from the constant y0_fill.  Where the solve begins with a persistent kernel (ICNN_BE_PATH_ROWS,
 * ICNN_BE_PATH_TILE) the workgroup that owns a sample for the whole solve writes its y row and control words in front of
 * round 0: one launch per solve instead of three and no separate pass over y.  On the other plans the entry enqueues the
 * reset itself in front of the first round.  st->pending is only reset there (nothing else writes it).  Same return
 * values and error codes as icnn_be_solve_fc; no host synchronisation, capturable in a HIP graph.  (Added within ABI 12.)
 */
ICNN_BE_API int icnn_be_solve_fc_reset(const icnn_be_fc_model *model, const float *ctx, const icnn_be_state *st,
                     float *f_work, float *g_work, const double *y0, double y0_fill, void *stream);

/* ---- x-only context producer and weight clamps ------------------------ */

/*
 * Weights of everything that depends on x alone, one column-wise concatenation per stage i = 0 .. n_layers-1
 * (stage i reads prev_i: x for i = 0, the u-path activation u_{i-1} otherwise):
 *   w_stage[i] = [ 'u{i}/W' (i < n_layers-1) | 'z{i}_yu_u/W' | 'z{i}_u/W' | 'z{i}_zu_u/W' (i > 0) ]   row-major
 *                [K_i][ld_i], K_0 = n_features, K_i = width[i-1], ld_i = the column count rounded up to a multiple of 4
 *                (pad columns zero);  b_stage[i] the biases in the same column order.
 * multi-label-cls/icnn_ebundle.py:339-347 (u-path), :354-374 (heads); RL/src/icnn.py:339-385.  Hidden u layers
 * are ReLU'd, and batch-normalised with the statistics of the batch when `batchnorm` (bn_gamma/bn_beta[i], i <
 * n_layers-2, epsilon bn_eps = 1e-5); the last u layer is linear, or ReLU'd (and never normalised) when u_last_relu != 0:
 * the PICNN of synthetic-cls/icnn.py:236-276, which applies the ReLU to every u layer.  The flag is read by the context
 * producers (icnn_be_fc_context*, _stage, _bn, _bn_dev) and by the x-only forward and backward of
 * icnn_be_fc_surrogate_grad*; the y-path never sees it.  icnn_be_adam_fc_obs, whose in-kernel producer keeps the last u layer
 * linear, returns ICNN_BE_EINVAL when it is set.  The field fills what used to be padding in front of the pointer arrays:
 * sizeof is unchanged and a zero-initialised struct is the linear last layer as before.  All pointers device memory.
 */
typedef struct icnn_be_fc_ctx {
    int n_features, n, n_layers;
    int width[ICNN_BE_MAX_LAYERS];      /* as icnn_be_fc_model.width */
    int batchnorm;
    float bn_eps;
    int u_last_relu;                    /* != 0: u_{n_layers-2} = relu(.) instead of linear */
    const float *w_stage[ICNN_BE_MAX_LAYERS];
    const float *b_stage[ICNN_BE_MAX_LAYERS];
    const float *bn_gamma[ICNN_BE_MAX_LAYERS];
    const float *bn_beta[ICNN_BE_MAX_LAYERS];
} icnn_be_fc_ctx;

/* floats of device scratch icnn_be_fc_context needs for a batch (the u-path activations) */
ICNN_BE_API size_t icnn_be_fc_context_work_floats(const icnn_be_fc_ctx *c, int batch);

/*
 * ctx[batch][ctx_width] from x[batch][n_features] (float32): the part of the reference's graph that does not depend
 * on y -- it sits inside `fg`'s sess.run on every bundle iteration there (multi-label-cls/icnn_ebundle.py:218-221)
 * and is computed once per minibatch here.  Row layout as icnn_be_fc_model expects (yu_i | zu_i | gate_i per layer).
 * BatchNorm uses the statistics of exactly these `batch` rows: shard AFTER this call.
 */
ICNN_BE_API int icnn_be_fc_context(const icnn_be_fc_ctx *c, const float *x, int batch, float *ctx, int ctx_width,
                                   float *work, void *stream);

/*
 * The same for DATA-PARALLEL ranks that each hold a shard of the minibatch: the u-path BatchNorm uses the
 * statistics of the GLOBAL batch (tflearn.batch_normalization in training mode, multi-label-cls/icnn_ebundle.py:345), so
 * the producer is issued stage by stage and the ranks all-reduce 2 x width[stage] doubles behind every normalised stage:
 *     for stage in 0 .. n_layers-1:
 *         rc = icnn_be_fc_context_stage(c, stage, x, batch, ctx, ctx_width, work, stats, stream)   // GEMM of the stage
 *         if rc == 1:      // u_stage is batch-normalised: stats[0..w) = sum u, stats[w..2w) = sum u^2 of THIS rank's rows
 *             all_reduce(stats, SUM)                                       // RCCL; 2 x 600 doubles for the Bibsonomy model
 *             icnn_be_fc_context_norm(c, stage, batch, batch_total, stats, work, stream)
 * `x` is this rank's [batch][n_features] rows (read by stage 0 only), `work` as for icnn_be_fc_context (the stages find their
 * inputs in it), `stats` a device buffer of 2 * max(width) doubles.  With one rank (batch_total = batch) the result equals
 * icnn_be_fc_context's up to the float32 rounding of the variance (E[u^2] - mean^2 in float64 here, two passes in float32 there).
 * icnn_be_fc_context_stage returns 1 when statistics were written, 0 when the stage has no BatchNorm, < 0 on error.
 */
ICNN_BE_API int icnn_be_fc_context_stage(const icnn_be_fc_ctx *c, int stage, const float *x, int batch, float *ctx, int ctx_width,
                                         float *work, double *stats, void *stream);
ICNN_BE_API int icnn_be_fc_context_norm(const icnn_be_fc_ctx *c, int stage, int batch, double batch_total, const double *stats,
                                        float *work, void *stream);

/* makeCvx (ICNN_BE_CLAMP_ABS, icnn_ebundle.py:143,:204) / proj (ICNN_BE_CLAMP_RELU, :144,:244-245) on the
 * 'z{i}_zu_proj/W' operands inside model->wpack (both packed orientations), in place on the device. */
#define ICNN_BE_CLAMP_ABS 0
#define ICNN_BE_CLAMP_RELU 1
#define ICNN_BE_CLAMP_ABS_HALF 2    /* |W| / 2: the completion model's makeCvx, completion/icnn_ebundle.py:145 */
ICNN_BE_API int icnn_be_fc_clamp(const icnn_be_fc_model *model, int mode, void *stream);

/*
 * The same for the convolutional PICNN of the completion experiment (completion/icnn_ebundle.py:346-367 u-path with
 * BatchNorm, :376-452 the x-only halves of every layer).  Operands that read the same input through the same window
 * are concatenated column-wise on the host (icnn_amd/picnn.py: ConvModel.repack_context): stage s is a device matrix
 * [K][ld] row-major float32, K = k*k*Cin in tflearn's [k][k][Cin][F] order read as [K][F], ld = columns rounded up to a
 * multiple of 4 (pad columns zero), b_stage[s] the biases in column order:
 *   0  x,  8x8 / 4 :  u0 (F0)            | zu0 = z0_u (F0)
 *   1  x,  3x3 / 1 :  yu0 = z0_yu_u (1)
 *   2  u0, 4x4 / 2 :  u1 (F1)            | zu1 = z1_u (F1)
 *   3  u0, 3x3 / 1 :  gate1 = z1_zu_u (F0) | yu1 = z1_yu_u (1)
 *   4  u1, 3x3 / 1 :  u2 (F2) | gate2 = z2_zu_u (F1) | yu2 = z2_yu_u (1) | zu2 = z2_u (F2)
 *   5  flat u2     :  u3 (fc_hidden)     | gate3 = z3_zu_u (flat) | zu3 = z3_u (fc_hidden)
 *   6  u3          :  gate4 = z4_zu_u (fc_hidden) | zu4 = z4_u (1)
 * u0..u3 are ReLU'd and batch-normalised with the statistics of the batch (bn_gamma/bn_beta[0..3], bn_eps = 1e-5),
 * gates are ReLU'd.  x is [batch][H][W][1] float32 (already h-flipped by the caller, :215); the context row layout is
 * the one icnn_be_conv_fg reads.  Seven GEMM launches (f32 MFMA, implicit im2col) + four BatchNorm launches.
 */
typedef struct icnn_be_conv_ctx {
    const float *w_stage[7];
    const float *b_stage[7];
    const float *bn_gamma[4];
    const float *bn_beta[4];
    float bn_eps;
} icnn_be_conv_ctx;
ICNN_BE_API size_t icnn_be_conv_context_work_floats(const icnn_be_conv_model *shape, int batch);
ICNN_BE_API int icnn_be_conv_context(const icnn_be_conv_model *shape, const icnn_be_conv_ctx *c, const float *x, int batch,
                                     float *ctx, float *work, void *stream);
/* makeCvx (ICNN_BE_CLAMP_ABS_HALF, completion/icnn_ebundle.py:145,:190) / proj (ICNN_BE_CLAMP_RELU, :146,:248-249)
 * on the 'z{1..4}_zu_proj/W' operands inside model->wpack (every packed orientation), in place on the device. */
ICNN_BE_API int icnn_be_conv_clamp(const icnn_be_conv_model *model, int mode, void *stream);

/* ---- BatchNorm moving statistics: inference mode and the folds of training mode (additive to ABI 12) ---- */

/*
 * tflearn.batch_normalization keeps, per batch-normalised u-layer, a moving mean (initialised to 0) and a moving variance
 * (initialised to 1).  In inference mode (tflearn.is_training(False): the completion test phase,
 * completion/icnn_ebundle.py:264-292; the RL agent's act() and target solve, RL/src/icnn.py:277,:316) the layer normalises
 * with them:  u <- (u - mean) gamma / sqrt(var + bn_eps) + beta.  In training mode every evaluation of the op folds the
 * batch mean mu and the biased batch variance sigma^2 it normalised with into them (assign_moving_average without
 * zero-debias, float32, d = 1 - decay):  mean <- mean - (mean - mu) d,  var <- var - (var - sigma^2) d.
 * mean[i] / var[i] are device float32 vectors, one pair per batch-normalised layer: FC u_i for i < n_layers-2 (width[i]
 * floats, NULL elsewhere); conv u0..u2 (filters[l], per channel) and u3 (fc_hidden, per column), indices 0..3.
 */
#define ICNN_BE_BN_BATCH 0     /* normalise with the statistics of the batch (training mode); `updates` folds them */
#define ICNN_BE_BN_MOVING 1    /* normalise with mv (inference mode); nothing is written to mv, valid at batch 1 */
typedef struct icnn_be_bn_moving {
    float *mean[ICNN_BE_MAX_LAYERS];
    float *var[ICNN_BE_MAX_LAYERS];
    float decay;               /* tflearn's default 0.9; in [0, 1] */
} icnn_be_bn_moving;

/* floats of device scratch the *_context_bn entries need (the *_context_work_floats plus the exported batch statistics) */
ICNN_BE_API size_t icnn_be_fc_context_bn_work_floats(const icnn_be_fc_ctx *c, int batch);
ICNN_BE_API size_t icnn_be_conv_context_bn_work_floats(const icnn_be_conv_model *shape, int batch);

/*
 * icnn_be_fc_context / icnn_be_conv_context with the BatchNorm mode chosen:
 *   mode ICNN_BE_BN_BATCH,  updates = 0   the plain call (the same bits; mv is not read)
 *   mode ICNN_BE_BN_BATCH,  updates > 0   the same context, and the batch statistics folded `updates` times into mv (the
 *                                         number of times the reference evaluates the op on this batch)
 *   mode ICNN_BE_BN_MOVING, updates = 0   inference mode: normalise with mv, read only.  Every row is independent of the
 *                                         others (the same bits at any batch size)
 * ICNN_BE_EINVAL before anything is launched for an unknown mode, updates < 0, updates > 0 with ICNN_BE_BN_MOVING, and --
 * when mv is needed (a BatchNorm model with ICNN_BE_BN_MOVING or updates > 0) -- mv == NULL, a NULL vector of a
 * batch-normalised layer or a decay outside [0, 1].  A model without BatchNorm ignores mv.  `work` holds
 * icnn_be_fc_context_bn_work_floats / icnn_be_conv_context_bn_work_floats floats.  No host synchronisation, no atomics.
 */
ICNN_BE_API int icnn_be_fc_context_bn(const icnn_be_fc_ctx *c, const icnn_be_bn_moving *mv, int mode, int updates, const float *x,
                                      int batch, float *ctx, int ctx_width, float *work, void *stream);
ICNN_BE_API int icnn_be_conv_context_bn(const icnn_be_conv_model *shape, const icnn_be_conv_ctx *c, const icnn_be_bn_moving *mv,
                                        int mode, int updates, const float *x, int batch, float *ctx, float *work, void *stream);

/* ---- implicit-differentiation feed of a training step ----------------- */
#define ICNN_BE_LOSS_XENT 0   /* crossEntrGrad, multi-label-cls/icnn_ebundle.py:390-417 */
#define ICNN_BE_LOSS_MSE 1    /* mseGrad,       completion/icnn_ebundle.py:493-522     */

/*
 * From a finished solve: one output row per active cut of every sample with a non-empty bundle,
 *   fd_y[r] = ys_{j,i},  fd_v[r] = lam_i c_y + c_lam,i (y*_j - ys_{j,i}),  fd_c[r] = c_lam,i,  fd_sample[r] = j,
 * rows of sample j starting at row_offset[j] (exclusive prefix sum of st->count, device).  y_true is
 * [B][n] float64.  Replaces train_step_fd (multi-label-cls/icnn_ebundle.py:296-314,
 * completion/icnn_ebundle.py:315-335) including the per-sample (k+1)x(k+1) KKT solve.
 */
ICNN_BE_API int icnn_be_implicit_feed(const icnn_be_state *st, const double *y_true, int loss,
                                      const int *row_offset, double *fd_y, double *fd_v, double *fd_c,
                                      int *fd_sample, void *stream);

/* ---- training step of the FC PICNN: gradient of the surrogate (ABI 12) ------------------------ */

/*
 * Floats of the packed parameter gradient of a model (0: shape rejected; host arithmetic, no GPU needed).  The variables
 * follow one another in this order, each row-major with the reference's [in][out] W shapes (K_0 = n_features,
 * K_i = width[i-1], L = n_layers - 1; the u-path has L layers of widths width[0..L-1]):
 *   for i = 0 .. L-1:  'u{i}/W' [K_i][width[i]], 'u{i}/b' [width[i]],
 *                      'u{i}/bn/gamma', 'u{i}/bn/beta' [width[i]]   (batchnorm and i < L-1 only)
 *   for i = 0 .. L:    'z{i}_zu_u/W' [K_i][width[i-1]], 'z{i}_zu_u/b' [width[i-1]], 'z{i}_zu_proj/W' [width[i-1]][width[i]]
 *                                                                                                   (i > 0 only)
 *                      'z{i}_yu_u/W' [K_i][n], 'z{i}_yu_u/b' [n], 'z{i}_yu/W' [n][width[i]],
 *                      'z{i}_u/W' [K_i][width[i]], 'z{i}_u/b' [width[i]]
 * (the order of tf.trainable_variables() in multi-label-cls/icnn_ebundle.py:316-388, RL/src/icnn.py:325-404;
 * icnn_amd.picnn.init_params returns its keys in the same order).  `c` supplies the x-only weights (stage
 * concatenations, BatchNorm parameters) and must describe the same shape as `model`.
 */
ICNN_BE_API size_t icnn_be_fc_grad_floats(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c);

/* floats of device scratch icnn_be_fc_surrogate_grad needs for `batch` samples and `rows` feed rows (0: rejected) */
ICNN_BE_API size_t icnn_be_fc_surrogate_grad_work_floats(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, int batch,
                                                         int rows);

/*
 * grad = d/dtheta  sum_r [ c_r E(x_s(r), y_r) + <dE/dy(x_s(r), y_r), v_r> ]  over every trainable variable theta,
 * float32, packed as icnn_be_fc_grad_floats describes -- what
 *   F_ = c_ * E_ + reduce_sum(dE_dy_ * v_, 1);  AdamOptimizer.compute_gradients(F_, theta_)
 * evaluates in multi-label-cls/icnn_ebundle.py:148-156 with the feed of train_step_fd (icnn_be_implicit_feed), and, with
 * v = NULL, the gradient of sum_r c_r E_r that the RL critic update needs (RL/src/icnn.py:90-109, c_r = dloss/dQ_r).
 *   x[batch][n_features] float32   the minibatch; the rows of sample j are row_offset[j] .. row_offset[j+1]-1 (int
 *                                  [batch+1], row_offset[0] = 0, row_offset[batch] = rows, non-decreasing: what
 *                                  icnn_be_implicit_feed emits); a sample may have no rows
 *   y, v[rows][n] float64, c[rows] float64   the feed (y rounded to float32 like a TensorFlow feed; action_box models
 *                                  see 2y-1, as icnn_be_fc_fg); v may be NULL
 *   F_rows[rows] float32 or NULL   F_r = c_r E_r + <dE/dy_r, v_r>
 *   work                           icnn_be_fc_surrogate_grad_work_floats(model, c, batch, rows) floats
 * Semantics of icnn_be_fc_fg (ReLU / leaky ReLU alpha, action_box); the u-path BatchNorm runs in training mode over
 * the feed rows (each sample counted once per row, as the reference's x_ = fd_xs), computed on the batch samples with
 * their multiplicities.  Deterministic (no atomics: the same bits on every call), no host synchronisation (capturable in a
 * HIP graph).  ICNN_BE_EINVAL / ICNN_BE_ELIMIT for a bad shape before anything is launched.
 */
ICNN_BE_API int icnn_be_fc_surrogate_grad(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, const float *x, int batch,
                                          const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                          float *grad, float *F_rows, float *work, void *stream);

/* ---- training step of the conv PICNN: gradient of the surrogate (additive to ABI 12) ----------- */

/*
 * Floats of the packed parameter gradient of the completion model (0: shape rejected; host arithmetic, no GPU needed).
 * The variables follow one another in the order of icnn_amd.picnn.init_conv_params (tf.trainable_variables() of
 * completion/icnn_ebundle.py:337-452), each row-major in tflearn's shapes -- [k][k][Cin][F] for a convolution, [in][out]
 * for a dense layer; (k, s, F) = (ksize, stride, filters)[l], Cin_0 = 1, Cin_l = F_{l-1}, flat = the size of flatten(u2),
 * fch = fc_hidden:
 *   for l = 0 .. 2:  'u{l}/W' [k][k][Cin][F], 'u{l}/b' [F], 'u{l}/bn/gamma' [F], 'u{l}/bn/beta' [F],
 *                    'z{l}_zu_u/W' [3][3][Cin][Cin], 'z{l}_zu_u/b' [Cin], 'z{l}_zu_proj/W' [k][k][Cin][F]   (l > 0 only)
 *                    'z{l}_yu_u/W' [3][3][Cin][1], 'z{l}_yu_u/b' [1], 'z{l}_yu/W' [k][k][1][F],
 *                    'z{l}_y_red/W' [k][k][1][1], 'z{l}_y_red/b' [1], 'z{l}_u/W' [k][k][Cin][F], 'z{l}_u/b' [F]
 *   'u3/W' [flat][fch], 'u3/b', 'u3/bn/gamma', 'u3/bn/beta' [fch], 'u4/W' [fch][1], 'u4/b' [1]
 *   'z3_zu_u/W' [flat][flat], 'z3_zu_u/b' [flat], 'z3_zu_proj/W' [flat][fch], 'z3_u/W' [flat][fch], 'z3_u/b' [fch]
 *   'z4_zu_u/W' [fch][fch], 'z4_zu_u/b' [fch], 'z4_zu_proj/W' [fch][1], 'z4_u/W' [fch][1], 'z4_u/b' [1]
 * 'u4/*' (us[4] is never read) and 'z2_y_red/*' (y_red after the last conv layer feeds only the commented-out fc
 * passthrough, :425-434) do not reach E: TensorFlow's compute_gradients returns None for them, their gradient here is 0.
 * `c` supplies the x-only weights (stage concatenations, BatchNorm parameters) of the same model.
 */
ICNN_BE_API size_t icnn_be_conv_grad_floats(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c);

/* floats of device scratch icnn_be_conv_surrogate_grad needs for `batch` samples and `rows` feed rows (0: rejected) */
ICNN_BE_API size_t icnn_be_conv_surrogate_grad_work_floats(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, int batch,
                                                           int rows);

/*
 * grad = d/dtheta  sum_r [ c_r E(x_s(r), y_r) + <dE/dy(x_s(r), y_r), v_r> ]  over every trainable variable theta,
 * float32, packed as icnn_be_conv_grad_floats describes -- what
 *   F_ = c_ * E_ + reduce_sum(dE_dyFlat_ * v_, 1);  AdamOptimizer.compute_gradients(F_, theta_)
 * evaluates in completion/icnn_ebundle.py:129-140 with the feed of train_step_fd (:315-335, icnn_be_implicit_feed with
 * ICNN_BE_LOSS_MSE).
 *   x[batch][H][W][1] float32      the minibatch, already h-flipped (:215); the rows of sample j are row_offset[j] ..
 *                                  row_offset[j+1]-1 (int [batch+1], row_offset[0] = 0, row_offset[batch] = rows,
 *                                  non-decreasing: what icnn_be_implicit_feed emits); a sample may have no rows
 *   y, v[rows][H*W] float64, c[rows] float64   the feed (y rounded to float32 like a TensorFlow feed); v may be NULL
 *   F_rows[rows] float32 or NULL   F_r = c_r E_r + <dE/dy_r, v_r>
 *   work                           icnn_be_conv_surrogate_grad_work_floats(model, c, batch, rows) floats
 * model->work is not used.  The u-path BatchNorm runs in training mode over the feed rows (each sample counted once per
 * row, as the reference's x_ = fd_xs), computed on the batch samples with their multiplicities; icnn_be_conv_context
 * keeps its plain batch statistics.  Deterministic (no atomics: the same bits on every call), no host synchronisation
 * (capturable in a HIP graph).  ICNN_BE_EINVAL / ICNN_BE_ELIMIT for a bad shape (the rule of icnn_be_conv_fg) or a NULL
 * required pointer before anything is launched.
 */
ICNN_BE_API int icnn_be_conv_surrogate_grad(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, const float *x, int batch,
                                            const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                            float *grad, float *F_rows, float *work, void *stream);

/*
 * icnn_be_fc_surrogate_grad / icnn_be_conv_surrogate_grad (mv = NULL, updates = 0) that also fold the BatchNorm statistics
 * of the feed rows -- the multiplicity-weighted statistics the training-mode normalisation used, BatchNorm over the R
 * gathered rows -- `updates` times into mv (icnn_be_bn_moving; 1 for the reference's train_step).  grad and F_rows are the
 * same bits as without the fold.  ICNN_BE_EINVAL for updates < 0 and, on a BatchNorm model with updates > 0, for
 * mv == NULL, a NULL vector or a decay outside [0, 1].  The work sizes are the *_surrogate_grad_work_floats.
 */
ICNN_BE_API int icnn_be_fc_surrogate_grad_bn(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, const float *x, int batch,
                                             const int *row_offset, int rows, const double *y, const double *v,
                                             const double *cvec, float *grad, float *F_rows, float *work,
                                             const icnn_be_bn_moving *mv, int updates, void *stream);
ICNN_BE_API int icnn_be_conv_surrogate_grad_bn(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, const float *x,
                                               int batch, const int *row_offset, int rows, const double *y, const double *v,
                                               const double *cvec, float *grad, float *F_rows, float *work,
                                               const icnn_be_bn_moving *mv, int updates, void *stream);

/* ---- the bundle-entropy training step without the host (be_train_bundle.hip, additive to ABI 12) -- */

/*
 * What the host used to read back between a solve and its training gradient, in one launch of B
 * workgroups from the state of a finished solve and the targets y_true [B][n]:
 *   row_offset [B+1]  exclusive scan of st->count (each count clamped to 0 .. slots); row_offset[B] is the row count
 *   counts [3]        the row count, the number of fg evaluations of the solve (what the reference's solveBatch called fg:
 *                     the outer iteration count while any sample is unfinished, else min(that, max n_iters + 2); variants
 *                     dual and pdipm), and the OR of the B status words
 *   loss_out [1]      ICNN_BE_LOSS_XENT: - sum_{y>0} t log y - sum_{y<1} (1-t) log(1-y) (multi-label-cls/icnn_ebundle.py:
 *                     419-421); ICNN_BE_LOSS_MSE: mean((255 (y - t))^2) (completion/icnn_ebundle.py:476-477).  float64,
 *                     summed per sample and then over the samples in one fixed order: the same bits on every call
 *   tallies [B][3]    cross entropy only, may be NULL: tp, fp, fn of example u over its labels with the prediction
 *                     y >= 0.5 and the truth (int)t != 0 (util.macroF1 averages F1 over the EXAMPLES)
 * work: icnn_be_feed_plan_work_bytes(batch) bytes, 8-byte aligned, ZEROED ONCE by the caller (the kernel re-arms it).
 * batch = 0: nothing is launched.  No host synchronisation.
 */
ICNN_BE_API size_t icnn_be_feed_plan_work_bytes(int batch);
ICNN_BE_API int icnn_be_feed_plan(const icnn_be_state *st, const double *y_true, int loss, int *row_offset, int *counts,
                                  double *loss_out, int *tallies, void *work, void *stream);

/*
 * Padding of a fixed-capacity feed: rows [*rows, row_cap) of fd_y / fd_v [row_cap][n], fd_c / fd_sample [row_cap] become
 * y = 0.5, v = 0, c = 0, sample = batch - 1; rows below *rows (icnn_be_implicit_feed wrote them) are left alone.  row_cap
 * = batch x st->slots holds every feed of a state, since a sample keeps at most `slots` cuts active.
 */
ICNN_BE_API int icnn_be_feed_pad(const int *rows, int batch, int n, int row_cap, double *fd_y, double *fd_v, double *fd_c,
                                 int *fd_sample, void *stream);

/*
 * The skip of a training step on a solver error (completion/icnn_ebundle.py:225-237) as device words,
 * one workgroup.  counts: the [3] int32 of icnn_be_feed_plan (rows, fg evaluations, OR of the status words); mask: the
 * ICNN_BE_ST_* bits that stop a step; gate: [3] int32 in device memory, ZEROED ONCE by the caller:
 *   gate[0]  "go"       1 if (counts[2] & mask) == 0, else 0
 *   gate[1]  "folds"    counts[1] if go, else 0 (the BatchNorm fold count of a step that goes)
 *   gate[2]  "skipped"  a running total: + 1 on every launch that does not go; the kernel never resets it
 * gate[0] is the word icnn_be_param_update_gated and icnn_be_gated_copy take as `go`.  EINVAL for counts or gate NULL before
 * anything is launched.  Vector stores only, no atomics, no host synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API int icnn_be_step_gate(const int *counts, int mask, int *gate, void *stream);

/*
 * icnn_be_fc_surrogate_grad_bn / icnn_be_conv_surrogate_grad_bn over a feed of `rows` = row_cap rows of which only the
 * first *rows_dev (a device int32, = row_offset[batch]) are real: the rest is padding as icnn_be_feed_pad writes it and
 * contributes exactly nothing.  The work size is icnn_be_{fc,conv}_surrogate_grad_dev_work_floats(model, c, batch, rows) --
 * larger than the compact entries' *_work_floats, which do not change: the forward products keep split-K partials for
 * whatever plan the device count asks for.  Every launch and every other split-K plan come from row_cap; the
 * multiplicity-weighted BatchNorm normalises by *rows_dev, so its statistics (and a fold into mv) and F_rows [0, *rows_dev)
 * are the same bits as the compact call's; F_rows beyond are 0.  *rows_dev = 0: a zero gradient, mv unchanged.
 * rows_dev = NULL is the compact entry.
 */
ICNN_BE_API size_t icnn_be_fc_surrogate_grad_dev_work_floats(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, int batch,
                                                            int rows);
ICNN_BE_API size_t icnn_be_conv_surrogate_grad_dev_work_floats(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c,
                                                              int batch, int rows);
ICNN_BE_API int icnn_be_fc_surrogate_grad_dev(const icnn_be_fc_model *model, const icnn_be_fc_ctx *c, const float *x, int batch,
                                              const int *row_offset, int rows, const double *y, const double *v,
                                              const double *cvec, float *grad, float *F_rows, float *work,
                                              const icnn_be_bn_moving *mv, int updates, const int *rows_dev, void *stream);
ICNN_BE_API int icnn_be_conv_surrogate_grad_dev(const icnn_be_conv_model *model, const icnn_be_conv_ctx *c, const float *x,
                                                int batch, const int *row_offset, int rows, const double *y, const double *v,
                                                const double *cvec, float *grad, float *F_rows, float *work,
                                                const icnn_be_bn_moving *mv, int updates, const int *rows_dev, void *stream);

/*
 * icnn_be_fc_context_bn / icnn_be_conv_context_bn in mode ICNN_BE_BN_BATCH whose fold count is read from the device:
 * *updates_dev (int32, clamped to 0 .. ICNN_BE_MAX_ITERS) folds, the same bits as the host count.  work: the
 * *_context_bn_work_floats.
 */
ICNN_BE_API int icnn_be_fc_context_bn_dev(const icnn_be_fc_ctx *c, const icnn_be_bn_moving *mv, const int *updates_dev,
                                          const float *x, int batch, float *ctx, int ctx_width, float *work, void *stream);
ICNN_BE_API int icnn_be_conv_context_bn_dev(const icnn_be_conv_model *shape, const icnn_be_conv_ctx *c,
                                            const icnn_be_bn_moving *mv, const int *updates_dev, const float *x, int batch,
                                            float *ctx, float *work, void *stream);

/* ---- the back-optimisation training step's feed (be_train_gd.hip, additive to ABI 12) ---------- */

/*
 * What lies between icnn_be_fc_gd (trajectory) and icnn_be_fc_surrogate_grad in a back-optimisation training step with the
 * loss mean((y_K - t)^2) over B n (synthetic-cls/icnn.py:117-139, multi-label-cls/icnn-back.py), in ONE launch of B
 * workgroups.  From yK [B][n] (float64 holding float32 values, icnn_be_fc_gd's y_out), the targets t [B][n] (float32) and the
 * step coefficients coef [K] (float64, dy_K / dg_k), per element in float32 and without contraction
 *   d = (float)yK - t;   ybar = (d * 2.0f) * scale        scale = float32(1) / float32(B n), formed by the caller
 * and then
 *   v_rows [B K][n]   v_rows[j K + k][i] = coef[k] * (double)ybar[j][i]          (one float64 product)
 *   c_rows [B K]      0
 *   row_offset [B+1]  row_offset[j] = K j
 *   loss [1]          float32 of ( sum d^2 ) * (1.0 / (B n)): every d * d formed in float64 (exact), summed per sample by a
 *                     fixed tree, the per-sample sums added by the last workgroup to take a ticket (each thread its samples
 *                     in index order, then the same tree), rounded once -- the same bits on every call
 *   f1_tallies [B][3] may be NULL: tp, fp, fn of example j over its labels with the prediction yK >= 0.5 and the truth
 *                     (int)t != 0, the layout of icnn_be_feed_plan's tallies
 * the (y, v, c) rows and row_offset of icnn_be_fc_surrogate_grad with y = the trajectory.  work:
 * icnn_be_gd_feed_work_bytes(B) bytes, 8-byte aligned, ZEROED ONCE by the caller (the kernel re-arms it).  EINVAL for B, n
 * or K < 1 or a NULL pointer other than f1_tallies, ELIMIT when B K exceeds INT_MAX, before anything is launched.  No
 * accumulating atomics, no host synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API size_t icnn_be_gd_feed_work_bytes(int B);
ICNN_BE_API int icnn_be_gd_feed(const double *yK, const float *t, const double *coef, int B, int n, int K, float scale,
                                double *v_rows, double *c_rows, int *row_offset, float *loss, int *f1_tallies, void *work,
                                void *stream);

/*
 * icnn_be_gd_feed for the completion model's back-optimisation loss mean((px (y_K - t))^2) over B n, px = 255
 * (completion/icnn.back.py:149), between icnn_be_conv_gd (trajectory) and icnn_be_conv_surrogate_grad; additive to ABI 12.
 * Per element in float32, every operation rounded, without contraction
 *   d = (float)yK - t;   u = px * d;   ybar = ((u * 2.0f) * scale) * px      scale = float32(1) / float32(B n)
 * the order in which TensorFlow's gradient of reduce_mean(square(255. * (yn - trueY))) multiplies.  Like the rest of the
 * PICNN arithmetic this order is NOT pinned at the TensorFlow boundary (its graph optimiser may reassociate the constants);
 * px cannot be folded into scale without changing the float32 rounding of ybar.  Then
 *   v_rows [B K][n]   v_rows[j K + k][i] = coef[k] * (double)ybar[j][i]          (one float64 product)
 *   c_rows [B K]      0
 *   row_offset [B+1]  row_offset[j] = K j
 *   loss [1]          float32 of ( sum (double)u * (double)u ) * (1.0 / (B n)): every product exact, icnn_be_gd_feed's
 *                     per-sample tree and its fixed order over the per-sample sums; only a ticket is atomic and it re-arms
 *                     itself -- the same bits on every call
 * With px = 1.0f every output is bit-equal to icnn_be_gd_feed's on the same inputs.  The grid is B x S workgroups: a sample's
 * [K][n] block is written as S = ceil(K n / 8192) contiguous chunks of ceil(K n / S) elements (a boundary may fall inside a
 * row), and the first workgroup of a sample alone forms its sum; no output bit depends on S.
 *
 * Loss only (the test phase, icnn.back.py:241-253): v_rows, c_rows and row_offset NULL, all three together; coef may then be
 * NULL too and nothing but loss is written.  work: icnn_be_gd_feed_px_work_bytes(B, n, K) bytes (0 for an argument < 1),
 * 8-byte aligned, ZEROED ONCE by the caller.  EINVAL for B, n or K < 1, for yK, t, loss or work NULL, for one or two of the
 * three row pointers NULL, for coef NULL with rows; ELIMIT when B K exceeds INT_MAX or S exceeds 65535 -- all before anything
 * is launched.  Vector stores only, no accumulating atomics, no host synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API size_t icnn_be_gd_feed_px_work_bytes(int B, int n, int K);
ICNN_BE_API int icnn_be_gd_feed_px(const double *yK, const float *t, const double *coef, int B, int n, int K, float scale,
                                   float px, double *v_rows, double *c_rows, int *row_offset, float *loss, void *work,
                                   void *stream);

/* ---- the epoch level of the training scripts (be_train_epoch.hip, additive to ABI 12) ---- */

/*
 * The loss-only form of icnn_be_gd_feed: the test phase of the FC back-optimisation trainer
 * (multi-label-cls/icnn-back.py:208-216), one launch of B workgroups behind icnn_be_fc_gd.  From yK [B][n] (float64 holding
 * float32 values) and t [B][n] (float32) it writes
 *   loss [1]          float32, the bits icnn_be_gd_feed writes for the same yK, t, B, n: the same float64 products, the same
 *                     per-sample tree, the same fixed order over the per-sample sums (one copy of the device code serves both)
 *   f1_tallies [B][3] may be NULL: the words icnn_be_gd_feed writes
 * and nothing else.  work: icnn_be_gd_eval_work_bytes(B) bytes (0 for B < 1), 8-byte aligned, ZEROED ONCE by the caller (the
 * kernel re-arms its ticket).  EINVAL for B or n < 1 or yK, t, loss or work NULL, before anything is launched.  Vector stores
 * only, no accumulating atomics, no host synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API size_t icnn_be_gd_eval_work_bytes(int B);
ICNN_BE_API int icnn_be_gd_eval(const double *yK, const float *t, int B, int n, float *loss, int *f1_tallies, void *work,
                                void *stream);

/*
 * util.macroF1 of the reference from per-example tallies [B][3] (tp, fp, fn; icnn_be_feed_plan's and icnn_be_gd_feed's
 * layout): f1 [1] (float64, device memory) = the mean over the B examples of 2 tp / (2 tp + fp + fn), 0 where the
 * denominator is 0.  One launch of one workgroup, which loops over B; every quotient is an IEEE float64 division, each
 * thread adds its examples in index order and a fixed tree adds the threads, so every call on the same tallies gives the
 * same bits.  EINVAL for B < 1 or a NULL pointer, before anything is launched.  Vector stores only, no atomics, no host
 * synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API int icnn_be_macro_f1(const int *tallies, int B, double *f1, void *stream);

/*
 * "Keep the model when the score is better" (multi-label-cls/icnn_ebundle.py:274-277, synthetic-cls/icnn.py:206-209) as
 * device words, one workgroup.  score: one float32, or with score_is_f64 != 0 one float64, in device memory; mode:
 * ICNN_BE_KEEP_MIN (smaller is better) or ICNN_BE_KEEP_MAX (larger is better); best: [1] float64 in device memory, which the
 * CALLER initialises; gate: [3] int32 in device memory, ZEROED ONCE by the caller:
 *   gate[0]  "go"      1 if the score is STRICTLY better than *best, else 0; a NaN score is never better
 *   gate[1]  "offers"  a running total: + 1 on every launch
 *   gate[2]  "kept"    a running total: + 1 on every launch that goes
 * and *best = score when it goes.  gate[0] is the word icnn_be_gated_copy takes as `go`: the snapshot of the kept model is
 * icnn_be_gated_copy(snapshot, live, n, gate, 1).  EINVAL for score, best or gate NULL or a mode outside {0, 1}, before
 * anything is launched.  Vector stores only, no atomics, no host synchronisation (capturable in a HIP graph).
 */
#define ICNN_BE_KEEP_MIN 0
#define ICNN_BE_KEEP_MAX 1
ICNN_BE_API int icnn_be_keep_best(const void *score, int score_is_f64, int mode, double *best, int *gate, void *stream);

/* ---- parameter update on the device (be_train_update.hip, additive to ABI 12) ------------------ */

/*
 * One tf.train.AdamOptimizer step over the flat parameter vector theta (the order of the *_surrogate_grad gradient), the
 * reference's proj clamp, and the scatter of every new theta[j] into each copy the kernels read (the weight arena: wpack,
 * the x-only stage operands, BatchNorm gamma / beta).  Per element j, float32, in this order and without contraction:
 *   m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + (1 - beta2) * (g * g);
 *   theta = theta - (lr_t * m) / (sqrt(v) + eps);  theta = 0 if theta < 0 and j lies in a proj range;
 *   arena[dest[k]] = theta  for dest_off[j] <= k < dest_off[j + 1]
 * with beta1, 1 - beta1, beta2, 1 - beta2 (computed in double) and eps rounded to float, and
 *   lr_t = (float)(lr * sqrt(1 - beta2^t) / (1 - beta1^t))   in double, t = step[0] + 1
 * step[0] (updates done) lives in device memory and the launch advances it: the last workgroup to finish (ticket step[1],
 * zero between launches) writes t back.  A captured launch replayed k times is therefore k updates.
 * theta, m, v, grad: 16-byte aligned.  dest[] entries >= arena_floats are skipped.  EINVAL for a NULL pointer, n < 1,
 * a misaligned stream, n_proj outside [0, ICNN_BE_MAX_PROJ_RANGES], a bad range, beta outside [0, 1) or eps <= 0,
 * before anything is launched.  No host synchronisation (capturable in a HIP graph).
 */
#define ICNN_BE_MAX_PROJ_RANGES 8
typedef struct icnn_be_param_update_args {
    long long n;                   /* floats of theta */
    float *theta, *m, *v;          /* [n] float32, updated in place */
    const float *grad;             /* [n] float32 */
    const int *dest_off;           /* [n + 1] CSR offsets into dest */
    const int *dest;               /* arena float offsets */
    float *arena;
    long long arena_floats;
    int *step;                     /* [2] int32: updates done, ticket */
    double lr, beta1, beta2;
    float eps;
    int n_proj;                    /* [proj_begin[i], proj_end[i]) of theta are clamped at 0 */
    long long proj_begin[ICNN_BE_MAX_PROJ_RANGES], proj_end[ICNN_BE_MAX_PROJ_RANGES];
} icnn_be_param_update_args;

ICNN_BE_API int icnn_be_param_update(const icnn_be_param_update_args *a, void *stream);

/*
 * icnn_be_param_update behind one int32 of device memory (icnn_be_step_gate's gate[0]), read once per workgroup.
 * *go != 0: icnn_be_param_update, bit for bit -- theta, m, v, every arena copy, step[0].  *go == 0: nothing is written to
 * theta, m, v or the arena, step[0] stays and the ticket step[1] stays zero, so a later launch is exactly the update it would
 * have been without this one.  *go must not change while the launch runs.  EINVAL for go NULL and for everything
 * icnn_be_param_update refuses, before anything is launched.  No host synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API int icnn_be_param_update_gated(const icnn_be_param_update_args *a, const int *go, void *stream);

/*
 * dst[0, n) = src[0, n) (float32) when (*go != 0) == (want != 0); otherwise dst is left alone.  With want = 0 it puts back
 * what a skipped step must not have changed -- the BatchNorm moving statistics, from a shadow taken before the step's folds.
 * *go is read once per workgroup.  EINVAL for dst, src or go NULL or n < 0; n = 0 launches nothing.  Vector stores only, no
 * host synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API int icnn_be_gated_copy(float *dst, const float *src, long long n, const int *go, int want, void *stream);

/* ---- the RL agent's critic step: TD target, loss, decay, Adam, proj, soft target update (be_rl_train.hip, additive to ABI 12) */

/*
 * The TD part of the critic's training step (RL/src/icnn.py:56-93, FLAGS.icnn_opt == 'adam'), per sample j < batch,
 * float32 in this order and without contraction, with tot(a) = sum_i pen(a_i) summed sequentially in float32 (the
 * entropy term of be_adam.hip, pen from the float32 action):
 *   q  = -(e_critic[j] + tot(act[j]))                                   q_entr at (obs, act)
 *   q2 = -q2_src[j]  when act2 == NULL (q2_src already holds negQ_entr: the inner Adam's f_best),
 *        -(q2_src[j] + tot(act2[j]))  otherwise (q2_src holds the target's negQ at act2)
 *   y  = term[j] ? rew[j] : rew[j] + discount * q2;   y = max(q - 1, y);   y = min(q + 1, y)
 *   td[j] = q - y;   c[j] = (double)(-((1 / batch) * (2 * td[j])))       the weight of E_j in the loss gradient
 * and the loss, in double from float32 inputs, rounded once to float32:
 *   loss = sum_j td_j^2 / batch + l2norm * (wd * sum_{i: decay[i]} theta[i]^2 / 2)
 * decay[i] != 0 marks the elements of theta under the L2 regulariser (the W of every fully connected layer).  The sums
 * have a fixed order for a given batch and n_theta (per-workgroup partials, then the last workgroup by ticket), so the
 * result is bitwise repeatable.  work: ICNN_BE_RL_TD_WORK_BYTES bytes, zero before the first call (the call leaves it
 * re-armed).  EINVAL for batch < 1, n < 1, n_theta < 1, a NULL or misaligned pointer (act, act2, c: 8 bytes; work: 16
 * bytes), a non-finite discount, negative l2norm or wd, a misaligned stream, before anything is launched.  No host
 * synchronisation (capturable in a HIP graph).
 */
#define ICNN_BE_RL_TD_MAX_BLOCKS 256
#define ICNN_BE_RL_TD_WORK_BYTES (8 * ICNN_BE_RL_TD_MAX_BLOCKS + 16)
ICNN_BE_API int icnn_be_rl_td(int batch, int n, const float *e_critic, const double *act, const float *rew,
                              const unsigned char *term, const float *q2_src, const double *act2, float discount,
                              const float *theta, long long n_theta, const unsigned char *decay, float l2norm, float wd,
                              float *td, double *c, float *loss, void *work, void *stream);

/*
 * The critic's weight update and the soft update of the target network in one launch.  Per element j of the flat theta
 * (float32, in this order, without contraction; u = adam):
 *   read theta_old = u.theta[j], theta_t = target_theta[j], m, v, g = u.grad[j]
 *   target_theta[j] = theta_t - tau * (theta_t - theta_old)      (RL/src/icnn.py:104-105, from the critic's theta BEFORE
 *                                                                  this step's Adam update)
 *   g = g + k * theta_old  if decay[j],  k = (float)l2norm * (float)wd rounded to float32   (the L2 regulariser's gradient)
 *   the TF-Adam step and proj of icnn_be_param_update with that g (same rules, same device step counter)
 *   u.arena[dest[d]] = theta,  target_arena[dest[d]] = target_theta[j]   for u.dest_off[j] <= d < u.dest_off[j + 1]
 * The critic and the target share one shape and therefore one map; the target is never projected.  target_theta: 16-byte
 * aligned; decay: 4-byte aligned.  EINVAL for everything icnn_be_param_update refuses, a NULL target_theta /
 * target_arena / decay, a misaligned pointer, tau outside [0, 1], negative l2norm or wd, before anything is launched.  No
 * host synchronisation (capturable in a HIP graph).
 */
typedef struct icnn_be_rl_update_args {
    icnn_be_param_update_args adam;   /* the critic: theta, m, v, grad, the map, its arena, the step counter, Adam */
    float *target_theta;              /* [adam.n] float32, updated in place */
    float *target_arena;              /* the target's arena: adam.arena_floats floats, the same map */
    const unsigned char *decay;       /* [adam.n] nonzero: the element is under the L2 regulariser */
    float tau, l2norm, wd;
} icnn_be_rl_update_args;

ICNN_BE_API int icnn_be_rl_critic_update(const icnn_be_rl_update_args *a, void *stream);

/*
 * The inner optimiser of the RL agent with FLAGS.icnn_opt == 'bundle_entropy' (RL/src/icnn.py:148-158): the bundle-entropy
 * solve of variant RL on an action_box model, with the action and its value out of the same launch.  Bit for bit
 *     icnn_be_solve_fc_reset(model, ctx, st, f_work, g_work, NULL, y0_fill)
 *     act_out[u][j] = 2.0 * st->y[u][j] - 1.0                                   (float64, no contraction)
 *     q_out[u]      = the f[u] of icnn_be_fc_fg(model, ctx, st->y, ...)         (negQ at act_out; q_out may be NULL)
 * in ONE launch of the persistent per-sample kernel: behind the last round every sample of the workgroup -- one that the
 * stall rule finished early included -- is evaluated once more at its float64 st->y.  f_work and g_work are left as the
 * solve leaves them.  A singular system leaves a nonzero status word and the sample keeps its iterate, as everywhere.
 * EINVAL before any launch: a NULL model, ctx, st, f_work, g_work or act_out, model->action_box == 0, st->variant not RL,
 * st->cut_dtype not F32, a non-finite y0_fill, and whatever icnn_be_solve_fc refuses.  ELIMIT: the plan of this model and
 * state is not ICNN_BE_PATH_ROWS (more than four samples per CU, icnn_be_debug_solve_plan); the caller then composes the
 * three steps above.  Returns the rounds like icnn_be_solve_fc (0 for an empty batch).  No host synchronisation,
 * capturable in a HIP graph.  (Added within ABI 12.)
 */
ICNN_BE_API int icnn_be_rl_bundle_solve(const icnn_be_fc_model *model, const float *ctx, const icnn_be_state *st,
                                        float *f_work, float *g_work, double y0_fill, double *act_out, float *q_out,
                                        void *stream);

/* ---- the RL agent's replay memory: enqueue and minibatch sampling (be_rl_replay.hip, additive to ABI 12) ---- */

/*
 * A replay memory of `size` transitions in device memory (RL/src/replay_memory.py).  ctrl: ICNN_BE_REPLAY_CTRL_INTS int32,
 * zero for an empty memory: [0] the cursor i, [1] the fill n, [2] the draw counter, [3] the status word (an OR of
 * ICNN_BE_REPLAY_ST_*), [4] a ticket the sampling kernel re-arms.  They live on the device so that a captured
 * [sample, critic step] reads the current values on every replay; i and n are deterministic (i = enqueues % size,
 * n = min(size - 1, enqueues)), so the host mirrors them without a synchronisation.
 */
#define ICNN_BE_REPLAY_CTRL_INTS 8
#define ICNN_BE_REPLAY_MAX_ATTEMPTS 256
#define ICNN_BE_REPLAY_ST_EXHAUSTED 1     /* a sample spent ICNN_BE_REPLAY_MAX_ATTEMPTS candidates and kept the last one */
#define ICNN_BE_REPLAY_ST_STATE 2         /* the control block held a cursor or a fill outside the arrays */
/* bytes of the staging row of icnn_be_replay_enqueue: action float64 [dimA], observation float32 [dimO], reward float32,
 * terminal uint32 (nonzero: set), in this order */
#define ICNN_BE_REPLAY_STAGE_BYTES(dimO, dimA) (8 * (size_t)(dimA) + 4 * (size_t)(dimO) + 8)
typedef struct icnn_be_replay {
    int size, dimO, dimA;
    float *observations;              /* [size, dimO] */
    float *actions;                   /* [size, dimA]: float32, as the reference stores them */
    float *rewards;                   /* [size] */
    unsigned char *terminals;         /* [size] */
    int *ctrl;                        /* [ICNN_BE_REPLAY_CTRL_INTS] */
} icnn_be_replay;

/*
 * replay_memory.py:27-34: the transition in the device staging row `stage` (layout above, 8-byte aligned) goes to slot i
 * (the float64 action rounded to float32), then i <- (i + 1) % size and n <- min(size - 1, n + 1).  One launch, stream
 * ordered after the copy that filled the row.  EINVAL for a NULL m or stage, size < 3, dimO < 1, dimA < 1, a NULL or
 * misaligned array (4 bytes; stage 8), a misaligned stream, before anything is launched.  No host synchronisation.
 */
ICNN_BE_API int icnn_be_replay_enqueue(const icnn_be_replay *m, const void *stage, void *stream);

/*
 * replay_memory.py:36-55 as written: for each k < batch a candidate uniform on [0, n - 2] is drawn until it is neither
 * the cursor i nor a terminal slot; then obs[k] = observations[idx], act[k] = (double)actions[idx], rew[k] = rewards[idx],
 * ob2[k] = observations[idx + 1], term[k] = terminals[idx + 1] (no wrap handling), idx[k] = idx.  Candidate number
 * `attempt` of sample k in draw d is the high 32 bits of word * (n - 1), word = word 0 of Philox4x32-10 at counter
 * (d, k, attempt, 0) and key (seed low, seed high); d is the device's draw counter, which the launch advances by one.  At
 * most ICNN_BE_REPLAY_MAX_ATTEMPTS candidates per sample: a sample that spends them keeps the last one (in range) and
 * ICNN_BE_REPLAY_ST_EXHAUSTED is ORed into the status word.  fill: the host's mirror of n.  EINVAL for what
 * icnn_be_replay_enqueue refuses in m, batch < 1, fill < 2 or > size - 1, a NULL or misaligned output (act 8 bytes, the
 * others 4, term 1), a misaligned stream, before anything is launched.  No host synchronisation (capturable).
 */
ICNN_BE_API int icnn_be_replay_sample(const icnn_be_replay *m, int fill, int batch, unsigned long long seed, float *obs,
                                      double *act, float *rew, float *ob2, unsigned char *term, int *idx, void *stream);

/* ---- E environments a step: the vector replay memory and the exploration noise (be_rl_replay.hip, additive to ABI 12) ---- */

/*
 * The replay memory of n_envs environments that step in lockstep: `steps` time rows of n_envs transitions each, so every one
 * of the n_envs columns is the memory of RL/src/replay_memory.py.  ctrl as in icnn_be_replay; the cursor and the fill count
 * time rows.  steps * n_envs must fit an int (ICNN_BE_ELIMIT).
 */
typedef struct icnn_be_vec_replay {
    int steps, n_envs, dimO, dimA;
    float *observations;              /* [steps][n_envs][dimO] */
    float *actions;                   /* [steps][n_envs][dimA]: float32 */
    float *rewards;                   /* [steps][n_envs] */
    unsigned char *terminals;         /* [steps][n_envs] */
    int *ctrl;                        /* [ICNN_BE_REPLAY_CTRL_INTS] */
} icnn_be_vec_replay;

/*
 * One launch writes time row i for every environment from DEVICE buffers -- obs float32 [n_envs][dimO], act float64
 * [n_envs][dimA] (rounded to float32), rew float32 [n_envs], term uint8 [n_envs] (nonzero: set) -- then i <- (i + 1) % steps and
 * n <- min(steps - 1, n + 1), as replay_memory.py:33-34.  EINVAL for a NULL m, steps < 3, n_envs, dimO or dimA < 1, a NULL or
 * misaligned pointer (act 8 bytes, obs and rew 4), a misaligned stream.  No host data, no synchronisation: capturable.
 */
ICNN_BE_API int icnn_be_vec_replay_enqueue(const icnn_be_vec_replay *m, const float *obs, const double *act, const float *rew,
                                           const unsigned char *term, void *stream);

/*
 * icnn_be_replay_sample's rule per column.  For sample k, attempt a, draw d: the time index c = hi32(w0 * (n - 1)), w0 = word
 * 0 of Philox4x32-10 at counter (d, k, a, 0), and the environment e = hi32(w2 * n_envs), w2 = word 0 at counter (d, k, a, 2),
 * key (seed low, seed high).  The draw is valid when c is not the cursor and terminals[c][e] == 0.  Outputs from (c, e) and its
 * successor (c + 1, e) -- two rows n_envs * dimO floats apart; idx[k] = c * n_envs + e.  Attempt bound, status words, ticket
 * and draw counter as icnn_be_replay_sample; with n_envs = 1 every output and the control block equal that entry's on the same
 * transitions.  Refusals as there (fill: the host's mirror of n, 2 <= fill <= steps - 1).  Capturable.
 */
ICNN_BE_API int icnn_be_vec_replay_sample(const icnn_be_vec_replay *m, int fill, int batch, unsigned long long seed, float *obs,
                                          double *act, float *rew, float *ob2, unsigned char *term, int *idx, void *stream);

/*
 * The Ornstein-Uhlenbeck exploration of n_envs actions in one launch (RL/src/icnn.py:276-283 per environment).  raw: the
 * optimiser's or the policy's output [n_envs][dimA], float64, or float32 with raw_f32 != 0.  test == 0:
 *     noise <- noise - (theta * noise - sigma * z)     float64, no contraction
 *     action = min(max(raw + noise, -1), 1)
 * and the step counter *counter (device int32) advances by one, so a captured launch draws fresh numbers on every replay.
 * test != 0: action = min(max(raw, -1), 1); noise and counter are left alone.  z is the project's own stream (not
 * np.random.randn's): with (w0, w1, w2, w3) = Philox4x32-10 at counter (step, e, j, 3) and key (seed low, seed high),
 *     u1 = (((w1 << 32 | w0) >> 11) + 1) * 2^-53  in (0, 1],   u2 = ((w3 << 32 | w2) >> 11) * 2^-53  in [0, 1),
 *     z  = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2)      all float64.
 * noise float64 [n_envs][dimA], action float64 [n_envs][dimA] (may be raw).  EINVAL for n_envs or dimA < 1, a NULL or
 * misaligned pointer, a NaN theta or sigma; ICNN_BE_ELIMIT where n_envs * dimA does not fit an int.  No host synchronisation.
 */
ICNN_BE_API int icnn_be_explore(int n_envs, int dimA, const void *raw, int raw_f32, double *noise, int *counter, double theta,
                                double sigma, unsigned long long seed, int test, double *action, void *stream);

/* ---- the training set on the device: minibatch draw and step log (be_train_data.hip, additive to ABI 12) ---- */

/*
 * A training set of n_rows examples in device memory, as up to ICNN_BE_DATASET_MAX_ARRAYS arrays that share their first
 * dimension (trainX, trainY of multi-label-cls/icnn_ebundle.py:214, icnn-back.py:190, completion/icnn_ebundle.py:210,
 * icnn.back.py:216).  Array a has n_rows rows of row_words[a] 4-byte words: the draw copies words and knows no element type
 * (a float64 row of n values is 2 n words).  ctrl: ICNN_BE_DATASET_CTRL_INTS int32, zero for a fresh set: [0] the draw
 * counter, [1] the status word (an OR of ICNN_BE_DATASET_ST_*), [2] a ticket the draw re-arms, the rest reserved (zero).
 * They live on the device so that a captured draw reads the current counter on every replay.
 */
#define ICNN_BE_DATASET_MAX_ARRAYS 4
#define ICNN_BE_DATASET_CTRL_INTS 8
#define ICNN_BE_DATASET_ST_STATE 1        /* a launch found the ticket outside its grid: two draws of one set ran at once */
typedef struct icnn_be_dataset {
    int n_rows;                                        /* N >= 1 */
    int n_arrays;                                      /* 1 .. ICNN_BE_DATASET_MAX_ARRAYS */
    const void *src[ICNN_BE_DATASET_MAX_ARRAYS];       /* [n_rows][row_words[a]] words, 16-byte aligned */
    int row_words[ICNN_BE_DATASET_MAX_ARRAYS];         /* >= 1 */
    int *ctrl;                                         /* [ICNN_BE_DATASET_CTRL_INTS] */
} icnn_be_dataset;

/*
 * `I = npr.randint(nTrain, size=batch); trainX[I], trainY[I]` in one launch: for k < batch
 *   idx[k] = (word * N) >> 32,  word = word 0 of Philox4x32-10 at counter (draws, k, 0, 1) and key (seed low, seed high)
 * -- the map of icnn_be_replay_sample with the domain tag 1 in counter word 3, so that a training set and a replay memory
 * at one seed do not share a stream -- and row idx[k] of array a is copied bit for bit to row k of dst[a], for every array.
 * Rows are drawn independently, with replacement.  Every index has probability floor(2^32 / N) or ceil(2^32 / N) over
 * 2^32: a relative spread of at most N / 2^32.  draws is the device's draw counter, which the launch advances by one (the
 * last workgroup to take the ticket does, and re-arms the ticket): a captured launch replayed r times is r different
 * minibatches.  dst[a]: [batch][row_words[a]] words; idx: int32 [batch], never NULL.  One workgroup per sample; rows of
 * row_words % 4 == 0 move as 16-byte words, others word by word.  EINVAL for a NULL d, ctrl, idx, dst or any src / dst[a],
 * n_rows < 1, batch < 1, n_arrays outside [1, ICNN_BE_DATASET_MAX_ARRAYS], row_words < 1, a src, dst[a] or idx that is not
 * 16-byte aligned, a ctrl that is not 4-byte aligned, a misaligned stream, before anything is launched.  Vector stores
 * only, no accumulating atomics beyond the ticket, no host synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API int icnn_be_dataset_draw(const icnn_be_dataset *d, int batch, unsigned long long seed, void *const dst[], int *idx,
                                     void *stream);

/*
 * A ring of per-step scalars in device memory (what the scripts write to train.csv every iteration): rows float64
 * [cap][width]; ctrl int32 [ICNN_BE_LOG_CTRL_INTS], zero for an empty log, [0] the cursor = rows appended so far.  Column j is
 * one scalar in device memory, col[j], of kind[j] (ICNN_BE_LOG_F32 / _F64 / _I32).
 */
#define ICNN_BE_LOG_MAX_COLUMNS 8
#define ICNN_BE_LOG_CTRL_INTS 4
#define ICNN_BE_LOG_F32 0
#define ICNN_BE_LOG_F64 1
#define ICNN_BE_LOG_I32 2
typedef struct icnn_be_step_log {
    double *rows;                                      /* [cap][width], 8-byte aligned */
    int *ctrl;                                         /* [ICNN_BE_LOG_CTRL_INTS] */
    int cap;                                           /* >= 1 */
    int width;                                         /* 1 .. ICNN_BE_LOG_MAX_COLUMNS */
    const void *col[ICNN_BE_LOG_MAX_COLUMNS];
    int kind[ICNN_BE_LOG_MAX_COLUMNS];
} icnn_be_step_log;

/*
 * rows[cursor % cap][j] = (double)*col[j] for j < width (exact for all three kinds), then cursor <- cursor + 1.  One wave.
 * EINVAL for a NULL L, rows, ctrl or col[j], cap < 1, width outside [1, ICNN_BE_LOG_MAX_COLUMNS], an unknown kind, rows
 * not 8-byte aligned (ctrl and the columns: the alignment of their type), a misaligned stream, before anything is launched.
 * Vector stores only, no atomics, no host synchronisation (capturable in a HIP graph).
 */
ICNN_BE_API int icnn_be_log_row(const icnn_be_step_log *L, void *stream);

/* ---- the reference's return value (SURVEY.md 8(b) "Return / ownership") ------------------------ */

/*
 * From a finished solve: the ACTIVE cuts of every sample packed row by row, sample by sample in bundle order --
 *   G_rows[r] = G[u][active[u][i]] (cut dtype, n values),  ys_rows[r] = ys[u][active[u][i]],
 *   h_rows[r] = h[u][active[u][i]],  lam_rows[r] = lam[u][i]        r = row_offset[u] + i,  i < count[u]
 * (row_offset = exclusive prefix sum of st->count, device; the buffers hold sum(count) rows).  These are the ragged
 * Python lists A, xs, b, lam that solveBatch returns (lib/bundle_entropy_dual.py:131-134, :171-179), ready for ONE
 * device-to-host copy: what an unmodified multi-label-cls/icnn_ebundle.py:225-226 / :296-314 consumes.
 */
ICNN_BE_API int icnn_be_export_active(const icnn_be_state *st, const int *row_offset, void *G_rows, double *ys_rows,
                                      double *h_rows, double *lam_rows, void *stream);

/* ---- Adam inner optimiser of the RL agent ---------------------------- */

/* bytes of device scratch icnn_be_adam_fc needs for a batch (iterate, moments, per-iteration f and g, barrier) */
ICNN_BE_API size_t icnn_be_adam_workspace_bytes(int batch, int n);

/*
 * `Agent.adam(func, obs)` of RL/src/icnn.py:160-215 with func = `_fg_entr` (:59-63, :131; what act() and train()
 * pass, :270-272, :306-317): projected Adam on  negQ(obs, act) - H((act+1)/2)  over act in [-1+1e-8, 1-1e-8]^n from
 * act = 0 (b1 0.9, b2 0.999, alpha 0.01, eps 1e-8, step m_hat / (sqrt(v) + eps) with the UNcorrected v exactly as
 * :201 has it), best iterate per state, stop when the smoothed mean displacement of the best iterates is below
 * 1e-3 after more than 5 iterations (:184-192), else after max_iter (reference: 1000) evaluations.
 * model: the negQ PICNN with action_box = 0 (the action is fed as is); ctx[B][ctx_width] its x-only context.
 * Out (device): act_best[B][n] float64, f_best[B] float32 (negQ_entr at act_best), *iters = evaluations before the
 * rule fired (what the reference prints), max_iter if it never did.  One kernel launch, no host synchronisation.
 * The stopping rule couples the whole batch, so all ceil(B/16) workgroups must be resident at once: returns
 * ICNN_BE_ELIMIT beyond that (MI355X: one 1024-thread workgroup per CU, 256 CUs = 4096 states).  Up to 1024 states
 * (dim(action) <= 64) run with 1-4 states per CU on the VALU latency path, larger batches as 16-state MFMA tiles.
 */
ICNN_BE_API int icnn_be_adam_fc(const icnn_be_fc_model *model, const float *ctx, int batch, int max_iter,
                                double *act_best, float *f_best, int *iters, void *workspace, void *stream);

/*
 * icnn_be_adam_fc with the stopping rule applied to every state on its own (additive to ABI 12): row u of act_best, f_best and
 * iters[B] is, bit for bit, what icnn_be_adam_fc returns for the batch that consists of row u alone -- the smoothed
 * displacement is the state's own, a state whose rule has fired keeps its best iterate and takes no further step, and
 * iters[u] is the iteration at which its rule fired (max_iter if it never did).  What a vector of environments needs: an
 * action that does not depend on the other environments' observations.  Same arguments and the same refusals otherwise;
 * `workspace` as icnn_be_adam_workspace_bytes says.  One ordinary launch: no workgroup waits for another, so any batch runs
 * and there is no residency limit (ICNN_BE_ELIMIT only where no layout fits the LDS).  dim(action) <= 64 and at most four
 * states per resident workgroup: the latency path; 16-state MFMA tiles otherwise (icnn_be_debug_adam_each_plan).
 */
ICNN_BE_API int icnn_be_adam_fc_each(const icnn_be_fc_model *model, const float *ctx, int batch, int max_iter,
                                     double *act_best, float *f_best, int *iters, void *workspace, void *stream);

/*
 * The same from the observations themselves: obs[B][n_features] -> the x-only context rows (cx: the stage weights of
 * icnn_be_fc_context) -> the Adam loop, ONE launch: what `act()` does per environment step (RL/src/icnn.py:264-288).
 * Latency path only -- at most four states per workgroup (MI355X: B <= 1024), dim(action) <= 64, a model without
 * BatchNorm (the agent's default icnn_bn=False, RL/src/agent.py:23) -- otherwise ICNN_BE_ELIMIT: call
 * icnn_be_fc_context, then icnn_be_adam_fc.
 */
ICNN_BE_API int icnn_be_adam_fc_obs(const icnn_be_fc_model *model, const icnn_be_fc_ctx *cx, const float *obs, int batch,
                                    int max_iter, double *act_best, float *f_best, int *iters, void *workspace,
                                    void *stream);

/* ---- unrolled momentum gradient descent on y: back-optimisation inference (be_gd.hip, additive to ABI 12) ---- */

/* bytes of device scratch icnn_be_fc_gd / icnn_be_conv_gd need for `batch` samples of dim(y) = n (0: bad arguments) */
ICNN_BE_API size_t icnn_be_gd_workspace_bytes(int batch, int n);

/*
 * n_iter steps of momentum gradient descent on y inside the graph, as multi-label-cls/icnn-back.py:120-133 and
 * completion/icnn.back.py:136-147 build them: from v_0 = 0, for k = 0 .. n_iter-1
 *     g_k = dE/dy(x, y_k),  v_{k+1} = mu v_k - lr g_k,  y_{k+1} = (y_k - mu v_k) + (1+mu) v_{k+1}
 * in float32 (every operation rounded, no contraction; constants float32(lr), float32(mu), float32(1.0 + mu) with the sum
 * formed in double), no clipping to the box.  y0[B][n]: float64 holding float32 values, rounded on entry like a feed (may
 * alias y_out).  Out (device): y_out[B][n] = y_K (float64 holding float32 values); traj (may be NULL) [B][n_iter][n] =
 * y_0 .. y_{n_iter-1} -- the row layout of icnn_be_*_surrogate_grad with row_offset[j] = n_iter j; f_out (may be NULL)
 * [B] float32 = E(y_K) from one more evaluation.  E and dE/dy are evaluated with the operations of icnn_be_fc_fg /
 * icnn_be_conv_fg, so the result is bit-identical to a loop of those calls plus the float32 update.  Samples are
 * independent: every batch size runs.  FC: one launch; conv: 1 + n_iter (+1) rounds of launches (the model's `work` must
 * hold `batch`, SINGLE-STREAM as for icnn_be_conv_fg).  Enqueued on `stream`, no host synchronisation (capturable).
 * ICNN_BE_EINVAL before any launch for n_iter < 1, batch < 0, a non-finite lr / momentum (or float32 constant), a NULL
 * model, ctx, y0, y_out or workspace, an action_box model, or a shape the fg entries reject; ICNN_BE_ELIMIT for a model
 * whose evaluation does not fit the LDS.
 */
ICNN_BE_API int icnn_be_fc_gd(const icnn_be_fc_model *model, const float *ctx, const double *y0, int batch, int n_iter,
                              double lr, double momentum, double *y_out, double *traj, float *f_out, void *workspace,
                              void *stream);
ICNN_BE_API int icnn_be_conv_gd(const icnn_be_conv_model *model, const float *ctx, const double *y0, int batch, int n_iter,
                                double lr, double momentum, double *y_out, double *traj, float *f_out, void *workspace,
                                void *stream);

/* ---- projected gradient descent on E - H(y), objective traces, the bundle's lower bound (be_pgd.hip, additive to ABI 12) ---- */

/* bytes of device scratch icnn_be_fc_pgd / icnn_be_conv_pgd need for `batch` samples of dim(y) = n (0: bad arguments) */
ICNN_BE_API size_t icnn_be_pgd_workspace_bytes(int batch, int n);

/*
 * n_iter iterations of projected gradient descent on the entropy-scaled objective E(x, y) - H(y), H(y) = -sum_j [y_j log y_j
 * + (1 - y_j) log(1 - y_j)]: what multi-label-cls/ebundle-vs-gd.py:110-132 and completion/ebundle-iter.py:115-139 run through
 * bamos_opt.pgd.solve_batch with minIter == maxIter.  That module is not part of the reference tree: the iteration is
 * defined HERE (parity unpinned), and its stopping rule, which those scripts switch off, is not built.  From
 * y_0 = clip(y0, lo, hi) (the scripts start inside the box; it keeps the logarithms finite), for k = 0 .. n_iter-1
 *     yf      = float64(float32(y_k))                          what the float32 energy is fed
 *     E, g    = the float32 energy and dE/dy at yf, by the operations of icnn_be_fc_fg / icnn_be_conv_fg
 *     e_k     = float64(E) + sum_j [yf log yf + (1 - yf) log(1 - yf)]      float64; a NaN term counts 0 (the scripts' entr())
 *     G_k     = (float64(g) + log yf) - log(1 - yf)
 *     y_{k+1} = min(max(y_k - lr G_k, lo), hi)                 float64, every operation rounded, no contraction
 * The scripts' box is lo = 1e-6, hi = 1 - 1e-6.  y0 [B][n] float64 (may alias y_out).  Out (device): y_out [B][n] = y_K;
 * obj (may be NULL) [n_iter][B] = e_k, what the scripts' callback sees before the update; obj_final (may be NULL) [B] = e_K
 * from one more evaluation.  Samples are independent and a sample's e_k does not depend on its batch.  FC: one launch;
 * conv: 1 + 5 n_iter (+5) launches (the model's `work` must hold `batch`, SINGLE-STREAM as for icnn_be_conv_fg).  Enqueued
 * on `stream`, no host synchronisation (capturable).  ICNN_BE_EINVAL before any launch for n_iter < 1, batch < 0, a
 * non-finite lr, a box that violates 0 < float32(lo), float32(hi) < 1, lo < hi, a NULL model, ctx, y0, y_out or workspace,
 * an action_box model, or a shape the fg entries reject; ICNN_BE_ELIMIT for a model whose evaluation does not fit the LDS.
 */
ICNN_BE_API int icnn_be_fc_pgd(const icnn_be_fc_model *model, const float *ctx, const double *y0, int batch, int n_iter,
                               double lr, double lo, double hi, double *y_out, double *obj, double *obj_final,
                               void *workspace, void *stream);
ICNN_BE_API int icnn_be_conv_pgd(const icnn_be_conv_model *model, const float *ctx, const double *y0, int batch, int n_iter,
                                 double lr, double lo, double hi, double *y_out, double *obj, double *obj_final,
                                 void *workspace, void *stream);

/* out[u] = float64(E[u]) - H(y[u]) for E [B] float32 and y [B][n] float64 (not rounded), the entropy summed in float64 with
 * the scripts' convention: an element whose term is NaN (0 log 0 at y = 0 and y = 1, any y outside [0, 1]) counts 0. */
ICNN_BE_API int icnn_be_entropy_objective(const float *E, const double *y, int batch, int n, double *out, void *stream);

/*
 * The entropy-scaled objective per outer iteration of a finished fused solve, variants DUAL and PDIPM: what a
 * callback(t, f, x) that records f - entr(x) would have seen (lib/bundle_entropy_dual.py:144-145), from st->fvals, st->ys,
 * st->t_next, st->finished and st->y alone.  obj [st->slots][B] (device): obj[t][u] = f_t(u) - H(x_t(u)), where a sample that
 * has left the loop keeps its iterate and its last energy and a sample that stopped on its own cut (rank test) is read from
 * slot t_next.  calls (device int32): the number of callback invocations -- st->slots, or 1 + the iteration in which the
 * last sample finished --; rows t >= *calls are NaN.  ICNN_BE_EINVAL for variant RL (its callback has no x, and its stall
 * rule needs one more evaluation) or a state without fvals; ICNN_BE_ELIMIT when st->iters != 0 (recycled slots hold no
 * per-iteration history).
 */
ICNN_BE_API int icnn_be_bundle_trace(const icnn_be_state *st, double *obj, int *calls, void *stream);

/*
 * The bundle's lower bound of min_y E(y) - H(y): with lam the multipliers of sample u's active cuts (g_i, h_i) and
 * a = sum_i lam_i g_i,  out[u] = sum_i lam_i h_i - sum_j log(1 + exp(-a_j))  in float64 -- every cut under-estimates the convex
 * E, so for lam on the simplex  min_y E - H >= min_y <a, y> + lam . h - H(y), whose minimum is that value.  float32 and
 * float64 cuts; a sample without a cut gives -inf.
 */
ICNN_BE_API int icnn_be_dual_bound(const icnn_be_state *st, double *out, void *stream);

/* ---- fully input-convex network, FICNN (synthetic-cls/icnn.py; be_ficnn.hip, be_train_ficnn.hip, additive to ABI 12) --- */

#define ICNN_BE_FICNN_HEAD_SUM 0     /* the reference's f_ficnn: E = sum_k z_{L-1,k} (its last layer never reassigns z) */
#define ICNN_BE_FICNN_HEAD_LINEAR 1  /* the paper's FICNN: E = a_L, a linear scalar layer */

/*
 * Shape + packed weights of a FICNN (synthetic-cls/icnn.py:213-234, f_ficnn) with xy = concat(x, y):
 *   a_i = xy W_x_i + b_i  (+ z_{i-1} W_z_i for i > 0, no bias),   z_i = relu(a_i)   for i = 0 .. L-1,
 * E = sum_k z_{L-1,k} (head SUM) or E = a_L (head LINEAR), width[L] = 1.  W_x_i is 'z_x{i}/W' [n_features + n][width[i]]
 * (x rows first), b_i 'z_x{i}/b', W_z_i 'z_z{i}_proj/W' [width[i-1]][width[i]].  The x-only context row of a sample is
 *   c_0[width[0]] | c_1[width[1]] | ... ,  c_i = x W_x_i[:n_features] + b_i,
 * over the layers the head evaluates: i < L (SUM) or i <= L (LINEAR); ctx_width is its length.
 */
typedef struct icnn_be_ficnn_model {
    int n_features;                     /* dim(x) */
    int n;                              /* dim(y) */
    int n_layers;                       /* L+1: the hidden layers and the scalar head layer (2 .. ICNN_BE_MAX_LAYERS) */
    int width[ICNN_BE_MAX_LAYERS];      /* s_0 .. s_L, s_L == 1 */
    int head;                           /* ICNN_BE_FICNN_HEAD_* */
    int ctx_width;                      /* floats per context row (checked against the shape) */
    const float *wpack;                 /* packed weights, icnn_be_ficnn_pack_floats() floats */
} icnn_be_ficnn_model;

/* Number of floats of the packed weight buffer (0 if the shape is rejected: layer count, widths, head, ctx_width, or an
 * evaluation tile that does not fit the LDS).  Host arithmetic. */
ICNN_BE_API size_t icnn_be_ficnn_pack_floats(const icnn_be_ficnn_model *shape);

/*
 * Pack every weight the FICNN kernels read (host -> host; upload the result and store the device pointer in
 * model->wpack): w_x_host[i] = 'z_x{i}/W' [n_features + n][width[i]], b_host[i] = 'z_x{i}/b' [width[i]], w_z_host[i]
 * (i >= 1) = 'z_z{i}_proj/W' [width[i-1]][width[i]], row-major float32 as tflearn stores them.  The head layer's
 * pointers (i = L) are read only for head LINEAR and may be NULL for head SUM.  Every packed float is a copy of one
 * parameter element or zero (padding).
 */
ICNN_BE_API int icnn_be_ficnn_pack(const icnn_be_ficnn_model *shape, const float *const *w_x_host, const float *const *b_host,
                                   const float *const *w_z_host, float *out_host);

/* floats of device scratch icnn_be_ficnn_context needs for a batch (0: rejected) */
ICNN_BE_API size_t icnn_be_ficnn_context_work_floats(const icnn_be_ficnn_model *model, int batch);

/*
 * ctx[batch][ctx_width] from x[batch][n_features] (float32): c_i = x W_x_i[:n_features] + b_i for every layer the head
 * evaluates, one f32-MFMA GEMM against the concatenated x rows of those layers plus the bias row.  work:
 * icnn_be_ficnn_context_work_floats(model, batch) floats.  No host synchronisation (capturable).
 */
ICNN_BE_API int icnn_be_ficnn_context(const icnn_be_ficnn_model *model, const float *x, int batch, float *ctx, float *work,
                                      void *stream);

/*
 * E[B] and dE/dy[B][n] (float32) of the FICNN at y (float64, rounded to float32 on entry like a TensorFlow feed):
 * what sess.run(tf.gradients(E_, y_)) evaluates in synthetic-cls/icnn.py:125 (tf.gradients sums over the [B, width[L-1]]
 * outputs of head SUM).  ctx[B][ctx_width] is the x-only part.  Rows whose finished[u] != 0 are left untouched
 * (finished may be NULL).  One workgroup per 16 samples, f32 MFMA.
 */
ICNN_BE_API int icnn_be_ficnn_fg(const icnn_be_ficnn_model *model, const float *ctx, const double *y, int batch, float *f,
                                 float *g, const int *finished, void *stream);

/*
 * n_iter steps of momentum gradient descent on y for the FICNN: the recurrence, float32 arithmetic, arguments, outputs and
 * errors of icnn_be_fc_gd (workspace: icnn_be_gd_workspace_bytes(batch, n)), synthetic-cls/icnn.py:117-131.  One
 * persistent launch, a workgroup per 16 samples; bit-identical to a loop of icnn_be_ficnn_fg plus the float32 update.
 */
ICNN_BE_API int icnn_be_ficnn_gd(const icnn_be_ficnn_model *model, const float *ctx, const double *y0, int batch, int n_iter,
                                 double lr, double momentum, double *y_out, double *traj, float *f_out, void *workspace,
                                 void *stream);

/*
 * solveBatch on the device for a FICNN energy: the rounds of { icnn_be_ficnn_fg ; dual step } with the scheduling of
 * icnn_be_solve_conv (lockstep unless ICNN_BE_FLAG_TIME_SLICE).  f_work[B], g_work[B][n] are scratch; the state must
 * have been reset with icnn_be_state_init and st->cut_dtype must be F32.  Returns the number of rounds issued (> 0) or
 * a negative error code.
 */
ICNN_BE_API int icnn_be_solve_ficnn(const icnn_be_ficnn_model *model, const float *ctx, const icnn_be_state *st,
                                    float *f_work, float *g_work, void *stream);

/*
 * Floats of the packed parameter gradient of a FICNN (0: shape rejected; host arithmetic).  For i = 0 .. L, in the order
 * of tf.trainable_variables() in synthetic-cls/icnn.py:213-234 (icnn_amd.ficnn.init_params):
 *   'z_x{i}/W' [n_features + n][width[i]], 'z_x{i}/b' [width[i]], 'z_z{i}_proj/W' [width[i-1]][width[i]] (i > 0 only)
 * With head SUM the head layer's variables do not reach E (compute_gradients returns None, :137-139): their gradient is 0.
 */
ICNN_BE_API size_t icnn_be_ficnn_grad_floats(const icnn_be_ficnn_model *model);

/* floats of device scratch icnn_be_ficnn_surrogate_grad needs for `batch` samples and `rows` rows (0: rejected) */
ICNN_BE_API size_t icnn_be_ficnn_surrogate_grad_work_floats(const icnn_be_ficnn_model *model, int batch, int rows);

/*
 * grad = d/dtheta  sum_r [ c_r E(x_s(r), y_r) + <dE/dy(x_s(r), y_r), v_r> ]  over every variable, float32, packed as
 * icnn_be_ficnn_grad_floats describes; the arguments are those of icnn_be_fc_surrogate_grad (row_offset, y, v, c, F_rows,
 * v may be NULL).  With c = 0 and v_k = coefficient_k dL/dy_K over the trajectory of icnn_be_ficnn_gd it is the gradient
 * of L(y_K) through the unrolled inference (synthetic-cls/icnn.py:133-139).  Deterministic (no atomics), no host
 * synchronisation (capturable).  ICNN_BE_EINVAL / ICNN_BE_ELIMIT for a bad shape or a NULL required pointer before
 * anything is launched.
 */
ICNN_BE_API int icnn_be_ficnn_surrogate_grad(const icnn_be_ficnn_model *model, const float *x, int batch, const int *row_offset,
                                             int rows, const double *y, const double *v, const double *cvec, float *grad,
                                             float *F_rows, float *work, void *stream);

/* ---- convolutional PICNN (completion/icnn_ebundle.py) ---------------------------------------- */

/* Number of floats of the packed weight buffer (0 if the shape is rejected). */
ICNN_BE_API size_t icnn_be_conv_pack_floats(const icnn_be_conv_model *shape);

/* floats of device scratch an evaluation of `batch` samples needs (model->work). */
ICNN_BE_API size_t icnn_be_conv_work_floats(const icnn_be_conv_model *shape, int batch);

/*
 * Pack the y-path weights (host -> host), all row-major float32 as tflearn stores them:
 *   w_yu_host[l]  'z{l}_yu/W'      [k][k][1][F_l]            l = 0..2   (:390-392)
 *   w_yr_host[l]  'z{l}_y_red/W'   [k][k][1][1], b_yr_host[l] its bias [1],  l = 0, 1   (:394-396)
 *   w_zu_host[l]  'z{l}_zu_proj/W' [k][k][F_{l-1}][F_l]      l = 1, 2   (:385-387; [0] ignored)
 *   w_fc3_host    'z3_zu_proj/W'   [flat][fc_hidden],  w_fc4_host 'z4_zu_proj/W' [fc_hidden][1]  (:418-420)
 */
ICNN_BE_API int icnn_be_conv_pack(const icnn_be_conv_model *shape, const float *const *w_yu_host,
                                  const float *const *w_yr_host, const float *const *b_yr_host,
                                  const float *const *w_zu_host, const float *w_fc3_host,
                                  const float *w_fc4_host, float *out_host);

/*
 * E[B] and dE/dy[B][H*W] (float32) at y (float64, flat [B][H*W], rounded to float32 on entry).
 * Replaces sess.run([E_, dE_dyFlat_]) of completion/icnn_ebundle.py:217-221 for the y-dependent
 * part.  Rows whose finished[u] != 0 are skipped (finished may be NULL).
 */
ICNN_BE_API int icnn_be_conv_fg(const icnn_be_conv_model *model, const float *ctx, const double *y, int batch,
                                float *f, float *g, const int *finished, void *stream);

/* The whole solveBatch loop for the conv PICNN (completion/icnn_ebundle.py:226-227); see icnn_be_solve_fc. */
ICNN_BE_API int icnn_be_solve_conv(const icnn_be_conv_model *model, const float *ctx, const icnn_be_state *st,
                                   float *f_work, float *g_work, void *stream);

/*
 * Diagnostic hooks (no reference counterpart; used by tools/dual_phase_profile.py, tools/fc_phase_profile.py,
 * tools/conv_dual_phase_profile.py).  While a buffer is set, the kernels add per-phase cycle counts (s_memtime laps of lane 0)
 * to it and the dispatcher picks the instrumented kernels; NULL switches the hooks off again.  Process-wide, not thread-safe,
 * not for production use.  The laps are compiled into the PROFILING variant of the library only (the same sources with
 * -DICNN_BE_PROF=1: `python -m icnn_amd.build --prof` -> icnn_amd/csrc/prof/libicnn_be.so, what the tools load): in the production
 * library they would cost the benchmark solve 1.8 %, and there these calls set a pointer that no kernel reads.
 *   icnn_be_debug_profile       device_buf [max(B, 4096) + 8][16] int64: dual-step phases per sample
 *   icnn_be_debug_profile_fc    device_buf int64, FC-PICNN phases per workgroup and wave: [ceil(B / 16)][16][16] for the tile
 *                               kernels (icnn_be_fc_fg, the persistent tile solve); the per-sample kernels (up to four samples
 *                               per CU: fused_rows_solve_kernel) index it [ceil(B / per_wg)][8][16] with per_wg =
 *                               ceil(B / CUs) -- up to B workgroups: size the buffer max(ceil(B / 16) * 16, B * 8) * 16
 *                               entries to cover both (tools/rows_phase_profile.py)
 *   icnn_be_debug_profile_conv  device_buf: conv-PICNN phases per workgroup and wave
 */
ICNN_BE_API void icnn_be_debug_profile(long long *device_buf);
/* Per-round timeline of the persistent tile kernel's grouped dual phase (nIter > 15; profiling variant only,
 * tools/c4_timeline.py): device_buf [B][ICNN_BE_MAX_ITERS][4] int64, per sample and round the shader-clock stamps of
 * { the tile's dual phase starting, this sample's dual step starting (behind its wait for a staging region), its end } and
 * the sample's Newton updates before the round.  NULL switches it off. */
ICNN_BE_API void icnn_be_debug_trace(long long *device_buf);
/* counters per sample of icnn_be_debug_profile's buffer (16): size the buffer from this, not from a literal */
ICNN_BE_API int icnn_be_debug_profile_phases(void);
/*
 * The exp / log / softplus / sigmoid the INNER iterations use in place of the math library's (be_dual_math.h: fast_exp,
 * fast_log, softplus_fast, sigmoid_fast -- lean argument reductions + Horner polynomials; values that are final, y =
 * 1 / (1 + exp(A^T lam)) of lib/bundle_entropy_dual.py:165, keep the library routines), evaluated on caller-supplied
 * arguments: out[i] = f(x[i]), which = 0 exp, 1 log, 2 softplus (logexp1p, dual :6-12), 3 sigmoid.  Lets a test bound
 * their error against extended precision (tests/test_gpu_parity.py: relative error <= 5e-16 on the ranges the iterations
 * feed them, exact limits at the clamp +-750 and at +-inf).  NaN: the argument clamp of fast_exp (v_max / v_min) maps NaN
 * to a finite value, so fast_exp(NaN) = exp(-750) = 0 and sigmoid_fast(NaN) is finite: a non-finite A^T lam inside the Newton
 * loop is NOT propagated by these routines; it surfaces at the y update, whose library exp yields NaN and sets
 * ICNN_BE_ST_NONFINITE (non-finite energies / gradients are caught before, when the cut is taken).
 */
ICNN_BE_API int icnn_be_debug_fast_math(int which, const double *x, double *out, int count, void *stream);
ICNN_BE_API void icnn_be_debug_profile_fc(long long *device_buf);
ICNN_BE_API void icnn_be_debug_profile_conv(long long *device_buf);
/*
 * The plan icnn_be_solve_fc follows for this model and state on a device with `cus` CUs (cus < 1: the current device's):
 * returns an ICNN_BE_PATH_* code and fills out = { samples per workgroup of the persistent kernel (0: launch pairs), Newton
 * updates per sample and round (0: unlimited), the value icnn_be_solve_fc returns }, or a negative error code (batch 0:
 * ICNN_BE_EINVAL, nothing is planned).  Host arithmetic only: needs neither a GPU nor any buffer of the model or the state.
 */
ICNN_BE_API int icnn_be_debug_solve_plan(const icnn_be_fc_model *model, const icnn_be_state *st, int cus, int out[3]);
/*
 * The launch icnn_be_adam_fc makes for this model and batch on the current device: returns an ICNN_BE_ADAM_* code and fills
 * out = { states per workgroup, workgroups, 1 if the launch is cooperative (several workgroups, all resident), 1 if
 * icnn_be_adam_fc_obs accepts this model with the context description cx (0 with cx == NULL, and wherever that entry answers
 * ICNN_BE_ELIMIT) }; ICNN_BE_ADAM_NONE (out all zero) where icnn_be_adam_fc answers ICNN_BE_ELIMIT.  A negative error code for
 * what both entries refuse as a bad argument (batch 0: ICNN_BE_EINVAL, nothing is planned).  Enqueues nothing and reads no
 * buffer of the model or of cx; with more than four states it asks the runtime how many workgroups a CU holds, so it needs
 * a device.
 */
ICNN_BE_API int icnn_be_debug_adam_plan(const icnn_be_fc_model *model, const icnn_be_fc_ctx *cx, int batch, int out[4]);
/*
 * The launch icnn_be_adam_fc_each makes (additive to ABI 12): returns ICNN_BE_ADAM_ROWS or ICNN_BE_ADAM_TILE and fills
 * out = { states per workgroup, workgroups }; ICNN_BE_ADAM_NONE (out all zero) where no layout fits the LDS.  Never cooperative.
 * Errors and device use as icnn_be_debug_adam_plan.
 */
ICNN_BE_API int icnn_be_debug_adam_each_plan(const icnn_be_fc_model *model, int batch, int out[2]);
/*
 * The kernel instance icnn_be_dual_step(st, t, ...) launches (additive to ABI 12): returns 0 and fills out = { cut type of the
 * instance (ICNN_BE_CUT_*), its bundle tile KT (16 or 32; small kernel: its KS, 5, 8 or 16), waves per workgroup, its variant
 * (ICNN_BE_VARIANT_*), 1 if the bundle is staged in st->scratch instead of LDS, the kernel (ICNN_BE_DUAL_PLAN_*), bytes of
 * dynamic LDS, bundle rows the staging area holds }, or a negative error code where icnn_be_dual_step refuses the shape or t
 * (ICNN_BE_EINVAL also for batch 0, where nothing is launched, and where no instance fits).  It is the launcher's own choice,
 * taken by the launcher's own code, without the launch: host arithmetic on the shape fields, the flags and on whether
 * st->scratch is set.  Needs no GPU; the buffer pointers of the state are neither read nor checked.
 */
ICNN_BE_API int icnn_be_debug_dual_plan(const icnn_be_state *st, int t, int out[8]);
/*
 * One round of a dual body that only the persistent tile kernel's Bibsonomy instances contain, without the tile kernel around it
 * (additive to ABI 12; tests/test_dual_body_probe.py).  Semantics of icnn_be_dual_step(st, t, f, g): one launch, one wave per
 * sample, no update budget, the same operations in the same order -- so the same bits, newton_iters and status included, wherever
 * both form their sums by the same routine.  The body is called the way the tile kernel calls it: its arguments first in the
 * kernel-argument struct, the two constant rows shared in LDS, the sample's LDS region sized by the tile layout.
 *   which 1      the body of ICNN_BE_SHAPE_BIBTEX_KT16 from round 8 on (and of every round under ICNN_BE_FLAG_NO_ROUND_CLASSES)
 *   which 2      the body of its rounds 0..7: compiled for at most eight cuts, no MFMA sweep in it
 *   which 3      the body of ICNN_BE_SHAPE_BIBTEX_KT32_GROUPED
 *   rows_mode 0  the staging holds min(t + 1, slots) rows, as in the ungrouped round loop
 *   rows_mode 1  per sample count + 1 rows (at most slots), as the grouped loop sizes it; a finished sample, or one whose own
 *                iteration counter is past the last iteration, is left alone.  With which 1 and 3.
 * ICNN_BE_EINVAL, before any launch, unless: the variant is dual with float32 cuts; n is the instances' 159; slots <= 15 for
 * which 1 and 2, slots > 15 for which 3; for which 2 t < 8 and ICNN_BE_FLAG_MFMA_CONTRACTION is not set; neither
 * ICNN_BE_FLAG_GLOBAL_BUNDLE nor ICNN_BE_FLAG_TIME_SLICE is set; and whatever icnn_be_dual_step refuses.  Batch 0: 0, nothing
 * is launched.  Not for production use.
 */
ICNN_BE_API int icnn_be_debug_dual_step_body(const icnn_be_state *st, int t, const void *f, const void *g, int which,
                                             int rows_mode, void *stream);
/*
 * The instance of the persistent tile kernel icnn_be_solve_fc launches for this model and state on the current device
 * (additive to ABI 12): ICNN_BE_SHAPE_GENERIC -- the kernel that reads the network's shape from its arguments; also where the
 * plan (icnn_be_debug_solve_plan) is not ICNN_BE_PATH_TILE -- or the id of an instance compiled for one shape.  Such an instance
 * is taken only where n, the number of layers, every width and the context width of the model equal its constants, the variant
 * is dual, the cuts are float32, the launch has no update budget, and the layout decision (the dual phase in groups or not) is
 * the instance's; ICNN_BE_FLAG_GENERIC_SHAPE switches them off.  It is the launcher's own choice, taken by the launcher's own
 * code: host arithmetic, no GPU needed (without one the plan is that of a 256-CU device).  A negative error code for what
 * icnn_be_solve_fc refuses (batch 0: ICNN_BE_EINVAL), but for a float64 cut dtype: ICNN_BE_SHAPE_GENERIC, as for every other
 * state no instance was compiled for.
 */
#define ICNN_BE_SHAPE_GENERIC 0
#define ICNN_BE_SHAPE_BIBTEX_KT16 1           /* n = 159, widths 600 / 159 / 1 (the Bibsonomy net), up to 15 slots, not grouped */
#define ICNN_BE_SHAPE_BIBTEX_KT32_GROUPED 2   /* the same net, 16..32 slots, the dual phase in groups */
ICNN_BE_API int icnn_be_debug_shape_instance(const icnn_be_fc_model *model, const icnn_be_state *st);
/*
 * The deal of one tile evaluation of this model (additive to ABI 12): which of the workgroup's 16 waves runs which unit in which
 * barrier interval, as the tile kernels read it (fc_deal, be_picnn_fc_dev.h; the same for every kernel around fc_fg_tile and for
 * the shape instances).  With L = n_layers - 1 hidden layers an evaluation has the intervals 0 .. L-1 (forward layers 0 .. L-1),
 * L .. 2L-1 (backward layers L-1 .. 0) and 2L (behind the last barrier).  One record of six ints per unit:
 *   { kind, layer, tile, interval, wave, interval in which the unit's result is written }
 * kind ICNN_BE_UNIT_FWD_Y: tile `tile` of (y * yu_layer) Wyu_layer; FWD_Z: the same accumulator continued with
 * (z_{layer-1} gate_layer) Wzu_layer (layer >= 1); DELTA: delta_layer Wzu_layer^T (layer >= 1); DEDY: delta_layer Wyu_layer^T,
 * added into the gradient (the last field is 2L where the accumulator crosses the last barrier and g is stored from it);
 * E: energy row `tile` of the 16.  Returns the number of records, writing the first `cap` of them (out may be null with cap 0),
 * or a negative error code for a model icnn_be_fc_check refuses.  Host arithmetic, no GPU needed.
 */
#define ICNN_BE_UNIT_FWD_Y 0
#define ICNN_BE_UNIT_FWD_Z 1
#define ICNN_BE_UNIT_DELTA 2
#define ICNN_BE_UNIT_DEDY 3
#define ICNN_BE_UNIT_E 4
ICNN_BE_API int icnn_be_debug_fc_deal(const icnn_be_fc_model *model, int *out, int cap);

/* ---- the DDPG agent: fused actor-critic step, EMA targets, act (be_ddpg.hip, additive to ABI 12) ---- */

/*
 * DDPG of RL/src/ddpg.py with the networks of ddpg_nets_dm.py, all float32.  A net is one flat vector in the order W1, b1,
 * W2, b2, W3, b3, every W row-major [in][out]:
 *   policy  a = tanh(relu(relu(o W1 + b1) W2 + b2) W3 + b3)          W1 [dimO][l1], W2 [l1][l2], W3 [l2][dimA]
 *   critic  q = relu([relu(o W1 + b1), a] W2 + b2) W3 + b3           W1 [dimO][l1], W2 [l1 + dimA][l2], W3 [l2][1]
 * One step on the minibatch (obs, act, rew, ob2, term), everything read from the parameters as they are when it begins:
 *   a2 = pi(ob2; target_p), q2 = Q(ob2, a2; target_q), y = term ? rew : rew + discount q2
 *   td = Q(obs, act; theta_q) - y, loss_q = mean td^2 + l2norm sum theta_q^2 / 2 (all six variables), g_q = d loss_q / d theta_q
 *   loss_p = -mean Q(obs, pi(obs; theta_p); theta_q) + pl2norm sum theta_p^2 / 2, g_p = d loss_p / d theta_p
 *   TF-Adam on both nets (icnn_be_param_update's element arithmetic with eps as given and no proj; lr = rate for theta_q,
 *   prate for theta_p; each net its own m, v and step count), then target <- target - tau (target - theta_new).
 * icnn_be_ddpg_chain does the per-sample part (one launch) and leaves the layer inputs and pre-activation deltas in the
 * workspace; icnn_be_ddpg_grads forms grad_q and grad_p from them (one launch, one fma chain over the batch per element, no atomics);
 * icnn_be_ddpg_update updates both nets and both targets in one launch and writes loss_q; icnn_be_ddpg_step is the three in
 * that order.  act: float64, rounded to float32 once on load.
 *
 * The workspace: icnn_be_ddpg_work_bytes bytes, 16-byte aligned; icnn_be_ddpg_work_offsets gives the offset in floats of
 * each piece ICNN_BE_DDPG_W_* ([batch][width] float32 unless said otherwise); the chain writes nothing outside the rows
 * < batch of its pieces.  step: ICNN_BE_DDPG_STEP_INTS int32, zero for fresh nets: [0] updates of the critic, [1] of the
 * policy, [2] a ticket (zero between launches); a captured step replayed k times is k steps.
 *
 * Sizes: 1 <= dimO <= ICNN_BE_DDPG_MAX_OBS, 1 <= dimA <= ICNN_BE_DDPG_MAX_ACT, 1 <= l1, l2 <= ICNN_BE_DDPG_MAX_HIDDEN,
 * batch >= 1.  EINVAL for anything else, a NULL or misaligned pointer (the nets, m, v, the gradients and work 16 bytes, act 8,
 * the rest 4), tau outside [0, 1], a non-finite discount, a negative or non-finite l2norm / pl2norm, beta outside [0, 1),
 * eps <= 0, a non-finite rate, before anything is launched.  No entry synchronises; all are capturable.
 */
#define ICNN_BE_DDPG_MAX_OBS 600
#define ICNN_BE_DDPG_MAX_ACT 32
#define ICNN_BE_DDPG_MAX_HIDDEN 600
#define ICNN_BE_DDPG_STEP_INTS 4
#define ICNN_BE_DDPG_W_A2 0    /* pi(ob2; target_p) [dimA] */
#define ICNN_BE_DDPG_W_Y 1     /* y [1] */
#define ICNN_BE_DDPG_W_Q 2     /* Q(obs, act) [1] */
#define ICNN_BE_DDPG_W_TD 3    /* td [1] */
#define ICNN_BE_DDPG_W_A 4     /* pi(obs) [dimA] */
#define ICNN_BE_DDPG_W_QPI 5   /* Q(obs, pi(obs)) [1] */
#define ICNN_BE_DDPG_W_XA 6    /* the critic's [h1, act] [l1 + dimA] */
#define ICNN_BE_DDPG_W_H2Q 7   /* the critic's h2 at (obs, act) [l2] */
#define ICNN_BE_DDPG_W_D3Q 8   /* the critic's deltas: 2 td / batch [1], [l2], [l1] */
#define ICNN_BE_DDPG_W_D2Q 9
#define ICNN_BE_DDPG_W_D1Q 10
#define ICNN_BE_DDPG_W_H1P 11  /* the policy's h1 [l1], h2 [l2] at obs */
#define ICNN_BE_DDPG_W_H2P 12
#define ICNN_BE_DDPG_W_H2C 13  /* the critic's h2 at (obs, pi(obs)) [l2] */
#define ICNN_BE_DDPG_W_D3P 14  /* the policy's deltas [dimA], [l2], [l1] */
#define ICNN_BE_DDPG_W_D2P 15
#define ICNN_BE_DDPG_W_D1P 16
#define ICNN_BE_DDPG_W_SQ 17   /* float64 [tiles of 16 samples]: each tile's sum of td^2 */
#define ICNN_BE_DDPG_W_UPD 18  /* float64: the update's partial sums of theta_q^2 */
#define ICNN_BE_DDPG_WORK_PIECES 19
typedef struct icnn_be_ddpg_args {
    int batch, dimO, dimA, l1, l2;
    const float *obs;                 /* [batch][dimO] */
    const double *act;                /* [batch][dimA] */
    const float *rew;                 /* [batch] */
    const float *ob2;                 /* [batch][dimO] */
    const unsigned char *term;        /* [batch] */
    float *theta_q, *theta_p, *target_q, *target_p;
    float *m_q, *v_q, *m_p, *v_p;     /* Adam's moments */
    float *grad_q, *grad_p;           /* the step's gradients, before the decay term */
    int *step;                        /* [ICNN_BE_DDPG_STEP_INTS] */
    float *loss;                      /* loss_q of the step */
    void *work;
    double rate, prate, beta1, beta2;
    float eps, tau, discount, l2norm, pl2norm;
} icnn_be_ddpg_args;                  /* icnn_be_struct_size(13) */

/* floats of theta_p (*np) and theta_q (*nq); EINVAL for sizes out of range */
ICNN_BE_API int icnn_be_ddpg_param_floats(int dimO, int dimA, int l1, int l2, long long *np, long long *nq);
/* 0 for sizes out of range */
ICNN_BE_API size_t icnn_be_ddpg_work_bytes(int batch, int dimO, int dimA, int l1, int l2);
ICNN_BE_API int icnn_be_ddpg_work_offsets(int batch, int dimO, int dimA, int l1, int l2, long long off[ICNN_BE_DDPG_WORK_PIECES]);
ICNN_BE_API int icnn_be_ddpg_chain(const icnn_be_ddpg_args *a, void *stream);
ICNN_BE_API int icnn_be_ddpg_grads(const icnn_be_ddpg_args *a, void *stream);
ICNN_BE_API int icnn_be_ddpg_update(const icnn_be_ddpg_args *a, void *stream);
ICNN_BE_API int icnn_be_ddpg_step(const icnn_be_ddpg_args *a, void *stream);
/*
 * out[batch][dimA] = pi(obs; theta_p): what act() pays per environment step, one workgroup per 16 observations (batch 1:
 * one workgroup), the bits of the chain's ICNN_BE_DDPG_W_A.  icnn_be_ddpg_q: out[batch] = Q(obs, act; theta_q), the bits of
 * ICNN_BE_DDPG_W_Q.  EINVAL as above (theta 16 bytes, act 8, obs and out 4).
 */
ICNN_BE_API int icnn_be_ddpg_act(int dimO, int dimA, int l1, int l2, const float *theta_p, const float *obs, int batch, float *out,
                                 void *stream);
ICNN_BE_API int icnn_be_ddpg_q(int dimO, int dimA, int l1, int l2, const float *theta_q, const float *obs, const double *act,
                               int batch, float *out, void *stream);

/* ---- the NAF agent: fused Q step with the L-matrix head, act (be_naf.hip, additive to ABI 12) ---- */

/*
 * NAF of RL/src/naf.py with the networks of naf_nets_dm.py and naf_bn False, all float32.  Three nets theta_l, theta_u,
 * theta_v, each one flat vector in the order W1, b1, W2, b2, W3, b3, every W row-major [in][out] (the layout of DDPG's
 * policy) with W1 [dimO][l1], W2 [l1][l2] and W3 [l2][dimA^2] (L), [l2][dimA] (U), [l2][1] (V);
 * mlp(o; theta) = relu(relu(o W1 + b1) W2 + b2) W3 + b3.  Per sample:
 *   l = mlp(obs; theta_l) read as a row-major [dimA][dimA] matrix; Lm[i][j] = l[i][j] below the diagonal, exp(l[i][i]) on
 *   it, 0 above;  u = tanh(mlp(obs; theta_u));  delta = act - u;  h[j] = sum_{i >= j} delta[i] Lm[i][j] (an fma chain in
 *   ascending i);  A = -1/2 sum_j h[j]^2 (ascending j);  q = mlp(obs; theta_v) + A.
 * One step on the minibatch (obs, act, rew, ob2, term), everything read from the parameters as they are when it begins:
 *   y = term ? rew : rew + discount mlp(ob2; target_v)     (the target's advantage is the constant 0)
 *   td = q - y, loss_q = mean td^2 + l2norm sum theta^2 / 2 over all 18 variables, g = d loss_q / d (theta_l, theta_u, theta_v)
 *   ONE TF-Adam over the three vectors (icnn_be_param_update's element arithmetic with eps as given and no proj, one step
 *   count), then target_v <- target_v - tau (target_v - theta_v_new).
 * icnn_be_naf_chain does the per-sample part (one launch) and leaves the layer inputs and pre-activation deltas in the
 * workspace; icnn_be_naf_grads forms grad_l, grad_u and grad_v from them (one launch, one fma chain over the batch per
 * element, no atomics); icnn_be_naf_update updates the three nets and the target in one launch and writes loss_q;
 * icnn_be_naf_step is the three in that order.  act: float64, rounded to float32 once on load.
 *
 * The workspace: icnn_be_naf_work_bytes bytes, 16-byte aligned; icnn_be_naf_work_offsets gives the offset in floats of each
 * piece ICNN_BE_NAF_W_* ([batch][width] float32 unless said otherwise); the chain writes nothing outside the rows < batch of
 * its pieces.  step: ICNN_BE_NAF_STEP_INTS int32, zero for fresh nets: [0] the updates, [1] a ticket (zero between
 * launches); a captured step replayed k times is k steps.
 *
 * Sizes: 1 <= dimO <= ICNN_BE_NAF_MAX_OBS, 1 <= dimA <= ICNN_BE_NAF_MAX_ACT, 1 <= l1, l2 <= ICNN_BE_NAF_MAX_HIDDEN,
 * batch >= 1; at these maxima the chain kernel takes 148864 bytes of LDS (the obs rows and the dimA^2 = 1024 wide l rows
 * share one buffer).  EINVAL for anything else, a NULL or misaligned pointer (the nets, m, v, the gradients and work 16
 * bytes, act 8, the rest 4), tau outside [0, 1], a non-finite discount, a negative or non-finite l2norm, beta outside [0, 1),
 * eps <= 0, a non-finite rate, before anything is launched.  No entry synchronises; all are capturable.
 */
#define ICNN_BE_NAF_MAX_OBS 600
#define ICNN_BE_NAF_MAX_ACT 32
#define ICNN_BE_NAF_MAX_HIDDEN 600
#define ICNN_BE_NAF_STEP_INTS 4
#define ICNN_BE_NAF_W_Y 0      /* y [1] */
#define ICNN_BE_NAF_W_U 1      /* u [dimA] */
#define ICNN_BE_NAF_W_L 2      /* l [dimA^2] */
#define ICNN_BE_NAF_W_LD 3     /* the diagonal of Lm, exp(l[i][i]) [dimA] */
#define ICNN_BE_NAF_W_H 4      /* h [dimA] */
#define ICNN_BE_NAF_W_ADV 5    /* A [1] */
#define ICNN_BE_NAF_W_Q 6      /* q [1] */
#define ICNN_BE_NAF_W_TD 7     /* td [1] */
#define ICNN_BE_NAF_W_H1L 8    /* the hidden layers of the L net [l1], [l2] */
#define ICNN_BE_NAF_W_H2L 9
#define ICNN_BE_NAF_W_H1U 10   /* of the U net */
#define ICNN_BE_NAF_W_H2U 11
#define ICNN_BE_NAF_W_H1V 12   /* of the V net */
#define ICNN_BE_NAF_W_H2V 13
#define ICNN_BE_NAF_W_D3L 14   /* the deltas of the L net: d loss / d l [dimA^2], [l2], [l1] */
#define ICNN_BE_NAF_W_D2L 15
#define ICNN_BE_NAF_W_D1L 16
#define ICNN_BE_NAF_W_D3U 17   /* of the U net: before the tanh [dimA], [l2], [l1] */
#define ICNN_BE_NAF_W_D2U 18
#define ICNN_BE_NAF_W_D1U 19
#define ICNN_BE_NAF_W_D3V 20   /* of the V net: 2 td / batch [1], [l2], [l1] */
#define ICNN_BE_NAF_W_D2V 21
#define ICNN_BE_NAF_W_D1V 22
#define ICNN_BE_NAF_W_SQ 23    /* float64 [tiles of 16 samples]: each tile's sum of td^2 */
#define ICNN_BE_NAF_W_UPD 24   /* float64: the update's partial sums of theta^2 */
#define ICNN_BE_NAF_WORK_PIECES 25
typedef struct icnn_be_naf_args {
    int batch, dimO, dimA, l1, l2;
    const float *obs;                 /* [batch][dimO] */
    const double *act;                /* [batch][dimA] */
    const float *rew;                 /* [batch] */
    const float *ob2;                 /* [batch][dimO] */
    const unsigned char *term;        /* [batch] */
    float *theta_l, *theta_u, *theta_v, *target_v;      /* separately allocated */
    float *m_l, *v_l, *m_u, *v_u, *m_v, *v_v;           /* Adam's moments */
    float *grad_l, *grad_u, *grad_v;  /* the step's gradients, before the decay term */
    int *step;                        /* [ICNN_BE_NAF_STEP_INTS] */
    float *loss;                      /* loss_q of the step */
    void *work;
    double rate, beta1, beta2;
    float eps, tau, discount, l2norm;
} icnn_be_naf_args;                   /* icnn_be_struct_size(14) */

/* floats of theta_l (*nl), theta_u (*nu) and theta_v (*nv); EINVAL for sizes out of range */
ICNN_BE_API int icnn_be_naf_param_floats(int dimO, int dimA, int l1, int l2, long long *nl, long long *nu, long long *nv);
/* 0 for sizes out of range */
ICNN_BE_API size_t icnn_be_naf_work_bytes(int batch, int dimO, int dimA, int l1, int l2);
ICNN_BE_API int icnn_be_naf_work_offsets(int batch, int dimO, int dimA, int l1, int l2, long long off[ICNN_BE_NAF_WORK_PIECES]);
ICNN_BE_API int icnn_be_naf_chain(const icnn_be_naf_args *a, void *stream);
ICNN_BE_API int icnn_be_naf_grads(const icnn_be_naf_args *a, void *stream);
ICNN_BE_API int icnn_be_naf_update(const icnn_be_naf_args *a, void *stream);
ICNN_BE_API int icnn_be_naf_step(const icnn_be_naf_args *a, void *stream);
/*
 * icnn_be_naf_act: out[batch][dimA] = u(obs; theta_u), what act() pays per environment step: the U net has the layout and
 * the function of DDPG's policy, so this is icnn_be_ddpg_act's launch on theta_u, and the bits of the chain's
 * ICNN_BE_NAF_W_U.  icnn_be_naf_q: out[batch] = q(obs, act; theta_l, theta_u, theta_v), the bits of ICNN_BE_NAF_W_Q.
 * EINVAL as above (theta 16 bytes, act 8, obs and out 4).
 */
ICNN_BE_API int icnn_be_naf_act(int dimO, int dimA, int l1, int l2, const float *theta_u, const float *obs, int batch, float *out,
                                void *stream);
ICNN_BE_API int icnn_be_naf_q(int dimO, int dimA, int l1, int l2, const float *theta_l, const float *theta_u, const float *theta_v,
                              const float *obs, const double *act, int batch, float *out, void *stream);

/* ---- the feed-forward baseline of the multi-label experiment (be_ff.hip, additive to ABI 12) ---- */

/*
 * multi-label-cls/ff.py, all float32.  n_layers = L hidden layers of widths width[0 .. L-1]; w_0 = n_features:
 *   a_i = relu(h_{i-1} W_i + b_i),  h_i = (a_i - mu_i) gamma_i / sqrt(sigma2_i + bn_eps) + beta_i,  h_0 = x
 *   yhat = sigmoid(h_L W_o + b_o),  loss = - sum y log(yhat + 1e-10) - sum (1 - y) log(1 - yhat + 1e-10)  over batch and labels
 * theta is one flat vector: for i = 1..L  W_i [w_{i-1}][w_i], b_i, gamma_i, beta_i;  then W_o [w_L][n_labels], b_o.  m, v and
 * grad have its layout.  mv.mean[i] / mv.var[i] are the moving pair of hidden layer i + 1 (width[i] floats).
 *
 * In ICNN_BE_BN_BATCH mode mu is the batch mean and sigma2 the biased two-pass variance; in ICNN_BE_BN_MOVING mode they are
 * the moving pair, every row is independent of the others and nothing is written to mv.
 *   icnn_be_ff_forward   the L layers and the head in `mode`: yhat, and with true_y != NULL the loss, the F1 tallies (unless
 *                        NULL) and, in batch mode, d loss / d logits.  L + 1 launches.
 *   icnn_be_ff_backward  after a batch-mode forward with true_y: the pre-activation deltas of every hidden layer, and
 *                        d gamma, d beta into grad.  L launches.
 *   icnn_be_ff_grads     the weight and bias gradients into grad: one launch, one fma chain over the batch per element.
 *   icnn_be_ff_update    one TF-Adam over theta with the step count step[0]: one launch.
 *   icnn_be_ff_step      forward (batch mode), backward, grads, update, and ONE fold of every layer's (mu, sigma2) into mv:
 *                        2 L + 4 launches.  loss and yhat are those at the weights the step began with.
 *   icnn_be_ff_eval      forward in moving mode with true_y: yhat, loss, tallies.
 * loss is the float64 sum of the head's per-workgroup float64 partials in index order, rounded to float32 once.  f1_tallies
 * [batch][3] = (tp, fp, fn) of yhat >= 0.5 against (int)y per example, icnn_be_macro_f1's layout.  No float atomics: every
 * run gives the same bits.  No host synchronisation (capturable in a HIP graph).
 *
 * The workspace: icnn_be_ff_work_bytes bytes, 16-byte aligned, ZEROED ONCE by the caller (it holds the ticket the head's
 * workgroups count themselves with; the kernel re-arms it); icnn_be_ff_work_offsets gives the offset in floats of each piece
 * ICNN_BE_FF_W_*.  Nothing outside the rows < batch of a piece is written.  step: ICNN_BE_FF_STEP_INTS int32, zero for a fresh
 * model: [0] the updates, [1] a ticket.
 *
 * Sizes: 1 <= n_layers <= ICNN_BE_FF_MAX_LAYERS, 1 <= n_features <= ICNN_BE_FF_MAX_FEATURES, 1 <= width[i], n_labels <=
 * ICNN_BE_FF_MAX_WIDTH; batch-mode entries 2 <= batch <= ICNN_BE_FF_MAX_BATCH, moving mode any batch >= 1.  Anything else, a
 * NULL pointer an entry needs, theta / m / v / grad / work not 16-byte aligned, another pointer not 4-byte aligned, or a decay
 * outside [0, 1] is ICNN_BE_EINVAL before any launch (0 from icnn_be_ff_work_bytes).
 */
#define ICNN_BE_FF_MAX_LAYERS 4
#define ICNN_BE_FF_MAX_FEATURES 4096
#define ICNN_BE_FF_MAX_WIDTH 1024
#define ICNN_BE_FF_MAX_BATCH 512
#define ICNN_BE_FF_STEP_INTS 4
#define ICNN_BE_FF_W_A 0       /* + i: a_{i+1} [batch][width[i]], i < ICNN_BE_FF_MAX_LAYERS (empty beyond n_layers) */
#define ICNN_BE_FF_W_H 4       /* + i: h_{i+1} */
#define ICNN_BE_FF_W_STAT 8    /* + i: mu [width[i]] then sigma2 [width[i]], what a batch-mode forward normalised with */
#define ICNN_BE_FF_W_DZ 12     /* + i: d loss / d (h_i W_{i+1} + b_{i+1}) */
#define ICNN_BE_FF_W_DLOGIT 16 /* d loss / d logits [batch][n_labels] */
#define ICNN_BE_FF_W_PART 17   /* float64: the head's partial sums of the loss */
#define ICNN_BE_FF_W_CTL 18    /* int32: the head's ticket */
#define ICNN_BE_FF_WORK_PIECES 19
typedef struct icnn_be_ff_args {
    int batch, n_features, n_labels, n_layers;
    int width[ICNN_BE_FF_MAX_LAYERS];
    const float *x;                   /* [batch][n_features] */
    const float *true_y;              /* [batch][n_labels] */
    float *theta, *m, *v, *grad;
    icnn_be_bn_moving mv;
    int *step;                        /* [ICNN_BE_FF_STEP_INTS] */
    float *loss;                      /* [1] */
    float *yhat;                      /* [batch][n_labels] */
    int *f1_tallies;                  /* [batch][3], may be NULL */
    void *work;
    double lr, beta1, beta2;
    float eps, bn_eps;
} icnn_be_ff_args;                    /* icnn_be_struct_size(16) */

/* floats of theta; EINVAL for sizes out of range */
ICNN_BE_API int icnn_be_ff_param_floats(int n_features, int n_labels, int n_layers, const int *width, long long *n);
/* 0 for sizes out of range */
ICNN_BE_API size_t icnn_be_ff_work_bytes(int batch, int n_features, int n_labels, int n_layers, const int *width);
ICNN_BE_API int icnn_be_ff_work_offsets(int batch, int n_features, int n_labels, int n_layers, const int *width,
                                        long long off[ICNN_BE_FF_WORK_PIECES]);
ICNN_BE_API int icnn_be_ff_forward(const icnn_be_ff_args *a, int mode, void *stream);
ICNN_BE_API int icnn_be_ff_backward(const icnn_be_ff_args *a, void *stream);
ICNN_BE_API int icnn_be_ff_grads(const icnn_be_ff_args *a, void *stream);
ICNN_BE_API int icnn_be_ff_update(const icnn_be_ff_args *a, void *stream);
ICNN_BE_API int icnn_be_ff_step(const icnn_be_ff_args *a, void *stream);
ICNN_BE_API int icnn_be_ff_eval(const icnn_be_ff_args *a, void *stream);

/* ---- the FCN baseline of the completion experiment (be_fcn.hip, additive to ABI 12) ----
 *
 * completion/baseline.py's fully convolutional net on single-channel images [batch][H][W], all float32:
 *   conv1..3   3x3, stride 2, dilation 2, padding 2 (1 -> k, k -> k, k -> k): output i reads inputs 2i-2, 2i, 2i+2
 *   up1..3     transposed 3x3, stride 2, padding 1, output_padding 1 (k -> k): out[o] += in[i] w[t], o = 2i - 1 + t
 *   up4        transposed 1x1 (k -> 1);  ReLU behind every layer but up4;  yhat = up4's output
 *   loss = mean((pixel_scale (yhat - t))^2) over batch H W;  torch's Adam (eps outside the bias correction).
 * theta: one flat vector in the order and layouts of torch's model.parameters(): conv_i.weight [k][Cin][3][3], conv_i.bias,
 * up_i.weight [Cin][Cout][3][3], up_i.bias, up4.weight [k][1][1][1], up4.bias: 45 k^2 + 16 k + 1 floats.
 *
 *   icnn_be_fcn_forward   the seven layers: the six ReLU outputs into the workspace (channels last: [batch][h][w][k]) and yhat;
 *                         with t != NULL also loss, d loss / d yhat and up3's delta (batch <= ICNN_BE_FCN_MAX_BATCH).
 *   icnn_be_fcn_backward  after a forward with t: the pre-activation deltas of up2 ... conv1.
 *   icnn_be_fcn_grads     the flat gradient into grad: partial sums over fixed chunks of positions, added in index order.
 *   icnn_be_fcn_update    one torch-Adam over theta with the step count step[0], which advances by one: one launch.
 *   icnn_be_fcn_step      forward, backward, grads, update.
 *   icnn_be_fcn_eval      forward and loss alone: yhat, loss and the activations; no delta, nothing of the model.
 * No entry synchronises; every entry is capturable; results have the same bits on every run.
 *
 * The workspace: icnn_be_fcn_work_bytes bytes, 16-byte aligned, ZEROED ONCE by the caller (it holds the ticket of the loss;
 * the kernel re-arms it); icnn_be_fcn_work_offsets gives the offset in floats of each piece ICNN_BE_FCN_W_*.  step:
 * ICNN_BE_FCN_STEP_INTS int32, zero for a fresh optimiser (the updates done, the update's ticket).
 *
 * Sizes: k a multiple of 16 in [16, ICNN_BE_FCN_MAX_K]; H and W multiples of 8 in [8, ICNN_BE_FCN_MAX_HW]; 1 <= batch <=
 * ICNN_BE_FCN_MAX_BATCH for every entry that trains (forward with t, backward, grads, step), 1 <= batch <=
 * ICNN_BE_FCN_MAX_EVAL_BATCH otherwise.  Anything else, a NULL or misaligned pointer (16 bytes: theta, m, v, grad, work; 4
 * bytes: the rest), betas outside [0, 1) or eps <= 0 is ICNN_BE_EINVAL before any launch (0 from icnn_be_fcn_work_bytes). */
#define ICNN_BE_FCN_MAX_K 64
#define ICNN_BE_FCN_MAX_HW 128
#define ICNN_BE_FCN_MAX_BATCH 128
#define ICNN_BE_FCN_MAX_EVAL_BATCH 65536
#define ICNN_BE_FCN_STEP_INTS 4
#define ICNN_BE_FCN_W_H 0       /* + i, i < 6: the ReLU output of conv1, conv2, conv3, up1, up2, up3 [batch][h_i][w_i][k] */
#define ICNN_BE_FCN_W_DY 6      /* d loss / d yhat [batch][H][W] */
#define ICNN_BE_FCN_W_DZ 7      /* + i, i < 6: d loss / d (pre-activation of layer i), zero where the ReLU is off */
#define ICNN_BE_FCN_W_WPART 13  /* the chunk partials of the gradient */
#define ICNN_BE_FCN_W_LPART 14  /* float64: the partial sums of the loss and of d yhat, two per workgroup */
#define ICNN_BE_FCN_W_CTL 15    /* [0] int32: the loss's ticket; [1] float: sum of d yhat (up4.bias's gradient) */
#define ICNN_BE_FCN_WORK_PIECES 16
typedef struct icnn_be_fcn_args {
    int batch, H, W, k;
    const float *x;                   /* [batch][H][W] */
    const float *t;                   /* [batch][H][W]; NULL in icnn_be_fcn_forward: yhat alone */
    float *theta, *m, *v, *grad;
    int *step;                        /* [ICNN_BE_FCN_STEP_INTS] */
    float *loss;                      /* [1] */
    float *yhat;                      /* [batch][H][W] */
    void *work;
    double lr, beta1, beta2;
    float eps, pixel_scale;
} icnn_be_fcn_args;                   /* icnn_be_struct_size(18) */

/* floats of theta; EINVAL for sizes out of range */
ICNN_BE_API int icnn_be_fcn_param_floats(int H, int W, int k, long long *n);
/* 0 for sizes out of range */
ICNN_BE_API size_t icnn_be_fcn_work_bytes(int batch, int H, int W, int k);
ICNN_BE_API int icnn_be_fcn_work_offsets(int batch, int H, int W, int k, long long off[ICNN_BE_FCN_WORK_PIECES]);
ICNN_BE_API int icnn_be_fcn_forward(const icnn_be_fcn_args *a, void *stream);
ICNN_BE_API int icnn_be_fcn_backward(const icnn_be_fcn_args *a, void *stream);
ICNN_BE_API int icnn_be_fcn_grads(const icnn_be_fcn_args *a, void *stream);
ICNN_BE_API int icnn_be_fcn_update(const icnn_be_fcn_args *a, void *stream);
ICNN_BE_API int icnn_be_fcn_step(const icnn_be_fcn_args *a, void *stream);
ICNN_BE_API int icnn_be_fcn_eval(const icnn_be_fcn_args *a, void *stream);

/* ---- NAF with BatchNorm, naf_bn True (be_naf_bn.hip, additive to ABI 12) ----
 *
 * RL/src/naf_nets_dm.py:18-34 with naf_bn True: a BatchNorm (decay 0.999, epsilon 1e-3, a trainable beta, no gamma) in front of
 * the first layer and between each hidden product and its ReLU, in all three nets.  One site, S = dimO + l1 + l2 columns in all:
 *   batch mode   mu, var = the mean and the biased two-pass variance of a column over the batch; out = (x - mu) / sqrt(var +
 *                bn_eps) + beta
 *   moving mode  the same with the net's moving pair
 *   h0 = BN0(obs);  h1 = relu(BN1(h0 W1 + b1));  h2 = relu(BN2(h1 W2 + b2));  out = h2 W3 + b3;  the head is icnn_be_naf_*'s.
 * theta_l, theta_u, theta_v: the flat vector of icnn_be_naf_* (W1, b1, W2, b2, W3, b3) with beta0 [dimO], beta1 [l1], beta2
 * [l2] behind it; m, v and grad have that layout.  target_v: W and b alone, the flat vector of icnn_be_naf_*.  mv_l, mv_u,
 * mv_v: the moving pairs of a net, 2 S floats: mean0, var0 [dimO each], mean1, var1 [l1], mean2, var2 [l2] (fresh: means 0,
 * variances 1).  The target pass mlp(ob2) reads target_v's W and b with theta_v's betas (naf.py:42-71, the reuse arguments).
 *
 * One step: the four passes (L, U, V at obs, the target at ob2) in batch mode, each on the statistics of its own input; y, the
 * head, td, loss_q = mean td^2 + l2norm sum theta^2 / 2 over the 18 W and b (the betas stay out), its gradient with respect to
 * the W, b and the nine betas (the target under stop_gradient); ONE TF-Adam over the three vectors, the decay term for W and b
 * alone; target_v from the new W and b of V; then the fold  m <- m - (m - batch) (1 - bn_decay)  in float32 of L's and U's pairs
 * once and of V's twice, first with the statistics at obs, then with those at ob2.
 *   icnn_be_naf_bn_chain    forward and backward down to every pre-activation delta and the nine d beta (in grad): 7 launches
 *   icnn_be_naf_bn_grads    the eighteen weight and bias gradients: one launch
 *   icnn_be_naf_bn_update   the update and loss_q: one launch;  no fold
 *   icnn_be_naf_bn_step     chain, grads, update, fold: 10 launches
 *   icnn_be_naf_bn_act      out[batch][dimA] = u(obs) in `mode` (ICNN_BE_BN_BATCH / ICNN_BE_BN_MOVING)
 *   icnn_be_naf_bn_q        out[batch] = q(obs, act) in `mode`
 * act and q go through a workspace of icnn_be_naf_bn_work_bytes(batch, ...) bytes of their own batch; they write nothing
 * of the model.  No entry synchronises; all are capturable; no float atomics: every run gives the same bits.
 *
 * The workspace: 16-byte aligned; icnn_be_naf_bn_work_offsets gives the offset in floats of each piece ICNN_BE_NAF_BN_W_*
 * ([batch][width] float32 unless said otherwise); nothing outside the rows < batch of a piece is written.  A piece "+ p" exists
 * per pass p = 0 (L), 1 (U), 2 (V), 3 (the target at ob2).  step: as icnn_be_naf_*.
 *
 * Sizes: those of icnn_be_naf_* and 1 <= batch <= ICNN_BE_NAF_BN_MAX_BATCH in every entry (a workgroup holds a column of the
 * whole batch); batch 1 is legal: var = 0 and a site's output is beta.  EINVAL as icnn_be_naf_*, also for a mode that is neither,
 * bn_eps <= 0 or bn_decay outside [0, 1], before anything is launched (0 from icnn_be_naf_bn_work_bytes).
 */
#define ICNN_BE_NAF_BN_MAX_BATCH 512
#define ICNN_BE_NAF_BN_PASSES 4
#define ICNN_BE_NAF_BN_VARS 9     /* W1, b1, W2, b2, W3, b3, beta0, beta1, beta2 */
#define ICNN_BE_NAF_BN_W_Y 0      /* the per-sample pieces of icnn_be_naf_*: y, u, l, diag Lm, h, A, q, td */
#define ICNN_BE_NAF_BN_W_U 1
#define ICNN_BE_NAF_BN_W_L 2
#define ICNN_BE_NAF_BN_W_LD 3
#define ICNN_BE_NAF_BN_W_H 4
#define ICNN_BE_NAF_BN_W_ADV 5
#define ICNN_BE_NAF_BN_W_Q 6
#define ICNN_BE_NAF_BN_W_TD 7
#define ICNN_BE_NAF_BN_W_D3 8     /* + p, p < 3: layer 3's delta [dimA^2], [dimA], [1] */
#define ICNN_BE_NAF_BN_W_H0 11    /* + p: BN0's output [dimO] */
#define ICNN_BE_NAF_BN_W_H1 15    /* + p: relu(BN1(.)) [l1] */
#define ICNN_BE_NAF_BN_W_H2 19    /* + p: relu(BN2(.)) [l2] */
#define ICNN_BE_NAF_BN_W_XH1 23   /* + p: the normalised pre-activation of BN1, before beta [l1] */
#define ICNN_BE_NAF_BN_W_XH2 27   /* + p: of BN2 [l2] */
#define ICNN_BE_NAF_BN_W_D1 31    /* + p, p < 3: d loss / d (h0 W1 + b1) [l1] */
#define ICNN_BE_NAF_BN_W_D2 34    /* + p, p < 3: d loss / d (h1 W2 + b2) [l2] */
#define ICNN_BE_NAF_BN_W_STAT 37  /* + p: [2 S] the batch statistics in the layout of mv_* */
#define ICNN_BE_NAF_BN_W_SQ 41    /* float64 [tiles of 16 samples]: each tile's sum of td^2 */
#define ICNN_BE_NAF_BN_W_UPD 42   /* float64: the update's partial sums of theta^2 */
#define ICNN_BE_NAF_BN_WORK_PIECES 43
typedef struct icnn_be_naf_bn_args {
    int batch, dimO, dimA, l1, l2;
    const float *obs;                 /* [batch][dimO] */
    const double *act;                /* [batch][dimA] */
    const float *rew;                 /* [batch] */
    const float *ob2;                 /* [batch][dimO] */
    const unsigned char *term;        /* [batch] */
    float *theta_l, *theta_u, *theta_v, *target_v;      /* separately allocated */
    float *m_l, *v_l, *m_u, *v_u, *m_v, *v_v;           /* Adam's moments */
    float *grad_l, *grad_u, *grad_v;  /* the step's gradients, before the decay term */
    float *mv_l, *mv_u, *mv_v;        /* the moving pairs, [2 S] each */
    int *step;                        /* [ICNN_BE_NAF_STEP_INTS] */
    float *loss;                      /* loss_q of the step */
    void *work;
    double rate, beta1, beta2, bn_decay;
    float eps, tau, discount, l2norm, bn_eps;
} icnn_be_naf_bn_args;                /* icnn_be_struct_size(20) */

/* floats of theta_l (*nl), theta_u (*nu), theta_v (*nv), target_v (*nt) and of one net's moving pairs (*ns = 2 S) */
ICNN_BE_API int icnn_be_naf_bn_param_floats(int dimO, int dimA, int l1, int l2, long long *nl, long long *nu, long long *nv,
                                            long long *nt, long long *ns);
/* off[i]: where variable i (ICNN_BE_NAF_BN_VARS, in the order W1 .. b3, beta0 .. beta2) of net `which` (0 L, 1 U, 2 V) begins */
ICNN_BE_API int icnn_be_naf_bn_layout(int dimO, int dimA, int l1, int l2, int which, long long off[ICNN_BE_NAF_BN_VARS]);
/* 0 for sizes out of range */
ICNN_BE_API size_t icnn_be_naf_bn_work_bytes(int batch, int dimO, int dimA, int l1, int l2);
ICNN_BE_API int icnn_be_naf_bn_work_offsets(int batch, int dimO, int dimA, int l1, int l2,
                                            long long off[ICNN_BE_NAF_BN_WORK_PIECES]);
ICNN_BE_API int icnn_be_naf_bn_chain(const icnn_be_naf_bn_args *a, void *stream);
ICNN_BE_API int icnn_be_naf_bn_grads(const icnn_be_naf_bn_args *a, void *stream);
ICNN_BE_API int icnn_be_naf_bn_update(const icnn_be_naf_bn_args *a, void *stream);
ICNN_BE_API int icnn_be_naf_bn_step(const icnn_be_naf_bn_args *a, void *stream);
ICNN_BE_API int icnn_be_naf_bn_act(int dimO, int dimA, int l1, int l2, const float *theta_u, const float *mv_u, float bn_eps,
                                   int mode, const float *obs, int batch, float *out, void *work, void *stream);
ICNN_BE_API int icnn_be_naf_bn_q(int dimO, int dimA, int l1, int l2, const float *theta_l, const float *theta_u,
                                 const float *theta_v, const float *mv_l, const float *mv_u, const float *mv_v, float bn_eps,
                                 int mode, const float *obs, const double *act, int batch, float *out, void *work, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ICNN_BE_H */
