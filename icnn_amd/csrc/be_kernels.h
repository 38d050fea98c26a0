// Internal launch interfaces between the C ABI (be_api.hip) and the kernels, and between the units.  Only what a second
// translation unit calls is declared here: an entry that takes no icnn_be_state, model or context descriptor is defined in
// its own unit (be_api.hip has the rule), and that unit's launchers are file-local.
#pragma once
#include <hip/hip_runtime.h>

#include "be_common.h"
#include "icnn_be.h"

namespace icnn_be {

struct DualArgs {
    icnn_be_state st;
    const void *f;
    const void *g;
    int round;       // launch round: index into st.pending
    int budget;      // Newton updates a sample may spend in this launch; 0 = unlimited
    int n_pad;   // n rounded up to a multiple of 16 (four f64 MFMA k-steps, unrolled)
    int ldA;     // LDS row pitch of the staged bundle, in elements
    int rows;    // bundle rows the LDS staging area holds in this launch (<= round + 1)
    long long *prof;   // optional [B][DUAL_PROF_PHASES] cycle counters (diagnostic), else nullptr
    PairwisePlan plan;
};
constexpr int DUAL_PROF_PHASES = 16;
void set_dual_profile_buffer(long long *buf);
void set_fc_profile_buffer(long long *buf);
void set_conv_profile_buffer(long long *buf);

// Row pitch with pitch % 32 == 2: the MFMA operand gather (16 rows x 2 adjacent
// columns per 32-lane group) then touches 32 distinct LDS banks.
constexpr int dual_row_pitch(int n_pad) {
    int p = n_pad;
    while (p % 32 != 2) ++p;
    return p;
}

// Shape policies of the persistent tile kernel (be_fused.hip) and of the device functions it inlines: where the hot paths
// take their geometry from.  Two policies, one interface.  DynShape reads what the launcher put into the arguments (DualArgs,
// FcArgs): every kernel but the fixed instances.  FixedShape<n, widths...> (be_picnn_fc_dev.h, on top of FixedDual<n> here)
// yields the same quantities as constant expressions, derived by the very functions the launchers fill the arguments with
// (dual_row_pitch, pw_build, fc_geom): the compiler folds them into immediates instead of keeping them live in SGPRs.
struct DynShape {
    static constexpr bool FIXED = false;
    static constexpr int LAYER_UNROLL = 1;                      // the layer loops of fc_fg_tile stay loops
    template <typename A> static __device__ __forceinline__ int n(const A &a) { return a.st.n; }
    template <typename A> static __device__ __forceinline__ int n_pad(const A &a) { return a.n_pad; }
    template <typename A> static __device__ __forceinline__ int ldA(const A &a) { return a.ldA; }
    template <typename A> static __device__ __forceinline__ const auto &plan(const A &a) { return a.plan; }
    template <typename A> static __device__ __forceinline__ const A &fc(const A &a) { return a; }
};
constexpr PairwisePlan pw_plan(int n) {
    PairwisePlan p{};
    pw_build(p, n);
    return p;
}
template <int N>
struct FixedDual {
    static constexpr bool FIXED = true;
    static constexpr int N_ROW = N, N_PAD = (N + 15) & ~15, LDA = dual_row_pitch(N_PAD);
    static constexpr PairwisePlan PLAN = pw_plan(N);
    static_assert(N >= 1 && N <= 128 * PW_MAX_LEAVES / 2, "n beyond the pairwise-sum plan");
    template <typename A> static __device__ __forceinline__ int n(const A &) { return N_ROW; }
    template <typename A> static __device__ __forceinline__ int n_pad(const A &) { return N_PAD; }
    template <typename A> static __device__ __forceinline__ int ldA(const A &) { return LDA; }
    template <typename A> static __device__ __forceinline__ const PairwisePlan &plan(const A &) { return PLAN; }
};

// Per-device launch configuration (a process may drive several GPUs: the caches are keyed by device ordinal and
// guarded by a mutex).  ensure_dynamic_lds raises a kernel's dynamic-LDS limit on the CURRENT device when needed;
// device_cus is the CU count of the current device.
hipError_t ensure_dynamic_lds(const void *kernel, int bytes);
int device_cus();

// Every launch of the library: raise the dynamic-LDS limit beyond the default 48 KB where needed, launch, report.
template <typename... KArgs, typename... Args>
hipError_t launch_kernel(void (*kern)(KArgs...), dim3 grid, dim3 block, int lds, hipStream_t stream, Args... args) {
    if (lds > 48 * 1024)
        if (hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(kern), lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
    return hipGetLastError();
}

// The dual-step arguments of every launcher (dual step, persistent kernels); false: n beyond the pairwise-sum plan
inline bool make_dual_args(DualArgs &a, const icnn_be_state &st, const void *f, const void *g, int round, int budget, int rows,
                           long long *prof) {
    a = DualArgs{};
    a.st = st;
    a.f = f;
    a.g = g;
    a.round = round;
    a.budget = budget;
    a.n_pad = (st.n + 15) & ~15;
    a.ldA = dual_row_pitch(a.n_pad);
    a.rows = rows;
    a.prof = prof;
    return pw_build(a.plan, st.n);
}

int dual_lds_bytes(int n, int slots, int cut_dtype, int variant, int rows = 0);
// most bundle rows (<= slots) whose staging fits the 160 KB of LDS; 0: not even one
int dual_rows_fit(int n, int slots, int cut_dtype, int variant);
size_t scratch_bytes(const icnn_be_state &st);
hipError_t launch_state_init(const icnn_be_state &st, hipStream_t stream);
// The reset of a solve (icnn_be_solve_fc_reset): row u of st.y <- y0[u] ([B][n] float64), or the constant `fill` where y0 is
// NULL, and what launch_state_init writes.  on = 0: the state is reset already (icnn_be_solve_fc; every later launch of a solve).
struct SolveReset {
    int on;
    const double *y0;
    double fill;
};
// st.y <- y0 / fill as its own launch, for the plans whose first launch is not a persistent kernel
hipError_t launch_y_reset(const icnn_be_state &st, const SolveReset &rs, hipStream_t stream);
hipError_t launch_mark_unfinished(const icnn_be_state &st, hipStream_t stream);
hipError_t launch_dual_step(const icnn_be_state &st, int round, int budget, const void *f, const void *g,
                            hipStream_t stream);
// narrow rows (n <= 16), variant RL: four samples per wave, one per 16-lane DPP row (be_dual_small.hip)
bool dual_step_small_fits(const icnn_be_state &st, int budget);
hipError_t launch_dual_step_small(const icnn_be_state &st, int round, const void *f, const void *g, hipStream_t stream);
// Which kernel instance a dual-step launch runs (icnn_be_debug_dual_plan, ICNN_BE_DUAL_PLAN_*): written where the instance is
// picked, from the instance's own template arguments, and the launchers launch from it
struct DualStepPlan {
    int cut, kt, waves, variant, staged, kernel, lds, rows;
};
// the plan of launch_dual_step(st, round, 0, ...), no launch; false: no instance fits
bool plan_dual_step(const icnn_be_state &st, int round, DualStepPlan &p);
void plan_dual_step_small(const icnn_be_state &st, DualStepPlan &p);

hipError_t launch_fast_math(int which, const double *x, double *out, int count, hipStream_t stream);
hipError_t launch_export_active(const icnn_be_state &st, const int *row_offset, void *G_rows, double *ys_rows, double *h_rows,
                                double *lam_rows, hipStream_t stream);
hipError_t launch_implicit_feed(const icnn_be_state &st, const double *y_true, int loss, const int *row_offset,
                                double *fd_y, double *fd_v, double *fd_c, int *fd_sample, hipStream_t stream);

// ---- FC-PICNN energy / gradient --------------------------------------------------
int fc_check_model(const icnn_be_fc_model &m);
// the rows of a model's evaluation tile (icnn_be_fc_model.tile_rows): fc_narrow_model -- 8 or 4, LDS sized for that many;
// fc_tile_rows -- the largest of 16, 8, 4 that fits the LDS (icnn_be_fc_tile_rows), or ICNN_BE_ELIMIT / ICNN_BE_EINVAL
bool fc_narrow_model(const icnn_be_fc_model &m);
int fc_tile_rows(const icnn_be_fc_model &m);
int fc_deal_units(const icnn_be_fc_model &m, int *out, int cap);   // icnn_be_debug_fc_deal
size_t fc_pack_floats(const icnn_be_fc_model &m);
int fc_pack(const icnn_be_fc_model &m, const float *const *w_yu, const float *const *w_zu, float *out);
hipError_t launch_fc_fg(const icnn_be_fc_model &m, const float *ctx, const double *y, int batch,
                        float *f, float *g, const int *finished, hipStream_t stream);

// x-only context producer and clamps (be_context.hip)
int ctx_check(const icnn_be_fc_ctx &c);
int conv_ctx_check(const icnn_be_conv_ctx &c);      // the stage and BatchNorm pointers of every conv entry
size_t ctx_work_floats(const icnn_be_fc_ctx &c, int batch);
// columns of stage i's GEMM and their pitch in w_stage[i]; fc_ctx_u: u_i (i < n_layers - 1) inside `work`, pitch *ld
int ctx_stage_cols(const icnn_be_fc_ctx &c, int i);
int ctx_stage_ld(const icnn_be_fc_ctx &c, int i);
float *fc_ctx_u(const icnn_be_fc_ctx &c, int batch, float *work, int i, int *ld);
// widths of the batch-normalised layers (n[l] = 0: not normalised), ICNN_BE_MAX_LAYERS of them for the FC model, 4 for the conv
void fc_bn_widths(const icnn_be_fc_ctx &c, int *n);
// mv / mode / updates: BatchNorm mode (include/icnn_be.h icnn_be_fc_context_bn, arguments checked by the caller); the
// defaults are icnn_be_fc_context
hipError_t launch_fc_context(const icnn_be_fc_ctx &c, const float *x, int batch, float *ctx, int ctx_width, float *work,
                             hipStream_t stream, const icnn_be_bn_moving *mv = nullptr, int mode = ICNN_BE_BN_BATCH,
                             int updates = 0, const int *updates_dev = nullptr);
size_t ctx_bn_work_floats(const icnn_be_fc_ctx &c, int batch);
// `updates` folds of stat[l] (mean [n[l]] then biased variance [n[l]], device) into mv's layers 0 .. nl-1 (n[l] = 0: none),
// one launch.  updates_dev (device int32, may be NULL) replaces `updates` by a count read on the device; gate_dev (may be
// NULL): no fold when *gate_dev <= 0
hipError_t launch_bn_fold(const icnn_be_bn_moving &mv, float *const *stat, const int *n, int nl, int updates,
                          hipStream_t stream, const int *updates_dev = nullptr, const int *gate_dev = nullptr);
hipError_t launch_fc_context_stage(const icnn_be_fc_ctx &c, int i, const float *x, int batch, float *ctx, int ctx_width,
                                   float *work, hipStream_t stream);
int launch_fc_context_sums(const icnn_be_fc_ctx &c, int i, int batch, float *work, double *stats, hipStream_t stream,
                           hipError_t &err);
hipError_t launch_fc_context_norm(const icnn_be_fc_ctx &c, int i, int batch, double batch_total, const double *stats,
                                  float *work, hipStream_t stream);
hipError_t launch_clamp(float *w, size_t count, int mode, hipStream_t stream);
hipError_t launch_fc_clamp(const icnn_be_fc_model &m, int mode, hipStream_t stream);
// conv PICNN: geometry of the u-path / heads and the context row layout (filled by conv_ctx_shape, be_picnn_conv.hip)
struct ConvCtxShape {
    int H, W, F[3], K[3], S[3], pad[3], oh[3], ow[3], P[3];   // P = oh * ow
    int flat, fch, ctx_width;
    int c_yu[3], c_zu[3], c_gate[5], c_zu3, c_zu4;            // column offsets inside a context row
};
int conv_ctx_shape(const icnn_be_conv_model &m, ConvCtxShape &g);
size_t conv_ctx_work_floats(const ConvCtxShape &g, int batch);
hipError_t launch_conv_context(const ConvCtxShape &g, const icnn_be_conv_ctx &c, const float *x, int batch, float *ctx,
                               float *work, hipStream_t stream, const icnn_be_bn_moving *mv = nullptr,
                               int mode = ICNN_BE_BN_BATCH, int updates = 0, const int *updates_dev = nullptr);
size_t conv_ctx_bn_work_floats(const ConvCtxShape &g, int batch);
// one stage's GEMM of launch_conv_context (u-maps ReLU'd but not normalised); conv_ctx_u: u_l (l = 0..3) inside `work`
hipError_t launch_conv_context_stage(const ConvCtxShape &g, const icnn_be_conv_ctx &c, int stage, const float *x, int batch,
                                     float *ctx, float *work, hipStream_t stream);
float *conv_ctx_u(const ConvCtxShape &g, int batch, float *work, int l);
void conv_bn_widths(const ConvCtxShape &g, int *n);
hipError_t launch_conv_clamp(const icnn_be_conv_model &m, int mode, hipStream_t stream);

// training gradient of the FC PICNN (be_train_fc.hip): sizes (0 = shape rejected), shape check, launcher
size_t fc_grad_floats(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c);
// dev: the size of the device-count variant (rows_dev != NULL), whose forward products keep partials for any plan
size_t fc_surrogate_work_floats(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c, int batch, int rows, bool dev = false);
int fc_surrogate_shape(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c, int batch, int rows, bool with_v);
hipError_t launch_fc_surrogate_grad(const icnn_be_fc_model &m, const icnn_be_fc_ctx &c, const float *x, int batch,
                                    const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                    float *grad, float *F_rows, float *work, hipStream_t stream,
                                    const icnn_be_bn_moving *mv = nullptr, int updates = 0, const int *rows_dev = nullptr);
// shared by both training units (be_train_common.hip).  The strided f32-MFMA GEMM: C[M][N] (pitch ldc) = A B,
// A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn], split-K into `part` (tr_gemm_part_floats(M, N, K) floats) and summed
// in split order -- no atomics
// rows_dev (device int32, may be NULL) with m_per_row: the split-K plan of the product with m_per_row x *rows_dev rows is
// formed on the device (the bits of the compact call on the rows both share); part then holds tr_gemm_part_floats(M, N, K, true)
size_t tr_gemm_part_floats(int M, int N, int K, bool dev_plan = false);
hipError_t launch_tr_gemm(const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, int M, int N,
                          int K, float *C, long long ldc, float *part, hipStream_t stream, const int *rows_dev = nullptr,
                          int m_per_row = 0);
// the feed's rows: samp[r] = the sample of row r, mult[j] = the row count of sample j (a float); out [B][C] = the rows
// [R][C] of each sample summed in row order
hipError_t launch_tr_rows(const int *row_offset, int B, int R, int *samp, float *mult, hipStream_t stream);
hipError_t launch_tr_segment_sum(const float *rows, const int *row_offset, int B, int R, int C, float *out, hipStream_t stream);
// dst [(n + wprev)][w] = [ Wy ; Wz ] row-major out of the packed forward fragments at wpack + yf and wpack + zf (last: the
// width-1 head's plain vectors); count floats of zero (a kernel: a captured step keeps its node types); out[col] = the sum
// over the B rows of m[.][c0 + col] (pitch ld), rows in order
hipError_t launch_tr_unpack(const float *wpack, long long yf, long long zf, int n, int wprev, int w, bool last, float *dst,
                            hipStream_t stream);
hipError_t launch_tr_zero(float *p, size_t count, hipStream_t stream);
hipError_t launch_tr_colsum(const float *m, int ld, int B, int c0, int N, float *out, hipStream_t stream);

// training gradient of the conv PICNN (be_train_conv.hip), as the FC one above
size_t conv_grad_floats(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c);
size_t conv_surrogate_work_floats(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c, int batch, int rows, bool dev = false);
int conv_surrogate_shape(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c, int batch, int rows, bool with_v);
hipError_t launch_conv_surrogate_grad(const icnn_be_conv_model &m, const icnn_be_conv_ctx &c, const float *x, int batch,
                                      const int *row_offset, int rows, const double *y, const double *v, const double *cvec,
                                      float *grad, float *F_rows, float *work, hipStream_t stream,
                                      const icnn_be_bn_moving *mv = nullptr, int updates = 0, const int *rows_dev = nullptr);

// LDS layouts of the persistent kernels (be_fused.hip), host arithmetic only.  false: the shape does not fit that kernel.
// The solve plan (be_api.hip) and the launchers below take their fit decisions from these two functions alone.
struct FusedTileLayout {
    int lds, crow_off, sample_bytes;
    int grouped, group_cap, need_off;   // the dual phase in groups of samples whose bundles fit together (FusedArgs)
};
// per-tile solve, tile_rows samples per workgroup (4, 8 or 16); budget: Newton updates a sample may spend per round before
// it is parked (<= 0: unlimited, lockstep inside the tile)
bool fused_tile_layout(const icnn_be_fc_model &m, const icnn_be_state &st, int tile_rows, int budget, FusedTileLayout &out);
struct FusedRowsLayout {
    int lds, dual_off, sample_bytes, crow_off;
};
// per-sample solve, per_wg (1..4) samples per workgroup; resume: the finishing launch after budgeted rounds
bool fused_rows_layout(const icnn_be_fc_model &m, const icnn_be_state &st, int per_wg, bool resume, FusedRowsLayout &out);
// hipErrorInvalidValue: a shape the layout functions refuse (the plan never sends one)
// reset.on: every sample's owner (wave w of a tile; the waves below the workgroup's sample count) writes its y row and control
// words in front of round 0 -- the first launch of a solve only, never a `resume` or a budgeted launch
hipError_t launch_fused_fc_solve(const icnn_be_fc_model &m, const float *ctx, const icnn_be_state &st, float *f_work,
                                 float *g_work, long long *dual_prof, hipStream_t stream, int tile_rows, int budget,
                                 const SolveReset &reset = SolveReset{});
// value (icnn_be_rl_bundle_solve; variant RL, never with resume): behind the last round every sample of the workgroup is
// evaluated once more at its st.y: act[u][j] = 2 y[u][j] - 1 (float64 [B][n]) and q[u] = its energy (float32 [B], may be null)
struct RowsValue {
    double *act;
    float *q;
};
hipError_t launch_fused_rows_solve(const icnn_be_fc_model &m, const float *ctx, const icnn_be_state &st, float *f_work,
                                   float *g_work, int per_wg, long long *dual_prof, hipStream_t stream, bool resume,
                                   const SolveReset &reset = SolveReset{}, const RowsValue *value = nullptr);
// ICNN_BE_SHAPE_*: the instance of the persistent tile kernel launch_fused_fc_solve takes for these arguments (host arithmetic)
int fused_shape_instance(const icnn_be_fc_model &m, const icnn_be_state &st, int tile_rows, int budget);
// icnn_be_debug_dual_step_body: round `round` of a dual body that only the tile kernel's Bibsonomy instances contain, on its own
// (which: 1 the 16-slot body, 2 the same capped at the round class, 3 the 32-slot body; rows_mode: 0 rows_cap from the round, 1
// from the cuts each sample holds).  hipErrorInvalidValue, nothing launched: what the entry's contract in icnn_be.h refuses
hipError_t launch_dual_body_probe(const icnn_be_state &st, int round, const void *f, const void *g, int which, int rows_mode,
                                  hipStream_t stream);
int dual_waves(int n, int cut_dtype, int variant);
long long *dual_profile_buffer();
void set_dual_trace_buffer(long long *buf);
long long *dual_trace_buffer();
constexpr int DUAL_TRACE_WORDS = 4;     // per (sample, round): phase start, dual step start, dual step end, Newton updates so far
long long *fc_profile_buffer();

// Adam inner optimiser of the RL agent, whole loop in one launch (be_adam.hip); hipErrorNotSupported = the batch
// has more tiles than a cooperative launch keeps resident
size_t adam_workspace_bytes(int batch, int n);
hipError_t launch_adam_fc(const icnn_be_fc_model &m, const float *ctx, int batch, int max_iter, double *act_best,
                          float *f_best, int *iters, void *workspace, hipStream_t stream,
                          const icnn_be_fc_ctx *cx = nullptr, const float *obs = nullptr, bool each = false);
// The launch of launch_adam_fc for a model and a batch (icnn_be_debug_adam_plan); launch_adam_fc launches from exactly this.
// With `cx`, obs_ok: the observation form is accepted (else hipErrorNotSupported).  Enqueues nothing.
struct AdamPlan {
    int kernel;        // ICNN_BE_ADAM_ROWS, ICNN_BE_ADAM_TILE, or ICNN_BE_ADAM_NONE: hipErrorNotSupported
    int per_wg;        // states per workgroup
    int workgroups;
    int cooperative;   // several workgroups: all resident, the stopping rule's sum goes through a grid exchange
    int obs_ok;
};
// `each`: the stopping rule per state (icnn_be_adam_fc_each): iters is [batch], no workgroup waits for another, never cooperative.
hipError_t adam_fc_plan(const icnn_be_fc_model &m, const icnn_be_fc_ctx *cx, int batch, AdamPlan &plan, bool each = false);

// Unrolled momentum gradient descent on y (be_gd.hip): the FC form is one launch (persistent tiles or the per-sample rows
// path), the conv form 1 + K (+1) rounds of launches.  hipErrorNotSupported: the model's tile does not fit the LDS.
size_t gd_workspace_bytes(int batch, int n);
bool gd_constants_ok(double lr, double momentum);     // lr, momentum and their float32 constants finite
hipError_t launch_fc_gd(const icnn_be_fc_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                        double momentum, double *y_out, double *traj, float *f_out, void *workspace, hipStream_t stream);
hipError_t launch_conv_gd(const icnn_be_conv_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                          double momentum, double *y_out, double *traj, float *f_out, void *workspace, hipStream_t stream);
// Projected gradient descent on E - H(y), the objective's traces and the bundle's lower bound (be_pgd.hip): the forms and the
// dispatch rule of the GD launchers above.  obj [K][B] and obj_final [B] may be NULL.
size_t pgd_workspace_bytes(int batch, int n);
bool pgd_constants_ok(double lr, double lo, double hi);   // lr finite, 0 < float32(lo), float32(hi) < 1, lo < hi
hipError_t launch_fc_pgd(const icnn_be_fc_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                         double lo, double hi, double *y_out, double *obj, double *obj_final, void *workspace,
                         hipStream_t stream);
hipError_t launch_conv_pgd(const icnn_be_conv_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                           double lo, double hi, double *y_out, double *obj, double *obj_final, void *workspace,
                           hipStream_t stream);
hipError_t launch_bundle_trace(const icnn_be_state &st, double *obj, int *calls, hipStream_t stream);
hipError_t launch_dual_bound(const icnn_be_state &st, double *out, hipStream_t stream);
// ---- FICNN (be_ficnn.hip: context, energy / gradient, GD; be_train_ficnn.hip: training gradient) ----
int ficnn_check_model(const icnn_be_ficnn_model &m);
size_t ficnn_pack_floats(const icnn_be_ficnn_model &m);
int ficnn_pack(const icnn_be_ficnn_model &m, const float *const *w_x, const float *const *b, const float *const *w_z, float *out);
size_t ficnn_context_work_floats(const icnn_be_ficnn_model &m, int batch);
hipError_t launch_ficnn_context(const icnn_be_ficnn_model &m, const float *x, int batch, float *ctx, float *work,
                                hipStream_t stream);
hipError_t launch_ficnn_fg(const icnn_be_ficnn_model &m, const float *ctx, const double *y, int batch, float *f, float *g,
                           const int *finished, hipStream_t stream);
hipError_t launch_ficnn_gd(const icnn_be_ficnn_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                           double momentum, double *y_out, double *traj, float *f_out, void *workspace, hipStream_t stream);
size_t ficnn_grad_floats(const icnn_be_ficnn_model &m);
size_t ficnn_surrogate_work_floats(const icnn_be_ficnn_model &m, int batch, int rows);
int ficnn_surrogate_shape(const icnn_be_ficnn_model &m, int batch, int rows, bool with_v);
hipError_t launch_ficnn_surrogate_grad(const icnn_be_ficnn_model &m, const float *x, int batch, const int *row_offset, int rows,
                                       const double *y, const double *v, const double *cvec, float *grad, float *F_rows,
                                       float *work, hipStream_t stream);
// ---- conv PICNN energy / gradient -------------------------------------------------
int conv_check_model(const icnn_be_conv_model &m);
// where the raw single-channel pieces and the forward MFMA operands of the convex weights sit inside wpack (floats)
struct ConvPackOffsets {
    long long w_yu[3], w_yr[2], b_yr[2], w_fc4, p_l2, p_l3, p_fc3;
};
int conv_pack_offsets(const icnn_be_conv_model &m, ConvPackOffsets &o);
size_t conv_pack_floats(const icnn_be_conv_model &m);
size_t conv_work_floats(const icnn_be_conv_model &m, int batch);
int conv_pack(const icnn_be_conv_model &m, const float *const *w_yu, const float *const *w_yr,
              const float *const *b_yr, const float *const *w_zu, const float *w_fc3, const float *w_fc4,
              float *out);
hipError_t launch_conv_fg(const icnn_be_conv_model &m, const float *ctx, const double *y, int batch, float *f,
                          float *g, const int *skip, hipStream_t stream);

// ---- the bundle-entropy training step's feed plan (be_train_bundle.hip) ------------
struct FeedPlanLaunch {
    icnn_be_state st;
    const double *y_true;
    int loss;
    int *row_offset, *counts;     // [B + 1]; counts[3] = rows, fg evaluations, OR of the status words
    double *loss_out;
    int *tallies;                 // [B][3] tp / fp / fn (cross entropy; may be NULL)
    void *work;                   // icnn_be_feed_plan_work_bytes(B)
};
hipError_t launch_feed_plan(const FeedPlanLaunch &l, hipStream_t stream);

// ---- parameter update (be_train_update.hip): the workgroups of an n-element update, which the table update of
// be_train_table.hip and its callers size their partial sums by
long long param_update_blocks(long long n);

// ---- what the RL units call of one another ------------------------------------------------
// the sizes every icnn_be_ddpg_* / icnn_be_naf_* entry accepts: the limits of include/icnn_be.h and the chain kernel's LDS
bool ddpg_sizes_ok(int dimO, int dimA, int l1, int l2);
bool naf_sizes_ok(int dimO, int dimA, int l1, int l2);
// pi(obs) (critic false, act NULL) or Q(obs, act) of DDPG's nets for B rows; icnn_be_naf_act runs NAF's U net through it
hipError_t launch_ddpg_forward(bool critic, int dimO, int dimA, int l1, int l2, const float *theta, const float *obs,
                               const double *act, int B, float *out, hipStream_t stream);

}  // namespace icnn_be
