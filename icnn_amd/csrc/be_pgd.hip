// Projected gradient descent on the entropy-scaled objective E(x, y) - H(y) of a PICNN, and the objective's traces and lower
// bound.  The reference's solver comparison (multi-label-cls/ebundle-vs-gd.py:110-132,
// completion/ebundle-iter.py:115-139) runs bamos_opt.pgd.solve_batch with minIter == maxIter on this objective; that module is
// not part of the reference tree, so the iteration is DEFINED here (parity unpinned): from y_0 = clip(y0, lo, hi), for
// k = 0 .. K-1
//     yf      = float64(float32(y_k))                                   what the float32 energy is fed
//     E, g    = the model's float32 energy and dE/dy at yf
//     e_k     = float64(E) + sum_j [ yf log yf + (1 - yf) log(1 - yf) ]  float64; a NaN term counts 0 (the scripts' entr())
//     G_k     = (float64(g) + log yf) - log(1 - yf)
//     y_{k+1} = min(max(y_k - lr G_k, lo), hi)                          float64, no contraction
// K iterations always (no stopping rule), no coupling between samples.  This unit is the iterate loop of be_gd_dev.h with
// PgdRule, in the three forms and under the dispatch rule that be_gd.hip gives the momentum rule:
//     pgd_fc_kernel     gd_tile_loop around fc_fg_tile: y in the caller's y_out, g and E in the workspace
//     pgd_rows_kernel   gd_rows_loop (be_gd_rows_dev.h): at most two samples per CU, context rows and the float64 iterate in LDS
//     pgd_init_kernel / pgd_conv_update_kernel / pgd_conv_final_kernel   the conv model's launches inside conv_gd_rounds: a
//                       workgroup per sample doing the update and e_k
// A sample's entropy sum is formed in an order that depends on n alone (lane-strided partials in index order, then a fixed
// butterfly; the conv form: thread-strided partials and a fixed tree), so e_k has the same bits whatever the batch.
// Beside the loop: entropy_objective_kernel (E - H(y) of given E and y), bundle_trace_kernel (the objective per iteration of
// a finished fused solve, the device form of bundle_entropy._replay_callbacks) and dual_bound_kernel (the bundle's lower
// bound of min_y E - H).
#include <cmath>

#include "be_api_check.h"
#include "be_kernels.h"
#include "be_gd_rows_dev.h"

namespace icnn_be {

namespace {

// y log y + (1 - y) log(1 - y) of one element; the scripts' entr() zeroes an element whose term is NaN (0 log 0 at y = 0 and
// y = 1, and every y outside [0, 1])
__device__ __forceinline__ double entr_term(double y, double ly, double l1) {
#pragma clang fp contract(off)
    const double om = 1.0 - y;
    const double t = y * ly + om * l1;
    return t != t ? 0.0 : t;
}

// One element of the update: the entropy term of e_k (returned) and y <- y_{k+1}
__device__ __forceinline__ double pgd_step(double &y, float g, double lr, double lo, double hi) {
#pragma clang fp contract(off)
    const double yf = (double)(float)y;
    const double ly = log(yf), l1 = log(1.0 - yf);
    const double G = ((double)g + ly) - l1;
    const double step = lr * G;
    y = fmin(fmax(y - step, lo), hi);
    return entr_term(yf, ly, l1);
}

// the entropy term alone, at float64(float32(y)) (round32) or at y itself
__device__ __forceinline__ double entr_at(double y, bool round32) {
    const double yf = round32 ? (double)(float)y : y;
    return entr_term(yf, log(yf), log(1.0 - yf));
}

__device__ __forceinline__ double clip(double y, double lo, double hi) { return fmin(fmax(y, lo), hi); }

// ---- the PGD rule: a float64 y from clip(y0); e_k = float64(E) + the wave's sum of the entropy terms per iteration, e_K
// from the final evaluation ----
template <typename FA>
struct PgdTileArgs {
    FA fa;                 // fa.y = y (the iterate), fa.g = per-iteration dE/dy, fa.f = per-iteration E
    const double *y0;      // [B][n] start
    double *y;             // [B][n] the iterate, y_K on exit (the caller's y_out)
    double *obj;           // [K][B] e_k, or nullptr
    double *obj_final;     // [B] e_K, or nullptr: no final evaluation
    int n_iter;
    double lr, lo, hi;
};
typedef PgdTileArgs<FcArgs> PgdArgs;

struct PgdRule {
    template <typename FA> using Args = PgdTileArgs<FA>;
    static constexpr bool sums = true;
    static constexpr size_t ws_state_bytes = 0;
    typedef double Elem;
    struct Iter { double lr, lo, hi; };
    template <typename A> ICNN_BE_RULE_FN Elem start(const A &a, double y0) { return clip(y0, a.lo, a.hi); }
    ICNN_BE_RULE_FN float fed(Elem y) { return (float)y; }
    ICNN_BE_RULE_FN double result(Elem y) { return y; }
    template <typename A> ICNN_BE_RULE_FN Iter iter(const A &a, int, int) { return {a.lr, a.lo, a.hi}; }
    ICNN_BE_RULE_FN double step(const Iter &it, Elem &y, const float *g, int) { return pgd_step(y, *g, it.lr, it.lo, it.hi); }
    ICNN_BE_RULE_FN double term(Elem y) { return entr_at(y, true); }
    template <typename A> ICNN_BE_RULE_FN bool wants_final(const A &a) { return a.obj_final != nullptr; }
    template <typename A> ICNN_BE_RULE_FN double *out(const A &a, int k, bool final) {
        return final ? a.obj_final : (a.obj ? a.obj + (size_t)k * a.fa.batch : nullptr);
    }
    // global memory: the caller's y_out.  LDS: per sample y[npad] in float64 (the rows layout ends 16-byte aligned)
    template <typename A> ICNN_BE_RULE_FN Elem load(const A &a, size_t i) { return a.y[i]; }
    template <typename A> ICNN_BE_RULE_FN void store(const A &a, size_t i, Elem y) { a.y[i] = y; }
    static constexpr int lds_floats(int npad) { return 2 * npad; }
    ICNN_BE_RULE_FN Elem lds_load(const float *s, int, int j) { return reinterpret_cast<const double *>(s)[j]; }
    ICNN_BE_RULE_FN void lds_store(float *s, int, int j, Elem y) { reinterpret_cast<double *>(s)[j] = y; }
};

__global__ __launch_bounds__(NTHREADS) void pgd_fc_kernel(PgdArgs a) { gd_tile_loop<FcTile, PgdRule>(a); }

__global__ __launch_bounds__(RTHREADS) void pgd_rows_kernel(GdRowsArgs<PgdRule> r) { gd_rows_loop(r); }

// ---- conv model: elementwise start, and a workgroup per sample for the update around the conv fg launches ----
constexpr int CTHREADS = 256;

__global__ void pgd_init_kernel(const double *y0, double *y, size_t count, double lo, double hi) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    y[i] = clip(y0[i], lo, hi);
}

__global__ __launch_bounds__(CTHREADS) void pgd_conv_update_kernel(double *y, const float *g, const float *f, double *obj_k,
                                                                   int n, double lr, double lo, double hi) {
#pragma clang fp contract(off)
    __shared__ double red[CTHREADS];
    const int u = blockIdx.x;
    const size_t row = (size_t)u * n;
    double part = 0.0;
    for (int j = threadIdx.x; j < n; j += CTHREADS) {
        double yj = y[row + j];
        part += pgd_step(yj, g[row + j], lr, lo, hi);
        y[row + j] = yj;
    }
    const double ent = block_tree_sum<CTHREADS>(part, red);
    if (obj_k && threadIdx.x == 0) obj_k[u] = (double)f[u] + ent;
}

// the conv form's e_K: the entropy sum in the update kernel's order
__global__ __launch_bounds__(CTHREADS) void pgd_conv_final_kernel(const double *y, const float *f, double *out, int n) {
#pragma clang fp contract(off)
    __shared__ double red[CTHREADS];
    const int u = blockIdx.x;
    const size_t row = (size_t)u * n;
    double part = 0.0;
    for (int j = threadIdx.x; j < n; j += CTHREADS) part += entr_at(y[row + j], true);
    const double ent = block_tree_sum<CTHREADS>(part, red);
    if (threadIdx.x == 0) out[u] = (double)f[u] + ent;
}

// ---- out[u] = float64(E[u]) - H(y[u]) of a given E and y: a wave per sample ----
constexpr int OTHREADS = 256, OWAVES = OTHREADS / 64;

__global__ __launch_bounds__(OTHREADS) void entropy_objective_kernel(const float *E, const double *y, int batch, int n,
                                                                     double *out) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.x * OWAVES + wave;
    if (u >= batch) return;
    const double *yu = y + (size_t)u * n;
    double part = 0.0;
    for (int j = lane; j < n; j += 64) part += entr_at(yu[j], false);
    const double ent = wave_sum(part);
    if (lane == 0) out[u] = (double)E[u] + ent;
}

// ---- the objective per iteration of a finished fused solve (variants dual and pdipm) ----
// What bundle_entropy._replay_callbacks reconstructs on the host, for one sample: slots 0 .. filled-1 hold the sample's
// evaluations; a sample that finished WITHOUT moving (rank test, error) holds the cut of its last iteration in slot t_next.
struct TraceRow {
    int filled;            // slots that hold evaluations of this sample
    int left_at;           // the iteration in which it left the loop (T - 1: it never did)
};
__device__ __forceinline__ TraceRow trace_row(const icnn_be_state &st, int u, int lane) {
    const int T = st.slots, n = st.n;
    const int fin = st.finished[u] != 0, tn = st.t_next[u];
    int at_cut = 0;
    if (fin && tn < T) {
        const double *cut = st.ys + ((size_t)u * T + (tn < 0 ? 0 : tn)) * n, *yf = st.y + (size_t)u * n;
        int same = 1;
        for (int j = lane; j < n; j += 64) same &= cut[j] == yf[j];
        at_cut = __all(same);
    }
    TraceRow r;
    r.filled = at_cut ? tn + 1 : tn;
    r.filled = r.filled < 0 ? 0 : (r.filled > T ? T : r.filled);
    r.left_at = fin ? r.filled - 1 : T - 1;
    return r;
}

__global__ void trace_zero_kernel(int *calls) { *calls = 0; }

// calls = 1 + the iteration in which the last sample left the loop (T while any sample is unfinished): a wave per sample
__global__ __launch_bounds__(OTHREADS) void trace_calls_kernel(icnn_be_state st, int *calls) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.x * OWAVES + wave;
    if (u >= st.batch) return;
    const TraceRow r = trace_row(st, u, lane);
    if (lane == 0) atomicMax(calls, r.left_at + 1);
}

// obj[t][u] = f_t(u) - H(x_t(u)) for t < calls, NaN beyond: a wave per (sample, iteration)
__global__ __launch_bounds__(OTHREADS) void bundle_trace_kernel(icnn_be_state st, const int *calls, double *obj) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.x * OWAVES + wave, t = blockIdx.y;
    if (u >= st.batch) return;
    const int T = st.slots, n = st.n;
    double *out = obj + (size_t)t * st.batch + u;
    if (t >= *calls) {
        if (lane == 0) *out = __builtin_nan("");
        return;
    }
    const TraceRow r = trace_row(st, u, lane);
    const bool have = t < r.filled;
    const int last = r.filled - 1 < 0 ? 0 : r.filled - 1;
    const int slot = t < last ? t : last;
    // a sample that has left the loop keeps its iterate and its last energy
    const double *x = have ? st.ys + ((size_t)u * T + slot) * n : st.y + (size_t)u * n;
    double part = 0.0;
    for (int j = lane; j < n; j += 64) part += entr_at(x[j], false);
    const double ent = wave_sum(part);
    if (lane == 0) *out = st.fvals[(size_t)u * T + slot] + ent;
}

// ---- d[u] = lam . h - sum_j softplus(-a_j), a = G^T lam over the sample's active cuts: a wave per sample ----
__device__ __forceinline__ double softplus_stable(double x) {
#pragma clang fp contract(off)
    return fmax(x, 0.0) + log1p(exp(-fabs(x)));
}

template <typename CutT>
__global__ __launch_bounds__(OTHREADS) void dual_bound_kernel(icnn_be_state st, double *out) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.x * OWAVES + wave;
    if (u >= st.batch) return;
    const int T = st.slots, n = st.n;
    int cnt = st.count[u];
    cnt = cnt < 0 ? 0 : (cnt > T ? T : cnt);
    if (cnt == 0) {                                      // no cut, no multipliers: no bound
        if (lane == 0) out[u] = -__builtin_inf();
        return;
    }
    const int *act = st.active + (size_t)u * T;
    const double *lam = st.lam + (size_t)u * T, *h = st.h + (size_t)u * T;
    const CutT *G = static_cast<const CutT *>(st.G) + (size_t)u * T * n;
    double lh = 0.0;
    for (int i = 0; i < cnt; ++i) {
        const int s = act[i];
        if (s < 0 || s >= T) continue;
        lh += lam[i] * h[s];
    }
    double part = 0.0;
    for (int j = lane; j < n; j += 64) {
        double aj = 0.0;
        for (int i = 0; i < cnt; ++i) {
            const int s = act[i];
            if (s < 0 || s >= T) continue;
            aj += (double)G[(size_t)s * n + j] * lam[i];
        }
        part += softplus_stable(-aj);
    }
    const double sp = wave_sum(part);
    if (lane == 0) out[u] = lh - sp;
}

}  // namespace

size_t pgd_workspace_bytes(int batch, int n) { return gd_workspace(batch, n, PgdRule::ws_state_bytes).total; }

bool pgd_constants_ok(double lr, double lo, double hi) {
    return std::isfinite(lr) && 0.f < (float)lo && (float)hi < 1.f && lo < hi;
}

hipError_t launch_fc_pgd(const icnn_be_fc_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                         double lo, double hi, double *y_out, double *obj, double *obj_final, void *ws, hipStream_t stream) {
    PgdArgs a{};
    int lds = 0;
    if (fill_args(m, a.fa, lds) != 0) return hipErrorInvalidValue;
    gd_fill_loop(a, y0, y_out, n_iter, ws, batch, PgdRule::ws_state_bytes);
    a.obj = obj; a.obj_final = obj_final;
    a.lr = lr; a.lo = lo; a.hi = hi;
    a.fa.ctx = ctx; a.fa.prof = fc_profile_buffer();
    return launch_fc_gd_rule<PgdRule>(m, a, batch, lds, pgd_fc_kernel, pgd_rows_kernel, stream);
}

hipError_t launch_conv_pgd(const icnn_be_conv_model &m, const float *ctx, const double *y0, int batch, int n_iter, double lr,
                           double lo, double hi, double *y_out, double *obj, double *obj_final, void *ws,
                           hipStream_t stream) {
    const int n = m.H * m.W;
    const GdWorkspace w = gd_workspace(batch, n, PgdRule::ws_state_bytes);
    unsigned char *base = static_cast<unsigned char *>(ws);
    float *g = reinterpret_cast<float *>(base + w.g), *f = reinterpret_cast<float *>(base + w.f);
    const size_t count = (size_t)batch * n;
    const dim3 grid((unsigned)((count + CTHREADS - 1) / CTHREADS));
    return conv_gd_rounds(
        m, ctx, y_out, batch, n_iter, f, g, obj_final != nullptr, stream,
        [&] { return launch_kernel(pgd_init_kernel, grid, dim3(CTHREADS), 0, stream, y0, y_out, count, lo, hi); },
        [&](int k) {
            return launch_kernel(pgd_conv_update_kernel, dim3(batch), dim3(CTHREADS), 0, stream, y_out, (const float *)g,
                                 (const float *)f, obj ? obj + (size_t)k * batch : nullptr, n, lr, lo, hi);
        },
        [&] {
            return launch_kernel(pgd_conv_final_kernel, dim3(batch), dim3(CTHREADS), 0, stream, (const double *)y_out,
                                 (const float *)f, obj_final, n);
        });
}

hipError_t launch_bundle_trace(const icnn_be_state &st, double *obj, int *calls, hipStream_t stream) {
    const dim3 grid((st.batch + OWAVES - 1) / OWAVES);
    if (hipError_t e = launch_kernel(trace_zero_kernel, dim3(1), dim3(1), 0, stream, calls); e != hipSuccess) return e;
    if (hipError_t e = launch_kernel(trace_calls_kernel, grid, dim3(OTHREADS), 0, stream, st, calls); e != hipSuccess) return e;
    return launch_kernel(bundle_trace_kernel, dim3(grid.x, st.slots), dim3(OTHREADS), 0, stream, st, (const int *)calls, obj);
}

hipError_t launch_dual_bound(const icnn_be_state &st, double *out, hipStream_t stream) {
    const dim3 grid((st.batch + OWAVES - 1) / OWAVES);
    if (st.cut_dtype == ICNN_BE_CUT_F64)
        return launch_kernel(dual_bound_kernel<double>, grid, dim3(OTHREADS), 0, stream, st, out);
    return launch_kernel(dual_bound_kernel<float>, grid, dim3(OTHREADS), 0, stream, st, out);
}

}  // namespace icnn_be

using namespace icnn_be;

extern "C" {

int icnn_be_entropy_objective(const float *E, const double *y, int batch, int n, double *out, void *stream) {
    if (!E || !y || !out || batch < 0 || n < 1) return ICNN_BE_EINVAL;
    if (batch == 0) return 0;
    return api_done(launch_kernel(entropy_objective_kernel, dim3((batch + OWAVES - 1) / OWAVES), dim3(OTHREADS), 0,
                                  static_cast<hipStream_t>(stream), E, y, batch, n, out));
}

}  // extern "C"
