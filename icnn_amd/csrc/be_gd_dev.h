// The one iterate loop of the gradient solvers on y: K times the model's energy/gradient, then an update rule per element.
// The rule is a template parameter (MomentumRule here: be_gd.hip's recurrence; PgdRule: be_pgd.hip); the loop has three forms:
//     gd_tile_loop    a persistent workgroup per TM-sample tile alternating phase A (the model's energy/gradient tile) and
//                     phase B (the rule, one wave per sample), the state in global memory.  Instantiated by gd_fc_kernel
//                     (be_gd.hip), ficnn_gd_kernel (be_ficnn.hip) and pgd_fc_kernel (be_pgd.hip); a unit that includes this
//                     needs -mllvm -disable-machine-licm (build.py)
//     gd_rows_loop    at most two samples per CU, context rows and state in LDS (be_gd_rows_dev.h)
//     conv_gd_rounds  the conv model's host loop around the rule's elementwise launches
// A rule gives:  Args<FA> (the kernel's arguments: fa, y0, y, n_iter and the rule's own), Elem (one element's state),
// start(a, y0) -> Elem, fed(e) (the float32 the model is fed), result(e) (the float64 left in y), Iter iter(a, u, k) (what a
// wave holds over sample u's elements in iteration k), step(it, e, g, j) (g points at the element's dE/dy, so that the rule
// reads it where its own per-element record allows: the momentum rule behind its trajectory store), wants_final(a),
// load / store (state of element i in global memory), lds_floats(npad) and lds_load / lds_store (a sample's state in LDS),
// ws_state_bytes (workspace bytes per element of state beside y), and `sums`: step returns a float64 term, term(e) is the
// same term of a final evaluation, and lane 0 writes float64(E) + the wave's sum of them to out(a, k, final)[u] unless null.
// A rule that does not sum leaves E of the final evaluation in fa.f, which its host side points at the caller's buffer.
#pragma once
#include "be_picnn_fc_dev.h"

namespace icnn_be {

// The one workspace carving of every entry (byte offsets, each part 256-byte aligned): state_bytes per element of rule
// state (icnn_be_gd_workspace_bytes: 4, the momentum; icnn_be_pgd_workspace_bytes: 0), g and f.  The float32 constants of
// the momentum recurrence.  Both defined in be_gd.hip.
struct GdWorkspace {
    size_t v, g, f, total;
};
GdWorkspace gd_workspace(int batch, int n, size_t state_bytes);
struct GdConstants {
    float lr, mu, c1;      // float32(lr), float32(mu), float32(1.0 + mu)
};
GdConstants gd_constants(double lr, double momentum);

namespace {

// The loop fields of a launch whose a.fa the model has filled (a.fa.n): the caller's buffers, g / f out of the workspace and
// the tile's y / g / f / batch / finished.  a.fa.ctx (and what else the tile reads) stays the caller's.  Returns the base of
// the rule's state in the workspace.
template <typename A>
unsigned char *gd_fill_loop(A &a, const double *y0, double *y_out, int n_iter, void *ws, int batch, size_t state_bytes) {
    const GdWorkspace w = gd_workspace(batch, a.fa.n, state_bytes);
    unsigned char *base = static_cast<unsigned char *>(ws);
    a.y0 = y0; a.y = y_out; a.n_iter = n_iter;
    a.fa.y = y_out; a.fa.batch = batch; a.fa.finished = nullptr;
    a.fa.g = reinterpret_cast<float *>(base + w.g);
    a.fa.f = reinterpret_cast<float *>(base + w.f);
    return base + w.v;
}

// ---- the momentum rule: float32 y and v from y_0 rounded to float32 and v = 0; traj before the step; f_out at the end ----
template <typename FA>     // FA: the arguments of the model's energy/gradient tile (FcArgs, FicnnArgs)
struct GdTileArgs {
    FA fa;                 // fa.y = y (the iterate), fa.g = per-iteration dE/dy, fa.f = f_out or scratch
    const double *y0;      // [B][n] start (float32 values after rounding on entry)
    double *y;             // [B][n] the iterate, y_K on exit (the caller's y_out)
    float *v;              // [B][n] momentum (workspace)
    double *traj;          // [B][K][n] y_0 .. y_{K-1}, or nullptr
    float *f_out;          // [B] E(y_K), or nullptr: no final evaluation
    int n_iter;
    float lr, mu, c1;      // float32(lr), float32(mu), float32(1.0 + mu)
};

template <typename FA>
void gd_fill_args(GdTileArgs<FA> &a, const double *y0, double *y_out, double *traj, float *f_out, int n_iter, double lr,
                  double momentum, void *ws, int batch) {
    const GdConstants c = gd_constants(lr, momentum);
    a.v = reinterpret_cast<float *>(gd_fill_loop(a, y0, y_out, n_iter, ws, batch, sizeof(float)));
    a.traj = traj; a.f_out = f_out;
    a.lr = c.lr; a.mu = c.mu; a.c1 = c.c1;
    if (f_out) a.fa.f = f_out;
}

// One step of the recurrence for one element (shared by every path: the same float32 operations in the same order)
__device__ __forceinline__ void gd_step(float &y, float &v, float g, float lr, float mu, float c1) {
#pragma clang fp contract(off)
    const float mv = mu * v;
    const float vn = mv - lr * g;
    y = (y - mv) + c1 * vn;
    v = vn;
}

#define ICNN_BE_RULE_FN static __device__ __forceinline__
struct MomentumRule {
    template <typename FA> using Args = GdTileArgs<FA>;
    static constexpr bool sums = false;
    static constexpr size_t ws_state_bytes = sizeof(float);
    struct Elem { float y, v; };
    struct Iter { double *traj; float lr, mu, c1; };
    template <typename A> ICNN_BE_RULE_FN Elem start(const A &, double y0) { return {(float)y0, 0.f}; }   // rounded like a feed
    ICNN_BE_RULE_FN float fed(const Elem &e) { return e.y; }
    ICNN_BE_RULE_FN double result(const Elem &e) { return (double)e.y; }
    template <typename A> ICNN_BE_RULE_FN Iter iter(const A &a, int u, int k) {
        return {a.traj ? a.traj + ((size_t)u * a.n_iter + k) * a.fa.n : nullptr, a.lr, a.mu, a.c1};
    }
    ICNN_BE_RULE_FN void step(const Iter &it, Elem &e, const float *g, int j) {
        if (it.traj) it.traj[j] = (double)e.y;
        gd_step(e.y, e.v, *g, it.lr, it.mu, it.c1);      // g read behind the trajectory store
    }
    template <typename A> ICNN_BE_RULE_FN bool wants_final(const A &a) { return a.f_out != nullptr; }
    // global memory: y in the caller's y_out, v in the workspace.  LDS: per sample y[npad] | v[npad]
    template <typename A> ICNN_BE_RULE_FN Elem load(const A &a, size_t i) { return {(float)a.y[i], a.v[i]}; }
    template <typename A> ICNN_BE_RULE_FN void store(const A &a, size_t i, const Elem &e) { a.y[i] = (double)e.y; a.v[i] = e.v; }
    static constexpr int lds_floats(int npad) { return 2 * npad; }
    ICNN_BE_RULE_FN Elem lds_load(const float *s, int npad, int j) { return {s[j], s[npad + j]}; }
    ICNN_BE_RULE_FN void lds_store(float *s, int npad, int j, const Elem &e) { s[j] = e.y; s[npad + j] = e.v; }
};

// ---- the tile form ----
// Phase A reads its arguments from the kernel-argument segment and is inlined into the iteration loop, with the thread
// index read opaquely (thread_id) and -mllvm -disable-machine-licm for the unit: the recipe of be_fused.hip / be_adam.hip.
// Tile::run(fa, tile, lds) is the model's energy/gradient tile, Tile::rows(fa) the samples it holds (TM; the FC-PICNN's narrow
// tiles 8 or 4): tile t owns samples t * rows .. , wave w < rows the w-th of them.
template <typename Tile, typename KArgs>
__device__ __forceinline__ void gd_phase_fg(KArgs *kp, int tile) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    asm volatile("" : "+s"(kp), "+s"(tile));
    Tile::run(kp->fa, tile, lds);
}

// Phase B: wave w updates sample tile * rows + w (g and E from phase A through global memory); final: no update, the summing
// rule's record of the final evaluation alone
template <typename Tile, typename Rule, typename KArgs>
__device__ __forceinline__ void gd_phase_update(KArgs *kp, int tile, int k, bool final) {
#pragma clang fp contract(off)
    asm volatile("" : "+s"(kp), "+s"(tile), "+s"(k));
    const int tid = thread_id(), wave = tid >> 6, lane = tid & 63;
    const int TR = Tile::rows(kp->fa);
    const int n = kp->fa.n, u = tile * TR + wave;
    if (wave >= TR || u >= kp->fa.batch) return;
    const size_t row = (size_t)u * n;
    const typename Rule::Iter it = Rule::iter(*kp, u, k);
    [[maybe_unused]] double part = 0.0;
    for (int j = lane; j < n; j += 64) {
        typename Rule::Elem e = Rule::load(*kp, row + j);
        if constexpr (Rule::sums) {
            if (final) {
                part += Rule::term(e);
                continue;
            }
            part += Rule::step(it, e, &kp->fa.g[row + j], j);
        } else {
            Rule::step(it, e, &kp->fa.g[row + j], j);
        }
        Rule::store(*kp, row + j, e);
    }
    if constexpr (Rule::sums) {
        const double sum = wave_sum(part);
        double *out = Rule::out(*kp, k, final);
        if (out && lane == 0) out[u] = (double)kp->fa.f[u] + sum;
    }
}

// The body of a __global__ __launch_bounds__(NTHREADS) kernel whose only parameter is `a`, one workgroup per tile
template <typename Tile, typename Rule, typename Args>
__device__ __forceinline__ void gd_tile_loop(const Args &a) {
#pragma clang fp contract(off)
    typedef const __attribute__((address_space(4))) Args KArgs;
    KArgs *kp = (KArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int tile = blockIdx.x;
    {
        const int tid = thread_id(), wave = tid >> 6, lane = tid & 63;
        const int TR = Tile::rows(a.fa);
        const int n = a.fa.n, u = tile * TR + wave;
        if (wave < TR && u < a.fa.batch)
            for (int j = lane; j < n; j += 64) {
                const size_t i = (size_t)u * n + j;
                Rule::store(a, i, Rule::start(a, a.y0[i]));
            }
    }
    __syncthreads();
    const int K = a.n_iter;
    for (int k = 0; k < K; ++k) {
        gd_phase_fg<Tile>(kp, tile);
        __syncthreads();                                 // g and E of the tile visible to its update waves
        gd_phase_update<Tile, Rule>(kp, tile, k, false);
        __syncthreads();                                 // y_{k+1} visible to the tile's next phase A
    }
    if (Rule::wants_final(a)) {
        gd_phase_fg<Tile>(kp, tile);                     // E(y_K) -> fa.f
        if constexpr (Rule::sums) {
            __syncthreads();
            gd_phase_update<Tile, Rule>(kp, tile, K, true);
        }
    }
}

// ---- the conv form: init(), then K x (the conv fg launches into f and g, update(k)), then when `final` one more evaluation
// and fin().  The three are the rule's launches. ----
template <typename Init, typename Update, typename Final>
hipError_t conv_gd_rounds(const icnn_be_conv_model &m, const float *ctx, const double *y, int batch, int n_iter, float *f,
                          float *g, bool final, hipStream_t stream, Init init, Update update, Final fin) {
    if (hipError_t e = init(); e != hipSuccess) return e;
    for (int k = 0; k < n_iter; ++k) {
        if (hipError_t e = launch_conv_fg(m, ctx, y, batch, f, g, nullptr, stream); e != hipSuccess) return e;
        if (hipError_t e = update(k); e != hipSuccess) return e;
    }
    if (!final) return hipSuccess;
    if (hipError_t e = launch_conv_fg(m, ctx, y, batch, f, g, nullptr, stream); e != hipSuccess) return e;
    return fin();
}

}  // namespace
}  // namespace icnn_be
