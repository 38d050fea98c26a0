// Dual step for narrow rows (n <= 16, variant RL): four samples per wave64 (device code: be_dual_small_dev.h).
#include "be_dual_small_dev.h"

namespace icnn_be {

namespace {

template <typename CutT, int KS>
__global__ __launch_bounds__(256) void dual_step_small_kernel(SmallArgs a) {
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    dual_step_quad_rl<CutT, KS>(a, 4 * wave, 4, a.round);
}

}  // namespace

bool dual_step_small_fits(const icnn_be_state &st, int budget) {
    return st.variant == ICNN_BE_VARIANT_RL && st.n <= 16 && st.slots <= 15 && (st.iters == 0 || st.iters == st.slots) && budget == 0 &&
           // time-sliced solves park samples mid-Newton (st.phase, st.park): the quad kernel restarts a solve from scratch, so
           // the finishing rounds of such a solve stay with the wave-per-sample kernel that honours the parked state
           !(st.flags & (ICNN_BE_FLAG_WAVE_PER_SAMPLE | ICNN_BE_FLAG_TIME_SLICE)) && dual_profile_buffer() == nullptr;
}

namespace {
typedef void (*SmallKernel)(SmallArgs);
struct SmallStepLaunch : DualStepPlan {
    SmallKernel kern;
};

template <typename CutT, int KS>
void pick_small(SmallStepLaunch &c) {
    c.kern = dual_step_small_kernel<CutT, KS>;
    c.cut = sizeof(CutT) == 8 ? ICNN_BE_CUT_F64 : ICNN_BE_CUT_F32;
    c.kt = KS;
}

// Which dual_step_small_kernel instance a state that dual_step_small_fits gets: four waves per workgroup, four samples per wave
void choose_dual_step_small(const icnn_be_state &st, SmallStepLaunch &c) {
    const bool f64 = st.cut_dtype == ICNN_BE_CUT_F64;
    if (st.slots <= 5) f64 ? pick_small<double, 5>(c) : pick_small<float, 5>(c);
    else if (st.slots <= 7) f64 ? pick_small<double, 8>(c) : pick_small<float, 8>(c);
    else f64 ? pick_small<double, 16>(c) : pick_small<float, 16>(c);
    c.waves = 4;
    c.variant = ICNN_BE_VARIANT_RL;
    c.staged = 0;
    c.kernel = ICNN_BE_DUAL_PLAN_SMALL;
    c.lds = 0;
    c.rows = st.slots;
}
}  // namespace

void plan_dual_step_small(const icnn_be_state &st, DualStepPlan &p) {
    SmallStepLaunch c;
    choose_dual_step_small(st, c);
    p = c;
}

hipError_t launch_dual_step_small(const icnn_be_state &st, int round, const void *f, const void *g, hipStream_t stream) {
    SmallArgs a;
    a.st = st;
    a.f = f;
    a.g = g;
    a.round = round;
    SmallStepLaunch c;
    choose_dual_step_small(st, c);
    return launch_kernel(c.kern, dim3((st.batch + 15) / 16), dim3(64 * c.waves), c.lds, stream, a);
}

}  // namespace icnn_be
