// The entropy term of the RL agent's `_fg_entr` (RL/src/icnn.py:59-63, 455-458) for one action element, shared by the
// inner Adam (be_adam.hip, both paths) and the critic's TD target (be_rl_train.hip), so that the two evaluate it with
// the same operations (oracle/adam_oracle.py entropy_terms restates them):
//   p = clip((a + 1) / 2, 1e-4, 0.9999) from the float32 action, pen = p log p + (1 - p) log(1 - p) with float64 logs
//   rounded to float32, d pen / d a = (log p - log(1 - p)) / 2 inside the clip and 0 outside (clip_by_value passes no
//   gradient there).  The caller sums pen over the action sequentially in float32.
#pragma once
#include <hip/hip_runtime.h>

namespace icnn_be {

struct EntropyTerm {
    float pen, dpen;
};

__device__ __forceinline__ EntropyTerm rl_entropy_term(float af) {
#pragma clang fp contract(off)
    const float half = (af + 1.f) * 0.5f;
    const float p = fminf(fmaxf(half, 1e-4f), 0.9999f);          // tf.clip_by_value, :456
    const float q = 1.f - p;
    const float lp = (float)log((double)p), lq = (float)log((double)q);
    const bool inside = half >= 1e-4f && half <= 0.9999f;
    return {p * lp + q * lq, inside ? 0.5f * (lp - lq) : 0.f};
}

}  // namespace icnn_be
