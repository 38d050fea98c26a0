// What the C entries that are defined beside their kernels share: the error report and the argument tests that more than
// one unit makes.  Host only.  An entry lives in its unit unless it takes an icnn_be_state, a model or a context descriptor
// (be_api.hip has the rule); a new unit costs a header entry, a ctypes entry and its own .hip file.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "icnn_be.h"

namespace icnn_be {

// 0, or the C ABI's error code with the HIP error kept for icnn_be_last_hip_error (defined in be_api.hip)
int api_done(hipError_t e);

// NULL, or not a multiple of `to` bytes
inline bool misaligned(const void *p, uintptr_t to) { return !p || reinterpret_cast<uintptr_t>(p) % to; }

// a hipStream_t is a pointer to the runtime's object (NULL: the default stream)
inline bool stream_ok(void *stream) { return reinterpret_cast<uintptr_t>(stream) % 8 == 0; }

// TF-Adam's constants; the rate is each caller's own (some accept an infinite one)
inline bool adam_constants_ok(double beta1, double beta2, float eps) {
    return beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.f;
}

// What the replay-step descriptors (icnn_be_ddpg_args, icnn_be_naf_args, icnn_be_naf_bn_args) share: the minibatch, the
// step count, the workspace and the constants.  need_loss: loss may not be NULL.  The unit adds its sizes, its networks'
// pointers and its own constants.
template <typename Args>
int check_replay_step(const Args &a, void *stream, bool need_loss) {
    if (a.batch < 1 || !stream_ok(stream)) return ICNN_BE_EINVAL;
    if (misaligned(a.obs, 4) || misaligned(a.rew, 4) || misaligned(a.ob2, 4) || misaligned(a.step, 4) || misaligned(a.act, 8) ||
        !a.term || misaligned(a.work, 16))
        return ICNN_BE_EINVAL;
    if (need_loss ? misaligned(a.loss, 4) : reinterpret_cast<uintptr_t>(a.loss) % 4 != 0) return ICNN_BE_EINVAL;
    if (!(a.tau >= 0.f && a.tau <= 1.f) || !std::isfinite(a.discount)) return ICNN_BE_EINVAL;
    if (!(a.l2norm >= 0.f) || !std::isfinite(a.l2norm)) return ICNN_BE_EINVAL;
    if (!adam_constants_ok(a.beta1, a.beta2, a.eps) || !std::isfinite(a.rate)) return ICNN_BE_EINVAL;
    return 0;
}

}  // namespace icnn_be
