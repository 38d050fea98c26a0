// tf.train.AdamOptimizer's step on one element, and the register form of the float streams it runs over: what the two update
// kernels share (param_update_kernel of be_train_update.hip, param_sets_update_kernel of be_train_table.hip).  Device code
// only.  float32, correctly rounded at every operation, no contraction (the NumPy restatement of tests/test_device_update.py
// reproduces it bit for bit):
//   m = b1 * m + c1 * g                 b1 = (float)beta1, c1 = (float)(1 - beta1)
//   v = b2 * v + c2 * (g * g)           b2 = (float)beta2, c2 = (float)(1 - beta2)
//   theta = theta - (lr_t * m) / (sqrt(v) + eps)
#pragma once
#include <hip/hip_runtime.h>

namespace icnn_be {

constexpr int ADAM_THREADS = 256;        // a workgroup of either kernel
constexpr int ADAM_PER_THREAD = 4;       // consecutive elements of a thread: 16 bytes of every stream

// lr_t in double from the step count t (the update about to be done is number t), as train.TFAdam computes it
__device__ __forceinline__ float tf_adam_lr_t(double lr, double beta1, double beta2, int t) {
    return (float)(lr * sqrt(1.0 - pow(beta2, (double)t)) / (1.0 - pow(beta1, (double)t)));
}

// the new theta; m and v are updated in place (theta by value: taken by reference, the compiler schedules the register
// initialisation of param_sets_update_kernel in another order)
__device__ __forceinline__ float tf_adam_element(float th, float &m, float &v, float g, float b1, float c1, float b2, float c2,
                                                float lr_t, float eps) {
#pragma clang fp contract(off)
    // plain operators under a pragma of this body's own: a header function is outside the scope of its caller's pragma, and the
    // compiler fused the products of the __f*_rn helpers into the sums.  sqrt: the float of the double root (correctly rounded
    // both times, and 53 >= 2 * 24 + 2 bits make the double rounding innocuous); v_sqrt_f32 alone is 1 ulp
    m = b1 * m + c1 * g;
    v = b2 * v + c2 * (g * g);
    const float root = (float)__builtin_sqrt((double)v);
    return th - (lr_t * m) / (root + eps);
}

// The four elements of a thread in one float stream as registers: one 16-byte load or store, p on a 16-byte boundary.  A
// thread with fewer than four elements left takes a scalar tail instead; its kernel decides between the two forms ONCE for
// all of its streams (a branch per stream makes either kernel a tenth longer), so the tail stays with the kernel.
__device__ __forceinline__ void load_quad(float (&x)[ADAM_PER_THREAD], const float *p) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
}
__device__ __forceinline__ void store_quad(float *p, const float (&x)[ADAM_PER_THREAD]) {
    *reinterpret_cast<float4 *>(p) = make_float4(x[0], x[1], x[2], x[3]);
}

}  // namespace icnn_be
