// The two table kernels of the flat-vector trainers (be_train_table.hip; be_ddpg.hip, be_naf.hip, be_naf_bn.hip, be_ff.hip fill the
// tables): the weight and bias gradients of a table of layers in one launch, and the update of a table of parameter sets in one.
#pragma once
#include "be_kernels.h"

namespace icnn_be {

constexpr int GRAD_PRODUCTS = 9;         // the longest table: the three nets of NAF

struct GradProd {
    const float *X, *D;                  // the layer's input [B][in] and pre-activation delta [B][out]
    float *G;                            // dW [in][out], then db [out]: one [(in + 1)][out] block of the flat gradient
    int in, out, wave0;                  // wave0: the first wave of this layer
};
struct GradArgs {
    GradProd p[GRAD_PRODUCTS];
    int B, waves, count;                 // count: the products in use, at most GRAD_PRODUCTS (layer() does not check)
    // the next product in the order of a flat gradient: W and b of a layer are one [(in + 1)][out] block at g
    void layer(const float *X, int in, const float *D, int out, float *&g) {
        p[count++] = GradProd{X, D, g, in, out, waves};
        waves += ((in + 1 + 15) / 16) * ((out + 31) / 32);
        g += (size_t)(in + 1) * out;
    }
};
hipError_t launch_grad_table(const GradArgs &a, hipStream_t stream);

constexpr int UPDATE_SETS = 3;

struct ParamSet {
    float *theta, *m, *v, *target;       // target NULL: a set without one
    const float *grad;
    long long n;
    int blocks, slot;                    // blocks: param_update_blocks(n); slot: which step count this set reads
    float k;                             // the decay coefficient
    double lr;
    long long tail;                      // the last `tail` elements (NAF-BN's betas) get no decay, stay out of sum theta^2 and
                                         // have no target: the target holds n - tail floats
};
struct ParamSetsArgs {
    ParamSet set[UPDATE_SETS];
    int sets;
    int *step;                           // [0, slots) the step counts, [slots] the ticket
    int slots;
    double beta1, beta2;
    float b1, c1, b2, c2, eps, tau;
    float *loss;                         // NULL: no loss
    const double *sq;                    // [tiles] the chain kernel's sums of td^2
    int tiles, batch;
    double l2norm;
    int reg_blocks;                      // the workgroups of the leading sets whose sum theta_old^2 enters the loss
    double *partial;                     // [reg_blocks]
};
// b1, c1, b2, c2 from the betas
void update_coefficients(ParamSetsArgs &u, double beta1, double beta2);
hipError_t launch_param_sets_update(const ParamSetsArgs &u, hipStream_t stream);

}  // namespace icnn_be
