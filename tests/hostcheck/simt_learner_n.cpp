// simt_learner_n.cpp -- TEST-ONLY: the wide-shape A2C kernels of csrc/azul_learner.hpp (azul_a2c_grad_n_kernel<IN, A>: three workgroup roles
// per part, gradient tiles in registers; azul_a2c_reduce_n_kernel and azul_a2c_apply_n_kernel on the shape's flat layout), UNMODIFIED, as workgroups of emulated
// wavefronts (simt/simt.hpp) -- a CPU check of their arithmetic against torch and, under ASan / UBSan, of every LDS and global index.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_selfplay_kernels.hpp"
#include "azul_policy.hpp"
#include "azul_rollout2.hpp"
#include "azul_learner.hpp"
#include "simt_a2c_launch.hpp"

extern "C" {

unsigned long long sln_buffer_oob() { return simt::g_buffer_oob; }
int sln_flat_size(int in, int act) { return (int)a2c_shape_n((u32)in, (u32)act).params; }

// the gradient kernel of the wide shape (in, act) on n samples with its grid (parts, 3), then azul_a2c_reduce_n_kernel's sum in part order -> grad [flat + 4]
// (n_dev / inv_n_dev: the sample count and 1 / count "in device memory", overriding n and inv_n as on the device-count path)
long long sln_gradients_dev(int in, int act, int n, int parts, const float *obs, const uint8_t *mask, const i32 *action, const float *qvals,
                            const i32 *index, float inv_n, const i32 *n_dev, const float *inv_n_dev, const float *w1t, const float *b1,
                            const float *w2c, const float *b2c, const float *w2a_t, const float *b2a, const float *w2a, float *partial, float *grad)
{
    LearnerArgs a;
    memset(&a, 0, sizeof(a));
    a.obs = obs; a.mask = mask; a.action = action; a.qvals = qvals; a.n = (u32)n; a.inv_n = inv_n; a.w2a = w2a;
    a.partial = partial; a.index = index; a.n_dev = n_dev; a.inv_n_dev = inv_n_dev;
    if (a2c_reference_layout(a2c_shape_n((u32)in, (u32)act))) return -1;      // (the reference shape is simt_learner.cpp's)
    const long long ops = run_gradients(in, act, 0, {w1t, b1, w2c, b2c, w2a_t, b2a}, a, parts);
    if (!ops) return -1;
    return ops + run_reduce(a2c_shape_n((u32)in, (u32)act), partial, parts, grad);
}

long long sln_gradients(int in, int act, int n, int parts, const float *obs, const uint8_t *mask, const i32 *action, const float *qvals,
                        const i32 *index, float inv_n, const float *w1t, const float *b1, const float *w2c, const float *b2c, const float *w2a_t,
                        const float *b2a, const float *w2a, float *partial, float *grad)
{
    return sln_gradients_dev(in, act, n, parts, obs, mask, action, qvals, index, inv_n, nullptr, nullptr, w1t, b1, w2c, b2c, w2a_t, b2a, w2a,
                             partial, grad);
}

// azul_a2c_apply_n_kernel (one Adam step, host-side bias corrections of step `step`)
long long sln_adam(int in, int act, const float *grad, float *flat, float *m, float *v, float lr, float beta1, float beta2, float eps, int step,
                   float *c1w, float *c1b, float *c2w, float *c2b, float *a1w, float *a1b, float *a2w, float *a2b)
{
    AdamJob j = {a2c_shape_n((u32)in, (u32)act), grad, flat, m, v, lr, beta1, beta2, eps, (float)(1.0 - pow((double)beta1, (double)step)),
                 (float)sqrt(1.0 - pow((double)beta2, (double)step)), {c1w, c1b, c2w, c2b, a1w, a1b, a2w, a2b}, nullptr, nullptr, nullptr, 0};
    return run_adam(j);
}

}
