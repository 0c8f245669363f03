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

struct GradNJob { PolicyWeights W; LearnerArgs a; };
template <int IN, int A>
static void grad_n_lane(void *arg) { GradNJob *j = (GradNJob *)arg; azul_a2c_grad_n_kernel<IN, A>(j->W, j->a); }

extern "C" {

unsigned long long sln_buffer_oob() { return simt::g_buffer_oob; }
int sln_flat_size(int in, int act) { return (int)a2c_shape_n((u32)in, (u32)act).params; }

// azul_a2c_grad_n_kernel<in, act> on n samples with grid (parts, 3), then azul_a2c_reduce_n_kernel's sum in part order -> grad [flat + 4]
// (n_dev / inv_n_dev: the sample count and 1 / count "in device memory", overriding n and inv_n as on the device-count path)
long long sln_gradients_dev(int in, int act, int n, int parts, const float *obs, const uint8_t *mask, const i32 *action, const float *qvals,
                            const i32 *index, float inv_n, const i32 *n_dev, const float *inv_n_dev, const float *w1t, const float *b1,
                            const float *w2c, const float *b2c, const float *w2a_t, const float *b2a, const float *w2a, float *partial, float *grad)
{
    GradNJob j;
    memset(&j, 0, sizeof(j));
    j.W = {w1t, b1, w2c, b2c, w2a_t, b2a};
    j.a.obs = obs; j.a.mask = mask; j.a.action = action; j.a.qvals = qvals; j.a.n = (u32)n; j.a.inv_n = inv_n; j.a.w2a = w2a;
    j.a.partial = partial; j.a.index = index; j.a.n_dev = n_dev; j.a.inv_n_dev = inv_n_dev;
    void (*fn)(void *) = nullptr;
    if (in == 188 && act == 180) fn = grad_n_lane<188, 180>;
    else if (in == 240 && act == 180) fn = grad_n_lane<240, 180>;
    else if (in == 198 && act == 240) fn = grad_n_lane<198, 240>;
    else if (in == 260 && act == 300) fn = grad_n_lane<260, 300>;
    else return -1;
    simt::g_grid_dim = {(unsigned)parts, 3, 1};
    long long ops = 0;
    for (int role = 0; role < 3; role++)
        for (int blk = 0; blk < parts; blk++) {
            simt::g_block_idx = {(unsigned)blk, (unsigned)role, 0};
            ops += (long long)simt::run_workgroup(fn, &j, (int)LN_WAVES, 512u << 10);
        }
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
