// simt_ppo.cpp -- TEST-ONLY: the PPO instantiations (OBJ = 1) of the gradient kernels of csrc/azul_learner.hpp -- for ActorCritic(136, 180,
// 180) and for p4_d9 (260, 300) -- UNMODIFIED, as workgroups of emulated wavefronts (simt/simt.hpp), picked by the selector
// azul_ppo_gradients launches through (a2c_grad with obj 1) and followed by the shape's reduce (simt_a2c_launch.hpp): a CPU check of
// the clipped-surrogate head against the float64 restatement of tests/ppo_grad_ref.py.
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

unsigned long long sp_buffer_oob() { return simt::g_buffer_oob; }
int sp_flat_size(int in, int act) { return (int)a2c_shape_n((u32)in, (u32)act).params; }

// (in, act) = (136, 180): `parts` workgroups of the reference shape's kernel; (260, 300): grid (parts, 3) of p4_d9's;
// then the reduce in part order -> grad [flat + 4].  n_dev / inv_n_dev: the device-count path.  logp_out: optional [n].
long long sp_gradients(int in, int act, int n, int parts, const float *obs, const uint8_t *mask, const i32 *action, const float *returns,
                       const float *old_logp, const float *advantage, float clip_eps, float value_coeff, float entropy_coeff, const i32 *index,
                       float inv_n, const i32 *n_dev, const float *inv_n_dev, const float *w1t, const float *b1, const float *w2c, const float *b2c,
                       const float *w2a_t, const float *b2a, const float *w2a, float *partial, float *grad, float *logp_out)
{
    const bool reference = in == PF_IN && act == PF_ACT;
    if (!reference && !(in == 260 && act == 300)) return -1;
    LearnerArgs a;
    memset(&a, 0, sizeof(a));
    a.obs = obs; a.mask = mask; a.action = action; a.qvals = returns; a.n = (u32)n; a.inv_n = inv_n; a.w2a = w2a;
    a.partial = partial; a.index = index; a.n_dev = n_dev; a.inv_n_dev = inv_n_dev;
    a.old_logp = old_logp; a.advantage = advantage; a.clip_eps = clip_eps; a.value_coeff = value_coeff; a.entropy_coeff = entropy_coeff;
    a.logp_out = logp_out;
    return run_gradients(in, act, 1, {w1t, b1, w2c, b2c, w2a_t, b2a}, a, parts) + run_reduce(a2c_shape_n((u32)in, (u32)act), partial, parts, grad);
}

}
