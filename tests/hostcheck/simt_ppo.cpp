// simt_ppo.cpp -- TEST-ONLY: the PPO instantiations (OBJ = 1) of the gradient kernels of csrc/azul_learner.hpp -- azul_a2c_grad_kernel<1> for
// ActorCritic(136, 180, 180) and azul_a2c_grad_n_kernel<260, 300, 1> (p4_d9) -- UNMODIFIED, as workgroups of emulated wavefronts
// (simt/simt.hpp), launched as azul_ppo_gradients launches them and followed by the shape's reduce (simt_a2c_launch.hpp): a CPU check of
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

struct PpoJob { PolicyWeights W; LearnerArgs a; };
static void ppo_lane(void *arg) { PpoJob *j = (PpoJob *)arg; azul_a2c_grad_kernel<1>(j->W, j->a); }
static void ppo_n_lane(void *arg) { PpoJob *j = (PpoJob *)arg; azul_a2c_grad_n_kernel<260, 300, 1>(j->W, j->a); }

extern "C" {

unsigned long long sp_buffer_oob() { return simt::g_buffer_oob; }
int sp_flat_size(int in, int act) { return (int)a2c_shape_n((u32)in, (u32)act).params; }

// (in, act) = (136, 180): `parts` workgroups of azul_a2c_grad_kernel<1>; (260, 300): grid (parts, 3) of azul_a2c_grad_n_kernel<260, 300, 1>;
// then the reduce in part order -> grad [flat + 4].  n_dev / inv_n_dev: the device-count path.  logp_out: optional [n].
long long sp_gradients(int in, int act, int n, int parts, const float *obs, const uint8_t *mask, const i32 *action, const float *returns,
                       const float *old_logp, const float *advantage, float clip_eps, float value_coeff, float entropy_coeff, const i32 *index,
                       float inv_n, const i32 *n_dev, const float *inv_n_dev, const float *w1t, const float *b1, const float *w2c, const float *b2c,
                       const float *w2a_t, const float *b2a, const float *w2a, float *partial, float *grad, float *logp_out)
{
    const bool reference = in == PF_IN && act == PF_ACT;
    if (!reference && !(in == 260 && act == 300)) return -1;
    PpoJob j;
    memset(&j, 0, sizeof(j));
    j.W = {w1t, b1, w2c, b2c, w2a_t, b2a};
    j.a.obs = obs; j.a.mask = mask; j.a.action = action; j.a.qvals = returns; j.a.n = (u32)n; j.a.inv_n = inv_n; j.a.w2a = w2a;
    j.a.partial = partial; j.a.index = index; j.a.n_dev = n_dev; j.a.inv_n_dev = inv_n_dev;
    j.a.old_logp = old_logp; j.a.advantage = advantage; j.a.clip_eps = clip_eps; j.a.value_coeff = value_coeff; j.a.entropy_coeff = entropy_coeff;
    j.a.logp_out = logp_out;
    const unsigned roles = reference ? 1u : 3u;
    simt::g_grid_dim = {(unsigned)parts, roles, 1};
    long long ops = 0;
    for (unsigned role = 0; role < roles; role++)
        for (int blk = 0; blk < parts; blk++) {
            simt::g_block_idx = {(unsigned)blk, role, 0};
            ops += (long long)simt::run_workgroup(reference ? ppo_lane : ppo_n_lane, &j, reference ? (int)LG_WAVES : (int)LN_WAVES, 512u << 10);
        }
    return ops + run_reduce(a2c_shape_n((u32)in, (u32)act), partial, parts, grad);
}

}
