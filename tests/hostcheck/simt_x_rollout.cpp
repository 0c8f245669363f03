// simt_x_rollout.cpp -- TEST-ONLY: the window kernel of wide batches (azul_x_policy_rollout_kernel of csrc/azul_rollout2.hpp: env phases on
// azul_rules_x.hpp's P-seat GameRunner, matrix phases on v_mfma_f32_16x16x4_f32, the head of azul_policy_head_n_kernel), UNMODIFIED, as a
// workgroup of eight emulated wavefronts (simt/simt.hpp: run_workgroup) on the kernel's own LDS.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_ops2.hpp"
#include "azul_policy.hpp"
#include "azul_rollout2.hpp"
#include "simt_x_common.hpp"

struct XJob { azx::XBatchDev b; PolicyWeights W; RolloutArgs a; u32 id_base; int opp; };

template <u32 P, u32 D>
static void lane_run(void *arg)
{
    XJob *j = (XJob *)arg;
    if (j->opp) azul_x_policy_rollout_kernel<P, D, 1>(j->b, j->W, j->a, j->id_base);
    else azul_x_policy_rollout_kernel<P, D, 0>(j->b, j->W, j->a, j->id_base);
}

extern "C" {

unsigned long long sxr_buffer_oob() { return simt::g_buffer_oob; }

// one launch over n_games wide records (a multiple of 16 or not: the last workgroup is ragged) for n_steps moves; `w` = the six weight
// arrays in the layouts of azul_policy_forward (w1t [obs_size][360], b1, w2c, b2c, w2a_t [180][NA], b2a).  Returns the number of
// cross-lane operations executed, or a negative number on bad arguments.
long long sxr_rollout(int n_games, int players, int displays, int opp, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck,
                      double *stat_sum, int first_player, int pool, int end_bonus, int short_deal, unsigned id_base, const float *const *w, int n_steps,
                      float *obs, uint8_t *mask, uint8_t *player, i32 *action, i32 *reward, uint8_t *done, float *value, float *logp, float *entropy,
                      uint8_t *status, unsigned long long seed, unsigned long long counter)
{
    lane_fn fn = SIMT_X_PICK(lane_run, players, displays);
    const double2 *tab = table_for(displays);
    if (!fn || !tab || n_games <= 0) return -1;
    XJob j;
    memset(&j, 0, sizeof(j));
    j.b = x_batch(n_games, state, mt, mtpos, episodes, stuck, stat_sum, first_player, pool, end_bonus, short_deal, tab);
    j.W = {w[0], w[1], w[2], w[3], w[4], w[5]};
    j.a.n_steps = n_steps; j.a.obs = obs; j.a.mask = mask; j.a.player = player; j.a.action = action; j.a.reward = reward; j.a.done = done;
    j.a.value = value; j.a.logp = logp; j.a.entropy = entropy; j.a.status = status; j.a.seed = seed; j.a.counter = counter;
    j.id_base = id_base; j.opp = opp;
    return x_launch(fn, &j, ((unsigned)n_games + PF_GAMES - 1u) / PF_GAMES, PR2_WAVES);
}

}
