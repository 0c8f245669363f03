// simt_x_rollout_greedy.cpp -- TEST-ONLY: the window kernel of wide batches with GREEDY_MARGIN seats (azul_x_policy_rollout_kernel<P, D, 3> of
// csrc/azul_rollout2.hpp: the agent's pass, then reply rounds answered by azx::greedy_pick_x inside the wave that holds the game),
// UNMODIFIED, as a workgroup of eight emulated wavefronts (simt/simt.hpp: run_workgroup) on the kernel's own LDS.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_ops2.hpp"
#include "azul_policy.hpp"
#include "azul_rollout2.hpp"
#include "simt_x_common.hpp"

struct XJobGreedy { azx::XBatchDev b; PolicyWeights W; RolloutArgs a; u32 id_base, max_replies; };

template <u32 P, u32 D>
static void lane_run(void *arg)
{
    XJobGreedy *j = (XJobGreedy *)arg;
    azul_x_policy_rollout_kernel<P, D, 3>(j->b, j->W, j->a, j->id_base, j->max_replies);
}

extern "C" {

unsigned long long sxg_buffer_oob() { return simt::g_buffer_oob; }

// one launch over n_games wide records for n_steps agent steps; `w` = the agent's six weight arrays in the layouts of azul_policy_forward.
// opp_action / opp_logp [T][opp_slots][N] and opp_replies [T][N] are optional (opp_logp is handed to the kernel only to show that it is
// never written).  Returns the number of cross-lane operations executed, or a negative number on bad arguments.
long long sxg_rollout(int n_games, int players, int displays, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum,
                      int first_player, int pool, int end_bonus, int short_deal, unsigned id_base, const float *const *w, int n_steps, float *obs,
                      uint8_t *mask, uint8_t *player, i32 *action, i32 *reward, uint8_t *done, float *value, float *logp, float *entropy,
                      uint8_t *status, i32 *opp_action, float *opp_logp, uint8_t *opp_replies, int opp_slots, unsigned long long seed,
                      unsigned long long counter, int max_replies)
{
    lane_fn fn = SIMT_X_PICK(lane_run, players, displays);
    if (!fn || n_games <= 0 || max_replies < 1) return -1;
    XJobGreedy j;
    memset(&j, 0, sizeof(j));
    j.b = x_batch(n_games, state, mt, mtpos, episodes, stuck, stat_sum, first_player, pool, end_bonus, short_deal, nullptr);
    j.W = {w[0], w[1], w[2], w[3], w[4], w[5]};
    j.a.n_steps = n_steps; j.a.obs = obs; j.a.mask = mask; j.a.player = player; j.a.action = action; j.a.reward = reward; j.a.done = done;
    j.a.value = value; j.a.logp = logp; j.a.entropy = entropy; j.a.status = status; j.a.seed = seed; j.a.counter = counter;
    j.a.opp_action = opp_action; j.a.opp_logp = opp_logp; j.a.opp_replies = opp_replies; j.a.opp_slots = opp_slots;
    j.id_base = id_base;
    j.max_replies = (u32)max_replies;
    return x_launch(fn, &j, ((unsigned)n_games + PF_GAMES - 1u) / PF_GAMES, PR2_WAVES);
}

}
