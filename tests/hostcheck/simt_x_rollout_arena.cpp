// simt_x_rollout_arena.cpp -- TEST-ONLY: the window kernel of wide batches as an ARENA (azul_x_policy_rollout_vs_kernel<P, D, true, true> of
// csrc/azul_rollout2.hpp: every 16-game workgroup takes its agent and its opponent from the members of the one stacked pool its two bytes
// name), UNMODIFIED, as workgroups of eight emulated wavefronts on the kernel's own LDS.  The arguments are simt_x_rollout_league.cpp's
// with the pool in place of the agent too.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_ops2.hpp"
#include "azul_policy.hpp"
#include "azul_rollout2.hpp"
#include "simt_x_common.hpp"

struct XJobAr { azx::XBatchDev b; PolicyWeights W; RolloutArgs a; u32 id_base, max_replies; };

template <u32 P, u32 D>
static void lane_run(void *arg)
{
    XJobAr *j = (XJobAr *)arg;
    azul_x_policy_rollout_vs_kernel<P, D, true, true>(j->b, j->W, j->a, j->id_base, j->max_replies);
}

extern "C" {

unsigned long long sxa_buffer_oob() { return simt::g_buffer_oob; }

// `wp` = the pool's six STACKED weight arrays (pool_size members each); agent_member / opp_member [ceil(n_games / 16)]: the pair of every group
long long sxa_rollout_arena(int n_games, int players, int displays, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum,
                            int first_player, int pool, int end_bonus, int short_deal, unsigned id_base, const float *const *wp, int pool_size,
                            const uint8_t *agent_member, const uint8_t *opp_member, int n_steps, float *obs, uint8_t *mask, uint8_t *player,
                            i32 *action, i32 *reward, uint8_t *done, float *value, float *logp, float *entropy, uint8_t *status, i32 *opp_action,
                            float *opp_logp, uint8_t *opp_replies, int opp_slots, unsigned long long seed, unsigned long long opp_seed,
                            unsigned long long counter, int max_replies)
{
    lane_fn fn = SIMT_X_PICK(lane_run, players, displays);
    if (!fn || n_games <= 0 || max_replies < 1 || !agent_member || !opp_member || pool_size < 1 || pool_size > 255) return -1;
    XJobAr j;
    memset(&j, 0, sizeof(j));
    j.b = x_batch(n_games, state, mt, mtpos, episodes, stuck, stat_sum, first_player, pool, end_bonus, short_deal, nullptr);
    j.W = {wp[0], wp[1], wp[2], wp[3], wp[4], wp[5]};
    j.a.n_steps = n_steps; j.a.obs = obs; j.a.mask = mask; j.a.player = player; j.a.action = action; j.a.reward = reward; j.a.done = done;
    j.a.value = value; j.a.logp = logp; j.a.entropy = entropy; j.a.status = status; j.a.seed = seed; j.a.counter = counter;
    j.a.Wopp = j.W;
    j.a.opp_seed = opp_seed; j.a.opp_action = opp_action; j.a.opp_logp = opp_logp; j.a.opp_replies = opp_replies; j.a.opp_slots = opp_slots;
    j.a.opp_member = opp_member; j.a.opp_pool = (u32)pool_size;
    j.a.agent_member = agent_member; j.a.agent_pool = (u32)pool_size;
    j.id_base = id_base;
    j.max_replies = (u32)max_replies;
    return x_launch(fn, &j, ((unsigned)n_games + PF_GAMES - 1u) / PF_GAMES, PR2_WAVES);
}

}
