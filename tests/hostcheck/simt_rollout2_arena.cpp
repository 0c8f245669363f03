// simt_rollout2_arena.cpp -- TEST-ONLY: the persistent policy rollout kernel as an ARENA (csrc/azul_rollout2.hpp:
// azul_policy_rollout2_kernel<LID, 2, true> -- every 16-game workgroup reads the pool member of its agent seat and the member it plays
// against once and takes BOTH nets' biases and weight streams from those members of the one stacked pool), UNMODIFIED, as workgroups of
// eight emulated wavefronts (simt/simt.hpp: run_workgroup).  The arguments are simt_rollout2_league.cpp's with the pool in place of the
// agent too.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_ops2.hpp"
#include "azul_policy.hpp"
#include "azul_rollout2.hpp"

static_assert(AZUL_LEAGUE_GROUP_GAMES == PF_GAMES, "an arena group is one workgroup's games");

struct Job { BatchDev b; PolicyWeights W; RolloutArgs a; int lid; };

static void lane_main(void *arg)
{
    Job *j = (Job *)arg;
    if (j->lid) azul_policy_rollout2_kernel<true, 2, true>(j->b, j->W, j->a);
    else azul_policy_rollout2_kernel<false, 2, true>(j->b, j->W, j->a);
}

extern "C" {

unsigned long long sr2a_buffer_oob() { return simt::g_buffer_oob; }

// `wp` = the pool's six STACKED weight arrays (pool_size members each); agent_member / opp_member [ceil(n_games / 16)]: the pair of every group
long long sr2a_rollout_arena(int n_games, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum, int first_player,
                             int tile_pool, unsigned id_base, const float *const *wp, int pool_size, const uint8_t *agent_member,
                             const uint8_t *opp_member, int n_steps, float *obs, uint8_t *mask, uint8_t *player, i32 *action, i32 *reward,
                             uint8_t *done, float *value, float *logp, float *entropy, uint8_t *status, float *returns, float gamma,
                             unsigned long long seed, unsigned long long opp_seed, unsigned long long counter, i32 *opp_action, float *opp_logp,
                             uint8_t *opp_replies, int opp_slots)
{
    static double T[T_PAIRS * 2];
    if (!build_sample_pairs(T_ROWS, T)) return -2;
    if (!agent_member || !opp_member || pool_size < 1 || pool_size > 255) return -1;
    Job j;
    memset(&j, 0, sizeof(j));
    j.b.state = state; j.b.mt = mt; j.b.mtpos = mtpos; j.b.tab = (const double2 *)T; j.b.episodes = episodes; j.b.stuck = stuck; j.b.stat_sum = stat_sum;
    j.b.n = (u32)n_games; j.b.rules.first_player = (u32)first_player; j.b.rules.tile_pool = (u32)tile_pool; j.b.draw_margin = AZ_DRAW_MARGIN;
    j.b.id_base = id_base;
    j.W = {wp[0], wp[1], wp[2], wp[3], wp[4], wp[5]};
    j.a.n_steps = n_steps; j.a.obs = obs; j.a.mask = mask; j.a.player = player; j.a.action = action; j.a.reward = reward; j.a.done = done;
    j.a.value = value; j.a.logp = logp; j.a.entropy = entropy; j.a.status = status; j.a.returns = returns; j.a.gamma = gamma;
    j.a.seed = seed; j.a.counter = counter; j.a.counter_dev = nullptr;
    j.a.Wopp = j.W;
    j.a.opp_seed = opp_seed; j.a.opp_action = opp_action; j.a.opp_logp = opp_logp; j.a.opp_replies = opp_replies; j.a.opp_slots = opp_slots;
    j.a.opp_member = opp_member; j.a.opp_pool = (u32)pool_size;
    j.a.agent_member = agent_member; j.a.agent_pool = (u32)pool_size;
    j.lid = tile_pool == POOL_LID;
    const unsigned blocks = ((unsigned)n_games + PF_GAMES - 1u) / PF_GAMES;
    simt::g_grid_dim = {blocks, 1, 1};
    long long ops = 0;
    for (unsigned blk = 0; blk < blocks; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        ops += (long long)simt::run_workgroup(lane_main, &j, (int)PR2_WAVES);
    }
    return ops;
}

}
