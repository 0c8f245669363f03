// simt_x_rollout.cpp -- TEST-ONLY: the window kernels of wide batches (azul_x_policy_rollout_kernel and azul_x_policy_rollout_vs_kernel of
// csrc/azul_rollout2.hpp: env phases on azul_rules_x.hpp's P-seat GameRunner, matrix phases on v_mfma_f32_16x16x4_f32, the head of
// azul_policy_head_n_kernel; with a network or greedy_margin seats the agent's pass, then reply rounds while any game of the workgroup
// owes an opponent_move()), UNMODIFIED, as workgroups of eight emulated wavefronts (simt/simt.hpp: run_workgroup) on the kernels' own LDS.
// ONE entry for every kind of wide window (simt_window_call.hpp), every kind compiled for the five shapes of SIMT_X_PICK.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_ops2.hpp"
#include "azul_policy.hpp"
#include "azul_rollout2.hpp"
#include "simt_x_common.hpp"
#include "simt_window_call.hpp"

static_assert(AZUL_LEAGUE_GROUP_GAMES == PF_GAMES, "a league / arena group is one workgroup's games");

struct XJob { azx::XBatchDev b; PolicyWeights W; RolloutArgs a; u32 id_base, max_replies; int opp; bool league, arena; };

// the kernel of a call, chosen as the wide branch of rollout_window chooses it (csrc/azul_kernels.hip)
template <u32 P, u32 D>
static void lane_run(void *arg)
{
    XJob *j = (XJob *)arg;
    if (j->opp == 2 && j->arena) azul_x_policy_rollout_vs_kernel<P, D, true, true>(j->b, j->W, j->a, j->id_base, j->max_replies);
    else if (j->opp == 2 && j->league) azul_x_policy_rollout_vs_kernel<P, D, true>(j->b, j->W, j->a, j->id_base, j->max_replies);
    else if (j->opp == 2) azul_x_policy_rollout_vs_kernel<P, D>(j->b, j->W, j->a, j->id_base, j->max_replies);
    else if (j->opp == 3) azul_x_policy_rollout_kernel<P, D, 3>(j->b, j->W, j->a, j->id_base, j->max_replies);
    else if (j->opp) azul_x_policy_rollout_kernel<P, D, 1>(j->b, j->W, j->a, j->id_base);
    else azul_x_policy_rollout_kernel<P, D, 0>(j->b, j->W, j->a, j->id_base);
}

extern "C" {

unsigned long long sxr_buffer_oob() { return simt::g_buffer_oob; }
unsigned long long sxr_call_bytes() { return sizeof(SimtWindowCall); }

// one launch over n_games wide records (a multiple of 16 or not: the last workgroup is ragged) for n_steps moves / agent steps; the weight
// arrays in the layouts of azul_policy_forward (w1t [obs_size][360], b1, w2c, b2c, w2a_t [180][NA], b2a).  opp_action / opp_logp
// [T][opp_slots][N] and opp_replies [T][N] are optional.  Returns the number of cross-lane operations executed, or a negative number on
// bad arguments.
long long sxr_window(const SimtWindowCall *c)
{
    lane_fn fn = SIMT_X_PICK(lane_run, c->players, c->displays);
    const bool replies = c->opp == 2 || c->opp == 3;        // the kinds with reply rounds: no sampling table, a bound on the rounds
    const double2 *tab = !fn || replies ? nullptr : table_for(c->displays);
    XJob j;
    memset(&j, 0, sizeof(j));
    if (!fn || (!replies && !tab) || (replies && c->max_replies < 1) || window_args(*c, true, j.W, j.a, j.league, j.arena)) return -1;
    j.b = x_batch(c->n_games, c->state, c->mt, c->mtpos, c->episodes, c->stuck, c->stat_sum, c->first_player, c->pool, c->end_bonus,
                  c->short_deal, tab);
    j.id_base = c->id_base; j.opp = c->opp;
    j.max_replies = replies ? (u32)c->max_replies : 0u;
    return x_launch(fn, &j, ((unsigned)c->n_games + PF_GAMES - 1u) / PF_GAMES, PR2_WAVES);
}

}
