// simt_x_rollout.cpp -- TEST-ONLY: the window kernels of wide batches (azul_x_policy_rollout_kernel and azul_x_policy_rollout_vs_kernel of
// csrc/azul_rollout2.hpp: env phases on azul_rules_x.hpp's P-seat GameRunner, matrix phases on v_mfma_f32_16x16x4_f32, the head of
// azul_policy_head_n_kernel; with a network or greedy_margin seats the agent's pass, then reply rounds while any game of the workgroup
// owes an opponent_move()), UNMODIFIED, as workgroups of eight emulated wavefronts (simt/simt.hpp: run_workgroup) on the kernels' own LDS.
// ONE entry for every kind of wide window (simt_window_call.hpp); which kind and shape runs, on which arguments, is the library's own
// choice: x_rollout_kernel and window_pack of csrc/azul_rollout2.hpp.
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

struct XJob { x_rollout_kernel_t kernel; azx::XBatchDev b; PolicyWeights W; RolloutArgs a; u32 id_base, max_replies; };

static void lane_run(void *arg)
{
    XJob *j = (XJob *)arg;
    j->kernel(j->b, j->W, j->a, j->id_base, j->max_replies);
}

extern "C" {

unsigned long long sxr_buffer_oob() { return simt::g_buffer_oob; }
unsigned long long sxr_call_bytes() { return sizeof(SimtWindowCall); }

// one launch over n_games wide records (a multiple of 16 or not: the last workgroup is ragged) for n_steps moves / agent steps; the weight
// arrays in the layouts of azul_policy_forward (w1t [obs_size][360], b1, w2c, b2c, w2a_t [180][NA], b2a).  opp_action / opp_logp
// [T][opp_slots][N] and opp_replies [T][N] are optional.  Returns the number of cross-lane operations executed, or a negative number on
// bad arguments (a kind or a shape x_rollout_kernel has no kernel for among them).
long long sxr_window(const SimtWindowCall *c)
{
    XJob j;
    memset(&j, 0, sizeof(j));
    bool league, arena;
    if (window_args(*c, true, j.W, j.a, league, arena)) return -1;
    j.kernel = x_rollout_kernel(c->players, c->displays, c->opp, league, arena);
    const bool replies = c->opp == 2 || c->opp == 3;        // the kinds with reply rounds: no sampling table, a bound on the rounds
    const double2 *tab = !j.kernel || replies ? nullptr : table_for(c->displays);
    if (!j.kernel || (!replies && !tab) || (replies && c->max_replies < 1)) return -1;
    j.b = x_batch(c->n_games, c->state, c->mt, c->mtpos, c->episodes, c->stuck, c->stat_sum, c->first_player, c->pool, c->end_bonus,
                  c->short_deal, tab);
    j.id_base = c->id_base;
    j.max_replies = replies ? (u32)c->max_replies : 0u;
    return x_launch(lane_run, &j, ((unsigned)c->n_games + PF_GAMES - 1u) / PF_GAMES, PR2_WAVES);
}

}
