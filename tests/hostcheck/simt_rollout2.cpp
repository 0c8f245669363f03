// simt_rollout2.cpp -- TEST-ONLY: the persistent policy rollout kernel itself (csrc/azul_rollout2.hpp: azul_policy_rollout2_kernel, env
// phases on csrc/azul_env2.hpp, matrix phases on v_mfma_f32_16x16x4_f32 with weights streamed through buffer loads, the sampling head of
// csrc/azul_policy.hpp), UNMODIFIED, as workgroups of eight emulated wavefronts (simt/simt.hpp: run_workgroup) -- a CPU check of the
// kernel's logic and, under ASan / UBSan, of every LDS and global index it forms.  ONE entry for every kind of two-player window
// (simt_window_call.hpp): the policy on both seats, RandomAgent / network / greedy opponent, league, arena.  Which of the ten
// instantiations runs, on which arguments, is the library's own choice: rollout2_kernel and window_pack of csrc/azul_rollout2.hpp.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_ops2.hpp"
#include "azul_policy.hpp"
#include "azul_rollout2.hpp"
#include "simt_window_call.hpp"

static_assert(AZUL_LEAGUE_GROUP_GAMES == PF_GAMES, "a league / arena group is one workgroup's games");

struct Job { rollout2_kernel_t kernel; BatchDev b; PolicyWeights W; RolloutArgs a; };

static void lane_run(void *arg)
{
    Job *j = (Job *)arg;
    j->kernel(j->b, j->W, j->a);
}

extern "C" {

unsigned long long sr2_buffer_oob() { return simt::g_buffer_oob; }
unsigned long long sr2_call_bytes() { return sizeof(SimtWindowCall); }

// one launch over n_games (a multiple of 16 or not: the last workgroup is ragged) for n_steps moves / agent steps.  Returns the number of
// cross-lane operations executed, or a negative number on bad arguments (an opp rollout2_kernel has no kernel for among them).  A league
// is <LID, 2> with RolloutArgs::opp_member set.
long long sr2_window(const SimtWindowCall *c)
{
    static double T[T_PAIRS * 2];
    const bool greedy = c->opp == 3;                        // the sampler's table pointer stays NULL: OPP == 3 must not read it
    if (!greedy && !build_sample_pairs(T_ROWS, T)) return -2;
    Job j;
    memset(&j, 0, sizeof(j));
    bool league, arena;
    if (window_args(*c, false, j.W, j.a, league, arena)) return -1;
    j.kernel = rollout2_kernel(c->pool == POOL_LID, c->opp, arena);
    if (!j.kernel) return -1;
    j.b.state = c->state; j.b.mt = c->mt; j.b.mtpos = c->mtpos; j.b.tab = greedy ? nullptr : (const double2 *)T; j.b.episodes = c->episodes;
    j.b.stuck = c->stuck; j.b.stat_sum = c->stat_sum; j.b.n = (u32)c->n_games; j.b.rules.first_player = (u32)c->first_player;
    j.b.rules.tile_pool = (u32)c->pool; j.b.draw_margin = AZ_DRAW_MARGIN; j.b.move_limit = c->move_limit; j.b.id_base = c->id_base;
    const unsigned blocks = ((unsigned)c->n_games + PF_GAMES - 1u) / PF_GAMES;
    simt::g_grid_dim = {blocks, 1, 1};
    long long ops = 0;
    for (unsigned blk = 0; blk < blocks; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        ops += (long long)simt::run_workgroup(lane_run, &j, (int)PR2_WAVES);
    }
    return ops;
}

}
