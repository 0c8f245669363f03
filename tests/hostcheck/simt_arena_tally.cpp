// simt_arena_tally.cpp -- TEST-ONLY: the arena's book-keeping kernel (csrc/azul_policy.hpp: azul_arena_tally_kernel -- per ordered pair
// (agent member, opponent member) the episodes and statistic sums its groups' games gained since the marks, added game by game in
// ascending order, then the marks moved up), UNMODIFIED, one emulated wavefront per agent member (simt/simt.hpp), launched as
// azul_arena_tally launches it.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_policy.hpp"

struct TallyJob { const u64 *episodes; const double *stat_sums; u64 *mark_episodes; double *mark_sums; const uint8_t *agent, *opp; u32 n, K; double *results; };
static void tally_lane(void *arg)
{
    TallyJob *j = (TallyJob *)arg;
    azul_arena_tally_kernel(j->episodes, j->stat_sums, j->mark_episodes, j->mark_sums, j->agent, j->opp, j->n, j->K, j->results);
}

extern "C" {

// episodes [n], stat_sums [n][10], the marks of the same shapes, agent_member / opp_member [ceil(n / 16)], results [pool_size][pool_size][11]
long long sat_tally(const u64 *episodes, const double *stat_sums, u64 *mark_episodes, double *mark_sums, const uint8_t *agent_member,
                    const uint8_t *opp_member, int n_games, int pool_size, double *results)
{
    if (n_games < 1 || pool_size < 1 || pool_size > 255) return -1;
    TallyJob j = {episodes, stat_sums, mark_episodes, mark_sums, agent_member, opp_member, (u32)n_games, (u32)pool_size, results};
    simt::g_grid_dim = {(unsigned)pool_size, 1, 1};
    long long ops = 1;
    for (unsigned blk = 0; blk < (unsigned)pool_size; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        ops += (long long)simt::run_workgroup(tally_lane, &j, 1);
    }
    return ops;
}

}
