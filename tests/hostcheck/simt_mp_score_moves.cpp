// simt_mp_score_moves.cpp -- TEST-ONLY: azul_x_score_moves_kernel (csrc/azul_x_kernels.hpp on azx::score_moves_body_x of csrc/azul_rules_x.hpp,
// UNMODIFIED) compiled by g++ and run lane by lane in lockstep (simt/simt.hpp) on host memory over a BATCH of 256-byte wide records, two
// games per wave (an odd count leaves the last wave's upper half without a game), so that it can be diffed against the model composed from
// the oracle (tests/mp_score_moves_model.py) before a GPU sees it.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_x_kernels.hpp"
#include "simt_x_common.hpp"

struct SJob { azx::XBatchDev b; azx::XScoreMoves a; };

template <u32 P, u32 D>
static void lane_run(void *arg)
{
    SJob *j = (SJob *)arg;
    azul_x_score_moves_kernel<P, D>(j->b, j->a);
}

extern "C" {

// rows of active / scores / best belong to games 0 .. n_games - 1; scores ([n_games][30 (displays + 1)]) and best are each optional.  The
// batch's MT19937 states, positions and counters are handed in like every wide shim's, so that the caller can compare them before and after;
// the sampler table stays NULL: the kernel must not read it.  Returns the number of cross-lane operations executed, or a negative number
// on bad arguments.
long long shx_score_moves(int n_games, int players, int displays, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum,
                          int first_player, int pool, int end_bonus, int short_deal, int persp, const uint8_t *active, i32 *scores, i32 *best)
{
    lane_fn fn = x_for_shape(players, displays, [](auto s) { return (lane_fn)lane_run<s.P, s.D>; });
    if (!fn || n_games <= 0) return -1;
    SJob j;
    memset(&j, 0, sizeof(j));
    j.b = x_batch(n_games, state, mt, mtpos, episodes, stuck, stat_sum, first_player, pool, end_bonus, short_deal, nullptr);
    j.a.active = active; j.a.scores = scores; j.a.best = best; j.a.persp = persp;
    return x_launch(fn, &j, ((unsigned)n_games + 1u) / 2u, 1u);
}

}
