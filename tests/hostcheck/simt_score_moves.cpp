// simt_score_moves.cpp -- TEST-ONLY: azul_score_moves_kernel (csrc/azul_selfplay_kernels.hpp on azul_ops2.hpp, azul_env2.hpp and azul_selfplay2.hpp, all
// UNMODIFIED), compiled by g++ and run lane by lane in lockstep (simt/simt.hpp) on host memory over a BATCH of 128-byte records, two games
// per wave (an odd count leaves the last wave's upper half without a game), in the manner of simt_ops2.cpp's sh2_op_batch.
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_selfplay_kernels.hpp"

struct ScoreJob { BatchDev b; ScoreMovesArgs a; int lid; };
static void score_main(void *arg)
{
    ScoreJob *j = (ScoreJob *)arg;
    if (j->lid) azul_score_moves_kernel<true>(j->b, j->a); else azul_score_moves_kernel<false>(j->b, j->a);
}

extern "C" {

// rows of active / scores / best belong to games 0 .. n - 1; scores and best are each optional.  The kernel takes no MT19937 state and
// no counters: the batch's pointers to them stay NULL, so a write to either would fault here.
int shs_score_moves(int n, const uint8_t *recs, int tile_pool, int persp, const uint8_t *active, i32 *scores, i32 *best)
{
    if (n <= 0) return -1;
    ScoreJob j;
    memset(&j, 0, sizeof(j));
    j.b.state = (uint8_t *)recs; j.b.n = (u32)n;
    j.b.rules.first_player = 0; j.b.rules.tile_pool = (u32)tile_pool; j.b.draw_margin = AZ_DRAW_MARGIN;
    j.a.active = active; j.a.scores = scores; j.a.best = best; j.a.persp = persp;
    j.lid = tile_pool == POOL_LID;
    const unsigned blocks = ((unsigned)n + 1u) / 2u;
    simt::g_grid_dim = {blocks, 1, 1};
    for (unsigned blk = 0; blk < blocks; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        simt::run_workgroup(score_main, &j, 1, simt::STACK_BYTES);
    }
    return 0;
}

}
