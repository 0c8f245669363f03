// simt_playout_policy.cpp -- TEST-ONLY: the playout kernels under a chosen playout policy (azul_playout_moves_kernel / azul_playout_policy_kernel of
// csrc/azul_selfplay_kernels.hpp on azul_ops2.hpp, azul_env2.hpp and azul_selfplay2.hpp, with the Philox block of azul_policy.hpp, all
// UNMODIFIED), compiled by g++ and run lane by lane in lockstep (simt/simt.hpp) on host memory over a BATCH of 128-byte records, two games
// per wave, in the manner of simt_playout_moves.cpp.  The instantiation is the library's choice: playout_moves_kernel(lid, policy).
#define __HIPCC__ 1
#include "azul_hip.h"
#include "azul_common.hpp"
#include "azul_tables.hpp"
using namespace az;
#include "azul_selfplay_kernels.hpp"
#include "azul_policy.hpp"

struct PlayoutJob { BatchDev b; PlayoutMovesArgs a; playout_moves_kernel_t k; };
static void playout_main(void *arg)
{
    PlayoutJob *j = (PlayoutJob *)arg;
    j->k(j->b, j->a);
}

extern "C" {

// shp_playout_moves' arguments (simt_playout_moves.cpp) and the policy's two; the ranges are the library entry's (the shim launches, it does
// not validate: the caller passes what azul_batch_playout_moves_policy admits)
int shp_playout_policy(int n, const uint8_t *recs, int tile_pool, uint32_t id_base, int persp, int playouts, int policy, int explore,
                       uint64_t seed, uint32_t call, const uint8_t *active, i32 *sums, i32 *best)
{
    if (n <= 0 || (policy != AZUL_PLAYOUT_UNIFORM && policy != AZUL_PLAYOUT_GREEDY) || explore < 0 || explore > 255) return -1;
    PlayoutJob j;
    memset(&j, 0, sizeof(j));
    j.b.state = (uint8_t *)recs; j.b.n = (u32)n; j.b.id_base = id_base;
    j.b.rules.first_player = 0; j.b.rules.tile_pool = (u32)tile_pool; j.b.draw_margin = AZ_DRAW_MARGIN;
    j.a.active = active; j.a.sums = sums; j.a.best = best; j.a.persp = persp;
    j.a.playouts = (u32)playouts; j.a.seed = seed; j.a.call = call; j.a.policy = (u32)policy; j.a.explore = (u32)explore;
    j.k = playout_moves_kernel(tile_pool == POOL_LID, policy);
    const unsigned blocks = ((unsigned)n + 1u) / 2u;
    simt::g_grid_dim = {blocks, 1, 1};
    for (unsigned blk = 0; blk < blocks; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        simt::run_workgroup(playout_main, &j, 1, simt::STACK_BYTES);
    }
    return 0;
}

}
