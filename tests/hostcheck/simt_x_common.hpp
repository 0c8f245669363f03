// simt_x_common.hpp -- TEST-ONLY: what the shims of the WIDE kernels share (simt_rules_x.cpp, simt_runner_x.cpp, simt_net_x.cpp,
// simt_mp_score_moves.cpp, simt_x_rollout.cpp): the RandomAgent table of a display count, the azx::XBatchDev every entry builds from its
// arguments, and the launch loop.  The shims call the product's __global__ functions (csrc/azul_x_kernels.hpp, csrc/azul_rollout2.hpp),
// picked for a (players, displays) by the product's own selectors over its one list of shapes (csrc/azul_x_kernels.hpp: x_for_shape),
// and declare no LDS of their own.  Included after those headers.
#pragma once

typedef void (*lane_fn)(void *);

// the sampling table of a batch with `displays` displays (azul_batch_create builds the same: 5 (displays + 1) + 1 rows), or nullptr
static const double2 *table_for(int displays)
{
    static double tabs[3][51 * T_STRIDE * 2];
    static bool built[3] = {false, false, false};
    const int i = displays == 5 ? 0 : displays == 7 ? 1 : 2;
    if (!built[i]) { if (!build_sample_pairs(5 * (displays + 1) + 1, tabs[i])) return nullptr; built[i] = true; }
    return (const double2 *)tabs[i];
}

// the arguments every shx_* / sxr_* entry takes -> the batch as the kernels see it (margin 0: the library's default)
static azx::XBatchDev x_batch(int n_games, uint8_t *state, u32 *mt, u32 *mtpos, u64 *episodes, u32 *stuck, double *stat_sum, int first_player, int pool,
                              int end_bonus, int short_deal, const double2 *tab, unsigned long long margin = 0)
{
    return {state, mt, mtpos, episodes, stuck, stat_sum, (u32)n_games, margin ? margin : AZ_DRAW_MARGIN,
            {(u32)first_player, (u32)pool, (u32)end_bonus, (u32)short_deal}, tab, nullptr};
}

// one launch: `blocks` workgroups of `waves` wavefronts, blockIdx.x / gridDim.x as the launch gives them.  Returns the number of
// cross-lane operations executed.
static long long x_launch(lane_fn fn, void *job, unsigned blocks, unsigned waves)
{
    simt::g_grid_dim = {blocks, 1, 1};
    long long ops = 0;
    for (unsigned blk = 0; blk < blocks; blk++) {
        simt::g_block_idx = {blk, 0, 0};
        ops += (long long)simt::run_workgroup(fn, job, (int)waves, waves == 1u ? (size_t)simt::STACK_BYTES : (size_t)(256u << 10));
    }
    return ops;
}
