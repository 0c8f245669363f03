// azul_x_kernels.hpp -- the rule kernels of WIDE batches (the 256-byte record: 3 / 4 players, extended rules; row N4) as a header, the wide
// twin of azul_selfplay_kernels.hpp: the __global__ functions that own the LDS around azul_rules_x.hpp's bodies.  azul_kernels.hip
// includes this file; tests/hostcheck/simt_rules_x.cpp, simt_runner_x.cpp and simt_net_x.cpp compile it UNMODIFIED with g++ and launch
// these kernels under the lockstep wave emulation, so the CPU check and the sanitizer passes cover the kernels themselves (the LDS as
// declared here, the XCD-aware game placement), not a restatement.  (The two window kernels of wide batches sit at the end of
// azul_rollout2.hpp, next to the two-player one.)
#pragma once
#include "azul_rules_x.hpp"

// Rule entries for batches of three / four players and for extended-rule batches (row N4): one launch = one rule call per game, two games
// per wavefront (azx::op_body_x).  grid = ceil(count / 2) one-wave workgroups.
template <u32 P, u32 D>
__global__ void __launch_bounds__(64) azul_x_op_kernel(azx::XBatchDev b, azx::XOp a)
{
    __shared__ u32 mt_lds[2][624];
    __shared__ double2 tab_lds[azx::Dim<D>::TROWS * T_STRIDE];
    azx::op_body_x<P, D>(b, a, blockIdx.x, mt_lds, tab_lds);
}

// Their flat random-agent self-play, persistent like azul_selfplay2_kernel (two games per wavefront, state in VGPRs, MT19937 streams and
// their tempered copies in LDS, XCD-aware game placement).
template <u32 P, u32 D, int OUT, bool PAD, bool BITS>
__global__ void __launch_bounds__(64) azul_x_selfplay_kernel(azx::XBatchDev b, azx::XTraj t)
{
    __shared__ u32 mt_lds[2][624];
    __shared__ u32 mtt_lds[2][624];
    __shared__ double2 tab_lds[azx::Dim<D>::TROWS * T_STRIDE];
    const u32 nb = gridDim.x, xcd = blockIdx.x & 7u, q8 = nb >> 3, rem = nb & 7u;
    const u32 wave_id = xcd * q8 + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);      // every XCD plays a contiguous range of games
    azx::selfplay_body_x<P, D, OUT, PAD, BITS>(b, t, wave_id, mt_lds, mtt_lds, tab_lds);
}

// GameRunner for P seats on the wide record (azul_batch_mp_* entries; azx::runner_body_x in azul_rules_x.hpp): one runner call per game, two games per wavefront
// (azx::runner_body_x), the game in VGPRs from the agent's move through the replies, the reset and the observation.
template <u32 P, u32 D>
__global__ void __launch_bounds__(64) azul_x_runner_kernel(azx::XBatchDev b, azx::XRun a)
{
    __shared__ u32 mt_lds[2][624];
    __shared__ double2 tab_lds[azx::Dim<D>::TROWS * T_STRIDE];
    azx::runner_body_x<P, D>(b, a, blockIdx.x, mt_lds, tab_lds);
}

// The same GameRunner with an EXTERNAL opponent (azul_batch_mp_net_* entries; azx::net_body_x): one cut of the protocol per launch -- the
// agent's move, one opponent_move() of every game that owes one, or the fresh game -- and what the opponent is handed.  A kernel of its own:
// azul_x_runner_kernel's register budget stays as it is.
template <u32 P, u32 D>
__global__ void __launch_bounds__(64) azul_x_net_kernel(azx::XBatchDev b, azx::XNet a)
{
    __shared__ u32 mt_lds[2][624];
    azx::net_body_x<P, D>(b, a, blockIdx.x, mt_lds);
}

// Every legal move's what-if margin and the greedy choice of wide batches (azx::score_moves_body_x), the games untouched: two games per
// wavefront, the game in VGPRs, no LDS.  grid = ceil(n / 2) one-wave workgroups.
template <u32 P, u32 D>
__global__ void __launch_bounds__(64) azul_x_score_moves_kernel(azx::XBatchDev b, azx::XScoreMoves a)
{
    azx::score_moves_body_x<P, D>(b, a, blockIdx.x);
}
