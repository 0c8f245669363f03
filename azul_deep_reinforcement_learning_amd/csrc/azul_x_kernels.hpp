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

// ---- host side: the five compiled (players, displays) shapes, the ONE list of them for the library (azul_kernels.hip) and the lockstep
// emulation (tests/hostcheck): f(XShape<P, D>()) -- a kernel of that shape, s.P and s.D being constants -- for a batch's shape, nullptr
// for any other (azul_batch_create_rules admits only these five)
template <u32 P_, u32 D_>
struct XShape { static constexpr u32 P = P_, D = D_; };

template <class F>
static auto x_for_shape(int players, int displays, F f) -> decltype(f(XShape<2, 5>()))
{
    const int pd = players * 16 + displays;
    if (pd == 2 * 16 + 5) return f(XShape<2, 5>());
    if (pd == 3 * 16 + 5) return f(XShape<3, 5>());
    if (pd == 3 * 16 + 7) return f(XShape<3, 7>());
    if (pd == 4 * 16 + 5) return f(XShape<4, 5>());
    if (pd == 4 * 16 + 9) return f(XShape<4, 9>());
    return nullptr;
}

// The flat self-play kernel of a shape for the trajectory streams `v` (azul_common.hpp: selfplay_variant).  The wide kernels have no
// unpadded OUT 1 form: such rows go through OUT 2's run-time subset.
typedef void (*x_selfplay_kernel_t)(azx::XBatchDev, azx::XTraj);
template <u32 P, u32 D>
static x_selfplay_kernel_t x_selfplay_kernel_of(SelfplayVariant v)
{
    if (v.out == 0) return azul_x_selfplay_kernel<P, D, 0, false, false>;
    if (v.out == 1 && v.pad && v.bits) return azul_x_selfplay_kernel<P, D, 1, true, true>;
    if (v.out == 1 && v.pad) return azul_x_selfplay_kernel<P, D, 1, true, false>;
    return azul_x_selfplay_kernel<P, D, 2, false, false>;
}
static x_selfplay_kernel_t x_selfplay_kernel(int players, int displays, SelfplayVariant v)
{
    return x_for_shape(players, displays, [&](auto s) { return x_selfplay_kernel_of<s.P, s.D>(v); });
}
