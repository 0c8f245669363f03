// azul_rollout2.hpp -- the persistent policy rollout (row N1 / N2: the batched NNRunner.run_episode loop, nn_runner.py:17-47) with the
// ENV SIDE ON THE VECTOR PIPE: a workgroup of 8 waves owns 16 games for a whole window, wave w plays games 2w and 2w + 1 in its two
// 32-lane halves with azul_selfplay2.hpp's rules (state in VGPRs, half-uniform), and the same 8 waves run the network on the f32
// matrix cores between the env phases.  Included by azul_kernels.hip after azul_policy.hpp; the __global__ functions of the wide window
// kernels are at the end of this file.
//
// Why on the vector pipe: rounds 1-2 ran sixteen one-game waves per workgroup whose rule code sat on the CU's ONE scalar ALU, and every
// move waited for the slowest of the sixteen games (env step 6.2 k + waiting 7.2 k of 33.2 k cycles per move; LABNOTES.md).  Here a move's
// env work is ~500 vector instructions per PAIR of games.
//
// Arithmetic per output element: the same k-ordered v_mfma_f32_16x16x4_f32 chain per hidden unit / logit, the same critic summation and
// the same head as azul_policy_forward_kernel, and the rules are azul_selfplay2.hpp's: the trajectories are bit-identical to the
// two-launches-per-move path (tests/test_policy_bridge.py, tests/test_full_size_configs.py).
// Four opponents (template parameter OPP): 0 the policy moves for both players; 1 GameRunner with its default RandomAgent inside the env
// phase; 2 GameRunner(opponent=Agent(...)) (game_runner.py:27-30) -- a SECOND network: after the agent's move the workgroup runs matrix phases
// on the opponent's weights while any of its 16 games owes an opponent_move() (azul_env2.hpp: the NET_* protocol); 3 the scripted greedy
// player of the reference's own reward (azul_env2.hpp: greedy_pick2) on the same protocol, answered inside the env phase by the wave itself.
// Reference lines: azulnet/azul.py:296-313 (step), azulnet/game_runner.py:27-30, 37-55 (opponent_move, GameRunner.step), :56-72 (get_state),
// :76-85 (reset), :87-97 (RandomAgent); azulnet/agent.py:64-81; azulnet/nn_runner.py:17-47.
#pragma once

#include "azul_env2.hpp"
#include "azul_x_kernels.hpp"   // the wide-record rules of x_policy_rollout_body below (azul_rules_x.hpp) and the list of compiled shapes

constexpr u32 PR2_WAVES = 8;
constexpr u32 PR2_AHEAD = 6;       // k-steps of layer-1 weights in flight (3..6 measured alike, 8 and 12 slower: profiles/round3_policy_rollout_phases.txt)
constexpr int PR2_ADEPTH = 4;      // A fragments read from LDS this many k-steps ahead

// The first weight fragments of a matrix phase are REQUESTED A PHASE EARLIER (layer 1's before the env step, layer 2's before layer 1's
// epilogue) and stay in flight across the LDS-only barriers: the matrix pipe does not wait for L2 after each barrier.
constexpr int PR2_HOIST1 = 4;
constexpr int PR2_HOIST2 = 6;      // (2..6 measured alike, 8 and 12 slower: too many layer-2 fragments in flight hold up layer 1's tail)
#define PR2_LOAD1(vo, s) __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs1, vo, (4 * (s)) * PF_H2 * 4, 0))
// waves 0..3: FOUR adjacent hidden columns per lane and k-step in one 16-byte load (two column pairs)
#define PR2_LOAD1Q(vo, s) __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs1, vo, (4 * (s)) * PF_H2 * 4, 0))
#define PR2_LOAD2(NT_, s) ((NT_) == 2 ? __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rs2, voff, (4 * (s)) * PF_ACT * 4, 0)) \
                                      : make_float2(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs2, voff, (4 * (s)) * PF_ACT * 4, 0)), 0.f))

__device__ __forceinline__ void pr2_request1(bool two, const __amdgpu_buffer_rsrc_t rs1, u32 voffA, u32 voffB, float2 (&preA)[PR2_HOIST1],
                                             float2 (&preB)[PR2_HOIST1])
{
    if (two) {
#pragma unroll
        for (int s = 0; s < PR2_HOIST1; s++) { const float4 t = PR2_LOAD1Q(voffA, s); preA[s] = make_float2(t.x, t.y); preB[s] = make_float2(t.z, t.w); }
    } else {
#pragma unroll
        for (int s = 0; s < PR2_HOIST1; s++) preA[s] = PR2_LOAD1(voffA, s);
    }
    (void)voffB;
}

__device__ __forceinline__ void pr2_request2(bool two, const __amdgpu_buffer_rsrc_t rs2, u32 voff, float2 (&pre)[PR2_HOIST2])
{
    if (two) {
#pragma unroll
        for (int s = 0; s < PR2_HOIST2; s++) pre[s] = PR2_LOAD2(2, s);
    } else {
#pragma unroll
        for (int s = 0; s < PR2_HOIST2; s++) pre[s] = PR2_LOAD2(1, s);
    }
}

// layer 1 of one wave: NP pairs of adjacent hidden columns per lane (8-byte loads), 136-deep, one 16-row tile
template <int NP>
__device__ __forceinline__ void pr2_layer1(const __amdgpu_buffer_rsrc_t rs1, u32 voffA, u32 voffB, const float *ap, const float2 (&preA)[PR2_HOIST1],
                                           const float2 (&preB)[PR2_HOIST1], pf_f32x4 (&acc)[4], u64 *t_loop = nullptr /* diagnostic build: stamp at the loop's entry */)
{
    float2 bwA[PF_IN / 4], bwB[PF_IN / 4];
#pragma unroll
    for (int s = 0; s < PR2_HOIST1; s++) { bwA[s] = preA[s]; if (NP == 2) bwB[s] = preB[s]; }
#pragma unroll
    for (int s = PR2_HOIST1; s < (int)PR2_AHEAD; s++) {
        if (NP == 2) { const float4 t = PR2_LOAD1Q(voffA, s); bwA[s] = make_float2(t.x, t.y); bwB[s] = make_float2(t.z, t.w); }
        else bwA[s] = PR2_LOAD1(voffA, s);
    }
    // A fragments PR2_ADEPTH k-steps ahead: a step is only 64..128 cycles of matrix pipe per wave, an LDS round trip is longer
    float af[PF_IN / 4];
#pragma unroll
    for (int s = 0; s < PR2_ADEPTH; s++) af[s] = ap[4 * s];
    __builtin_amdgcn_sched_barrier(0);
    if (t_loop) *t_loop = __builtin_amdgcn_s_memtime();
#pragma unroll
    for (int s = 0; s < PF_IN / 4; s++) {
        if (s + (int)PR2_AHEAD < PF_IN / 4) {
            if (NP == 2) { const float4 t = PR2_LOAD1Q(voffA, s + PR2_AHEAD); bwA[s + PR2_AHEAD] = make_float2(t.x, t.y); bwB[s + PR2_AHEAD] = make_float2(t.z, t.w); }
            else bwA[s + PR2_AHEAD] = PR2_LOAD1(voffA, s + PR2_AHEAD);
        }
        if (s + PR2_ADEPTH < PF_IN / 4) af[s + PR2_ADEPTH] = ap[4 * (s + PR2_ADEPTH)];
        const float av = af[s];
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bwA[s].x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bwA[s].y, acc[1], 0, 0, 0);
        if (NP == 2) {
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bwB[s].x, acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bwB[s].y, acc[3], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// layer 2 of one wave: NT logit columns per lane (NT == 2: one 8-byte load, NT == 1: one 4-byte load per k-step), 180-deep
// (`draw`: the wave also draws its head rows' uniforms -- Philox4x32-10 does not depend on the logits.  Its ten rounds are spread over
// the first twenty k-steps, half a round each: the quarter-rate 32-bit multiplies issue in the shadow of the MFMAs instead of holding
// up the head phase; philox_u32's arithmetic, statement for statement)
template <int NT>
__device__ __forceinline__ void pr2_layer2(const __amdgpu_buffer_rsrc_t rs2, u32 voff, const float *ap, const float2 (&pre)[PR2_HOIST2], pf_f32x4 &acc0,
                                           pf_f32x4 &acc1, bool draw, u64 seed, u64 ctr, u32 game, float &u_out, u64 *t_loop = nullptr)
{
    float2 bw[PF_HID / 4];
#pragma unroll
    for (int s = 0; s < PR2_HOIST2; s++) bw[s] = pre[s];
    float af[PF_HID / 4];
#pragma unroll
    for (int s = 0; s < PR2_ADEPTH; s++) af[s] = ap[4 * s];
    u32 c0 = (u32)ctr, c1 = (u32)(ctr >> 32), c2 = game, c3 = 0x415A554Cu, k0 = (u32)seed, k1 = (u32)(seed >> 32), hi0 = 0, lo0 = 0;
    __builtin_amdgcn_sched_barrier(0);
    if (t_loop) *t_loop = __builtin_amdgcn_s_memtime();
#pragma unroll
    for (int s = 0; s < PF_HID / 4; s++) {
        if (s + PR2_HOIST2 < PF_HID / 4) bw[s + PR2_HOIST2] = PR2_LOAD2(NT, s + PR2_HOIST2);
        if (s + PR2_ADEPTH < PF_HID / 4) af[s + PR2_ADEPTH] = ap[4 * (s + PR2_ADEPTH)];
        const float av = af[s];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[s].x, acc0, 0, 0, 0);
        if (NT == 2 && s < 20) {
            if (draw) {
                if ((s & 1) == 0) { hi0 = __umulhi(0xD2511F53u, c0); lo0 = 0xD2511F53u * c0; }
                else {
                    const u32 hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
                    const u32 n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
                    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
                    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
                }
            }
        }
        if (NT == 2) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[s].y, acc1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (NT == 2 && draw) u_out = (float)(c0 >> 8) * (1.0f / 16777216.0f);
}


// ---- network opponent (OPP == 2; game_runner.py:27-30 GameRunner(opponent=Agent(...))) ---------------------------------------------------
// The opponent only ever runs forward_actor (agent.py:73-81 -> model.py:28-41): layer 1 is the ACTOR half alone, 180 hidden columns
// (columns 180..359 of its k-major w1t), spread over the eight waves like layer 2's 180 logits -- waves 0..3 a column pair per lane
// (32w + 2c + j, one 8-byte load per k-step), waves 4..7 one column (128 + 16 (w - 4) + c): three 16x16 tiles per SIMD, 136-deep.  Each
// hidden unit is the same k-ordered v_mfma_f32_16x16x4_f32 chain as in azul_policy_forward_kernel, so a reply equals the per-move path's.
constexpr int PR2_HOISTO = 4;
constexpr u32 NET_MAX_REPLIES = 64;   // an opponent_move() takes tiles off the table: a chain of replies ends with the round (<= 21 moves)
#define PR2_LOADO(NT_, s) ((NT_) == 2 ? __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rso, voff, (4 * (s)) * PF_H2 * 4, 0)) \
                                      : make_float2(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rso, voff, (4 * (s)) * PF_H2 * 4, 0)), 0.f))

__device__ __forceinline__ void pr2_request_opp1(bool two, const __amdgpu_buffer_rsrc_t rso, u32 voff, float2 (&pre)[PR2_HOISTO])
{
    if (two) {
#pragma unroll
        for (int s = 0; s < PR2_HOISTO; s++) pre[s] = PR2_LOADO(2, s);
    } else {
#pragma unroll
        for (int s = 0; s < PR2_HOISTO; s++) pre[s] = PR2_LOADO(1, s);
    }
}

template <int NT>
__device__ __forceinline__ void pr2_opp_layer1(const __amdgpu_buffer_rsrc_t rso, u32 voff, const float *ap, const float2 (&pre)[PR2_HOISTO], pf_f32x4 &acc0,
                                               pf_f32x4 &acc1)
{
    float2 bw[PF_IN / 4];
#pragma unroll
    for (int s = 0; s < PR2_HOISTO; s++) bw[s] = pre[s];
    float af[PF_IN / 4];
#pragma unroll
    for (int s = 0; s < PR2_ADEPTH; s++) af[s] = ap[4 * s];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < PF_IN / 4; s++) {
        if (s + PR2_HOISTO < PF_IN / 4) bw[s + PR2_HOISTO] = PR2_LOADO(NT, s + PR2_HOISTO);
        if (s + PR2_ADEPTH < PF_IN / 4) af[s + PR2_ADEPTH] = ap[4 * (s + PR2_ADEPTH)];
        const float av = af[s];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[s].x, acc0, 0, 0, 0);
        if (NT == 2) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bw[s].y, acc1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// OPP: 0 the policy moves for both players, 1 GameRunner with the RandomAgent opponent, 2 GameRunner with a NETWORK opponent (a.Wopp),
// 3 GameRunner with the one-ply GREEDY opponent (az2::greedy_pick2: no weights, no matrix phase, no draw)
// ARENA (OPP 2 only; azul_batch_policy_rollout_arena): the kernel's weights are a stacked pool too and a.agent_member picks the workgroup's
// agent from it -- a base offset per array chosen once, wave-uniform; everything the agent side reads goes through W below.  A template
// flag, so that every other instantiation compiles exactly as before.
template <bool LID, int OPP, bool ARENA = false>
__global__ void __launch_bounds__(64 * PR2_WAVES) azul_policy_rollout2_kernel(BatchDev b, PolicyWeights Wk, RolloutArgs a)
{
    static_assert(!ARENA || OPP == 2, "the arena is the network-opponent kernel with a pool behind the agent seat");
    PolicyWeights W = Wk;
    if constexpr (ARENA) W = league_member<(u32)PF_IN, (u32)PF_ACT>(Wk, arena_agent_of_block(a));
    __shared__ float obsS[PF_GAMES * PF_OBS_STRIDE];
    __shared__ float hidS[PF_GAMES * PF_HID_STRIDE];
    __shared__ float lgS[PF_GAMES * PF_LOG_STRIDE];
    __shared__ float w2cS[PF_HID];
    __shared__ float b1S[PF_H2 + 24], b2aS[PF_ACT + 12];
    __shared__ u32 mtS[PF_GAMES][az2::MT_LDS_WORDS];
    __shared__ double2 tabfs_lds[T_PAIRS];
    __shared__ u64 maskS[PF_GAMES][4];
    __shared__ i32 actS[PF_GAMES];
    __shared__ float b1oS[OPP == 2 ? PF_HID + 12 : 1], b2aoS[OPP == 2 ? PF_ACT + 12 : 1];      // the opponent's actor biases
    __shared__ u32 oweS[PF_GAMES];                       // OPP == 2: does game i of the workgroup owe an opponent_move()?
    const u32 tid = threadIdx.x, lane = tid & 63u, l = lane & 31u, half = lane >> 5, c = lane & 15u, q = (lane >> 4) & 3u;
    const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const u32 n = b.n, g0 = blockIdx.x * PF_GAMES, gl = 2u * w + half, gi = g0 + gl;
    const bool live = gi < n;
    const u32 gic = live ? gi : n - 1u;
    u64 counter = a.counter;
    if (a.counter_dev) counter += a.counter_dev[0];
    if (tid < (u32)PF_HID) w2cS[tid] = W.w2c[tid];
    if (tid < (u32)(PF_H2 + 24)) b1S[tid] = tid < (u32)PF_H2 ? W.b1[tid] : 0.f;
    if (tid < (u32)(PF_ACT + 12)) b2aS[tid] = tid < (u32)PF_ACT ? W.b2a[tid] : 0.f;
    if (OPP == 1) {
        for (u32 i = tid; i < (u32)T_PAIRS; i += 64u * PR2_WAVES) tabfs_lds[i] = b.tab[i];
    }
    // the opponent's net (OPP == 2): a.Wopp itself, or with a league (a.opp_member) the pool member of this workgroup's 16 games -- a base
    // offset per array chosen once, wave-uniform; everything the workgroup reads of the opponent goes through Wo
    PolicyWeights Wo = OPP == 2 ? a.Wopp : W;
    if (OPP == 2) {
        if (a.opp_member) Wo = league_member<(u32)PF_IN, (u32)PF_ACT>(a.Wopp, league_member_of_block(a));
        if (tid < (u32)(PF_HID + 12)) b1oS[tid] = tid < (u32)PF_HID ? Wo.b1[PF_HID + tid] : 0.f;
        if (tid < (u32)(PF_ACT + 12)) b2aoS[tid] = tid < (u32)PF_ACT ? Wo.b2a[tid] : 0.f;
        if (tid < (u32)PF_GAMES) oweS[tid] = 0u;
    }
    const float b2c_v = W.b2c[0];

    // matrix-phase constants of this wave: layer 2 columns 32w + 2c + j (waves 0..3) or 128 + 16 (w - 4) + c (waves 4..7) -- three
    // 16x16 tiles per SIMD (waves w and w + 4 share one); layer 1 likewise with twice the tiles (see there)
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void *)W.w1t, 0, PF_IN * PF_H2 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs2 = __builtin_amdgcn_make_buffer_rsrc((void *)W.w2a_t, 0, PF_HID * PF_ACT * 4, 0x00020000);
    const bool two = w < 4u;
#define PR2_L2COL0 (two ? 32u * w + 2u * c : 128u + 16u * (w - 4u) + c)

    // env state of this half's game
    az2::K2 k;
    az2::k2_init(k);
    az2::rng2_set_move_limit(mtS[gl], b.move_limit, l);
    az2::Tab2 tab = {tabfs_lds};
    az2::G2 g;
    uint8_t *rec = b.state + (size_t)gic * AZUL_RECORD_BYTES;
    az2::g2_load(g, rec, l);
    az2::prime2(g, k);
    az2::Rng2 r;
    u32 *gmt = b.mt + (size_t)gic * 624u;
    az2::rng2_open(r, gmt, mtS[gl], b.mtpos[gic], l);
    const u64 margin = b.draw_margin;
    az2::Counters2 cnt;
    az2::counters2_open(cnt, b.episodes + gic, b.stuck + gic, b.stat_sum + (size_t)gic * 10, l);
    u32 st_last = ST_OK;
    i32 win_rew = 0;
    u32 win_done = 0;
    float *orow = obsS + gl * PF_OBS_STRIDE;
    __syncthreads();                                     // tables / biases staged

    // observation + legal mask of the current state -> LDS (network / head) and trajectory slot `slot`
    az2::Mask2 m;                                        // legal mask of the published state: the next env step tests the action against it
    // The env phase only writes LDS (observation row, packed mask bits) + the player byte; the trajectory slot's 544-byte observation and
    // 180-byte mask of every game are copied out of LDS by flush() below, on waves that idle during the head phase: eleven vector
    // stores per game pair leave the env phase, which every other phase of the move waits for.
    // (publish_rows: the mask `m` already holds, seen from `persp`)
    auto publish_rows = [&](u32 persp) {
        if (l == 0u) {                                   // the 180 bits packed: the six 30-bit row words concatenated
            maskS[gl][0] = (u64)m.m[0] | ((u64)m.m[1] << 30) | ((u64)m.m[2] << 60);
            maskS[gl][1] = ((u64)m.m[2] >> 4) | ((u64)m.m[3] << 26) | ((u64)m.m[4] << 56);
            maskS[gl][2] = ((u64)m.m[4] >> 8) | ((u64)m.m[5] << 22);
        }
        az2::observe2(g, persp, orow, nullptr, l);
    };
    auto publish = [&](u32 slot, bool mask_current) {
        if (!mask_current) az2::legal_mask2(g, k, m);
        if (l == 0u) a.player[(size_t)slot * n + gi] = (uint8_t)g.cur;
        publish_rows(OPP ? 0u : az2::me2(g));
    };
    // trajectory slot `slot` of the workgroup's 16 games <- the LDS rows: the 16 x 136 floats are contiguous in the [T+1][N][136]
    // array (16-byte chunks), the 16 x 180 mask bytes in [T+1][N][180] (dwords: four bits of the packed mask spread into four bytes).
    // `idx` in 0..191 over the three copying waves.
    auto flush = [&](u32 slot, u32 idx) {
        const size_t cell0 = (size_t)slot * n + g0;
        float *og = a.obs + cell0 * PF_IN;
#pragma unroll
        for (u32 rep = 0; rep < 3u; rep++) {
            const u32 j = idx + 192u * rep;              // 16-byte chunk: row j / 34, floats 4 (j % 34) ..
            const u32 row = j / 34u, c4 = j - 34u * row;
            if (j < 16u * 34u && g0 + row < n) *(float4 *)(og + 4u * j) = *(const float4 *)(obsS + row * PF_OBS_STRIDE + 4u * c4);
        }
        u32 *mg = (u32 *)(a.mask + cell0 * AZUL_NUM_ACTIONS);
#pragma unroll
        for (u32 rep = 0; rep < 4u; rep++) {
            const u32 d = idx + 192u * rep;              // dword: row d / 45, actions 4 (d % 45) ..
            const u32 row = d / 45u, a0 = 4u * (d - 45u * row);
            if (d < 16u * 45u && g0 + row < n) {
                const u32 nib = (u32)(maskS[row][a0 >> 6] >> (a0 & 63u)) & 0xfu;
                mg[d] = (nib * 0x00204081u) & 0x01010101u;
            }
        }
    };
    if (live) publish(0u, false);
    else {
        orow[l] = 0.f; orow[l + 32u] = 0.f; orow[l + 64u] = 0.f; orow[l + 96u] = 0.f;
        if (l < 8u) orow[l + 128u] = 0.f;
        if (l == 0u) { maskS[gl][0] = 0; maskS[gl][1] = 0; maskS[gl][2] = 0; }
        if constexpr (OPP == 3) m = az2::Mask2{};        // (a half without a game offers the greedy player's candidate loop nothing)
    }

    // (waves 0..3: lane c owns the FOUR adjacent columns 64w + 4c .. + 3 -- one 16-byte load per k-step; waves 4..7: a pair, 8 bytes)
    const u32 colA = two ? 64u * w + 4u * c : 256u + 32u * (w - 4u) + 2u * c, colB = colA + 2u;
    const bool liveA = colA < (u32)PF_H2, liveB = two && colB < (u32)PF_H2;
    const u32 voffA = ((liveA ? colA : 0u) + q * (u32)PF_H2) * 4u, voffB = ((liveB ? colB : 0u) + q * (u32)PF_H2) * 4u;
    const u32 voff2 = ((PR2_L2COL0 < (u32)PF_ACT ? PR2_L2COL0 : 0u) + q * (u32)PF_ACT) * 4u;
    float2 preA[PR2_HOIST1], preB[PR2_HOIST1], pre2[PR2_HOIST2];
    pr2_request1(two, rs1, voffA, voffB, preA, preB);
    // the opponent's matrices (OPP == 2): the actor half of its layer 1 and its layer 2, both in layer 2's column mapping
    const __amdgpu_buffer_rsrc_t rso1 = __builtin_amdgcn_make_buffer_rsrc((void *)Wo.w1t, 0, PF_IN * PF_H2 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t rso2 = __builtin_amdgcn_make_buffer_rsrc((void *)Wo.w2a_t, 0, PF_HID * PF_ACT * 4, 0x00020000);
    const u32 voffo1 = ((u32)PF_HID + (PR2_L2COL0 < (u32)PF_HID ? PR2_L2COL0 : 0u) + q * (u32)PF_H2) * 4u;
    float2 preo[PR2_HOISTO];
    az2::NetStep ns;
    ns.pending = az2::NET_READY; ns.replies = 0; ns.rew = 0; ns.dn = 0; ns.closed = false; ns.st = ST_OK;
#if defined(AZ_PROFILE_SEGMENTS)
    u64 pr_acc[6] = {0, 0, 0, 0, 0, 0}, pr_last = __builtin_amdgcn_s_memtime();
    const u64 pr_t0 = pr_last, pr_r0 = __builtin_amdgcn_s_memrealtime();
#define PR2_STAMP(i) do { u64 now_ = __builtin_amdgcn_s_memtime(); pr_acc[i] += now_ - pr_last; pr_last = now_; } while (0)
    // matrix sub-phases of the two waves of SIMD 1 (w == 1: four / two tiles, w == 5: two / one): prologue (barrier release -> loop entry), the
    // MFMA loop's issue span, the epilogue (waits for the last results, bias + relu, LDS writes), the wait at the closing barrier
    u64 sub[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ts[4] = {0, 0, 0, 0}, tl = 0;
    u64 *const tlp = &tl;
#define PR2_SUB(i) do { ts[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define PR2_SUBACC(o) do { sub[(o)] += tl - ts[0]; sub[(o) + 1] += ts[1] - tl; sub[(o) + 2] += ts[2] - ts[1]; sub[(o) + 3] += ts[3] - ts[2]; } while (0)
#else
#define PR2_STAMP(i) do { } while (0)
#define PR2_SUB(i) do { } while (0)
#define PR2_SUBACC(o) do { } while (0)
    u64 *const tlp = nullptr;
#endif
#pragma unroll 1
    for (int t = 0; t < a.n_steps; t++) {
        const size_t row_t = (size_t)t * n;
        float u_head = 0.f;
        PR2_STAMP(0);                                    // own env step + publish
        lds_barrier();                                   // observations and mask bits of all 16 games are in LDS
        PR2_STAMP(1);                                    // waiting for the slowest env wave
        PR2_SUB(0);
        {
            // layer 1: pairs of adjacent hidden columns per lane (one 8-byte load per k-step and pair: a 16-lane group reads 128 contiguous
            // bytes of a k-row).  Waves 0..3 own two pairs, FOUR adjacent columns 64w + 4c + j (one 16-byte load per k-step), waves 4..7 one (256 + 32 (w - 4) +
            // 2c + j): 24 tiles over 8 waves, six per SIMD.
            pf_f32x4 acc[4];
            for (int j = 0; j < 4; j++) acc[j] = (pf_f32x4){0.f, 0.f, 0.f, 0.f};
            const float *ap = obsS + c * PF_OBS_STRIDE + q;
            if (two) pr2_layer1<2>(rs1, voffA, voffB, ap, preA, preB, acc, tlp);
            else pr2_layer1<1>(rs1, voffA, voffB, ap, preA, preB, acc, tlp);
            PR2_SUB(1);
            pr2_request2(two, rs2, voff2, pre2);         // layer 2's first fragments: in flight across the epilogue and the barrier
            for (int rr = 0; rr < 4; rr++) {             // C layout: column = lane & 15, row = 4 (lane >> 4) + rr
                float *hp = hidS + (4u * q + rr) * PF_HID_STRIDE;
                if (liveA) {
                    const float h0 = acc[0][rr] + b1S[colA], h1 = acc[1][rr] + b1S[colA + 1u];
                    hp[colA] = h0 > 0.f ? h0 : 0.f;      // F.relu, model.py:24/30
                    hp[colA + 1u] = h1 > 0.f ? h1 : 0.f;
                }
                if (liveB) {
                    const float h0 = acc[2][rr] + b1S[colB], h1 = acc[3][rr] + b1S[colB + 1u];
                    hp[colB] = h0 > 0.f ? h0 : 0.f;
                    hp[colB + 1u] = h1 > 0.f ? h1 : 0.f;
                }
            }
        }
        PR2_SUB(2);
        lds_barrier();
        PR2_STAMP(2);                                    // layer 1 (incl. barrier)
        PR2_SUB(3);
        PR2_SUBACC(0);
        PR2_SUB(0);
        {
            // layer 2 (actor)
            const u32 col0 = PR2_L2COL0;
            const bool live2 = col0 < (u32)PF_ACT;
            pf_f32x4 acc0 = (pf_f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
            const float *ap = hidS + c * PF_HID_STRIDE + PF_HID + q;
            const u32 hg_ = g0 + 4u * w + q;             // waves 0..3: the head row of this 16-lane group
            if (two) pr2_layer2<2>(rs2, voff2, ap, pre2, acc0, acc1, true, a.seed, counter + (u64)t, b.id_base + (hg_ < n ? hg_ : n - 1u), u_head, tlp);
            else pr2_layer2<1>(rs2, voff2, ap, pre2, acc0, acc1, false, 0, 0, 0, u_head, tlp);
            PR2_SUB(1);
            if (live2)
                for (int rr = 0; rr < 4; rr++) {
                    float *lp = lgS + (4u * q + rr) * PF_LOG_STRIDE + col0;
                    lp[0] = acc0[rr] + b2aS[col0];
                    if (two) lp[1] = acc1[rr] + b2aS[col0 + 1u];
                }
        }
        PR2_SUB(2);
        lds_barrier();
        PR2_STAMP(3);                                    // layer 2 + critic (incl. barrier)
        PR2_SUB(3);
        PR2_SUBACC(4);
        if (w < 4u) {
            // head: waves 0..3 (one per SIMD) sample four games each, 16 lanes per game
            const u32 hrow = 4u * w + q, hg = g0 + hrow;
            float x[HEAD_PER_LANE];
            const float *lg = lgS + hrow * PF_LOG_STRIDE + (c < 15u ? 12u * c : 0u);
            for (int j = 0; j < HEAD_PER_LANE; j++) x[j] = lg[j];
            const u64 M0 = maskS[hrow][0], M1 = maskS[hrow][1], M2 = maskS[hrow][2];
            const u32 bitpos = 12u * c, word = bitpos >> 6, off = bitpos & 63u;
            const u64 lo = word == 0u ? M0 : (word == 1u ? M1 : M2), hi = word == 0u ? M1 : M2;
            u64 field = lo >> off;
            if (off > 52u) field |= hi << (64u - off);
            const u32 okbits = c < 15u ? (u32)field & 0xfffu : 0u;
            policy_head_rows(x, lgS + hrow * PF_LOG_STRIDE, okbits, a.seed, counter + (u64)t, hg < n ? hg : n - 1u, lane, hg < n, a.action + row_t, a.logp + row_t,
                             a.entropy + row_t, b.id_base, actS + 4u * w, &u_head);
        } else if (w < 7u) {
            flush((u32)t, 64u * (w - 4u) + lane);        // waves 4..6: the trajectory slot of this move's decision
        } else {
            // the critic, on a wave that idles during the head, summed exactly like azul_policy_forward_kernel: lane (row c, quarter q)
            // sums k = q (mod 4), then the quarters are added (model.py:22-26)
            float sum = 0.f;
            const float *hp = hidS + c * PF_HID_STRIDE;
#pragma unroll
            for (int s = 0; s < PF_HID / 4; s++) sum = fmaf(hp[4 * s + q], w2cS[4 * s + q], sum);
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            if (q == 0u && g0 + c < n) a.value[row_t + g0 + c] = sum + b2c_v;
        }
        lds_barrier();
        PR2_STAMP(4);                                    // head (incl. barrier)
        if constexpr (OPP == 3) {
            // GameRunner.step against the GREEDY opponent (game_runner.py:43-55 with :37-42 answered by az2::greedy_pick2): OPP == 1's control
            // flow -- no extra barrier, no matrix phase -- on OPP == 2's protocol.  The answer is a pure function of the game this half holds,
            // so the reply rounds stay inside the wave: while EITHER half owes an opponent_move() both halves price their candidates (the loop
            // is wave-uniform) and only the half that owes plays; its sibling's game, mask, stream and counters are not touched.
            // ONE env site per pass, as with the network opponent: pass 0 plays the agent's action, pass j > 0 reply j - 1 of the halves that owe it
#pragma unroll 1
            for (u32 j = 0; j <= NET_MAX_REPLIES; j++) {
                const bool go = live && (j == 0u || ns.pending != az2::NET_READY);
                if (!az2::wave_any(go)) break;
                i32 av = actS[gl];
                if (j > 0u) {
                    av = az2::greedy_pick2<LID>(g, m, k);
                    if (go && l == 0u && a.opp_action && j - 1u < (u32)a.opp_slots) a.opp_action[((size_t)t * (size_t)a.opp_slots + (j - 1u)) * n + gi] = av;
                }
                if (go) az2::net_move2<LID>(g, av, j == 0u, m, b.rules.first_player, r, margin, cnt, k, ns);
            }
            pr2_request1(two, rs1, voffA, voffB, preA, preB);    // the next step's layer 1: in flight during the publish
            if (live) {
                if (ns.pending != az2::NET_READY) {              // (NET_MAX_REPLIES hit: cannot happen with legal replies; the slot reports it and moves on)
                    ns.pending = az2::NET_READY;
                    if (!ns.st) ns.st = ST_STUCK;
                    az2::legal_mask2(g, k, m);
                }
                st_last = ns.st;
                if (l == 0u) {
                    a.reward[row_t + gi] = ns.rew; a.done[row_t + gi] = (uint8_t)ns.dn;
                    if (a.opp_replies) a.opp_replies[row_t + gi] = (uint8_t)(ns.replies < 255u ? ns.replies : 255u);
                }
                win_rew = l == ((u32)t & 31u) ? ns.rew : win_rew;
                win_done = l == ((u32)t & 31u) ? ns.dn : win_done;
                publish((u32)t + 1u, true);                      // azr::net_settle left the mask of this state in `m`
            }
        } else if constexpr (OPP != 2) {
            pr2_request1(two, rs1, voffA, voffB, preA, preB);    // the next move's layer 1: in flight during the env step
            if (live) {
                const i32 av = actS[gl];
                i32 rew = 0;
                u32 dn = 0;
                if constexpr (OPP == 1) st_last = az2::agent_step2<LID>(g, av, m, b.rules.first_player, r, tab, margin, cnt, k, rew, dn);
                else st_last = az2::policy_step2<LID>(g, av, m, b.rules.first_player, r, margin, cnt, k, rew, dn);
                if (l == 0u) { a.reward[row_t + gi] = rew; a.done[row_t + gi] = (uint8_t)dn; }
                win_rew = l == ((u32)t & 31u) ? rew : win_rew;       // lane t of the half keeps step t (the returns scan below)
                win_done = l == ((u32)t & 31u) ? dn : win_done;
                publish((u32)t + 1u, false);
            }
        } else {
            // GameRunner.step against the NETWORK opponent (game_runner.py:43-55 with :37-42 answered by a.Wopp): the agent's move, then
            // matrix phases on the opponent's weights WHILE ANY of the workgroup's 16 games owes an opponent_move() -- its own replies and
            // player 1's forced moves (:46), after an episode end the opening moves of the next (:84) -- the other games sit masked
            // ONE env site per pass: pass 0 plays the agent's action, pass j > 0 reply j - 1 of the games that owed it
#pragma unroll 1
            for (u32 j = 0;; j++) {
                pr2_request_opp1(two, rso1, voffo1, preo);       // (almost every step has a reply: requested ahead like layer 1; speculative after that)
                if (live && (j == 0u || ns.pending != az2::NET_READY)) {
                    az2::net_move2<LID>(g, actS[gl], j == 0u, m, b.rules.first_player, r, margin, cnt, k, ns);
                    if (ns.pending != az2::NET_READY) publish_rows(az2::me2(g));   // what opponent_move hands the opponent (:38-39)
                }
                if (l == 0u) oweS[gl] = live && ns.pending != az2::NET_READY ? 1u : 0u;
                PR2_STAMP(0);                                    // (diagnostic build: the reply rounds' phases are added to the agent pass's)
                lds_barrier();                                   // every game's debt, observation row and mask bits are in LDS
                PR2_STAMP(1);
                const bool any = __builtin_amdgcn_ballot_w64(oweS[lane & 15u] != 0u) != 0ull;      // (the same 16 words in every wave)
                if (!any || j >= NET_MAX_REPLIES) break;
                const u64 okey = a.opp_seed == AZUL_POLICY_ARGMAX ? a.opp_seed : a.opp_seed + (u64)j;      // reply j of a step: its own Philox key
                const u32 col0 = PR2_L2COL0;
                {
                    pf_f32x4 acc0 = (pf_f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
                    const float *ap = obsS + c * PF_OBS_STRIDE + q;
                    if (two) pr2_opp_layer1<2>(rso1, voffo1, ap, preo, acc0, acc1);
                    else pr2_opp_layer1<1>(rso1, voffo1, ap, preo, acc0, acc1);
                    pr2_request2(two, rso2, voff2, pre2);
                    if (col0 < (u32)PF_HID)
                        for (int rr = 0; rr < 4; rr++) {
                            float *hp = hidS + (4u * q + rr) * PF_HID_STRIDE + PF_HID + col0;
                            const float h0 = acc0[rr] + b1oS[col0];
                            hp[0] = h0 > 0.f ? h0 : 0.f;         // F.relu, model.py:30
                            if (two) { const float h1 = acc1[rr] + b1oS[col0 + 1u]; hp[1] = h1 > 0.f ? h1 : 0.f; }
                        }
                }
                lds_barrier();
                PR2_STAMP(2);
                {
                    pf_f32x4 acc0 = (pf_f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
                    const float *ap = hidS + c * PF_HID_STRIDE + PF_HID + q;
                    const u32 hg_ = g0 + 4u * w + q;
                    if (two) pr2_layer2<2>(rso2, voff2, ap, pre2, acc0, acc1, true, okey, counter + (u64)t, b.id_base + (hg_ < n ? hg_ : n - 1u), u_head);
                    else pr2_layer2<1>(rso2, voff2, ap, pre2, acc0, acc1, false, 0, 0, 0, u_head);
                    if (col0 < (u32)PF_ACT)
                        for (int rr = 0; rr < 4; rr++) {
                            float *lp = lgS + (4u * q + rr) * PF_LOG_STRIDE + col0;
                            lp[0] = acc0[rr] + b2aoS[col0];
                            if (two) lp[1] = acc1[rr] + b2aoS[col0 + 1u];
                        }
                }
                lds_barrier();
                PR2_STAMP(3);
                if (w < 4u) {                                    // the opponent's sampling head (agent.py:76-80), waves 0..3, four games each
                    const u32 hrow = 4u * w + q, hg = g0 + hrow;
                    float x[HEAD_PER_LANE];
                    const float *lg = lgS + hrow * PF_LOG_STRIDE + (c < 15u ? 12u * c : 0u);
                    for (int jj = 0; jj < HEAD_PER_LANE; jj++) x[jj] = lg[jj];
                    const u64 M0 = maskS[hrow][0], M1 = maskS[hrow][1], M2 = maskS[hrow][2];
                    const u32 bitpos = 12u * c, word = bitpos >> 6, off = bitpos & 63u;
                    const u64 lo = word == 0u ? M0 : (word == 1u ? M1 : M2), hi = word == 0u ? M1 : M2;
                    u64 field = lo >> off;
                    if (off > 52u) field |= hi << (64u - off);
                    const u32 okbits = c < 15u ? (u32)field & 0xfffu : 0u;
                    const bool tr = hg < n && oweS[hrow] != 0u && a.opp_action && j < (u32)a.opp_slots;
                    const size_t trow = ((size_t)t * (size_t)(a.opp_slots > 0 ? a.opp_slots : 1) + (j < (u32)a.opp_slots ? j : 0u)) * n;
                    policy_head_rows(x, lgS + hrow * PF_LOG_STRIDE, okbits, okey, counter + (u64)t, hg < n ? hg : n - 1u, lane, tr,
                                     a.opp_action ? a.opp_action + trow : nullptr, a.opp_logp ? a.opp_logp + trow : nullptr, nullptr, b.id_base, actS + 4u * w,
                                     &u_head);
                }
                lds_barrier();
                PR2_STAMP(4);
            }
            pr2_request1(two, rs1, voffA, voffB, preA, preB);    // the next step's layer 1 on the agent's weights
            if (live) {
                if (ns.pending != az2::NET_READY) {              // (NET_MAX_REPLIES hit: cannot happen with legal replies; the slot reports it and moves on)
                    ns.pending = az2::NET_READY;
                    if (!ns.st) ns.st = ST_STUCK;
                    az2::legal_mask2(g, k, m);
                }
                st_last = ns.st;
                if (l == 0u) {
                    a.reward[row_t + gi] = ns.rew; a.done[row_t + gi] = (uint8_t)ns.dn;
                    if (a.opp_replies) a.opp_replies[row_t + gi] = (uint8_t)(ns.replies < 255u ? ns.replies : 255u);
                }
                win_rew = l == ((u32)t & 31u) ? ns.rew : win_rew;
                win_done = l == ((u32)t & 31u) ? ns.dn : win_done;
                publish((u32)t + 1u, true);                      // azr::net_settle left the mask of this state in `m`
            }
        }
    }
    lds_barrier();                                       // the rows of the state after the last move
    if (w >= 4u && w < 7u) flush((u32)a.n_steps, 64u * (w - 4u) + lane);
#if defined(AZ_PROFILE_SEGMENTS)
    if (lane == 0u && w == 5u) {
        for (int i = 0; i < 5; i++) atomicAdd((unsigned long long *)(b.prof + i), (unsigned long long)pr_acc[i]);
        const u64 pr_r1 = __builtin_amdgcn_s_memrealtime();
        atomicAdd((unsigned long long *)(b.prof + 6), (unsigned long long)(__builtin_amdgcn_s_memtime() - pr_t0));
        atomicAdd((unsigned long long *)(b.prof + 7), (unsigned long long)(pr_r1 - pr_r0));
        atomicMax((unsigned long long *)(b.prof + 5), (unsigned long long)((1ull << 62) - pr_r0));
        atomicMax((unsigned long long *)(b.prof + 8), (unsigned long long)pr_r1);
    }
    if (lane == 0u && (w == 1u || w == 5u))
        for (int i = 0; i < 8; i++) atomicAdd((unsigned long long *)(b.prof + 16 + (w == 5u ? 8 : 0) + i), (unsigned long long)sub[i]);
#endif
    if (live && a.returns && a.n_steps <= 32) {
        // the window's discounted returns (azul_returns_kernel's scan, statement for statement: q = reward + gamma * q backwards, an
        // episode end resets q; nn_runner.py:70-76) from the rewards / done flags this half kept in its lanes: no second launch
        float q = 0.f;
        float mine = 0.f;
#pragma unroll 1
        for (int t = a.n_steps - 1; t >= 0; t--) {
            const i32 rt = (i32)az2::hread((u32)win_rew, (u32)t);
            const u32 dt = az2::hread(win_done, (u32)t);
            if (dt) q = 0.f;
            q = (float)rt + a.gamma * q;
            mine = l == (u32)t ? q : mine;
        }
        if (l < (u32)a.n_steps) a.returns[(size_t)l * n + gi] = mine;
    }
    if (live) {
        az2::g2_store(g, rec, l);
        az2::rng2_close(r, gmt, b.mtpos + gi, l);
        az2::counters2_close(cnt, l);
        if (a.status && l == 0u) a.status[gi] = (uint8_t)st_last;
    }
    if (a.counter_dev && tid == 0u) {
        __threadfence();
        u64 done_blocks = atomicAdd((unsigned long long *)(a.counter_dev + 1), 1ull);
        if (done_blocks == (u64)gridDim.x - 1ull) {
            a.counter_dev[1] = 0ull;
            a.counter_dev[0] += (u64)a.n_steps;
            __threadfence();
        }
    }
#undef PR2_L2COL0
#undef PR2_LOAD1
#undef PR2_LOAD1Q
#undef PR2_LOAD2
#undef PR2_LOADO
}


// ---- the persistent policy rollout for WIDE batches (3 / 4 players, extended rules; row N4): x_policy_rollout_body ----------------------
// The same window structure as azul_policy_rollout2_kernel -- eight waves own 16 games for a whole window, wave w plays games 2w and 2w + 1
// in its 32-lane halves, the same waves run the network on the f32 matrix cores between the env phases -- on azul_rules_x.hpp's P-seat
// GameRunner.  Per move: env phase -> layer 1 -> layer 2 -> head (+ critic, trajectory stores) -> env phase.
//   env       OPP 0: azx::policy_step_x (the policy moves for every seat, observation from the mover); OPP 1: azx::agent_step_x (GameRunner with
//             RandomAgent seats, observation from seat 0); OPP 2: GameRunner with a NETWORK opponent (azx::net_move_x, see there); OPP 3: the same
//             protocol answered by azx::greedy_pick_x inside the wave.  The game is loaded from / stored to its 256-byte record in LDS around each env
//             phase exactly as runner_body_x does around each launch (stored only when the step touched it), so nothing of the game is live
//             across the matrix phases; the MT19937 stream (LDS) and the counters stay open for the window.
//   matrix    hidden = relu(obs @ w1t + b1) over 23 column tiles of 16 (360 columns), K = obs_size zero-padded in LDS to a multiple of 32;
//             logits = hidden[:, 180:] @ w2a_t + b2a over ceil(NA / 16) tiles, K = 180.  Wave w owns tiles w, w + 8, w + 16; every tile is one
//             k-ordered v_mfma_f32_16x16x4_f32 chain, weights read k-major from L2 one chunk of k-steps ahead.
//   head      policy_head_rows<NPL>, the device code of azul_policy_head_n_kernel, on the LDS logits with the same Philox key: seed,
//             counter + t, id_base + the game's index.  Waves 0..3, four games each; wave 7 sums the critic, waves 4..6 copy slot t out.
// What is exact: the env and the head are the per-move path's device code, so for the same logits the trajectories are the same bits; the
// matrix sums run in a different order than the PyTorch GEMMs of the per-move path, so they agree to f32 rounding (bit for bit when every
// product and partial sum is exact).
template <u32 P, u32 D>
struct PXShape {
    static constexpr u32 IN = azx::obs_size<P, D>();
    static constexpr u32 KPAD = (IN + 31u) / 32u * 32u;            // layer 1's K: whole chunks of eight k-steps, zeros past IN
    static constexpr u32 OBS_STRIDE = KPAD + 4u;                   // 4 (mod 32), like PF_OBS_STRIDE
    static constexpr u32 NA = azx::Dim<D>::NA;
    static constexpr u32 NPL = (NA + 15u) / 16u;                   // the head's actions per lane (azul_policy_head_n_kernel<NA, NPL>)
    static constexpr u32 LOG_STRIDE = NA + (36u - NA % 32u) % 32u; // 4 (mod 32)
    static constexpr u32 T1 = (PF_H2 + 15) / 16;                   // 23 column tiles of layer 1
    static constexpr u32 T2 = (NA + 15u) / 16u;                    // 12 / 15 / 19 of layer 2
    static constexpr u32 NT1 = (T1 + PR2_WAVES - 1u) / PR2_WAVES, NT2 = (T2 + PR2_WAVES - 1u) / PR2_WAVES;
    static constexpr u32 TO = (PF_HID + 15) / 16;                  // OPP 2: 12 column tiles of the opponent's layer 1 (its actor half)
    static constexpr u32 NTO = (TO + PR2_WAVES - 1u) / PR2_WAVES;
};

template <u32 P, u32 D>
struct PXShared {                                                  // the workgroup's LDS (azul_x_policy_rollout_kernel below declares it)
    float obs[PF_GAMES * PXShape<P, D>::OBS_STRIDE];
    float hid[PF_GAMES * PF_HID_STRIDE];
    float lg[PF_GAMES * PXShape<P, D>::LOG_STRIDE];
    float w2c[PF_HID], b1[PF_H2], b2a[PXShape<P, D>::NA];
    u32 mt[PF_GAMES][624];
    u32 rec[PF_GAMES][AZUL_RECORD_BYTES_WIDE / 4];
    double2 tab[azx::Dim<D>::TROWS * T_STRIDE];
    u32 mask[PF_GAMES][PXShape<P, D>::NA / 4];                     // the legal masks as bytes (NA is a multiple of 4)
    i32 act[PF_GAMES];
};

// OPP 2's extra LDS (azul_x_policy_rollout_vs_kernel declares it next to PXShared): the opponent's actor biases, and per game the state of
// GameRunner.step's reply loop -- its NetStep, whether it owes an opponent_move() in this pass, the opponent head's answer
template <u32 D>
struct PXOpp {
    float b1[PF_HID], b2a[azx::Dim<D>::NA];                        // actor_linear1.bias, actor_linear2.bias of the opponent
    az2::NetStep ns[PF_GAMES];
    u32 owe[PF_GAMES];
    i32 ans[PF_GAMES];
};

// NT column tiles of one 16-row tile, K = 4 nsteps (nsteps a multiple of CH): acc[i] += A[16 x K] B_i[K x 16].  ap: LDS, row c, k = q;
// bp[i]: global, k-row 0, this lane's column of tile i; k-rows >= krows read as zeros.  One chunk of CH k-steps is requested ahead.
template <int NT, int CH>
AZ_FN void px_chain(const float *ap, const float *const (&bp)[NT], u32 bstride, u32 nsteps, u32 krows, u32 q, pf_f32x4 (&acc)[NT])
{
    float bb[CH][NT], av[CH], nb[CH][NT], na[CH];
    auto load = [&](u32 s0, float (&bd)[CH][NT], float (&ad)[CH]) {
#pragma unroll
        for (int s = 0; s < CH; s++) {
            const u32 kr = 4u * (s0 + (u32)s) + q;
            const bool in = kr < krows;
            const size_t off = (size_t)(in ? kr : 0u) * bstride;
#pragma unroll
            for (int i = 0; i < NT; i++) { const float v = bp[i][off]; bd[s][i] = in ? v : 0.f; }
            ad[s] = ap[4u * (s0 + (u32)s)];
        }
    };
    load(0u, bb, av);
#pragma unroll 1
    for (u32 s0 = 0; s0 < nsteps; s0 += (u32)CH) {
        const bool more = s0 + (u32)CH < nsteps;
        if (more) load(s0 + (u32)CH, nb, na);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < CH; s++)
#pragma unroll
            for (int i = 0; i < NT; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bb[s][i], acc[i], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (more) {
#pragma unroll
            for (int s = 0; s < CH; s++) {
                av[s] = na[s];
#pragma unroll
                for (int i = 0; i < NT; i++) bb[s][i] = nb[s][i];
            }
        }
    }
}

// One window of T moves for the workgroup's 16 games (blockIdx.x); 512 threads.  OPP: 0 the policy moves for every seat, 1 GameRunner with
// RandomAgent seats, 2 GameRunner with a network opponent (a.Wopp; O: PXOpp in LDS, max_replies: reply rounds per step before the loop gives
// up), 3 GameRunner with greedy_margin seats (azx::greedy_pick_x: no weights, no matrix phase, no draw, no PXOpp; max_replies as OPP 2).
// The returns are not written here (azul_batch_mp_policy_rollout / _vs / _greedy run azul_discounted_returns behind the launch).
// LEAGUE (OPP 2 only): a.opp_member picks the workgroup's member of a stacked pool behind a.Wopp.  A template flag, not a null check as in the
// two-player kernel: the null check in the one instantiation moved the register allocation of the existing azul_x_policy_rollout_vs_kernel
// (private segment +8 bytes for <2, 5>, or +4 for <4, 9> with only the member index kept live), so the single-opponent kernels compile
// exactly as before and the league has its own.
// ARENA (with LEAGUE): a.agent_member picks the agent seat's member of the pool behind W in the same way; its own instantiations.
template <u32 P, u32 D, int OPP, bool LEAGUE = false, bool ARENA = false>
AZ_FN void x_policy_rollout_body(const azx::XBatchDev &b, const PolicyWeights &Wk, const RolloutArgs &a, u32 id_base, PXShared<P, D> &S,
                                 PXOpp<D> *O = nullptr, u32 max_replies = 0)
{
    using Sh = PXShape<P, D>;
    constexpr u32 IN = Sh::IN, NA = Sh::NA, OS = Sh::OBS_STRIDE, LS = Sh::LOG_STRIDE, NPL = Sh::NPL;
    const u32 tid = threadIdx.x, lane = tid & 63u, l = lane & 31u, half = lane >> 5, c = lane & 15u, q = (lane >> 4) & 3u;
    const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const u32 n = b.n, g0 = blockIdx.x * PF_GAMES, gl = 2u * w + half, gi = g0 + gl;
    const bool live = gi < n;
    const u32 gic = live ? gi : n - 1u;
    u64 counter = a.counter;
    if (a.counter_dev) counter += a.counter_dev[0];
    static_assert(!ARENA || (OPP == 2 && LEAGUE), "the arena is the league kernel with a pool behind the agent seat");
    PolicyWeights Wm = Wk;                               // (ARENA: the workgroup's agent, a base offset per array chosen once, wave-uniform)
    if constexpr (ARENA) Wm = league_member<IN, NA>(Wk, arena_agent_of_block(a));
    const PolicyWeights &W = ARENA ? Wm : Wk;
    for (u32 i = tid; i < (u32)PF_HID; i += 64u * PR2_WAVES) S.w2c[i] = W.w2c[i];
    for (u32 i = tid; i < (u32)PF_H2; i += 64u * PR2_WAVES) S.b1[i] = W.b1[i];
    for (u32 i = tid; i < NA; i += 64u * PR2_WAVES) S.b2a[i] = W.b2a[i];
    if (OPP == 1)
        for (u32 i = tid; i < azx::Dim<D>::TROWS * (u32)T_STRIDE; i += 64u * PR2_WAVES) S.tab[i] = b.tab[i];
    // the opponent's net (OPP == 2): a.Wopp itself, or with a league (a.opp_member) the pool member of this workgroup's 16 games.  Only the
    // member (one scalar register, 0 without a pool) lives across the window: the arrays' bases are formed from it where they are read
    u32 lm = 0;
    if constexpr (OPP == 2) {
        if constexpr (LEAGUE) { if (a.opp_member) lm = league_member_of_block(a); }
        const PolicyWeights Wo = LEAGUE ? league_member<IN, NA>(a.Wopp, lm) : a.Wopp;
        for (u32 i = tid; i < (u32)PF_HID; i += 64u * PR2_WAVES) O->b1[i] = Wo.b1[PF_HID + i];
        for (u32 i = tid; i < NA; i += 64u * PR2_WAVES) O->b2a[i] = Wo.b2a[i];
        if (tid < PF_GAMES) {
            O->ns[tid] = {az2::NET_READY, 0u, 0, 0u, false, (u32)ST_OK};
            O->owe[tid] = 0u;
            O->ans[tid] = -1;
        }
    }
    for (u32 i = tid; i < PF_GAMES * OS; i += 64u * PR2_WAVES) S.obs[i] = 0.f;          // the K padding stays zero for the window
    for (u32 i = tid; i < PF_GAMES * NA / 4u; i += 64u * PR2_WAVES) S.mask[i / (NA / 4u)][i % (NA / 4u)] = 0u;
    constexpr u32 RW = AZUL_RECORD_BYTES_WIDE / 4u;
    for (u32 i = tid; i < PF_GAMES * RW; i += 64u * PR2_WAVES) {
        const u32 row = i / RW, g = g0 + row;
        S.rec[row][i % RW] = g < n ? ((const u32 *)(b.state + (size_t)g * AZUL_RECORD_BYTES_WIDE))[i % RW] : 0u;
    }
    const float b2c_v = W.b2c[0];
    __syncthreads();

    // env state of this half's game: the stream (LDS) and the counters stay open for the window.  Everything else of the env -- the game,
    // the rule constants -- is rebuilt in each env phase, so that the matrix phases do not carry it (the VGPR budget is 256 at 8 waves)
    const az2::Tab2 tab = {S.tab};
    uint8_t *rec = (uint8_t *)S.rec[gl];
    az2::Rng2 r;
    u32 *gmt = b.mt + (size_t)gic * 624u;
    az2::rng2_open(r, gmt, S.mt[gl], b.mtpos[gic], l);
    az2::Counters2 cnt;
    az2::counters2_open(cnt, b.episodes + gic, b.stuck + gic, b.stat_sum + (size_t)gic * 10, l);
    u32 st_last = ST_OK;

    // the decision of the state in `g` -> LDS (observation row, mask bytes) and the player byte of trajectory slot `slot` (runner_body_x's queries)
    auto publish = [&](const azx::GX<P, D> &g, const azx::KX<D> &K, u32 slot) {
        uint8_t *mrow = (uint8_t *)S.mask[gl];
        azx::MaskX<D> m;
        azx::legal_mask_x(g, K, m);
#pragma unroll
        for (u32 rr = 0; rr < 6u; rr++) {
            if (l < (azx::Dim<D>::Q < 32u ? azx::Dim<D>::Q : 32u)) mrow[azx::Dim<D>::Q * rr + l] = (uint8_t)m.bit[rr][0];
            if (azx::Dim<D>::NW > 1) { if (l + 32u < azx::Dim<D>::Q) mrow[azx::Dim<D>::Q * rr + 32u + l] = (uint8_t)m.bit[rr][azx::Dim<D>::NW - 1]; }
        }
        azx::observe_x(g, OPP ? 0u : azx::mex(g), S.obs + gl * OS, l);
        if (l == 0u) a.player[(size_t)slot * n + gi] = (uint8_t)g.cur;
    };
    // trajectory slot `slot` of the workgroup's games <- LDS: [T+1][N][IN] floats and [T+1][N][NA] bytes (dwords: NA is a multiple of 4);
    // the rows are not 16-byte aligned in general, so every store is a dword.  `idx` in 0..191 over waves 4..6.
    auto flush = [&](u32 slot, u32 idx) {
        const size_t cell0 = (size_t)slot * n + g0;
        float *og = a.obs + cell0 * IN;
#pragma unroll 1
        for (u32 e = idx; e < PF_GAMES * IN; e += 192u) {
            const u32 row = e / IN, k = e - row * IN;
            if (g0 + row < n) og[e] = S.obs[row * OS + k];
        }
        u32 *mg = (u32 *)(a.mask + cell0 * NA);
#pragma unroll 1
        for (u32 d = idx; d < PF_GAMES * NA / 4u; d += 192u) {
            const u32 row = d / (NA / 4u);
            if (g0 + row < n) mg[d] = S.mask[row][d - row * (NA / 4u)];
        }
    };
    if (live) {
        azx::KX<D> K;
        azx::kx_init(K);
        azx::GX<P, D> g;
        azx::gx_load(g, rec, l);
        azx::prime_x(g, K);
        publish(g, K, 0u);
    }

    // matrix phases: wave w owns column tiles j = w + 8 i, the lane column 16 j + c (clamped to a real column: dead tiles compute and are dropped)
#pragma unroll 1
    for (int t = 0; t < a.n_steps; t++) {
        const size_t row_t = (size_t)t * n;
        lds_barrier();                                   // observations and masks of all 16 games are in LDS
        {
            const float *bp1[Sh::NT1];
#pragma unroll
            for (u32 i = 0; i < Sh::NT1; i++) { const u32 col = 16u * (w + PR2_WAVES * i) + c; bp1[i] = W.w1t + (col < (u32)PF_H2 ? col : 0u); }
            pf_f32x4 acc[Sh::NT1];
#pragma unroll
            for (u32 i = 0; i < Sh::NT1; i++) acc[i] = (pf_f32x4){0.f, 0.f, 0.f, 0.f};
            px_chain<(int)Sh::NT1, 8>(S.obs + c * OS + q, bp1, (u32)PF_H2, Sh::KPAD / 4u, IN, q, acc);
#pragma unroll
            for (u32 i = 0; i < Sh::NT1; i++) {
                const u32 col = 16u * (w + PR2_WAVES * i) + c;
                if (col < (u32)PF_H2)
                    for (int rr = 0; rr < 4; rr++) {             // C layout: column = lane & 15, row = 4 (lane >> 4) + rr
                        const float h = acc[i][rr] + S.b1[col];
                        S.hid[(4u * q + rr) * PF_HID_STRIDE + col] = h > 0.f ? h : 0.f;       // F.relu, model.py:24/30
                    }
            }
        }
        lds_barrier();
        {
            const float *bp2[Sh::NT2];
#pragma unroll
            for (u32 i = 0; i < Sh::NT2; i++) { const u32 col = 16u * (w + PR2_WAVES * i) + c; bp2[i] = W.w2a_t + (col < NA ? col : 0u); }
            pf_f32x4 acc[Sh::NT2];
#pragma unroll
            for (u32 i = 0; i < Sh::NT2; i++) acc[i] = (pf_f32x4){0.f, 0.f, 0.f, 0.f};
            px_chain<(int)Sh::NT2, 9>(S.hid + c * PF_HID_STRIDE + PF_HID + q, bp2, NA, (u32)PF_HID / 4u, (u32)PF_HID, q, acc);
#pragma unroll
            for (u32 i = 0; i < Sh::NT2; i++) {
                const u32 col = 16u * (w + PR2_WAVES * i) + c;
                if (col < NA)
                    for (int rr = 0; rr < 4; rr++) S.lg[(4u * q + rr) * LS + col] = acc[i][rr] + S.b2a[col];
            }
        }
        lds_barrier();
        if (w < 4u) {
            // head: azul_policy_head_n_kernel's lane mapping on the LDS rows, four games per wave
            const u32 hrow = 4u * w + q, hg = g0 + hrow;
            const float *row = S.lg + hrow * LS;
            const uint8_t *mk = (const uint8_t *)S.mask[hrow];
            float x[NPL];
            u32 okbits = 0;
#pragma unroll
            for (u32 j = 0; j < NPL; j++) {
                const u32 i = NPL * c + j;
                const bool in = i < NA;
                x[j] = in ? row[i] : 0.f;
                okbits |= ((in && mk[in ? i : 0u] != 0) ? 1u : 0u) << j;
            }
            policy_head_rows<(int)NPL>(x, row, okbits, a.seed, counter + (u64)t, hg < n ? hg : n - 1u, lane, hg < n, a.action + row_t, a.logp + row_t,
                                       a.entropy + row_t, id_base, S.act + 4u * w);
        } else if (w < 7u) {
            flush((u32)t, 64u * (w - 4u) + lane);
        } else {
            // the critic: lane (row c, quarter q) sums k = q (mod 4), then the quarters are added (azul_policy_forward_kernel's order)
            float sum = 0.f;
            const float *hp = S.hid + c * PF_HID_STRIDE;
#pragma unroll
            for (int s = 0; s < PF_HID / 4; s++) sum = fmaf(hp[4 * s + q], S.w2c[4 * s + q], sum);
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            if (q == 0u && g0 + c < n) a.value[row_t + g0 + c] = sum + b2c_v;
        }
        lds_barrier();
        if constexpr (OPP == 2) {
            // GameRunner.step against the NETWORK opponent (game_runner.py:43-55, :37-42 answered by a.Wopp), azul_policy_rollout2_kernel<LID, 2>'s
            // loop on the wide record: pass 0 plays the agent's action, then while any of the workgroup's 16 games owes an opponent_move() (the
            // other seats' replies, the agent's forced moves, after an episode end the next one's openings) the opponent's forward_actor runs
            // on the mover-perspective rows of the games that owe (the others sit masked) and pass j + 1 plays answer j.  Round j draws with
            // Philox key opp_seed + j at counter + t, as PolicyRollout's per-cut path does.  The game, its NetStep and its debt live in LDS
            // between the passes (O->ns / O->owe), loaded and stored around each env pass: nothing new is live across the matrix phases.
#pragma unroll 1
            for (u32 j = 0;; j++) {
                if (live) {
                    az2::NetStep ns = O->ns[gl];
                    if (j == 0u || ns.pending != az2::NET_READY) {
                        azx::KX<D> K;
                        azx::kx_init(K);
                        azx::GX<P, D> g;
                        azx::gx_load(g, rec, l);
                        azx::prime_x(g, K);
                        azx::RunX s;
                        azx::runx_load(s, rec);
                        azx::MaskX<D> m;
                        const u32 st = azx::net_move_x(g, s, S.act[gl], j == 0u, m, b.rules, K, r, b.draw_margin, cnt, ns);
                        if (!(st == ST_ILLEGAL_MOVE || st == ST_BAD_ACTION)) {
                            azx::gx_store(g, rec, l);
                            azx::runx_store(s, rec, l);
                        }
                        if (ns.pending != az2::NET_READY) {         // what opponent_move() hands the opponent (game_runner.py:38-39): net_body_x's rows
                            uint8_t *mrow = (uint8_t *)S.mask[gl];
#pragma unroll
                            for (u32 rr = 0; rr < 6u; rr++) {
                                if (l < (azx::Dim<D>::Q < 32u ? azx::Dim<D>::Q : 32u)) mrow[azx::Dim<D>::Q * rr + l] = (uint8_t)m.bit[rr][0];
                                if (azx::Dim<D>::NW > 1) { if (l + 32u < azx::Dim<D>::Q) mrow[azx::Dim<D>::Q * rr + 32u + l] = (uint8_t)m.bit[rr][azx::Dim<D>::NW - 1]; }
                            }
                            azx::observe_x(g, azx::mex(g), S.obs + gl * OS, l);
                        }
                        if (l == 0u) O->ns[gl] = ns;
                    }
                    if (l == 0u) O->owe[gl] = ns.pending != az2::NET_READY ? 1u : 0u;
                }
                lds_barrier();                                   // every game's debt, observation row and mask are in LDS
                const bool any = __builtin_amdgcn_ballot_w64(O->owe[lane & 15u] != 0u) != 0ull;     // (the same 16 words in every wave)
                if (!any || j >= max_replies) break;
                const u64 okey = a.opp_seed == AZUL_POLICY_ARGMAX ? a.opp_seed : a.opp_seed + (u64)j;
                {
                    // layer 1 of forward_actor: columns 180..359 of the opponent's w1t, 12 tiles (wave w: tiles w, w + 8) -> hid[:, 180:]
                    const float *bpo[Sh::NTO];
#pragma unroll
                    for (u32 i = 0; i < Sh::NTO; i++) {
                        const u32 col = 16u * (w + PR2_WAVES * i) + c;
                        bpo[i] = (LEAGUE ? league_member<IN, NA>(a.Wopp, lm).w1t : a.Wopp.w1t) + PF_HID + (col < (u32)PF_HID ? col : 0u);
                    }
                    pf_f32x4 acc[Sh::NTO];
#pragma unroll
                    for (u32 i = 0; i < Sh::NTO; i++) acc[i] = (pf_f32x4){0.f, 0.f, 0.f, 0.f};
                    px_chain<(int)Sh::NTO, 8>(S.obs + c * OS + q, bpo, (u32)PF_H2, Sh::KPAD / 4u, IN, q, acc);
#pragma unroll
                    for (u32 i = 0; i < Sh::NTO; i++) {
                        const u32 col = 16u * (w + PR2_WAVES * i) + c;
                        if (col < (u32)PF_HID)
                            for (int rr = 0; rr < 4; rr++) {
                                const float h = acc[i][rr] + O->b1[col];
                                S.hid[(4u * q + rr) * PF_HID_STRIDE + PF_HID + col] = h > 0.f ? h : 0.f;       // F.relu, model.py:30
                            }
                    }
                }
                lds_barrier();
                {
                    const float *bp2[Sh::NT2];
#pragma unroll
                    for (u32 i = 0; i < Sh::NT2; i++) {
                        const u32 col = 16u * (w + PR2_WAVES * i) + c;
                        bp2[i] = (LEAGUE ? league_member<IN, NA>(a.Wopp, lm).w2a_t : a.Wopp.w2a_t) + (col < NA ? col : 0u);
                    }
                    pf_f32x4 acc[Sh::NT2];
#pragma unroll
                    for (u32 i = 0; i < Sh::NT2; i++) acc[i] = (pf_f32x4){0.f, 0.f, 0.f, 0.f};
                    px_chain<(int)Sh::NT2, 9>(S.hid + c * PF_HID_STRIDE + PF_HID + q, bp2, NA, (u32)PF_HID / 4u, (u32)PF_HID, q, acc);
#pragma unroll
                    for (u32 i = 0; i < Sh::NT2; i++) {
                        const u32 col = 16u * (w + PR2_WAVES * i) + c;
                        if (col < NA)
                            for (int rr = 0; rr < 4; rr++) S.lg[(4u * q + rr) * LS + col] = acc[i][rr] + O->b2a[col];
                    }
                }
                lds_barrier();
                if (w < 4u) {
                    // the opponent's head (agent.py:76-80): azul_policy_head_n's draw, waves 0..3, four games each.  A forward that is not
                    // finite answers -1, as PolicyRollout's per-cut path does (its logits' sum is tested): the env refuses it, the game keeps
                    // owing, and the reply cap ends the step
                    const u32 hrow = 4u * w + q, hg = g0 + hrow;
                    const float *row = S.lg + hrow * LS;
                    const uint8_t *mk = (const uint8_t *)S.mask[hrow];
                    float x[NPL], xs = 0.f;
                    u32 okbits = 0;
#pragma unroll
                    for (u32 jj = 0; jj < NPL; jj++) {
                        const u32 i = NPL * c + jj;
                        const bool in = i < NA;
                        x[jj] = in ? row[i] : 0.f;
                        xs += x[jj];
                        okbits |= ((in && mk[in ? i : 0u] != 0) ? 1u : 0u) << jj;
                    }
                    const bool finite = __builtin_isfinite(row_sum(xs));
                    const bool owes = O->owe[hrow] != 0u;
                    const bool tr = hg < n && owes && a.opp_action && j < (u32)a.opp_slots;
                    const size_t trow = ((size_t)t * (size_t)(a.opp_slots > 0 ? a.opp_slots : 1) + (j < (u32)a.opp_slots ? j : 0u)) * n;
                    policy_head_rows<(int)NPL>(x, row, okbits, okey, counter + (u64)t, hg < n ? hg : n - 1u, lane, tr, a.opp_action ? a.opp_action + trow : nullptr,
                                               a.opp_logp ? a.opp_logp + trow : nullptr, nullptr, id_base, O->ans + 4u * w);
                    if (c == 0u) {                               // (the lane that wrote the answer)
                        if (owes) S.act[hrow] = finite ? O->ans[hrow] : -1;
                        if (tr && !finite) a.opp_action[trow + hg] = -1;
                    }
                }
                lds_barrier();
            }
            if (live) {
                // close the step: a game still owing at the cap gives up as azul_policy_rollout2_kernel<LID, 2> does (pending cleared, AZUL_STUCK
                // unless the step already has a status, the legal mask of its state); then slot t + 1 from perspective 0, as OPP 1
                az2::NetStep ns = O->ns[gl];
                if (ns.pending != az2::NET_READY) {
                    ns.pending = az2::NET_READY;
                    if (!ns.st) ns.st = ST_STUCK;
                    if (l == 0u) O->ns[gl] = ns;
                }
                azx::KX<D> K;
                azx::kx_init(K);
                azx::GX<P, D> g;
                azx::gx_load(g, rec, l);
                azx::prime_x(g, K);
                if (l == 0u) {
                    a.reward[row_t + gi] = ns.rew; a.done[row_t + gi] = (uint8_t)ns.dn;
                    if (a.opp_replies) a.opp_replies[row_t + gi] = (uint8_t)(ns.replies < 255u ? ns.replies : 255u);
                }
                st_last = ns.st;
                publish(g, K, (u32)t + 1u);
            }
        } else if constexpr (OPP == 3) {
            // GameRunner.step against GREEDY_MARGIN seats (game_runner.py:43-55 with :37-42 answered by azx::greedy_pick_x), as
            // azul_policy_rollout2_kernel<LID, 3> does it: OPP 1's control flow -- no barrier, no matrix phase -- on OPP 2's protocol.  The
            // answer is a pure function of the game this half holds, so the reply rounds stay inside the wave and the game, its runner tail
            // and its NetStep stay in registers for the step: loaded from LDS once, stored once.  Pass 0 plays the agent's action, pass
            // j > 0 reply j - 1: while EITHER half owes an opponent_move() both halves price their candidates (the loop is wave-uniform; a
            // half without a game holds an empty mask) and only the half that owes plays; its sibling's game, stream and counters are not
            // touched.  A wave without a live game skips all of it.
            if (az2::wave_any(live)) {
                azx::KX<D> K;
                azx::kx_init(K);
                azx::GX<P, D> g;
                azx::gx_load(g, rec, l);                 // (a half without a game: a row of zeros)
                azx::prime_x(g, K);
                azx::RunX s;
                azx::runx_load(s, rec);
                az2::NetStep ns = {az2::NET_READY, 0u, 0, 0u, false, (u32)ST_OK};
                const bool end_bonus = b.rules.end_bonus != 0u;
                bool touched = false;                    // a refused move leaves the record as it was (OPP 2)
#pragma unroll 1
                for (u32 j = 0; j <= max_replies; j++) {
                    const bool go = live && (j == 0u || ns.pending != az2::NET_READY);
                    if (!az2::wave_any(go)) break;
                    i32 av = S.act[gl];
                    azx::MaskX<D> m;                     // (per pass: a mask carried through the move would cost its registers there)
                    if (j > 0u) {
                        azx::legal_mask_x(g, K, m);      // the mask net_move_x left; a half without a game is handed an empty one
                        if (!live) m = azx::MaskX<D>{};
                        av = azx::greedy_pick_x(g, m, K, end_bonus);
                        if (go && l == 0u && a.opp_action && j - 1u < (u32)a.opp_slots)
                            a.opp_action[((size_t)t * (size_t)a.opp_slots + (j - 1u)) * n + gi] = av;
                    }
                    if (go) {
                        const u32 st = azx::net_move_x(g, s, av, j == 0u, m, b.rules, K, r, b.draw_margin, cnt, ns);
                        touched = touched | !(st == ST_ILLEGAL_MOVE || st == ST_BAD_ACTION);
                    }
                }
                if (live) {
                    // close the step: a game still owing at the cap gives up as azul_x_policy_rollout_vs_kernel does (AZUL_STUCK unless the
                    // step already has a status; the debt ends with the step's NetStep); then slot t + 1 from perspective 0
                    if (ns.pending != az2::NET_READY && !ns.st) ns.st = ST_STUCK;
                    if (touched) azx::store_runner_x(g, s, rec, l);
                    if (l == 0u) {
                        a.reward[row_t + gi] = ns.rew; a.done[row_t + gi] = (uint8_t)ns.dn;
                        if (a.opp_replies) a.opp_replies[row_t + gi] = (uint8_t)(ns.replies < 255u ? ns.replies : 255u);
                    }
                    st_last = ns.st;
                    publish(g, K, (u32)t + 1u);
                }
            }
        } else if (live) {
            // one runner call of azul_x_runner_kernel (XRUN_AGENT_STEP / XRUN_POLICY_STEP) on the record in LDS
            azx::KX<D> K;
            azx::kx_init(K);
            azx::GX<P, D> g;
            azx::gx_load(g, rec, l);
            azx::prime_x(g, K);
            azx::RunX s;
            azx::runx_load(s, rec);
            const i32 av = S.act[gl];
            i32 rew = 0;
            u32 dn = 0, st;
            if constexpr (OPP == 1) st = azx::agent_step_x(g, s, av, b.rules, K, r, tab, b.draw_margin, cnt, rew, dn);
            else st = azx::policy_step_x(g, s, av, b.rules, K, r, b.draw_margin, cnt, rew, dn);
            if (!(st == ST_ILLEGAL_MOVE || st == ST_BAD_ACTION)) azx::store_runner_x(g, s, rec, l);
            if (l == 0u) { a.reward[row_t + gi] = rew; a.done[row_t + gi] = (uint8_t)dn; }
            st_last = st;
            publish(g, K, (u32)t + 1u);
        }
    }
    lds_barrier();                                       // the rows of the state after the last move; every record is final
    if (w >= 4u && w < 7u) flush((u32)a.n_steps, 64u * (w - 4u) + lane);
    if (live) {
        az2::rng2_close(r, gmt, b.mtpos + gi, l);
        az2::counters2_close(cnt, l);
        if (a.status && l == 0u) a.status[gi] = (uint8_t)st_last;
    }
    for (u32 i = tid; i < PF_GAMES * RW; i += 64u * PR2_WAVES) {
        const u32 row = i / RW, g = g0 + row;
        if (g < n) ((u32 *)(b.state + (size_t)g * AZUL_RECORD_BYTES_WIDE))[i % RW] = S.rec[row][i % RW];
    }
    if (a.counter_dev && tid == 0u) {
        __threadfence();
        u64 done_blocks = atomicAdd((unsigned long long *)(a.counter_dev + 1), 1ull);
        if (done_blocks == (u64)gridDim.x - 1ull) {
            a.counter_dev[1] = 0ull;
            a.counter_dev[0] += (u64)a.n_steps;
            __threadfence();
        }
    }
}

// The persistent policy rollout for wide batches (azul_batch_mp_policy_rollout; x_policy_rollout_body above): 16 games per
// workgroup of eight waves for a whole window, the workgroup's LDS declared here.
// OPP 3 (azul_batch_mp_policy_rollout_greedy): max_replies bounds the reply rounds of a step; the other two do not read it.
template <u32 P, u32 D, int OPP>
__global__ void __launch_bounds__(64 * PR2_WAVES) azul_x_policy_rollout_kernel(azx::XBatchDev b, PolicyWeights W, RolloutArgs a, u32 id_base,
                                                                                u32 max_replies = 0)
{
    __shared__ PXShared<P, D> S;
    x_policy_rollout_body<P, D, OPP>(b, W, a, id_base, S, nullptr, max_replies);
}

// ... with a NETWORK opponent (azul_batch_mp_policy_rollout_vs; OPP 2 of x_policy_rollout_body): the reply rounds inside the window, the
// opponent's biases and the games' reply-loop state in LDS next to PXShared.  LEAGUE (azul_batch_mp_policy_rollout_league): a pool of opponents
// behind a.Wopp, one member per workgroup (RolloutArgs::opp_member)
// ARENA (azul_batch_mp_policy_rollout_arena, <P, D, true, true>): the agent seat is a member of the pool behind W too (RolloutArgs::agent_member)
template <u32 P, u32 D, bool LEAGUE = false, bool ARENA = false>
__global__ void __launch_bounds__(64 * PR2_WAVES) azul_x_policy_rollout_vs_kernel(azx::XBatchDev b, PolicyWeights W, RolloutArgs a, u32 id_base,
                                                                                   u32 max_replies)
{
    __shared__ PXShared<P, D> S;
    __shared__ PXOpp<D> O;
    x_policy_rollout_body<P, D, 2, LEAGUE, ARENA>(b, W, a, id_base, S, &O, max_replies);
}

// ---- the host side of a window launch, stated ONCE: which instantiation runs and what it is handed.  rollout_window (azul_kernels.hip)
// and the lockstep emulation (tests/hostcheck/simt_rollout2.cpp, simt_x_rollout.cpp) launch what these return -------------------------
// opp = 0 the policy on every seat, 1 RandomAgent seats, 2 a network, 3 greedy; any other: nullptr.  A two-player league is <LID, 2>.
typedef void (*rollout2_kernel_t)(BatchDev, PolicyWeights, RolloutArgs);
template <bool LID>
static rollout2_kernel_t rollout2_kernel_of(int opp, bool arena)
{
    if (opp == 2 && arena) return azul_policy_rollout2_kernel<LID, 2, true>;
    if (opp == 3) return azul_policy_rollout2_kernel<LID, 3>;
    if (opp == 2) return azul_policy_rollout2_kernel<LID, 2>;
    if (opp == 1) return azul_policy_rollout2_kernel<LID, 1>;
    if (opp == 0) return azul_policy_rollout2_kernel<LID, 0>;
    return nullptr;
}
static rollout2_kernel_t rollout2_kernel(bool lid, int opp, bool arena)
{
    return lid ? rollout2_kernel_of<true>(opp, arena) : rollout2_kernel_of<false>(opp, arena);
}

// ... of a wide batch: six kinds over the shapes of x_for_shape.  opp 0 / 1 do not read the last argument, max_replies: pass 0
typedef void (*x_rollout_kernel_t)(azx::XBatchDev, PolicyWeights, RolloutArgs, u32, u32);
template <u32 P, u32 D>
static x_rollout_kernel_t x_rollout_kernel_of(int opp, bool league, bool arena)
{
    if (opp == 2 && arena) return azul_x_policy_rollout_vs_kernel<P, D, true, true>;
    if (opp == 2 && league) return azul_x_policy_rollout_vs_kernel<P, D, true>;
    if (opp == 2) return azul_x_policy_rollout_vs_kernel<P, D>;
    if (opp == 3) return azul_x_policy_rollout_kernel<P, D, 3>;
    if (opp == 1) return azul_x_policy_rollout_kernel<P, D, 1>;
    if (opp == 0) return azul_x_policy_rollout_kernel<P, D, 0>;
    return nullptr;
}
static x_rollout_kernel_t x_rollout_kernel(int players, int displays, int opp, bool league, bool arena)
{
    return x_for_shape(players, displays, [&](auto s) { return x_rollout_kernel_of<s.P, s.D>(opp, league, arena); });
}

// What a window kernel is handed, from the public structs (include/azul_hip.h) once rollout_window has checked them
struct DrawKeys { uint64_t seed, opp_seed, counter; uint64_t *counter_dev; };
// azul_batch_[mp_]policy_rollout_league: the pool behind `opponent`.  agent_member_dev (azul_batch_[mp_]policy_rollout_arena): the same pool is
// behind `agent` too, one member per group for the agent seat
struct League { int pool_size; const uint8_t *member_dev; const uint8_t *agent_member_dev; bool arena; };

static void window_pack(bool wide, int n_steps, int opp, const azul_net_weights_t *agent, const azul_net_weights_t *opponent, DrawKeys keys,
                        const azul_rollout_buffers_t *out, float gamma, const League *league, PolicyWeights &W, RolloutArgs &a)
{
    W = {agent->w1t, agent->b1, agent->w2c, agent->b2c, agent->w2a_t, agent->b2a};
    // returns: the two-player kernel writes a window of up to 32 steps itself (it keeps the rewards in 32 lanes); the wide kernels never do
    a = RolloutArgs{n_steps, out->obs, out->mask, out->player, out->action, out->reward, out->done, out->value, out->logp, out->entropy, out->status,
                    wide ? nullptr : out->returns, gamma, (u64)keys.seed, (u64)keys.counter, (u64 *)keys.counter_dev};
    if (opp == 2) {                                          // (without a network opponent the opponent fields of `out` are ignored)
        a.Wopp = {opponent->w1t, opponent->b1, opponent->w2c, opponent->b2c, opponent->w2a_t, opponent->b2a};
        a.opp_seed = (u64)keys.opp_seed;
        a.opp_action = out->opp_action; a.opp_logp = out->opp_logp; a.opp_replies = out->opp_replies; a.opp_slots = out->opp_slots;
        if (league) { a.opp_member = league->member_dev; a.opp_pool = (u32)league->pool_size; }      // a base offset per workgroup, nothing else
        if (league && league->arena) { a.agent_member = league->agent_member_dev; a.agent_pool = (u32)league->pool_size; }
    }
    if (opp == 3) {                                          // the greedy player's trace: its answers and their number (opp_logp is never written)
        a.opp_action = out->opp_action; a.opp_replies = out->opp_replies; a.opp_slots = out->opp_slots;
    }
}
