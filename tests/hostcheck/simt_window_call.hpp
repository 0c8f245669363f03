// simt_window_call.hpp -- TEST-ONLY: the ONE call block of the two window shims (simt_rollout2.cpp: sr2_window, simt_x_rollout.cpp:
// sxr_window), mirrored field by field by tests/hostcheck/window.py (WindowCall; <prefix>_call_bytes() guards the mirror).  Fixed-width
// integers and pointers only.  Zero / NULL = not used; the shape of the call follows rollout_window (csrc/azul_kernels.hip).
#pragma once
#include <stdint.h>

struct SimtWindowCall {
    // ---- the games (sr2_window ignores players / displays / end_bonus / short_deal; sxr_window ignores move_limit: wide batches have none)
    int32_t n_games, players, displays, first_player, pool, end_bonus, short_deal;
    uint32_t id_base, move_limit;
    uint8_t *state;
    uint32_t *mt, *mtpos;
    uint64_t *episodes;
    uint32_t *stuck;
    double *stat_sum;
    // ---- who plays: opp = 0 the policy on every seat, 1 RandomAgent seats, 2 a network, 3 greedy.  opp_member non-NULL = a league
    // (`opponent` is the stacked pool of pool_size members); both member arrays non-NULL = an arena (`agent` is the stacked pool,
    // `opponent` is not read)
    int32_t opp;
    const float *agent[6], *opponent[6];       // w1t, b1, w2c, b2c, w2a_t, b2a
    int32_t pool_size;
    const uint8_t *opp_member, *agent_member;  // [ceil(n_games / 16)]
    // ---- the window (sr2_window ignores max_replies; sxr_window ignores returns / gamma: the wide kernels never write returns)
    int32_t n_steps, max_replies;
    float *obs;
    uint8_t *mask, *player;
    int32_t *action, *reward;
    uint8_t *done;
    float *value, *logp, *entropy;
    uint8_t *status;
    float *returns;
    float gamma;
    uint64_t seed, opp_seed, counter;
    int32_t *opp_action;                       // the trace, opp 2 and 3 (opp_logp is handed to the greedy kernels to show it is never written)
    float *opp_logp;
    uint8_t *opp_replies;
    int32_t opp_slots;
};

#ifdef __HIPCC__               // ---- the shims' side; they include this after csrc/azul_policy.hpp
// The call -> the agent's weights and the RolloutArgs of its kind, as rollout_window fills them; `league` / `arena` = what the member
// arrays say.  Returns -1 where a call is refused: an unknown opp, no games, a league / arena with a missing member array or a pool_size
// outside 1..255.
static int window_args(const SimtWindowCall &c, bool wide, PolicyWeights &W, RolloutArgs &a, bool &league, bool &arena)
{
    const bool net = c.opp == 2;
    league = net && (c.opp_member || c.agent_member);
    arena = league && c.agent_member;
    if (c.opp < 0 || c.opp > 3 || c.n_games <= 0) return -1;
    if (league && (!c.opp_member || c.pool_size < 1 || c.pool_size > 255)) return -1;
    W = {c.agent[0], c.agent[1], c.agent[2], c.agent[3], c.agent[4], c.agent[5]};
    a = RolloutArgs{c.n_steps, c.obs, c.mask, c.player, c.action, c.reward, c.done, c.value, c.logp, c.entropy, c.status,
                    wide ? nullptr : c.returns, c.gamma, c.seed, c.counter, nullptr};
    if (net) {
        a.Wopp = arena ? W : PolicyWeights{c.opponent[0], c.opponent[1], c.opponent[2], c.opponent[3], c.opponent[4], c.opponent[5]};
        a.opp_seed = c.opp_seed;
        if (league) { a.opp_member = c.opp_member; a.opp_pool = (u32)c.pool_size; }
        if (arena) { a.agent_member = c.agent_member; a.agent_pool = (u32)c.pool_size; }
    }
    if (net || c.opp == 3) { a.opp_action = c.opp_action; a.opp_logp = c.opp_logp; a.opp_replies = c.opp_replies; a.opp_slots = c.opp_slots; }
    return 0;
}
#endif
