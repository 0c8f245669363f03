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

#ifdef __HIPCC__               // ---- the shims' side; they include this after csrc/azul_rollout2.hpp
// The call -> the public structs -> the agent's weights and the RolloutArgs of its kind, filled by the library's own window_pack
// (csrc/azul_rollout2.hpp; rollout_window calls the same); `league` / `arena` = what the member arrays say.  Returns -1 where a call cannot be
// emulated: no games, a league / arena with a missing member array or a pool_size outside 1..255.  (An unknown opp is the kernel
// selectors' refusal.)
static int window_args(const SimtWindowCall &c, bool wide, PolicyWeights &W, RolloutArgs &a, bool &league, bool &arena)
{
    league = c.opp == 2 && (c.opp_member || c.agent_member);
    arena = league && c.agent_member;
    if (c.n_games <= 0) return -1;
    if (league && (!c.opp_member || c.pool_size < 1 || c.pool_size > 255)) return -1;
    const azul_net_weights_t agent = {c.agent[0], c.agent[1], c.agent[2], c.agent[3], c.agent[4], c.agent[5]};
    const azul_net_weights_t opponent = {c.opponent[0], c.opponent[1], c.opponent[2], c.opponent[3], c.opponent[4], c.opponent[5]};
    const azul_rollout_buffers_t out = {c.obs, c.mask, c.player, c.action, c.reward, c.done, c.value, c.logp, c.entropy, c.status, c.returns,
                                        c.opp_action, c.opp_logp, c.opp_replies, c.opp_slots};
    const League lg = {c.pool_size, c.opp_member, c.agent_member, arena};
    window_pack(wide, c.n_steps, c.opp, &agent, arena ? &agent : &opponent, {c.seed, c.opp_seed, c.counter, nullptr}, &out, c.gamma,
                league ? &lg : nullptr, W, a);
    // the one difference from the library, which passes the greedy kernels no opp_logp: here they get it, so that the tests can show it is
    // never written
    if (c.opp == 3) a.opp_logp = c.opp_logp;
    return 0;
}
#endif
