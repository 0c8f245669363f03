// azul_runner.hpp -- THE GameRunner STEP PROTOCOL, stated once for both record shapes: GameRunner.step / GameRunner.reset of the reference
// (azulnet/game_runner.py:37-55, 76-85), the agent step of NNRunner.run_episode (azulnet/nn_runner.py:20-29), one env move of policy
// self-play, and the same two methods cut at their opponent_move() calls for an opponent that answers from outside the rule code.
// Every function is a template over an env adaptor E -- az2::Env2<LID> (azul_env2.hpp: the two-player 128-byte record, state in G2) or
// azx::EnvX<P, D> (azul_rules_x.hpp: the wide 256-byte record, state in GX + RunX) -- a struct of references to what the call site holds.
// What the families really do differently is the adaptor's members and nothing else:
//     E::Mask, legal_mask(out), count(mask)    the legal mask of the current state and its number of set bits
//     count_current()          policy_step's "no action" test: Env2 counts the mask it was handed (`m`), EnvX computes one
//     checked_step(a)          Azul.step with the legality test (azul.py:296-313): Env2 tests against `m`, EnvX against its own mask
//     mask_after_refusal()     `m` after a refused answer: Env2 leaves it (it IS the current state's), EnvX computes it
//     opponent_loop(opening)   the opponents' RandomAgent moves, GameRunner.step's loop (game_runner.py:46-47) or reset's (:84-85): the
//                              one piece kept per family (az2::opponent_loop2 / azx::opponent_loop_x: draw-before-eog vs eog-before-draw,
//                              ST_OK vs ST_STUCK at the guard)
//     potential(), phi(), moves()      game_runner.py:48-50 and GameRunner.player_score / move_counter (:35-36)
//     fresh_game()             the game of GameRunner.reset (:79-82), player_score = move_counter = 0
//     episode_stats()          game_runner.py:53-54
//     E::MOVE_LIMIT            can a move end in ST_TRUNCATED (azul_batch_set_move_limit)?  Env2 yes, EnvX no: every test of that status is
//                              `E::MOVE_LIMIT && ...` or sits behind `if constexpr`, so a family without a limit compiles none of them
// and the members g (with .cur, .over, .eog), m, cnt.  tests/hostcheck runs these functions, unmodified, in every emulated kernel that
// steps a GameRunner.
#pragma once
#include "azul_selfplay2.hpp"

namespace azr {
using namespace az;
using az2::wave_any;

constexpr u32 REPLY_GUARD = 4096;        // RandomAgent moves per opponent loop (a round takes tiles off the table: it ends long before)
constexpr u32 SETTLE_PASSES = 4;         // net_settle: reply closes the step -> reset -> opening -> ready is three passes

// One env move of policy-driven self-play (the policy plays every seat): Azul.step (azul.py:296-313) for the current player, the shaped
// reward of game_runner.py:48-52 per move, done, statistics and the auto-reset of game_runner.py:76-82 (ONE reset site; a fresh game, no
// opening replies).
// REWARD AT A MOVE-LIMIT CUT, kept as it is: this function credits phi - player_score for the move that was cut (done 3), while agent_step
// and net_move below credit 0 -- although include/azul_hip.h ("MOVE LIMIT": "policy entries: ... reward as for a stuck slot") says 0 for
// these entries too.  One rule for all paths changes behaviour and belongs to a change of its own.
template <class E>
AZ_FN u32 policy_step(E &e, i32 av, i32 &rew, u32 &dn)
{
    rew = 0; dn = 0;
    // "no action" is legitimate only when nothing is legal (hazard H3)
    bool stuck = false;
    if (AZ_UNLIKELY(wave_any(av < 0))) stuck = (av < 0) & (e.g.eog == 0u) & (e.count_current() == 0u);
    u32 st = ST_OK;
    bool restart = false;
    if (!stuck) {
        st = e.checked_step(av);
        const bool dirty = !(st == ST_ILLEGAL_MOVE || st == ST_GAME_ENDED || st == ST_BAD_ACTION);
        if (dirty) {
            e.moves() += 1u;
            const i32 phi = e.potential();                             // game_runner.py:48-50
            rew = phi - e.phi();
            e.phi() = phi;
            dn = e.g.over ? 1u : (E::MOVE_LIMIT && st == ST_TRUNCATED ? 3u : 0u);     // is_end_of_game(): the walls, not the record's flag; 3: cut by the move limit
            restart = dn && (st == ST_OK || (E::MOVE_LIMIT && st == ST_TRUNCATED));
        } else if (st == ST_GAME_ENDED) {                               // a finished game handed in: restart the slot, report done
            dn = 1u;
            restart = true;
        }
    }
    if (AZ_UNLIKELY(wave_any(stuck | restart))) {
        if (stuck | restart) {
            if (stuck) { e.cnt.stuck_add += 1u; dn = 2u; }
            else if (E::MOVE_LIMIT && st == ST_TRUNCATED) e.cnt.stuck_add += 1u;      // (a cut episode is no finished game)
            else if (st == ST_OK) e.episode_stats();                   // (a game handed in finished is not counted: st == ST_GAME_ENDED)
            const bool cut = E::MOVE_LIMIT && st == ST_TRUNCATED;
            u32 st0 = e.fresh_game();
            st = stuck ? (st0 ? st0 : (u32)ST_STUCK) : (cut ? (st0 ? st0 : (u32)ST_TRUNCATED) : st0);
        }
    }
    return st;
}

// GameRunner.step (game_runner.py:43-55): the agent's move, the opponents' RandomAgent replies, the shaped reward, done.  No reset.
template <class E>
AZ_FN u32 runner_step(E &e, i32 av, i32 &rew, u32 &dn)
{
    rew = 0;
    dn = e.g.over ? 1u : 0u;
    u32 st = e.checked_step(av);                                       // game_runner.py:44
    if (!st) {
        e.moves() += 1u;                                               // :45
        st = e.opponent_loop(false);                                  // :46-47
        if (!st) {
            const i32 phi = e.potential();                             // :48-50
            rew = phi - e.phi();                                       // :51
            e.phi() = phi;                                             // :52
            dn = e.g.over ? 1u : 0u;                                   // :55
        }
    }
    return st;
}

// One AGENT step of NNRunner.run_episode (nn_runner.py:24-29): GameRunner.step and, when the episode ends, its statistics and the
// GameRunner.reset() that opens the next run_episode (nn_runner.py:20 -> game_runner.py:76-85, incl. the opponents' opening moves), so the
// observation / mask taken afterwards are the next decision's.  done 2: nobody could move; 3: cut by the move limit (slot restarted).
template <class E>
AZ_FN u32 agent_step(E &e, i32 av, i32 &rew, u32 &dn)
{
    u32 st = runner_step(e, av, rew, dn);
    const bool dirty = !(st == ST_ILLEGAL_MOVE || st == ST_BAD_ACTION);
    if (st == ST_STUCK) { e.cnt.stuck_add += 1u; dn = 2u; rew = 0; }   // hazard H3: nobody can move
    else if (E::MOVE_LIMIT && st == ST_TRUNCATED) { e.cnt.stuck_add += 1u; dn = 3u; rew = 0; }      // the episode was cut at the end of a round
    else if (st == ST_GAME_ENDED) dn = 1u;
    else if (st == ST_OK && dn) e.episode_stats();
    if (dirty && dn) {
        u32 st2 = e.fresh_game();                                      // game_runner.py:79-82
        if (!st2) st2 = e.opponent_loop(true);                        // :84-85
        if (st == ST_OK || (E::MOVE_LIMIT && st == ST_TRUNCATED && st2)) st = st2;
    }
    return st;
}

// ---- GameRunner with an EXTERNAL opponent (game_runner.py:27-30: GameRunner(opponent=Agent(...)); scripts/run_batch.py:6-10) --------------
// The reference's GameRunner.step / reset call opponent.get_a_output(...) in a data-dependent loop (game_runner.py:46-47, :84-85).  When the
// opponent is a network the answer comes from OUTSIDE the rule code (the matrix phases of a window kernel, or a separate launch), so the
// two methods are cut at their opponent_move() calls into a three-state protocol per game:
//     NET_REPLY    inside GameRunner.step's loop (:46): the opponent moves while (current_player != 1 or player 1 has fewer than two legal
//                  moves) and the game is not over -- player 1's FORCED moves are the opponent's too
//     NET_OPENING  inside GameRunner.reset's loop (:84): the opponent moves while current_player != 1
//     NET_READY    nothing owed: the agent's next decision
// net_move plays the agent's action (:44-45) or one opponent_move() (:37-42) with the action somebody chose on the mask /
// perspective-rotated observation net_settle left; net_settle runs the loop conditions, closes the step (:48-55: shaped reward, done,
// statistics) and opens the next episode (nn_runner.py:20 -> game_runner.py:76-82) -- agent_step's bookkeeping, statement for statement,
// with the RandomAgent's draw replaced by "owed".  `e.m` is always the legal mask of the state left behind.  No reply guard here: the
// caller bounds its reply rounds.
enum : u32 { NET_READY = 0, NET_REPLY = 1, NET_OPENING = 2, NET_RESET = 3 /* internal: the next episode's game is due (never stored) */ };

struct NetStep {
    u32 pending;     // NET_*
    u32 replies;     // opponent moves played since the agent's action (opening moves of the next episode included)
    i32 rew;         // valid once `closed`
    u32 dn;
    bool closed;     // the agent step's reward / done are final
    u32 st;          // first status that was not ST_OK
};

// The loop conditions.  Leaves ns.pending = NET_REPLY / NET_OPENING (an opponent_move() is owed on the state and mask left behind) or
// NET_READY.  ONE site each for the episode reset and the legal mask: the window kernels inline this function once.
template <class E>
AZ_FN void net_settle(E &e, NetStep &ns)
{
#pragma unroll 1
    for (u32 pass = 0; pass < SETTLE_PASSES; pass++) {
        if (ns.pending == NET_RESET) {                                          // the next run_episode: nn_runner.py:20 -> game_runner.py:76-82
            const u32 st2 = e.fresh_game();
            if (!ns.st) ns.st = st2;
            ns.pending = st2 ? (u32)NET_READY : (u32)NET_OPENING;
            continue;
        }
        e.legal_mask(e.m);
        if (ns.pending == NET_READY) break;
        const u32 legal = e.count(e.m);
        if (ns.pending == NET_REPLY) {
            const bool keep = (e.g.cur != 1u || legal < 2u) && !e.g.over;      // game_runner.py:46
            if (keep && legal) break;                                           // :47 -- an opponent_move() is owed
            ns.closed = true;
            if (keep) {                                                         // nobody can move (hazard H3; an Agent raises IllegalMask, model.py:33-34)
                e.cnt.stuck_add += 1u; ns.dn = 2u; ns.rew = 0;
                if (!ns.st) ns.st = ST_STUCK;
            } else {
                const i32 phi = e.potential();                                 // :48-50
                ns.rew = phi - e.phi();                                        // :51
                e.phi() = phi;                                                 // :52
                ns.dn = e.g.over ? 1u : 0u;                                    // :55
                if (ns.dn) e.episode_stats();                                  // :53-54
            }
            ns.pending = ns.dn ? (u32)NET_RESET : (u32)NET_READY;
            if (!ns.dn) break;                                                  // (`m` is the mask of this state: the agent's next decision)
        } else {                                                                // NET_OPENING
            if (e.g.cur != 1u && legal) break;                                  // game_runner.py:84-85 -- an opponent_move() is owed
            if (e.g.cur != 1u && !ns.st) ns.st = ST_STUCK;
            ns.pending = NET_READY;
            break;
        }
    }
}

// One move of the protocol: the AGENT's action of GameRunner.step (game_runner.py:44-45; `agent`) or one opponent_move() (:37-42) of a game
// that owes one, then the loop conditions.  `e.m`: out, the legal mask of the state left behind.  Returns the status of the move itself.
// An opponent's answer that is not a legal action (ST_ILLEGAL_MOVE / ST_BAD_ACTION) leaves the game and the debt as they are (the reference
// lets IllegalMove escape from GameRunner.step); refused / failed agent moves follow agent_step's bookkeeping.
template <class E>
AZ_FN u32 net_move(E &e, i32 av, bool agent, NetStep &ns)
{
    if (agent) { ns.pending = NET_READY; ns.replies = 0; ns.rew = 0; ns.dn = e.g.over ? 1u : 0u; ns.closed = false; ns.st = ST_OK; }
    const u32 st = e.checked_step(av);                                          // :44 / :41
    if (st == ST_OK) {
        e.moves() += 1u;                                                        // :45 / :42
        if (agent) ns.pending = NET_REPLY; else ns.replies += 1u;
    } else {
        if (!ns.st) ns.st = st;
        if (st == ST_ILLEGAL_MOVE || st == ST_BAD_ACTION) {                     // state untouched
            if (agent) ns.closed = true;
            e.mask_after_refusal();
            return st;
        }
        const bool in_step = agent || ns.pending == NET_REPLY;                  // (runner_step returning a status: reward 0, done only for GAME_ENDED)
        ns.pending = NET_READY;
        if (in_step) {
            ns.closed = true; ns.rew = 0;
            ns.dn = st == ST_GAME_ENDED ? 1u : (E::MOVE_LIMIT && st == ST_TRUNCATED ? 3u : (agent ? ns.dn : 0u));
            if constexpr (E::MOVE_LIMIT) {
                if (st == ST_TRUNCATED) {                                       // move limit: the episode was cut at the end of a round
                    e.cnt.stuck_add += 1u;
                    if (!agent) ns.replies += 1u;                               // (the opponent's move WAS played: the round it ended is scored)
                }
            }
            if (ns.dn) ns.pending = NET_RESET;
        }
    }
    net_settle(e, ns);
    return st;
}

// GameRunner.reset() with an external opponent (game_runner.py:76-85): the fresh game, then the opening loop's condition
template <class E>
AZ_FN void net_reset(E &e, NetStep &ns)
{
    ns.pending = NET_RESET; ns.replies = 0; ns.rew = 0; ns.dn = 0; ns.closed = false; ns.st = ST_OK;
    net_settle(e, ns);
}

} // namespace azr
