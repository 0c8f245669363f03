// azul_env2.hpp -- GameRunner on the two-player rule book: GameRunner.get_state / RandomAgent.get_a_output / Azul.step with its legality
// test / the fresh game of GameRunner.reset, for TWO GAMES PER WAVEFRONT on top of azul_selfplay2.hpp's half-uniform rules (state in VGPRs,
// one game per 32-lane half), and Env2, the adaptor through which azul_runner.hpp's GameRunner.step / reset protocol runs on them.  Two users: the env side of the persistent policy rollout (azul_rollout2.hpp calls
// these between its matrix phases) and the two-player rule entries of the C ABI (azul_ops2.hpp).  tests/hostcheck/simt_env2.cpp and
// simt_ops2.cpp run THIS FILE, unmodified, lane by lane on the CPU against the oracle.
// Reference lines: azulnet/azul.py:296-313 (step), azulnet/game_runner.py:43-55 (GameRunner.step), :56-72 (get_state), :76-85 (reset),
// :87-97 (RandomAgent); azulnet/nn_runner.py:17-47.
#pragma once
#include "azul_selfplay2.hpp"
#include "azul_runner.hpp"

namespace az2 {

// ---- observation: game_runner.py:56-72, 136 values; value j of my game for j = lane + 32 i ------------------------------------------
// (layout: cells 0..30 | pattern_lines[order[0]] | pattern_lines[order[1]] | walls[order[0]] | walls[order[1]] |
// floors | scores | next first player, seen from player `persp`)
template <int I>
AZ_FN u32 observe_val2(const G2 &g, u32 o0 /* half-uniform: 0 / 1 */, u32 l)
{
    const u32 cpa = o0 ? g.cp1 : g.cp0, cpb = o0 ? g.cp0 : g.cp1;
    const u32 wall_a = o0 ? g.wall1 : g.wall0, wall_b = o0 ? g.wall0 : g.wall1;
    if (I == 0) {
        const u32 pa0 = hread(cpa, 0u);
        return l < 31u ? g.cs : pa0;                                   // j = 31: order[0]'s cell 0
    }
    if (I == 1) {                                                       // j = 32 + l: order[0] cells 1..24 (l < 24), order[1] cells 0..7
        const u32 va = hread(cpa, l + 1u), vb = hread(cpb, l - 24u);
        return l < 24u ? va : vb;
    }
    if (I == 2) {                                                       // j = 64 + l: order[1] cells 8..24 (l < 17), walls[order[0]] bits 0..14
        const u32 vb = hread(cpb, l + 8u);
        return l < 17u ? vb : (wall_a >> ((l - 17u) & 31u)) & 1u;
    }
    if (I == 3)                                                         // j = 96 + l: walls[order[0]] bits 15..24 (l < 10), walls[order[1]] bits 0..21
        return l < 10u ? (wall_a >> (l + 15u)) & 1u : (wall_b >> ((l - 10u) & 31u)) & 1u;
    // j = 128 + l (l < 8): walls[order[1]] bits 22..24, floors, scores, next first player
    const u32 floor_a = o0 ? g.floor1 : g.floor0, floor_b = o0 ? g.floor0 : g.floor1;
    const i32 score_a = o0 ? g.score1 : g.score0, score_b = o0 ? g.score0 : g.score1;
    const u32 pnfp = g.nfp > 0u ? (((g.nfp - 1u - o0) & 1u) + 1u) : 0u;     // game_runner.py:58-61
    u32 v = (wall_b >> ((l + 22u) & 31u)) & 1u;
    v = l == 3u ? floor_a : v;
    v = l == 4u ? floor_b : v;
    v = l == 5u ? (u32)score_a : v;
    v = l == 6u ? (u32)score_b : v;
    v = l == 7u ? pnfp : v;
    return v;
}

// writes the 136 floats of my game to `lds_row` (the network's A operand) and, when given, to `glob` (trajectory slot)
AZ_FN void observe2(const G2 &g, u32 persp, float *lds_row, float *glob, u32 l)
{
    const u32 o0 = persp & 1u;
    float v0 = (float)(i32)observe_val2<0>(g, o0, l), v1 = (float)(i32)observe_val2<1>(g, o0, l), v2 = (float)(i32)observe_val2<2>(g, o0, l),
          v3 = (float)(i32)observe_val2<3>(g, o0, l), v4 = (float)(i32)observe_val2<4>(g, o0, l);
    lds_row[l] = v0; lds_row[l + 32u] = v1; lds_row[l + 64u] = v2; lds_row[l + 96u] = v3;
    if (l < 8u) lds_row[l + 128u] = v4;
    if (glob) {          // (the rollout kernel passes NULL: its trajectory slot is filled from the LDS rows by waves that idle during the head phase)
        glob[l] = v0; glob[l + 32u] = v1; glob[l + 64u] = v2; glob[l + 96u] = v3;
        if (l < 8u) glob[l + 128u] = v4;
    }
}

// ---- the legal action of ordinal `want` (counted from 0, ascending action order) as a move code: p1 .. p5 are the counts of legal actions
// below mask words 1 .. 5.  The one statement of the step for random_agent2 and playout_agent2 below.
AZ_FN u32 ordinal_code2(const Mask2 &m, u32 want, u32 p1, u32 p2, u32 p3, u32 p4, u32 p5, const K2 &k)
{
    const u32 l = k.l;
    const bool g1 = want >= p1, g2 = want >= p2, g3 = want >= p3, g4 = want >= p4, g5 = want >= p5;
    // (the selects as a tree of depth three -- the g's are monotone, g5 => g4 => .. => g1 -- instead of a chain of five: -0.45 % on the headline kernel)
    const u32 w01 = g1 ? m.m[1] : m.m[0], w23 = g3 ? m.m[3] : m.m[2], w45 = g5 ? m.m[5] : m.m[4];
    const u32 b01 = g1 ? p1 : 0u, b23 = g3 ? p3 : p2, b45 = g5 ? p5 : p4;
    const u32 mword = g4 ? w45 : (g2 ? w23 : w01);
    const u32 base = g4 ? b45 : (g2 ? b23 : b01);
    const u32 prow_ = (u32)g1 + (u32)g2 + (u32)g3 + (u32)g4 + (u32)g5;
    // my bit is set AND its rank among the word's set bits is the wanted one, as ONE compare (a ballot of an and of two compares goes
    // through a 0 / 1 register): 2 (rank - wanted) + bit == 1
    const bool hit = (((u32)__popc(mword & ((1u << l) - 1u)) - (want - base)) << 1) + ((mword >> l) & 1u) == 1u;
    const u32 ln = (u32)__builtin_ctz(hb(hit) | 0x80000000u);
    return hbcast(k.lcode, ln) | (prow_ << 13) | ((30u * prow_ + ln) << 17);
}

// ---- RandomAgent.get_a_output (game_runner.py:87-97): selfplay_step2's decision as a function --------------------------------------
// Returns false when nothing is legal (ValueError in the reference, raised BEFORE random() is called: no words consumed).
AZ_FN bool random_agent2(const Mask2 &m, Rng2 &r, const Tab2 &T, const K2 &k, u32 &code)
{
    const u32 l = k.l;
    const u32 c0 = __popc(m.m[0]), c1 = __popc(m.m[1]), c2 = __popc(m.m[2]), c3 = __popc(m.m[3]), c4 = __popc(m.m[4]), c5 = __popc(m.m[5]);
    const u32 J = c0;
    const u32 p1 = c0, p2 = p1 + c1, p3 = p2 + c2, p4 = p3 + c3, p5 = p4 + c4, L = p5 + c5;
    code = 0;
    if (L == 0u) return false;
    // (floor-only masks, M == 0, take the table's ninth pair {fl(100 S[J]), 0} with the ordinal counted from 0: selfplay_step2, azul_tables.hpp)
    const u32 M = L - J, Mc = M ? M : 256u, Jc = J < 31u ? J : 30u;
    const u32 kbase = M ? J : 0u;
    const double2 fs = T.fs[9u * Jc + 31u - (u32)__builtin_clz(Mc)];
    const double sJ = fs.y;
    const double total = ((double)M + fs.x) + 0.0;
    const double u = rng2_random(r, l);
    const double x = u * total;
    const double d = x - sJ;
    const u32 fl = (u32)d;
    const double fr = d - (double)fl;
    u32 kg = kbase + fl + 1u;
    const bool edge = !(__builtin_fabs(fr - 0.5) < 0.5 - 1e-9) | (kg > L);
    if (AZ_UNLIKELY(edge)) {
        const double sT = M ? sJ : T.fs[9u * Jc].y;      // the boundary search works on CPython's own x = random() * (S[J] + 0.0)
        kg = sample_slow2(T, M ? x : u * (sT + 0.0), sT, J, M, L);
    }
    code = ordinal_code2(m, kg - 1u, p1, p2, p3, p4, p5, k);
    return true;
}

// ---- the flat Monte-Carlo playout's move (azul_ops2.hpp: playout_moves_body2): uniform over the legal pattern-line moves, the floor moves
// only when nothing else is legal; `w` is the 32-bit word that decides.  False (nothing played) when nothing is legal.
AZ_FN bool playout_agent2(const Mask2 &m, u32 w, const K2 &k, u32 &code)
{
    const u32 c0 = __popc(m.m[0]), c1 = __popc(m.m[1]), c2 = __popc(m.m[2]), c3 = __popc(m.m[3]), c4 = __popc(m.m[4]), c5 = __popc(m.m[5]);
    const u32 p1 = c0, p2 = p1 + c1, p3 = p2 + c2, p4 = p3 + c3, p5 = p4 + c4, L = p5 + c5;
    const u32 M = L - c0, n = M ? M : c0, base = M ? c0 : 0u;
    code = ordinal_code2(m, base + __umulhi(w, n), p1, p2, p3, p4, p5, k);      // (L == 0: ordinal 0 of an empty mask, a code nobody plays)
    return L != 0u;
}

// the same packing for an action given by number
AZ_FN u32 action_code2(u32 a, const K2 &k)
{
    const u32 prow_ = a / 30u, ln = a - 30u * prow_;
    return hbcast(k.lcode, ln) | (prow_ << 13) | (a << 17);
}

// ---- Azul.step's body for a legal move (azul.py:304-313: move, then end of round -> scoring -> end of game / next round), what-if caches kept
template <bool LID>
AZ_FN u32 apply_step2(G2 &g, u32 code, Rng2 &r, u64 margin, const K2 &k)
{
    const u32 me = me2(g);
    const bool filled = do_move2<LID>(g, code, g.B, k);               // azul.py:304
    g.B = hb(g.cs != 0u) & 0x7fffffffu;
    const bool eor = g.B == 0u;                                        // :306 (then count_score2 prices the lines for real and clears the cache)
    i32 wc = me ? g.wc1 : g.wc0;
    if (wave_any(filled & !eor)) {
        const i32 fresh = wall_points2(me ? g.wall1 : g.wall0, full_lines2(me ? g.cp1 : g.cp0, k), k);
        wc = filled ? fresh : wc;
    }
    const i32 wi = clamp0((me ? g.score1 : g.score0) + floor_penalty(me ? g.floor1 : g.floor0) + wc);
    g.wc0 = me ? g.wc0 : wc; g.wc1 = me ? wc : g.wc1;
    g.wi0 = me ? g.wi0 : wi; g.wi1 = me ? wi : g.wi1;
    g.cur = eor ? g.cur : (g.cur & 1u) + 1u;              // :313
    u32 st = ST_OK;
    // (rare events are tested per wave and kept out of line: two waves per SIMD cannot hide a taken branch's instruction refetch)
    if (AZ_UNLIKELY(wave_any(eor))) {
        if (eor) {
            count_score2<LID>(g, k);                                   // :307
            if (g.over) g.eog = 1;                                     // :308-309
            else if (g.moves + 1u >= rng2_move_limit(r)) st = ST_TRUNCATED;      // move limit (beyond the reference, off by default; the caller counts this move next)
            else st = new_round2<LID>(g, r, margin, k);                // :311
        }
    }
    return st;
}

// Azul.step with the legality test of azul.py:298-302; `m` is the mask of the current state
template <bool LID>
AZ_FN u32 checked_step2(G2 &g, i32 a, const Mask2 &m, Rng2 &r, u64 margin, const K2 &k)
{
    if (g.eog) return ST_GAME_ENDED;
    if (a < 0 || a >= 180) return ST_BAD_ACTION;
    const u32 row = (u32)a / 30u, bit = (u32)a - 30u * row;
    const u32 word = row == 0u ? m.m[0] : row == 1u ? m.m[1] : row == 2u ? m.m[2] : row == 3u ? m.m[3] : row == 4u ? m.m[4] : m.m[5];
    if (((word >> bit) & 1u) == 0u) return ST_ILLEGAL_MOVE;             // state untouched
    return apply_step2<LID>(g, action_code2((u32)a, k), r, margin, k);
}

AZ_FN u32 mask_count2(const Mask2 &m) { return __popc(m.m[0]) + __popc(m.m[1]) + __popc(m.m[2]) + __popc(m.m[3]) + __popc(m.m[4]) + __popc(m.m[5]); }

AZ_FN void episode_stats2(const G2 &g, Counters2 &cnt, u32 l)
{
    const double f0 = (double)(g.fps & 0xffffu), f1 = (double)(g.fps >> 16);
    counters2_episode(cnt, stat_lane(l, g.score0, g.score1, g.turn, f0 / (f0 + f1) * 100, g.fp0, g.mc0, g.cl0));
}

template <bool LID>
AZ_FN u32 reset2(G2 &g, u32 first_player, Rng2 &r, u64 margin, const K2 &k)
{
    u32 st = episode_reset2<LID>(g, first_player, r, margin, k);
    prime2(g, k);
    return st;
}

// GameRunner's opponent loop (game_runner.py:46-47 / :84), the ONE piece of the step protocol that stays per record shape (Env2's
// opponent_loop member): here the RandomAgent draws BEFORE the end-of-game test and a loop that hits the guard returns ST_OK; the wide
// loop (azx::opponent_loop_x) tests first and returns ST_STUCK.
template <bool LID>
AZ_FN u32 opponent_loop2(G2 &g, Rng2 &r, const Tab2 &T, u64 margin, const K2 &k, bool until_player1_only)
{
#pragma unroll 1
    for (u32 guard = 0; guard < azr::REPLY_GUARD; guard++) {
        Mask2 m;
        legal_mask2(g, k, m);
        const bool keep = until_player1_only ? (g.cur != 1u) : ((g.cur != 1u || mask_count2(m) < 2u) && !g.over);
        if (!keep) break;
        u32 code;
        if (!random_agent2(m, r, T, k, code)) return ST_STUCK;
        if (g.eog) return ST_GAME_ENDED;
        u32 st = apply_step2<LID>(g, code, r, margin, k);
        if (st) return st;
        g.moves += 1u;
    }
    return ST_OK;
}

// ---- the two-player env adaptor of azul_runner.hpp: GameRunner.step / reset and their cut-at-opponent_move() form (azr::policy_step,
// runner_step, agent_step, net_settle, net_move, net_reset) on a register-resident G2.  References to what the call site
// holds; `m` is the legal mask of the current state (in: checked_step tests the action against it; out: net_settle leaves the mask of the
// state left behind).  GameRunner.player_score / move_counter are the record's own g.pscore / g.moves.
template <bool LID>
struct Env2 {
    using Mask = Mask2;
    static constexpr bool MOVE_LIMIT = true;                 // apply_step2 can cut an episode (ST_TRUNCATED)
    G2 &g;
    Mask2 &m;
    const u32 &first_player;
    Rng2 &r;
    const Tab2 &tab;
    const u64 &margin;
    Counters2 &cnt;
    const K2 &k;

    AZ_MEMBER_FN void legal_mask(Mask2 &out) const { legal_mask2(g, k, out); }
    AZ_MEMBER_FN u32 count(const Mask2 &t) const { return mask_count2(t); }
    AZ_MEMBER_FN u32 count_current() const { return mask_count2(m); }                  // (`m` is the one that was published)
    AZ_MEMBER_FN u32 checked_step(i32 a) { return checked_step2<LID>(g, a, m, r, margin, k); }
    AZ_MEMBER_FN void mask_after_refusal() {}                                          // (state untouched: `m` is still its mask)
    AZ_MEMBER_FN u32 opponent_loop(bool opening) { return opponent_loop2<LID>(g, r, tab, margin, k, opening); }
    AZ_MEMBER_FN i32 potential() const { return g.wi0 - g.wi1; }                       // (the what-if caches are current)
    AZ_MEMBER_FN i32 &phi() { return g.pscore; }
    AZ_MEMBER_FN u32 &moves() { return g.moves; }
    AZ_MEMBER_FN u32 fresh_game() { return reset2<LID>(g, first_player, r, margin, k); }
    AZ_MEMBER_FN void episode_stats() { episode_stats2(g, cnt, k.l); }
};

// The entry points the kernels call: each builds the adaptor from its arguments and forwards.  They stay because calling the shared
// functions from the kernels directly (one adaptor per kernel) changed the instructions of 35 of the 110 kernels, with more scratch in
// some; through these wrappers every kernel compiles to the parent's instruction stream.  (`tab` / `cnt` / `first_player` that an entry
// does not take are never read on its path.)
template <bool LID>
AZ_FN u32 policy_step2(G2 &g, i32 av, Mask2 &m, u32 first_player, Rng2 &r, u64 margin, Counters2 &cnt, const K2 &k, i32 &rew, u32 &dn)
{ const Tab2 tab = {nullptr}; Env2<LID> e{g, m, first_player, r, tab, margin, cnt, k}; return azr::policy_step(e, av, rew, dn); }
template <bool LID>
AZ_FN u32 runner_step2(G2 &g, i32 av, Mask2 &m, Rng2 &r, const Tab2 &T, u64 margin, const K2 &k, i32 &rew, u32 &dn)
{ Counters2 cnt; const u32 fp = 0; Env2<LID> e{g, m, fp, r, T, margin, cnt, k}; return azr::runner_step(e, av, rew, dn); }
template <bool LID>
AZ_FN u32 agent_step2(G2 &g, i32 av, Mask2 &m, u32 first_player, Rng2 &r, const Tab2 &T, u64 margin, Counters2 &cnt, const K2 &k, i32 &rew, u32 &dn)
{ Env2<LID> e{g, m, first_player, r, T, margin, cnt, k}; return azr::agent_step(e, av, rew, dn); }
using azr::NetStep; using azr::NET_READY; using azr::NET_REPLY; using azr::NET_OPENING; using azr::NET_RESET;
template <bool LID>
AZ_FN void net_move2(G2 &g, i32 av, bool agent, Mask2 &m, u32 first_player, Rng2 &r, u64 margin, Counters2 &cnt, const K2 &k, NetStep &ns)
{ const Tab2 tab = {nullptr}; Env2<LID> e{g, m, first_player, r, tab, margin, cnt, k}; azr::net_move(e, av, agent, ns); }
template <bool LID>
AZ_FN void net_reset2(G2 &g, Mask2 &m, u32 first_player, Rng2 &r, u64 margin, Counters2 &cnt, const K2 &k, NetStep &ns)
{ const Tab2 tab = {nullptr}; Env2<LID> e{g, m, first_player, r, tab, margin, cnt, k}; azr::net_reset(e, ns); }

// ---- the one-ply greedy player of the reference's own reward (game_runner.py:48-50; azul_ops2.hpp: score_moves_body2's table) ----------------
// (score, lowest action) as ONE unsigned key for the half-wave maximum: a score difference lies in (-2^16, 2^16) -- both what-if scores
// are clamped at 0 and stay below 2^16 (the record keeps scores in 16 bits; the full lines of one round add at most 5 * 29 points) -- so
// score + 2^16 is a positive 17-bit number; below it 255 - a, so that among equal scores the LOWEST action is the maximum.  0 = no move.
AZ_FN u32 score_key(i32 score, u32 a) { return ((u32)(score + 65536) << 8) | (255u - a); }

// The mover's what-if score after candidate `act`: score[me] of a copy of the game after move(*nn_deserialize(act)) and count_score()
// (azul.py:118-161, :192-295; nothing committed).  Total for every action number: do_move2 decodes the source lane, display base, colour
// and row from the ACTION (K2::lcode), never from the state.  Each candidate starts from the game again (`t = g`): a move changes only the
// mover's line, floor and the source cells, so the copy is those few registers, not a second live game.
template <bool LID>
AZ_FN i32 whatif_after2(const G2 &g, u32 act, u32 me, const K2 &k)
{
    G2 t = g;
    do_move2<LID>(t, action_code2(act, k), g.B, k);                                                   // azul.py:118-161
    const i32 wc = wall_points2(me ? g.wall1 : g.wall0, full_lines2(me ? t.cp1 : t.cp0, k), k);       // :211-290
    return clamp0((me ? g.score1 : g.score0) + floor_penalty(me ? t.floor1 : t.floor0) + wc);        // :200-209, :292-295
}

// The greedy player's answer on a register-resident game and its legal mask `m`, from the MOVER's perspective: the first legal action
// with the maximal score[p] - score[1 - p] after move + count_score (np.argmax's rule), -1 when nothing is legal.  Reads the game only;
// draws nothing.  The candidate loop is wave-uniform (a candidate neither half's mask holds is skipped by a ballot; one that only ONE
// half's mask holds runs on both and the other half discards it): call it with the whole wave active.
template <bool LID>
AZ_FN i32 greedy_pick2(const G2 &g, const Mask2 &m, const K2 &k)
{
    const u32 me = me2(g);
    const i32 other = me ? g.wi0 : g.wi1;                // the opponent's what-if score: a move leaves it alone
    u32 key = 0;
#pragma unroll 1
    for (u32 row = 0; row < 6u; row++) {
        const u32 word = row == 0u ? m.m[0] : row == 1u ? m.m[1] : row == 2u ? m.m[2] : row == 3u ? m.m[3] : row == 4u ? m.m[4] : m.m[5];
#pragma unroll 1
        for (u32 ln = 0; ln < 30u; ln++) {
            const bool legal = ((word >> ln) & 1u) != 0u;
            if (!wave_any(legal)) continue;
            const u32 act = 30u * row + ln;
            const i32 v = whatif_after2<LID>(g, act, me, k) - other;
            key = (legal & (k.l == ln)) ? umax(key, score_key(v, act)) : key;
        }
    }
    const u32 top = hmax(key);                           // (lanes 30, 31 hold 0)
    return top ? (i32)(255u - (top & 0xffu)) : -1;
}

} // namespace az2
