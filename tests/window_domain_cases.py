"""TEST helper: the window kernels started from arbitrary in-domain records (tests/domain_records.py) -- the records of a config, the model
slots that hold them (tests/mp_runner_model.MPRunner.from_record), the replay that checks a window's trajectory and the batch state after it
against the model, and the census of what the records make a window do.  Plain numpy + the oracle: no project code.  The emulation
(tests/test_hostcheck_window_domain_records.py) and the GPU tests (tests/test_gpu_window_domain_records.py) share it.

A config's records: n records of the four families (dr.two_player / dr.wide) followed by n_ended of dr.ended.  The wide record keeps the
runner's tail in its padding (bytes 228..231): the generators leave it zero, here it gets a potential and a move count like the 128-byte
record's player_score / move_counter have.

The census (CLASSES) is a condition on the records, not a measurement: every class is forced by a record, whatever the policy answers --
  ok_done     a step that ends an episode (status OK, done = 1): the records with a complete wall row and the flag clear;
  stuck       status STUCK, done = 2: nothing legal for the seat to move.  Flat self-play (opp 0) only: under GameRunner (opp 1) an agent
              without a legal move answers -1, which is BAD_ACTION and leaves the slot as it is (game_runner.py:44), and the RandomAgent
              seats are stuck only behind a move that leaves the token alone in the centre -- no record forces that;
  game_ended  a step on a record whose ended flag is set (Azul.step's GameEnded; done = 1, the slot restarts);
  box_empty   status BOX_EMPTY: a round-ending table with nothing in box and lid, where the config can run dry (dr.unreachable);
  deal        a step that ends a round and deals the next one inside the episode (turn_counter moves on, status OK, done = 0).
`left_out` counts the post-states the record cannot hold (must be 0: change the SEED, as tests/domain_records.py has it)."""
import numpy as np

from oracle import oracle as oz
from tests import domain_records as dr
from tests.mp_runner_model import BOX_EMPTY, OK, STUCK, MPRunner

CLASSES = ("ok_done", "stuck", "game_ended", "box_empty", "deal")
RECORD_SEED, STREAM_SEED = 7100, 61000
# (config, n) whose default seed leaves a game out: the oracle's 128-byte record holds at most 15 tiles in a cell, and a long round of one
# of that batch's dense games collects 16 of a colour in the centre.  The next seed by 1000 that leaves none out under eight answer policies.
SEED_BUMP = {("p2d5-lid", 64): 1}


def required(cfg, opp):
    out = set(CLASSES)
    if "box_empty" in dr.unreachable(cfg):
        out.discard("box_empty")
    if opp:
        out.discard("stuck")
    return out


def is_two(cfg):
    return cfg in dr.TWO_CONFIGS


def records(cfg, n, n_ended, seed=None):
    """uint8 [n + n_ended][128 | 256]: n records of the four families, then n_ended of dr.ended."""
    P, ext, pool = cfg
    D = dr.displays(cfg)
    if seed is None:
        seed = RECORD_SEED + 1000 * SEED_BUMP.get((dr.config_id(cfg), n), 0)
    seed += 10 * P + ext + pool
    if is_two(cfg):
        recs = np.concatenate([dr.two_player(n, seed), dr.ended(n_ended, 2, 5, seed + 1, False)])
    else:
        recs = np.concatenate([dr.wide(n, P, D, seed), dr.ended(n_ended, P, D, seed + 1)])
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), -1).copy()
    if not is_two(cfg):
        rs = np.random.RandomState(seed + 2)
        raw[:, 228:230] = rs.randint(-20, 20, size=len(raw)).astype("<i2").view(np.uint8).reshape(-1, 2)
        raw[:, 230:232] = rs.randint(0, 60, size=len(raw)).astype("<u2").view(np.uint8).reshape(-1, 2)
    return raw


def models(cfg, raw, stream_seed=STREAM_SEED, cls=MPRunner):
    """One model slot (`cls`: MPRunner or a subclass) per record, record i on dr.stream_of(stream_seed, i); every record must come back
    from the model byte for byte."""
    out = []
    for i, r in enumerate(raw):
        m = cls.from_record(r, cfg, dr.stream_of(stream_seed, i))
        assert np.array_equal(m.record(), r), i
        out.append(m)
    return out


def streams(ms):
    """(mt uint32 [N][624], pos uint32 [N]) of the models' streams: what set_rng_range / the shims take."""
    pos = np.array([m.rng_state()[1] for m in ms], np.uint32)
    assert (pos <= 624).all()
    return np.stack([m.rng_state()[0] for m in ms]).astype(np.uint32), pos


def _step(m, opp, a, census):
    """One step of the model, booked in the census -> (status, reward, done)."""
    ended, turn = bool(m.g.end_of_game), int(m.g.turn_counter)
    st, rew, dn = (m.agent_step if opp else m.policy_step)(a)
    census["game_ended"] += int(ended)
    census["ok_done"] += int(not ended and st == OK and dn == 1)
    census["stuck"] += int(dn == 2)
    census["box_empty"] += int(st == BOX_EMPTY)
    census["deal"] += int(st == OK and dn == 0 and int(m.g.turn_counter) > turn)
    try:
        m.record()
    except (AssertionError, ValueError):
        census["left_out"] += 1
    return st, rew, dn


def new_census():
    return dict.fromkeys(CLASSES + ("left_out",), 0)


def model_census(cfg, opp, raw, T, seed=0):
    """The census of T steps per record on the model alone: a seeded random legal answer (-1 where nothing is legal)."""
    rs = np.random.RandomState(seed)
    census = new_census()
    for m in models(cfg, raw):
        for _ in range(T):
            legal = np.flatnonzero(m.mask())
            _step(m, opp, int(rs.choice(legal)) if len(legal) else -1, census)
    return census


def seat(m, opp):
    """The seat a slot is observed from: seat 0 under GameRunner, the mover in flat self-play."""
    return 0 if opp else (m.g.current_player - 1) % m.P


def replay(ms, opp, tr, T, census, tag=()):
    """A window's trajectory against the models, which move on by it: tr[k] arrays -- obs, mask, player [T + 1][N], action, reward, done,
    value, logp, entropy [T][N].  The kernel's own actions go through policy_step (opp 0) / agent_step (opp 1); obs, mask and player of
    every slot (slot T included), reward and done of every step must be the model's, exactly.  Of the network only: the action is legal,
    or -1 exactly where the mask is empty; value, log-prob and entropy are finite.  -> the status of every game's last step."""
    last = np.zeros(len(ms), np.int64)
    for g, m in enumerate(ms):
        for t in range(T + 1):
            at = tag + (g, t)
            mask = m.mask()
            assert np.array_equal(tr["obs"][t, g], m.obs(seat(m, opp)).astype(np.float32)), at + ("obs",)
            assert np.array_equal(tr["mask"][t, g], mask), at + ("mask",)
            assert int(tr["player"][t, g]) == m.g.current_player, at + ("player",)
            if t == T:
                break
            a = int(tr["action"][t, g])
            assert (0 <= a < len(mask) and mask[a]) if mask.any() else a == -1, at + ("action", a)
            assert np.isfinite([tr["value"][t, g], tr["logp"][t, g], tr["entropy"][t, g]]).all(), at + ("value / log-prob / entropy",)
            st, rew, dn = _step(m, opp, a, census)
            assert (int(tr["reward"][t, g]), int(tr["done"][t, g])) == (rew, dn), at + ("reward / done", int(tr["reward"][t, g]), int(tr["done"][t, g]), rew, dn, st)
            last[g] = st
    return last


def check_state(ms, last, state, mt, pos, episodes, stuck, stat_sums, status, tag=()):
    """The batch after a window against the models: record bytes (tail included), the 624 MT words and the index, the episodes, stuck and
    stat_sums counters, the per-game status -- exactly (an episode without any first-player count sums 0 / 0: NaN on both sides)."""
    state = np.ascontiguousarray(state).view(np.uint8).reshape(len(ms), -1)
    for g, m in enumerate(ms):
        at = tag + (g,)
        want = m.record()
        assert np.array_equal(state[g], want), at + ("record", np.flatnonzero(state[g] != want))
        mtm, posm = m.rng_state()
        assert int(pos[g]) == posm and np.array_equal(mt[g], mtm), at + ("stream", int(pos[g]), posm)
        assert (int(episodes[g]), int(stuck[g])) == (m.episodes, m.stuck), at + ("counters", int(episodes[g]), int(stuck[g]), m.episodes, m.stuck)
        assert np.array_equal(np.asarray(stat_sums[g], np.float64), m.stat_sum, equal_nan=True), at + ("stat_sums",)
        assert int(status[g]) == int(last[g]), at + ("status", int(status[g]), int(last[g]))


def assert_census(census, cfg, opp, tag=()):
    assert census["left_out"] == 0, tag + (census,)
    missing = [c for c in sorted(required(cfg, opp)) if census[c] == 0]
    assert not missing, tag + (missing, census)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
CPU_N, CPU_ENDED, CPU_T = 40, 9, 6                     # 49 games: a ragged last workgroup
GPU_N, GPU_ENDED, GPU_T, GPU_WINDOWS = 64, 3, 8, 2     # 67 games: an odd last wave / group; two windows of 8
CPU_WIDE = [dr.WIDE_CONFIGS[i] for i in (0, 2, 3, 4, 5)]
# the five shapes of tests/test_gpu_mp_fused_rollout.SHAPES as (players, ext, tile_pool): p2_d5x, p3_d5, p3_d7, p4_d5, p4_d9
GPU_WIDE = [(2, dr.END_BONUS, oz.POOL_LID), (3, 0, oz.POOL_LID), (3, dr.DISPLAYS_2P1, oz.POOL_LID), (4, 0, oz.POOL_LID),
            (4, dr.DISPLAYS_2P1 | dr.SHORT_DEAL, oz.POOL_RANDOM)]
