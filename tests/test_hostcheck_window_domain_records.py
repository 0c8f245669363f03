"""The window kernels on CPU, started from arbitrary in-domain records (tests/domain_records.py: mixed and overfull lines, floors at 7, dense
walls, round-ending tables, box / lid edges -- states no game reaches -- plus the `ended` records: the ended flag, an empty table, a
complete wall row with the flag clear): azul_policy_rollout2_kernel (both pools) and azul_x_policy_rollout_kernel (five wide configs), each
with opp 0 (the policy on every seat) and opp 1 (RandomAgent seats), compiled UNMODIFIED by g++ and run under the existing shims
(tests/hostcheck/window.py).  The other window tests start from reset() or from states legal play reaches and assert `stuck == 0`,
`status == 0`: here the stuck, GAME_ENDED and BOX_EMPTY paths, short deals, deals that straddle the MT19937 regeneration (every sixth
stream index lies within the last 30 words) and restarts run against the oracle's model (tests/window_domain_cases.py): observations,
masks, players, rewards, done flags, final records with the runner tail, streams, counters and statuses exactly; of the network only that
the action is legal (-1 exactly where nothing is) and value, log-prob and entropy are finite.  49 games leave the last workgroup ragged;
guard cells behind every output stay untouched.  The census of what the records forced is asserted from the kernel's own actions.
azul_x_policy_rollout_vs_kernel's body (a network opponent inside the window) runs from the same records against tests/mp_net_model.py."""
import numpy as np
import pytest

from oracle import oracle as oz
from tests import domain_records as dr
from tests import window_domain_cases as wd
from tests.hostcheck import window
from tests.hostcheck.window import GUARD, buf, games_fields, games_fields_x

N, T = wd.CPU_N + wd.CPU_ENDED, wd.CPU_T
FIRST = oz.FIRST_RANDOM


FILL = {"obs": -99, "mask": 0xEE, "player": 9, "action": -7, "reward": -7777, "done": 9, "value": np.nan, "logp": np.nan, "entropy": np.nan,
        "status": 99, "returns": np.nan}


def _outputs(n_obs, n_act, two):
    o, whole = {}, {}
    shapes = [("obs", (T + 1, N, n_obs), np.float32), ("mask", (T + 1, N, n_act), np.uint8), ("player", (T + 1, N), np.uint8),
              ("action", (T, N), np.int32), ("reward", (T, N), np.int32), ("done", (T, N), np.uint8), ("value", (T, N), np.float32),
              ("logp", (T, N), np.float32), ("entropy", (T, N), np.float32), ("status", (N,), np.uint8)]
    for k, shape, dt in shapes + ([("returns", (T, N), np.float32)] if two else []):
        whole[k], o[k] = buf(shape, dt, FILL[k])
    return o, whole


def _guards_untouched(whole):
    for k, a in whole.items():
        tail, fill = a[-GUARD:], FILL[k]
        assert np.isnan(tail).all() if np.isnan(fill) else (tail == fill).all(), k


def _run(cfg, opp):
    P, ext, pool = cfg
    two = wd.is_two(cfg)
    D = dr.displays(cfg)
    n_act, n_obs = (D + 1) * 30, 5 * D + 6 + 52 * P + 1
    raw = wd.records(cfg, wd.CPU_N, wd.CPU_ENDED)
    ms = wd.models(cfg, raw)
    state = raw.copy()
    mt, pos = wd.streams(ms)
    assert (pos[::6] >= 595).all()                         # a deal of these games straddles the regeneration
    ep, stuck, ss = np.zeros(N, np.uint64), np.zeros(N, np.uint32), np.zeros((N, 10))
    o, whole = _outputs(n_obs, n_act, two)
    if two:
        L = window.load2()
        oob, fields = L.sr2_buffer_oob, dict(games_fields(N, state, mt, pos, ep, stuck, ss, FIRST, pool), agent=window.weights2(60), gamma=0.9)
    else:
        L = window.load_x()
        oob = L.sxr_buffer_oob
        fields = dict(games_fields_x(N, P, D, state, mt, pos, ep, stuck, ss, FIRST, pool, ext, 1000), agent=window.weights_x(n_obs, n_act, 0x5EED + P))
    oob0 = oob()
    assert window.run(L, **fields, opp=opp, n_steps=T, **o, seed=4242, counter=17) > 0
    assert oob() == oob0
    _guards_untouched(whole)
    tag = (dr.config_id(cfg), opp)
    census = wd.new_census()
    last = wd.replay(ms, opp, o, T, census, tag)
    wd.check_state(ms, last, state, mt, pos, ep, stuck, ss, o["status"], tag)
    wd.assert_census(census, cfg, opp, tag)
    if two:                                                # the fused returns scan (nn_runner.py:70-76) on what the kernel recorded
        q, want = np.zeros(N, np.float32), np.zeros((T, N), np.float32)
        for t in range(T - 1, -1, -1):
            q = o["reward"][t].astype(np.float32) + np.float32(0.9) * np.where(o["done"][t] != 0, np.float32(0), q)
            want[t] = q
        assert np.array_equal(o["returns"], want), tag


@pytest.mark.parametrize("opp", [0, 1])
@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_two_player_window_kernel_from_domain_records_equals_the_model(cfg, opp):
    _run(cfg, opp)


@pytest.mark.parametrize("opp", [0, 1])
@pytest.mark.parametrize("cfg", wd.CPU_WIDE, ids=dr.config_id)
def test_wide_window_kernel_from_domain_records_equals_the_model(cfg, opp):
    _run(cfg, opp)


SLOTS = 64                     # trace slots per step: more than any step's reply rounds with legal answers


@pytest.mark.parametrize("cfg", [wd.CPU_WIDE[0], wd.CPU_WIDE[3]], ids=dr.config_id)
def test_wide_window_kernel_with_a_network_opponent_from_domain_records_equals_the_net_model(cfg):
    """azul_x_policy_rollout_vs_kernel's body from the same records: the kernel's agent actions and the answers it recorded, driven through
    tests/mp_net_model.MPNetRunner (GameRunner cut at its opponent_move() calls), give the recorded observations, masks, players, rewards,
    done flags and reply counts, then the records, streams, counters and statuses.  Every answer is legal for the seat that owed it, and
    the trace is written for the rounds a game owed, no other."""
    from tests.mp_net_model import READY, MPNetRunner
    P, ext, pool = cfg
    D = dr.displays(cfg)
    n_act, n_obs = (D + 1) * 30, 5 * D + 6 + 52 * P + 1
    raw = wd.records(cfg, wd.CPU_N, wd.CPU_ENDED)
    ms = wd.models(cfg, raw, cls=MPNetRunner)
    state = raw.copy()
    mt, pos = wd.streams(ms)
    ep, stuck, ss = np.zeros(N, np.uint64), np.zeros(N, np.uint32), np.zeros((N, 10))
    o, whole = _outputs(n_obs, n_act, False)
    fills = {"opp_action": -5, "opp_logp": 55.0, "opp_replies": 201}
    for k, shape, dt in (("opp_action", (T, SLOTS, N), np.int32), ("opp_logp", (T, SLOTS, N), np.float32), ("opp_replies", (T, N), np.uint8)):
        whole[k], o[k] = buf(shape, dt, fills[k])
    L = window.load_x()
    oob0 = L.sxr_buffer_oob()
    assert window.run(L, **games_fields_x(N, P, D, state, mt, pos, ep, stuck, ss, FIRST, pool, ext, 1000), opp=2,
                      agent=window.weights_x(n_obs, n_act, 0x5EED + P), opponent=window.weights_x(n_obs, n_act, 0x5EEE + P), n_steps=T, **o,
                      opp_slots=SLOTS, seed=4242, opp_seed=0x0770 + P, counter=17, max_replies=512) > 0
    assert L.sxr_buffer_oob() == oob0
    for k in fills:
        assert (whole[k][-GUARD:] == fills[k]).all(), k
    _guards_untouched({k: v for k, v in whole.items() if k not in fills})
    answers = ended = 0
    for g, m in enumerate(ms):
        tag = (dr.config_id(cfg), g)
        for t in range(T):
            mask = m.mask()
            assert np.array_equal(o["obs"][t, g], m.obs(0).astype(np.float32)) and np.array_equal(o["mask"][t, g], mask), tag + (t,)
            assert o["player"][t, g] == m.g.current_player, tag + (t,)
            a = int(o["action"][t, g])
            assert (0 <= a < n_act and mask[a]) if mask.any() else a == -1, tag + (t, a)
            ended += int(bool(m.g.end_of_game))
            m.net_begin(a)
            j = 0
            while m.pending != READY:
                assert j < SLOTS, tag + (t,)
                b = int(o["opp_action"][t, j, g])
                assert 0 <= b < n_act and m.mask()[b] and np.isfinite(o["opp_logp"][t, j, g]), tag + (t, j, b)
                m.net_reply(b)
                j += 1
            answers += j
            assert (o["opp_action"][t, j:, g] == -5).all() and (o["opp_logp"][t, j:, g] == 55.0).all(), tag + (t,)
            assert (o["reward"][t, g], o["done"][t, g], o["opp_replies"][t, g]) == (m.rew, m.dn, m.replies), tag + (t, m.rew, m.dn, m.replies)
        assert np.array_equal(o["obs"][T, g], m.obs(0).astype(np.float32)) and np.array_equal(o["mask"][T, g], m.mask()), tag
        assert o["player"][T, g] == m.g.current_player, tag
    wd.check_state(ms, [m.st for m in ms], state, mt, pos, ep, stuck, ss, o["status"], (dr.config_id(cfg),))
    assert answers > T * N // 2 and ended >= 3             # the opponent really moved; the ended records were stepped
