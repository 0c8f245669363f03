"""The window kernels on the MI355X, started from arbitrary in-domain records (tests/domain_records.py -- states no game reaches -- plus its
`ended` records; tests/window_domain_cases.py has the records, the model and the census): 64 + 3 games (an odd last wave / group), two
windows of 8 steps, handed in the way tests/test_policy_bridge.py hands in its unusual states -- set_records, set_rng_range,
reset_counters, observe_all into slot 0.

(a) azul_policy_rollout2_kernel (PolicyRollout(persistent=True), both pools) and azul_x_policy_rollout_kernel (fused_wide=True, the five
    shapes of tests/test_gpu_mp_fused_rollout.SHAPES), opponent None and "random": both windows replayed through the oracle's model --
    observations, masks, players, rewards, done flags, then records with the runner tail, MT19937 words and index, counters and status,
    exactly -- and compared bit for bit with the per-move path from the same hand-in (wide: dyadic weights, `_assert_exact` on the recorded
    observations -- larger here than in ordinary play -- is the premise, checked in fp64).  The census of what the records forced (stuck
    games, GAME_ENDED, BOX_EMPTY, episode ends, deals) is asserted on the kernel's own actions.
(b) The opponents inside the window kernels -- azul_x_policy_rollout_vs_kernel (fused_opponent=True, a network opponent) and the
    greedy_margin seats (fused_seats=True) on p3_d5 and p4_d9, the two-player opponent="greedy" (fused_opponent=True) -- against the per-cut
    path from the same hand-in, bit for bit: every trajectory array, opp_replies, the opponent's trace where a step's replies filled it,
    records, streams, counters, status and the Philox step counter.  A game that still owed a move at the reply cap would be marked in
    the status and the stuck counters, which are compared (the per-cut path raises instead: no game gets there)."""
import numpy as np
import pytest
import torch

from oracle import oracle as oz
from tests import domain_records as dr
from tests import window_domain_cases as wd
from tests.test_gpu_mp_fused_rollout import SHAPE_IDS, SHAPES, _assert_exact, _dyadic_policy, _eq

pytestmark = pytest.mark.gpu

N, T, WINDOWS, R = wd.GPU_N + wd.GPU_ENDED, wd.GPU_T, wd.GPU_WINDOWS, 6
TWO_RULES = {oz.POOL_LID: {"first_player": "Random", "tile_pool": "Lid"}, oz.POOL_RANDOM: {"first_player": "Random", "tile_pool": "Random"}}
TRAJ = ("obs", "mask", "player", "action", "reward", "done", "value", "log_prob", "entropy", "returns")


def _shape_cfg(shape):
    """SHAPES[shape] as a config of tests/domain_records.py, checked against the library's reading of the rules."""
    from azul_deep_reinforcement_learning_amd.multiplayer import MultiplayerAzul
    players, rules = SHAPES[shape]
    cfg = wd.GPU_WIDE[shape]
    env = MultiplayerAzul(1, rules=rules, players=players)
    assert cfg[0] == players and env.displays == dr.displays(cfg) and (rules["tile_pool"] == "Lid") == (cfg[2] == oz.POOL_LID)
    assert bool(cfg[1] & dr.END_BONUS) == (rules.get("bonuses") == "end") and bool(cfg[1] & dr.SHORT_DEAL) == bool(rules.get("short_deal"))
    return cfg


def _two_net():
    from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
    torch.manual_seed(3)
    return BatchedActorCritic(136, 180, 180)


def _hand_in(ro, cfg):
    """The records and streams of the config into the rollout's games -> the model slots that hold the same."""
    env = ro.envs[0]
    raw = wd.records(cfg, wd.GPU_N, wd.GPU_ENDED)
    ms = wd.models(cfg, raw)
    mt, pos = wd.streams(ms)
    ro.synchronize()
    env.set_records(raw.view(env.record_dtype).reshape(-1))                     # (set_state validates every record against the domain)
    env.set_rng_range(mt, pos)
    env.reset_counters()
    torch.cuda.synchronize()
    t = ro.traj[0]
    with torch.cuda.stream(ro.streams[0]):
        env.observe_all(ro._persp(), t["obs"][T], t["mask"][T], t["player"][T])      # slot 0 of the first window
    ro.synchronize()
    assert env.get_records().tobytes() == raw.tobytes()
    return ms


def _snapshot(ro):
    env = ro.envs[0]
    c = env.counters()
    mt, pos = env.get_rng_range()
    return {"rec": env.get_records().view(np.uint8).reshape(N, -1).copy(), "mt": mt, "pos": pos, "episodes": c["episodes"].copy(),
            "stuck": c["stuck"].copy(), "stat": c["stat_sums"].copy(), "status": ro.work[0]["status"].cpu().numpy().copy(),
            "philox": np.array(ro.work[0]["counter"].tolist())}


def _play(cfg, ro):
    """Two windows from the hand-in -> (model slots at the hand-in, per window the trajectory (CPU tensors) and the batch state after it)."""
    assert not ro.use_graph and ro.ring == 1 and ro.parts == 1
    ms = _hand_in(ro, cfg)
    wins, states = [], []
    for _ in range(WINDOWS):
        ro.run_window(gamma=0.99)
        ro.synchronize()
        torch.cuda.synchronize()
        wins.append({k: v.detach().cpu().clone() for k, v in ro.traj[0].items()})
        states.append(_snapshot(ro))
    return ms, wins, states


def _replay(cfg, opp, ms, wins, states, tag):
    census = wd.new_census()
    for w in range(WINDOWS):
        tr = {k: wins[w][k].numpy() for k in ("obs", "mask", "player", "action", "reward", "done", "entropy")}
        tr["value"], tr["logp"] = wins[w]["value"].numpy().reshape(T, N), wins[w]["log_prob"].numpy()
        last = wd.replay(ms, opp, tr, T, census, tag + (w,))
        s = states[w]
        wd.check_state(ms, last, s["rec"], s["mt"], s["pos"], s["episodes"], s["stuck"], s["stat"], s["status"], tag + (w,))
    wd.assert_census(census, cfg, opp, tag)


def _same(a, b, keys, tag):
    """Two runs (wins, states) bit for bit; opp_action / opp_logp where a step's replies filled the slot."""
    (wa, sa), (wb, sb) = a, b
    for w in range(WINDOWS):
        for k in keys:
            _eq(wa[w][k], wb[w][k], tag + (w, k))
        if "opp_replies" in wa[w]:
            _eq(wa[w]["opp_replies"], wb[w]["opp_replies"], tag + (w, "opp_replies"))
            owed = torch.arange(R).view(1, R, 1) < wa[w]["opp_replies"].long().unsqueeze(1)
            for k in ("opp_action", "opp_logp"):
                _eq(wa[w][k][owed], wb[w][k][owed], tag + (w, k))
        for k in sa[w]:
            assert np.array_equal(sa[w][k], sb[w][k], equal_nan=sa[w][k].dtype == np.float64), tag + (w, k)


# ---- (a) the policy on every seat / RandomAgent seats ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opponent", [None, "random"])
@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_two_player_window_kernel_from_domain_records(cfg, opponent):
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    runs = {}
    for persistent in (False, True):
        ro = PolicyRollout(_two_net(), n_games=N, rules=TWO_RULES[cfg[2]], seed_base=4242, window=T, use_graph=False, opponent=opponent,
                           persistent=persistent)
        assert ro.persistent == persistent and not ro.wide
        runs[persistent] = _play(cfg, ro)
    tag = (dr.config_id(cfg), opponent)
    ms, wins, states = runs[True]
    _replay(cfg, int(opponent is not None), ms, wins, states, tag)
    _same(runs[False][1:], runs[True][1:], TRAJ, tag)


@pytest.mark.parametrize("opponent", [None, "random"])
@pytest.mark.parametrize("shape", range(5), ids=SHAPE_IDS)
def test_wide_window_kernel_from_domain_records(shape, opponent):
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    players, rules = SHAPES[shape]
    cfg = _shape_cfg(shape)
    policy = _dyadic_policy(players, rules, 100 + shape).cuda()
    runs = {}
    for fused in (False, True):
        ro = PolicyRollout(policy, n_games=N, rules=rules, seed_base=11, window=T, opponent=opponent, players=players, fused_wide=fused,
                           sample_seed=0x1234, use_graph=False)
        assert ro.wide and ro.fused_wide == fused and (ro.window_entry is not None) == fused
        runs[fused] = _play(cfg, ro)
    tag = (SHAPE_IDS[shape], opponent)
    ms, wins, states = runs[True]
    for w in range(WINDOWS):
        _assert_exact(policy, wins[w]["obs"])
    _replay(cfg, int(opponent is not None), ms, wins, states, tag)
    _same(runs[False][1:], runs[True][1:], TRAJ, tag)


# ---- (b) the opponents inside the window kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["net", "greedy_margin"])
@pytest.mark.parametrize("shape", [1, 4], ids=[SHAPE_IDS[1], SHAPE_IDS[4]])
def test_wide_opponents_inside_the_window_kernel_from_domain_records(shape, kind):
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    players, rules = SHAPES[shape]
    cfg = _shape_cfg(shape)
    policy = _dyadic_policy(players, rules, 200 + shape).cuda()
    opponent = _dyadic_policy(players, rules, 300 + shape).cuda() if kind == "net" else "greedy_margin"
    switch = {"fused_opponent": True} if kind == "net" else {"fused_seats": True}
    runs = {}
    for fused in (False, True):
        ro = PolicyRollout(policy, n_games=N, rules=rules, seed_base=11, window=T, opponent=opponent, players=players, opponent_trace=R,
                           sample_seed=0x1234, use_graph=False, **(dict(switch, fused_wide=True) if fused else {}))
        assert ro.cut and (ro.window_entry is not None) == fused and ro.opp_slots == R
        runs[fused] = _play(cfg, ro)
    for w in range(WINDOWS):
        _assert_exact(policy, runs[True][1][w]["obs"])
        if kind == "net":
            _assert_exact(opponent, runs[True][1][w]["obs"])
    _same(runs[False][1:], runs[True][1:], TRAJ, (SHAPE_IDS[shape], kind))
    assert sum(int(w["opp_replies"].sum()) for w in runs[True][1]) > N * T      # the opponents really moved


@pytest.mark.parametrize("cfg", dr.TWO_CONFIGS, ids=dr.config_id)
def test_greedy_opponent_inside_the_two_player_window_kernel_from_domain_records(cfg):
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    runs = {}
    for fused in (False, True):
        ro = PolicyRollout(_two_net(), n_games=N, rules=TWO_RULES[cfg[2]], seed_base=4242, window=T, opponent="greedy", opponent_trace=R,
                           fused_opponent=fused)
        assert ro.cut and ro.persistent == fused and ro.opp_slots == R
        runs[fused] = _play(cfg, ro)
    _same(runs[False][1:], runs[True][1:], TRAJ, (dr.config_id(cfg), "greedy"))
    assert sum(int(w["opp_replies"].sum()) for w in runs[True][1]) > N * T // 2
