"""GPU: the league -- a pool of network opponents inside the window kernels (PolicyRollout(opponent=[net0, net1, ...]),
azul_batch_policy_rollout_league / azul_batch_mp_policy_rollout_league, azul_league_tally) and BatchedTrainer(opponent="league").

A game's trajectory is keyed by its global id (its Philox draws, its MT19937 stream), so the games of a 16-game group assigned to member m must
play exactly what they play in a rollout against member m alone: the league is compared BIT FOR BIT, group by group, with the single-opponent
rollouts, and the league's window kernel with the league on the per-cut path (two-player: any weights, the library's forward is the kernel's
arithmetic; wide: the dyadic exact-sum policies of tests/test_gpu_mp_fused_rollout.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from azul_deep_reinforcement_learning_amd import _lib as L
from azul_deep_reinforcement_learning_amd.batch import BatchedAzul, parse_ext_rules
from azul_deep_reinforcement_learning_amd.multiplayer import MultiplayerAzul
from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
from azul_deep_reinforcement_learning_amd.records import STAT_KEYS
from azul_deep_reinforcement_learning_amd.rollout import PolicyRollout
from tests.test_gpu_mp_fused_rollout import SHAPES, _assert_exact, _dims, _dyadic_policy, _eq, _state, _traj

pytestmark = pytest.mark.gpu

GROUP = 16
R = 6                          # opponent trace slots
GAME_AXIS = {"opp_action": 2, "opp_logp": 2}       # the game axis of a trajectory array (the others: axis 1)
RULES2 = {"first_player": "Random", "tile_pool": "Lid"}


def _net2(seed):
    torch.manual_seed(seed)
    return BatchedActorCritic().cuda()


def _wide(players, rules):
    """A batch of wide records (three / four players, or two under extended rules): its window kernels have their own switches."""
    return players != 2 or parse_ext_rules(rules, players) != 0


def _rollout(policy, opponent, n, T, players=2, rules=RULES2, kernel=True, selection="Distribution", **kw):
    sw = dict(fused_wide=kernel, fused_opponent=kernel) if _wide(players, rules) else dict(persistent=kernel)
    return PolicyRollout(policy, n_games=n, rules=rules, seed_base=11, window=T, opponent=opponent, players=players, opponent_trace=R,
                         action_selection=selection, opponent_selection=selection, sample_seed=0x1234, use_graph=False, **sw, **kw)


def _play(ro, windows, between=None):
    trajs = []
    for w in range(windows):
        ro.run_window(gamma=0.99)
        ro.synchronize()
        trajs.append(_traj(ro)[0])
        if between is not None and w + 1 < windows:
            between(ro, w)
    torch.cuda.synchronize()
    return trajs, _state(ro)


def _owed(tr):
    j = torch.arange(R).view(1, R, 1)
    return j < tr["opp_replies"].long().unsqueeze(1)


def _eq_games(a, b, idx, what, trace_owed_only=False):
    """Trajectory dicts a, b agree bit for bit on the games `idx` (a per-cut path's trace also holds answers of rounds a game did not owe)."""
    ix = torch.as_tensor(idx)
    for k in a:
        x, y = a[k].index_select(GAME_AXIS.get(k, 1), ix), b[k].index_select(GAME_AXIS.get(k, 1), ix)
        if trace_owed_only and k in ("opp_action", "opp_logp"):
            owed = _owed(a).index_select(2, ix)
            x, y = x[owed], y[owed]
        _eq(x, y, "%s: %s" % (what, k))


def _eq_state(sa, sb, idx, what):
    for k in sa:
        _eq(sa[k][0][idx], sb[k][0][idx], "%s: %s" % (what, k))


def _groups(n, members):
    return [(m, np.arange(g * GROUP, min(n, (g + 1) * GROUP))) for g, m in enumerate(members)]


# ---- 6. two-player: the league against the single-opponent rollouts, and kernel against per-cut -----------------------------------------
def test_two_player_league_equals_single_opponent_rollouts_per_group_and_the_per_cut_path():
    n, T, W = 48, 8, 2
    policy, a, b = _net2(1), _net2(2), _net2(3)
    ro = _rollout(policy, [a, b], n, T)
    assert ro.window_entry == "azul_batch_policy_rollout_league" and ro.pool_size == 2
    assert ro.assignment().tolist() == [[0, 1, 0]]                       # the default: group i -> member i % K
    lg, slg = _play(ro, W)
    singles = [_play(_rollout(policy, m, n, T), W) for m in (a, b)]
    for m, idx in _groups(n, [0, 1, 0]):
        for w in range(W):                                               # (slot 0 of window 0 holds the openings played at construction)
            _eq_games(lg[w], singles[m][0][w], idx, "member %d window %d" % (m, w))
        _eq_state(slg, singles[m][1], idx, "member %d" % m)
    assert not torch.equal(singles[0][0][0]["opp_action"], singles[1][0][0]["opp_action"])       # the members do answer differently
    assert int(lg[0]["opp_replies"].sum()) > n * T // 2
    cut = _rollout(policy, [a, b], n, T, kernel=False)
    assert cut.window_entry is None and cut.league
    pc, spc = _play(cut, W)
    for w in range(W):
        _eq_games(pc[w], lg[w], np.arange(n), "per-cut window %d" % w, trace_owed_only=True)
    _eq_state(spc, slg, np.arange(n), "per-cut")


# ---- 7. reassignment and the results --------------------------------------------------------------------------------------------------
def test_reassignment_between_windows_and_league_results_equal_a_host_recount():
    n, T, W = 48, 32, 2                                                  # 64 agent steps: episodes end in both windows
    policy, a, b = _net2(4), _net2(5), _net2(6)
    first, second = np.array([[0, 1, 0]]), np.array([[1, 0, 1]])
    snaps = []

    def swap(ro, w):
        snaps.append(ro.envs[0].counters())
        ro.set_assignment(second)

    ro, cut = _rollout(policy, [a, b], n, T), _rollout(policy, [a, b], n, T, kernel=False)
    with pytest.raises(ValueError, match="pool members 0..1"):
        ro.set_assignment(np.array([[0, 2, 0]]))                        # refused on the host
    with pytest.raises(ValueError, match="shape"):
        ro.set_assignment(np.array([0, 1, 0]))
    lg, slg = _play(ro, W, swap)
    assert ro.assignment().tolist() == second.tolist()
    pc, spc = _play(cut, W, lambda r, w: r.set_assignment(second))
    for w in range(W):
        _eq_games(pc[w], lg[w], np.arange(n), "window %d" % w, trace_owed_only=True)
    _eq_state(spc, slg, np.arange(n), "state")
    # after the swap group 0 plays member 1: its second window equals a single-opponent rollout's only if that rollout swaps too -- instead
    # the results: episodes from the done flags, statistic sums from the per-game counters, booked to the member of the window they ended in
    # (the sums in the tally's order -- per member the games ascending, counter - mark -- since percent_first_player is not a whole number)
    c1, c2 = snaps[0], ro.envs[0].counters()
    zero = {"episodes": np.zeros(n, np.uint64), "stat_sums": np.zeros((n, 10))}
    want_ep, want_ss = np.zeros(2, np.int64), np.zeros((2, 10))
    for assign, tr, lo, hi in ((first[0], lg[0], zero, c1), (second[0], lg[1], c1, c2)):
        for m, idx in sorted(_groups(n, assign), key=lambda x: x[0]):
            done = int((tr["done"][:, idx] == 1).sum())
            assert done == int((hi["episodes"][idx] - lo["episodes"][idx]).sum())            # the counters and the done flags agree
            want_ep[m] += done
            for g in idx:
                want_ss[m] = want_ss[m] + (hi["stat_sums"][g] - lo["stat_sums"][g])
    assert want_ep.min() > 0                                             # both members finished episodes
    for results in (ro.league_results(), cut.league_results(), ro.league_results(reset=True)):      # (a second read adds nothing)
        for m in range(2):
            assert results[m]["episodes"] == int(want_ep[m])
            for i, k in enumerate(STAT_KEYS):
                assert results[m][k] == want_ss[m, i] / want_ep[m], (m, k)
            assert 0.0 <= results[m]["win_percent"] <= 1.0
    assert [r["episodes"] for r in ro.league_results()] == [0, 0]        # reset=True zeroed them
    assert int(c2["episodes"].sum()) == int(want_ep.sum())


# ---- 8. wide: 3 players on 5 displays ---------------------------------------------------------------------------------------------------
def test_wide_league_equals_single_opponent_rollouts_per_group_general_weights():
    players, rules = SHAPES[1]
    n_obs, n_act = _dims(players, rules)
    n, T, W = 32, 8, 2
    torch.manual_seed(8)
    policy, a, b = (BatchedActorCritic(n_obs, n_act, 180).cuda() for _ in range(3))
    ro = _rollout(policy, [a, b], n, T, players, rules)
    assert ro.window_entry == "azul_batch_mp_policy_rollout_league" and ro.assignment().tolist() == [[0, 1]]
    lg, slg = _play(ro, W)
    singles = []
    for m in (a, b):
        single = _rollout(policy, m, n, T, players, rules)
        assert single.window_entry == "azul_batch_mp_policy_rollout_vs"
        singles.append(_play(single, W))
    for m, idx in _groups(n, [0, 1]):                                    # (the openings at construction included: slot 0 of window 0)
        for w in range(W):
            _eq_games(lg[w], singles[m][0][w], idx, "member %d window %d" % (m, w))
        _eq_state(slg, singles[m][1], idx, "member %d" % m)
    assert not torch.equal(singles[0][0][0]["opp_action"], singles[1][0][0]["opp_action"])       # the members do answer differently
    assert int(lg[0]["opp_replies"].sum()) > n * T // 2


def test_wide_league_kernel_equals_the_per_cut_path_with_exact_sums():
    players, rules = SHAPES[1]
    n, T, W = 32, 8, 2
    policy = _dyadic_policy(players, rules, 500).cuda()
    pool = [_dyadic_policy(players, rules, 501 + i).cuda() for i in range(2)]
    swap = lambda r, w: r.set_assignment(np.array([[1, 1]]))
    lg, slg = _play(_rollout(policy, pool, n, T, players, rules), W, swap)
    cut = _rollout(policy, pool, n, T, players, rules, kernel=False)
    assert cut.window_entry is None and cut.league and cut.wide
    pc, spc = _play(cut, W, swap)
    for w in range(W):
        _assert_exact(policy, pc[w]["obs"])
        for m in pool:
            _assert_exact(m, pc[w]["obs"])
        _eq_games(pc[w], lg[w], np.arange(n), "window %d" % w, trace_owed_only=True)
    _eq_state(spc, slg, np.arange(n), "state")
    assert int(lg[0]["opp_replies"].sum()) > n * T // 2


# ---- 9. the trainer ---------------------------------------------------------------------------------------------------------------------
def _trainer(tmp_path, sampling="uniform"):
    from azul_deep_reinforcement_learning_amd.training import BatchedTrainer
    torch.manual_seed(21)
    return BatchedTrainer(BatchedActorCritic(), n_games=128, window=16, device="cuda:0", opponent="league", league_size=3, opponent_refresh=2,
                          league_sampling=sampling, results_dir=str(tmp_path))


def _pool(tr):
    torch.cuda.synchronize()
    return {k: getattr(tr.rollout, "o" + k).detach().cpu().clone() for k in PolicyRollout._OPP_ARRAYS}


def _trainer_state(tr):
    torch.cuda.synchronize()
    return {"policy": {k: v.detach().cpu().clone() for k, v in tr.rollout.policy.state_dict().items()}, "pool": _pool(tr),
            "assignment": tr.rollout.assignment(), "results": tr.rollout.league_results(), "counts": (tr.snapshots, tr.redraws)}


def _same_state(a, b):
    for k in a["policy"]:
        _eq(a["policy"][k], b["policy"][k], "policy " + k)
    for k in a["pool"]:
        _eq(a["pool"][k], b["pool"][k], "pool " + k)
    assert np.array_equal(a["assignment"], b["assignment"]) and a["counts"] == b["counts"]
    assert repr(a["results"]) == repr(b["results"])                      # (NaN means of a member without episodes compare equal as text)


def test_trainer_league_refresh_writes_one_slot_and_a_resumed_run_equals_the_uninterrupted_one(tmp_path):
    tr = _trainer(tmp_path)
    ro = tr.rollout
    assert ro.league and ro.pool_size == 3 and ro.window_entry == "azul_batch_policy_rollout_league"
    start = _pool(tr)
    for k in start:                                                      # K copies of the initial policy
        assert all(torch.equal(start[k][0], start[k][m]) for m in (1, 2)), k
    before = start
    for batch in range(1, 5):
        tr.run_batch()
        now = _pool(tr)
        if batch % 2 == 0:
            slot = (batch // 2 - 1) % 3
            want = dict(ro._kmajor(ro.policy.state_dict().__getitem__, PolicyRollout._OPP_ARRAYS))
            for k in now:
                _eq(now[k][slot], want[k].cpu(), "refresh %d: slot %d %s" % (batch, slot, k))
                assert not torch.equal(now[k][slot], before[k][slot]) or k == "b2c", k      # (the policy has moved)
                for m in set(range(3)) - {slot}:
                    _eq(now[k][m], before[k][m], "refresh %d: slot %d untouched %s" % (batch, m, k))
            assert tr.snapshots == tr.redraws == batch // 2
            counts = np.bincount(ro.assignment()[0], minlength=3)
            assert counts.sum() == 128 // GROUP and counts.max() - counts.min() <= 1       # uniform by largest remainder
        else:
            for k in now:
                _eq(now[k], before[k], "batch %d: pool %s" % (batch, k))
        before = now
    whole = _trainer_state(tr)
    half = _trainer(tmp_path)
    for _ in range(2):
        half.run_batch()
    path = str(tmp_path / "league.pt")
    half.save_checkpoint(path)
    resumed = _trainer(tmp_path)
    resumed.load_checkpoint(path)
    for _ in range(2):
        resumed.run_batch()
    _same_state(whole, _trainer_state(resumed))


def test_trainer_pfsp_is_deterministic_across_constructions(tmp_path):
    states = []
    for _ in range(2):
        tr = _trainer(tmp_path, "pfsp")
        for _ in range(4):
            tr.run_batch()
        states.append(_trainer_state(tr))
    _same_state(states[0], states[1])
    assert states[0]["counts"] == (2, 2)


# ---- 10. the ABI's refusals on a live batch -----------------------------------------------------------------------------------------------
def test_league_entries_refuse_bad_pools_and_the_wrong_batch_family():
    two, wide = BatchedAzul(16, device="cuda:0"), MultiplayerAzul(16, device="cuda:0", players=3)
    one, f32 = C.c_void_p(256), C.c_float
    wts, bufs = L.NetWeights(*[one] * 6), L.RolloutBuffers(*[one] * 14, 0)
    wr, br = C.byref(wts), C.byref(bufs)
    flat = lambda b, K, mem: L.lib.azul_batch_policy_rollout_league(b._h, 4, wr, wr, K, mem, 136, 180, 180, 1, 2, 0, None, br, f32(0.9), None)
    mp = lambda b, K, mem: L.lib.azul_batch_mp_policy_rollout_league(b._h, 4, wr, wr, K, mem, 188, 180, 180, 1, 2, 0, None, 8, br, f32(0.9), None)
    for call, batch, name in ((flat, two, "azul_batch_policy_rollout_league"), (mp, wide, "azul_batch_mp_policy_rollout_league")):
        for K, mem, said in ((0, one, "pool_size"), (256, one, "pool_size"), (2, None, "member_dev")):
            assert call(batch, K, mem) == L.ERR_INVALID
            msg = L.lib.azul_last_error_string().decode()
            assert msg.startswith(name) and said in msg, msg
    assert flat(wide, 2, one) == L.ERR_INVALID                           # a wide batch handed to the two-player entry
    assert L.lib.azul_last_error_string().decode().startswith("azul_batch_policy_rollout_league")
    assert mp(two, 2, one) == L.ERR_INVALID                              # ... and the reverse: the message names the twin
    msg = L.lib.azul_last_error_string().decode()
    assert msg.startswith("azul_batch_mp_policy_rollout_league") and "use azul_batch_policy_rollout_league" in msg
    assert L.lib.azul_batch_policy_rollout_league(two._h, 4, wr, None, 2, one, 136, 180, 180, 1, 2, 0, None, br, f32(0.9), None) == L.ERR_INVALID
    torch.cuda.synchronize()                                             # nothing was launched: nothing to fault
