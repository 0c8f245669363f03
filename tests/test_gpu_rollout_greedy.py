"""The greedy opponent inside the two-player window kernel on the MI355X (azul_batch_policy_rollout_greedy, azul_policy_rollout2_kernel<LID, 3>;
PolicyRollout / BatchedTrainer(opponent="greedy", fused_opponent=True)) against the per-cut path (azul_batch_score_moves +
azul_batch_net_step_*), bit for bit: every trajectory array, the returns, the opponent's trace, the status, the records, the MT19937
states, the counters and the Philox step counter -- at one game (a wave whose upper half holds no game), one whole workgroup and a ragged
second one, with windows of 1, 8 and 33 steps (33 leaves the in-register returns scan); the edges play must reach (a step without a
reply, forced moves, siblings of a wave that owe different numbers of replies, an episode end whose next episode the opponent opens, more
replies than trace slots, a greedy tie), found in the oracle alone with a policy a host can predict (tests/greedy_rollout_cases.py);
handed-in states (nobody can move; one move before the end of the game); the move limit; the fused path alone replayed through the oracle
with the host model's greedy choice (tests/score_moves_model.py); sharding; the trajectory ring; the C ABI's refusals; the trainer and its
checkpoint.  The CPU suite runs the same kernel under the lockstep emulation (tests/test_hostcheck_rollout_greedy.py).

opp_action is compared where a step's replies filled the slot: the per-cut path copies the whole answer vector of a reply round into the
slot, so a slot a game did not fill holds that game's older answer there, while the window kernel leaves it as it was."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import greedy_rollout_cases as gc
from tests import score_moves_model as sm
from tests import training_ring_cases as rc

pytestmark = pytest.mark.gpu
CANARY = 0x5EED5EED
KEYS = ("obs", "mask", "player", "action", "reward", "done", "value", "log_prob", "entropy", "returns", "opp_replies")


def _random_net():
    from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
    torch.manual_seed(3)
    return BatchedActorCritic(136, 180, 180)


def _play(fused, n, T, windows, net=_random_net, trace=4, prepare=None, **kw):
    """One rollout against the greedy opponent: `windows` windows of part 0 as numpy copies, and everything else the two paths must agree on."""
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    ro = PolicyRollout(net(), n_games=n, window=T, opponent="greedy", opponent_trace=trace, fused_opponent=fused, **kw)
    assert ro.opponent == "greedy" and ro.cut and ro.persistent == fused and not ro.use_graph and ro.ring == 1 and ro.opp_slots == trace
    env = ro.envs[0]
    if prepare is not None:
        prepare(ro)
    start, (mt0, pos0) = env.get_records(), env.get_rng_range()
    wins = []
    for _ in range(windows):
        tr = ro.run_window()
        ro.synchronize()
        wins.append({k: v.cpu().numpy().copy() for k, v in tr[0].items()})
    mt, pos = env.get_rng_range()
    c = env.counters()
    return {"ro": ro, "wins": wins, "start": start, "mt0": mt0, "pos0": pos0, "records": env.get_records(), "mt": mt, "pos": pos,
            "counters": (c["episodes"].tobytes(), c["stuck"].tobytes(), c["stat_sums"].tobytes()), "status": ro.work[0]["status"].cpu().numpy().copy(),
            "philox": ro.work[0]["counter"].tolist()}


def _assert_same(a, b, trace):
    """The per-cut run `a` and the fused run `b`: torch.equal / byte equality throughout."""
    assert len(a["wins"]) == len(b["wins"])
    held = np.full_like(b["wins"][0]["opp_action"], -1)    # (ring 1: every window is written into the same buffer, filled with -1 at first)
    for wi, (wa, wb) in enumerate(zip(a["wins"], b["wins"])):
        for key in KEYS:
            assert wa[key].dtype == wb[key].dtype and wa[key].tobytes() == wb[key].tobytes(), (wi, key)
        rep = wa["opp_replies"].astype(int)
        valid = np.arange(trace)[None, :, None] < rep[:, None, :]               # [T][R][N]: slot j of a step holds a reply
        assert np.array_equal(wa["opp_action"][valid], wb["opp_action"][valid]), wi
        assert np.array_equal(wb["opp_action"][~valid], held[~valid]), wi      # the kernel writes the slots a step's replies fill, no other
        held = wb["opp_action"]
        assert (wa["opp_logp"] == 0).all() and (wb["opp_logp"] == 0).all(), wi
    assert a["records"].tobytes() == b["records"].tobytes()
    assert np.array_equal(a["mt"], b["mt"]) and np.array_equal(a["pos"], b["pos"])
    assert a["counters"] == b["counters"] and np.array_equal(a["status"], b["status"]) and a["philox"] == b["philox"]


def _cat(run, key):
    return np.concatenate([w[key] for w in run["wins"]])


@pytest.mark.parametrize("T,windows", [(1, 40), (8, 5), (33, 2)])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_fused_equals_the_per_cut_path_bit_for_bit(n, T, windows):
    kw = dict(seed_base=900, sample_seed=0xBEEF)
    a, b = _play(False, n, T, windows, **kw), _play(True, n, T, windows, **kw)
    _assert_same(a, b, 4)
    done = _cat(b, "done")
    assert (done != 0).any(axis=0).sum() * 2 >= n          # most games finished an episode
    assert _cat(b, "opp_replies").sum() >= T * windows * n // 2


def test_play_reaches_the_edges_and_both_paths_agree_there():
    """The policy a host can predict (tests/greedy_rollout_cases.py) from seed_base 900: found in the oracle alone, 17 games x 40 steps
    hold every class below.  Asserted on the compared data itself, and the data against the oracle's play."""
    n, T, windows = 17, 8, 5
    kw = dict(net=gc.priority_policy, seed_base=900, action_selection="Max")
    a, b = _play(False, n, T, windows, **kw), _play(True, n, T, windows, **kw)
    _assert_same(a, b, 4)
    rep, done, act = _cat(b, "opp_replies").astype(int), _cat(b, "done"), _cat(b, "action")
    first, pool = gc.RULESETS["lid_randomfirst"][1:]
    sims = [gc.simulate(900 + g, first, pool, T * windows) for g in range(n)]
    assert np.array_equal(act, np.array([[r["action"] for r in s] for s in sims]).T)
    assert np.array_equal(rep, np.array([[r["replies"] for r in s] for s in sims]).T)
    assert (rep == 0).any(), "no step without a reply"
    assert (rep >= 3).any(), "no step with forced moves of player 1"
    assert (rep[:, 0:16:2] != rep[:, 1:16:2]).any(), "no pair of sibling games with different reply counts"
    opened = np.array([[bool(r["done"]) and r["opening"] >= 1 for r in s] for s in sims]).T
    inside = np.ones_like(opened)
    inside[T - 1::T] = False                                # not the window's last step: the next episode opens inside the window
    assert (opened & inside & (done != 0)).any(), "no episode end inside a window whose next episode the opponent opens"
    # a greedy tie resolved to the lowest action: score_moves on the state before the reply shows it
    from azul_deep_reinforcement_learning_amd import BatchedAzul, _lib as L
    t, g = [(t, g) for g in range(n) for t in range(T) if sims[g][t]["ties"][:1] == [True]][0]
    log = _oracle_to_first_reply(900 + g, first, pool, [r["action"] for r in sims[g][:t + 1]])
    env = BatchedAzul(1, rules=gc.RULESETS["lid_randomfirst"][0], device="cuda", seed=1)
    env.set_records(np.ascontiguousarray(log["rec"]).view(env.record_dtype).reshape(-1))
    scores, best = env.score_moves(L.PERSP_CURRENT)
    scores = scores.cpu().numpy()[0].astype(np.int64)
    top = np.flatnonzero(scores == scores.max())
    assert len(top) >= 2 and int(best[0]) == int(top[0]) == int(b["wins"][0]["opp_action"][t, 0, g]), (t, g, top)
    # more replies than trace slots: played, counted, not recorded
    a1, b1 = _play(False, n, T, 2, trace=1, **kw), _play(True, n, T, 2, trace=1, **kw)
    _assert_same(a1, b1, 1)
    assert (_cat(b1, "opp_replies") > 1).any()
    for key in KEYS:
        assert b1["wins"][0][key].tobytes() == b["wins"][0][key].tobytes(), key


def _oracle_to_first_reply(seed, first, pool, actions):
    """Play game `seed` in the oracle up to the LAST of `actions` and keep the record the opponent's first reply to it was asked on."""
    from oracle import oracle as oz
    log = {"rec": None, "arm": False}

    def opponent(s, m):
        if log["arm"] and log["rec"] is None:
            log["rec"] = np.frombuffer(oz.pack(run.q).tobytes(), np.uint8).copy()
        return sm.greedy_of_game(run.q.game)

    run = oz.NetRunner(opponent, first, pool, seed=seed)
    assert run.reset() == 0
    for i, a in enumerate(actions):
        log["arm"] = i == len(actions) - 1
        rcode, _, dn = run.step(a)
        assert rcode == 0
        if dn and not log["arm"]:
            assert run.reset() == 0
    assert log["rec"] is not None
    return log


def _hand_in(ro):
    """Game 0: one display of four tiles of one colour and the token in the centre -- after the agent's move only the token is left, nobody
    can move (hazard H3).  Game 1: the same without the token, player 2's first wall row one tile short and that tile on its first pattern
    line -- the agent's move ends the round and the game."""
    env = ro.envs[0]
    recs = env.get_records()
    for g, token in ((0, 1), (1, 0)):
        r = recs[g]
        r["displays"][:] = 0
        r["center"][:] = 0
        r["displays"][0][2] = 4
        r["center"][5] = token
        r["flags"] = (int(r["flags"]) & 0xF8) | 1
    recs[1]["walls"][1] = 0x0f
    recs[1]["pattern_lines"][1][0][:] = 0
    recs[1]["pattern_lines"][1][0][4] = 1
    env.set_records(recs)
    t = ro.traj[0]
    with torch.cuda.stream(ro.streams[0]):
        env.observe_all(ro._persp(), t["obs"][ro.T], t["mask"][ro.T], t["player"][ro.T])      # slot 0 of the first window
    ro.synchronize()


def test_handed_in_edge_states():
    a, b = _play(False, 4, 4, 2, prepare=_hand_in, seed_base=70), _play(True, 4, 4, 2, prepare=_hand_in, seed_base=70)
    _assert_same(a, b, 4)
    for run in (a, b):
        d0 = run["wins"][0]["done"][0]
        assert d0[0] == 2 and d0[1] == 1 and run["wins"][0]["reward"][0, 0] == 0
        assert run["wins"][0]["mask"][0, :2].sum(axis=1).tolist() == [6, 6]
    c = b["ro"].envs[0].counters()
    assert int(c["stuck"][0]) == 1 and int(c["episodes"][1]) >= 1


def test_move_limit():
    a, b = _play(False, 16, 8, 5, seed_base=300, move_limit=20), _play(True, 16, 8, 5, seed_base=300, move_limit=20)
    _assert_same(a, b, 4)
    assert (_cat(b, "done") == 3).any()


@pytest.mark.parametrize("ruleset", ["lid_randomfirst", "random_first1"])
def test_fused_rollout_replays_through_the_oracle(ruleset):
    rules, first, pool = gc.RULESETS[ruleset]
    T, n = 8, 6
    b = _play(True, n, T, 2, rules=rules, seed_base=900)
    calls = 0
    for g in range(n):
        run, c = gc.replay_windows(b["wins"], T, g, b["start"][g], b["mt0"][g], b["pos0"][g], first, pool)
        calls += c["calls"]
        assert run.record().tobytes() == b["records"][g].tobytes(), g
        m_e, idx = run.rng_state()
        assert int(b["pos"][g]) == idx and np.array_equal(b["mt"][g], m_e), g
    assert calls >= 2 * T * n // 2                         # the opponent really moved: about one reply per agent step


def test_sharding():
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    runs = []
    for parts in (1, 2):
        ro = PolicyRollout(_random_net(), n_games=18, parts=parts, window=8, opponent="greedy", opponent_trace=4, fused_opponent=True, seed_base=500)
        wins = []
        for _ in range(3):
            tr = ro.run_window()
            ro.synchronize()
            wins.append({k: np.concatenate([p[k].cpu().numpy() for p in tr], axis=2 if k in ("opp_action", "opp_logp") else 1) for k in tr[0]})
        runs.append((wins, ro.counters()))
    for wa, wb in zip(runs[0][0], runs[1][0]):
        for key in KEYS + ("opp_action", "opp_logp"):
            assert wa[key].tobytes() == wb[key].tobytes(), key
    assert runs[0][1] == runs[1][1]


def test_ring_returns_chain_through_the_windows():
    from azul_deep_reinforcement_learning_amd import PolicyRollout
    T, n, gamma = 8, 17, 0.99
    ro = PolicyRollout(_random_net(), n_games=n, window=T, opponent="greedy", fused_opponent=True, ring=2, seed_base=900)
    assert ro.persistent and ro.ring == 2
    one = PolicyRollout(_random_net(), n_games=n, window=T, opponent="greedy", fused_opponent=True, seed_base=900)
    R = 2 * T
    want = np.zeros((R, n), np.float32)
    reward, done = [], []
    for w in range(5):                                      # the ring wraps twice
        ro.run_window(gamma)
        tr1 = one.run_window(gamma)
        ro.synchronize()
        one.synchronize()
        rg = ro.rings[0]
        rr, dd = rg["reward"].cpu().numpy(), rg["done"].cpu().numpy()
        played = (w + 1) * T
        want = rc.returns_ring(rr, dd, want, gamma, R, played, min(R, played))
        rc.compare_returns("window %d" % w, rg["returns"].cpu().numpy(), want)
        # the ring holds the windows the plain rollout plays
        lo = (w % 2) * T
        assert np.array_equal(rr[lo:lo + T], tr1[0]["reward"].cpu().numpy()) and np.array_equal(dd[lo:lo + T], tr1[0]["done"].cpu().numpy())
        reward.append(rr[lo:lo + T].copy())
        done.append(dd[lo:lo + T].copy())
        if w >= 1:
            # q = r + gamma * q over the two newest windows, concatenated, within episodes
            two, _ = rc.returns_window(np.concatenate(reward[-2:]), np.concatenate(done[-2:]), gamma, None)
            got = np.concatenate([rg["returns"].cpu().numpy()[((w - 1) % 2) * T:][:T], rg["returns"].cpu().numpy()[lo:lo + T]])
            rc.compare_returns("two windows %d" % w, got, two)
    assert (np.concatenate(done) != 0).any()


def test_c_abi_refusals_before_any_launch():
    from azul_deep_reinforcement_learning_amd import BatchedAzul, _lib as L
    n, T = 4, 2
    dev = "cuda"
    wt = [torch.zeros(s, device=dev) for s in ((136, 360), (360,), (180,), (1,), (180, 180), (180,))]
    w = L.NetWeights(*[t.data_ptr() for t in wt])
    i32 = lambda *s: torch.full(s, CANARY, dtype=torch.int32, device=dev)
    u8 = lambda *s: torch.full(s, 0xA5, dtype=torch.uint8, device=dev)
    f32 = lambda *s: torch.full(s, 1234.5, device=dev)
    bufs = [f32(T + 1, n, 136), u8(T + 1, n, 180), u8(T + 1, n), i32(T, n), i32(T, n), u8(T, n), f32(T, n), f32(T, n), f32(T, n), u8(n), f32(T, n),
            i32(T, 2, n), f32(T, 2, n), u8(T, n)]
    out = L.RolloutBuffers(*[t.data_ptr() for t in bufs], 2)
    ctr = torch.zeros(2, dtype=torch.int64, device=dev)
    env = BatchedAzul(n, device=dev, seed=1)
    env.runner_init()
    wide = BatchedAzul(n, players=3, device=dev, seed=1)
    wide.init()
    before = (env.get_records().tobytes(), wide.get_records().tobytes())
    call = lambda h, hidden, o: L.lib.azul_batch_policy_rollout_greedy(h, T, C.byref(w), 136, hidden, 180, 1, 0, C.c_void_p(ctr.data_ptr()), o,
                                                                      C.c_float(0.9), None)
    assert call(wide._h, 180, C.byref(out)) == L.ERR_INVALID
    assert b"wide batch" in L.lib.azul_last_error_string() and b"azul_batch_policy_rollout_greedy" in L.lib.azul_last_error_string()
    assert call(env._h, 64, C.byref(out)) == L.ERR_INVALID
    assert b"(136, 180, hidden 180)" in L.lib.azul_last_error_string()
    assert call(env._h, 180, None) == L.ERR_INVALID
    assert L.lib.azul_batch_policy_rollout_greedy(env._h, T, None, 136, 180, 180, 1, 0, None, C.byref(out), C.c_float(0.9), None) == L.ERR_INVALID
    torch.cuda.synchronize()
    for t, v in zip(bufs, (1234.5, 0xA5, 0xA5, CANARY, CANARY, 0xA5, 1234.5, 1234.5, 1234.5, 0xA5, 1234.5, CANARY, 1234.5, 0xA5)):
        assert bool((t == v).all())
    assert ctr.tolist() == [0, 0] and (env.get_records().tobytes(), wide.get_records().tobytes()) == before
    # and the call these refuse goes through
    assert call(env._h, 180, C.byref(out)) == L.SUCCESS
    torch.cuda.synchronize()
    assert ctr.tolist() == [T, 0] and not bool((bufs[3] == CANARY).any())


def test_trainer_and_its_checkpoint(tmp_path):
    from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
    from azul_deep_reinforcement_learning_amd.training import AGENT_STAT_KEYS, BatchedTrainer
    kw = dict(opponent="greedy", fused_opponent=True, n_games=8, window=8, results_dir=str(tmp_path))
    torch.manual_seed(4)
    tr = BatchedTrainer(BatchedActorCritic(136, 180, 180), seed_base=11, **kw)
    assert tr.rollout.opponent == "greedy" and tr.rollout.persistent and tr.rollout.ring == 3 and not tr.rollout.use_graph
    rows = [tr.run_batch() for _ in range(2)]
    torch.cuda.synchronize()
    assert tr.learner.updates == 2
    for r in rows:
        assert all(np.isfinite(r[k]) for k in AGENT_STAT_KEYS[1:]), r
    ck = os.path.join(str(tmp_path), "greedy.pt")
    tr.save_checkpoint(ck)
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    assert saved["ring"] == 3 and "ring_buffers" in saved and "opponent" not in saved
    state = lambda t: ({k: v.detach().cpu().clone() for k, v in t.rollout.policy.state_dict().items()}, t.rollout.envs[0].get_records().tobytes(),
                       t.rollout.envs[0].get_rng_range(), t.rollout.work[0]["counter"].tolist(),
                       {k: v.cpu().clone() for k, v in t.rollout.traj[0].items()})
    row_a = tr.run_batch()                                  # the third batch of the uninterrupted run
    tr.rollout.synchronize()
    want = state(tr)
    torch.manual_seed(99)
    tr2 = BatchedTrainer(BatchedActorCritic(136, 180, 180), seed_base=9000, **kw)
    tr2.load_checkpoint(ck)
    row_b = tr2.run_batch()
    tr2.rollout.synchronize()
    got = state(tr2)
    assert tr2.batch == 3
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k
    assert want[1] == got[1] and np.array_equal(want[2][0], got[2][0]) and np.array_equal(want[2][1], got[2][1]) and want[3] == got[3]
    for k in want[4]:
        assert torch.equal(want[4][k], got[4][k]), k
    for k in AGENT_STAT_KEYS[1:]:
        assert row_a[k] == row_b[k], k
