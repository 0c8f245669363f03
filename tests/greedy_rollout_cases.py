"""TEST helper of the greedy opponent inside the window kernel (azul_policy_rollout2_kernel<LID, 3>): the replay of a recorded rollout
through the oracle's callback GameRunner (oz.NetRunner) with the host model's greedy choice (tests/score_moves_model.py: greedy_of_game)
as the opponent, and a policy whose decisions a host can predict -- all weights zero but actor_linear2.bias, a fixed priority per action,
with action_selection "Max": the agent plays the legal action of the highest priority, so the whole rollout (PolicyRollout's start
included: random.seed(seed_base + g), GameRunner(), reset() with the greedy opponent opening) can be played in the oracle alone and
searched there for the seeds at which play reaches an edge."""
import functools

import numpy as np

from oracle import oracle as oz
from tests import score_moves_model as sm

RULESETS = {"lid_randomfirst": ({"first_player": "Random", "tile_pool": "Lid"}, oz.FIRST_RANDOM, oz.POOL_LID),
            "random_first1": ({"first_player": 1, "tile_pool": "Random"}, 1, oz.POOL_RANDOM)}
ST_STUCK, ST_TRUNCATED = 3, 6                            # csrc/azul_common.hpp


def replay(rec0, mt0, pos0, first, pool, action, opp_action, opp_replies, obs, mask, player, reward, done, move_limit=0):
    """GameRunner(opponent=greedy) in the oracle, fed the recorded agent actions: every env-side record, the number of opponent moves per
    step and every TRACED answer (reply j < R of a step; later replies are played and not recorded) must equal the rollout's.
    -> (the runner after the last step, {"calls", "forced", "opening", "ties", "cuts"})."""
    S, R = len(action), opp_action.shape[1]
    cur = {"t": 0, "j": 0, "calls": 0, "forced": 0, "opening": 0, "ties": 0, "cuts": 0}

    def opponent(s, m):
        game = run.q.game
        a = sm.greedy_of_game(game)
        assert a >= 0 and m[a], ("greedy answer not legal", cur["t"], cur["j"], a)
        if cur["j"] < R:
            assert a == int(opp_action[cur["t"], cur["j"]]), ("traced opp_action", cur["t"], cur["j"], a, int(opp_action[cur["t"], cur["j"]]))
        assert np.array_equal(s, oz.get_state(game, game.current_player - 1))
        cur["j"] += 1
        cur["calls"] += 1
        cur["forced"] += int(game.current_player == 1)
        return a

    run = oz.NetRunner(opponent, first, pool, rec=rec0, mt=mt0, pos=pos0)
    for t in range(S):
        cur["t"], cur["j"] = t, 0
        m = run.get_valid_moves()
        assert np.array_equal(np.asarray(mask[t]).astype(bool), m), ("mask", t)
        assert np.array_equal(np.asarray(obs[t]).astype(np.int64), run.get_state(0)), ("obs", t)
        assert int(player[t]) == 1 == int(run.q.game.current_player) and int(m.sum()) >= 2, ("player", t)
        a = int(action[t])
        assert 0 <= a < 180 and m[a], ("agent action", t, a)
        rc, rew, dn = run.step(a, move_limit)
        assert rc == 0 and rew == int(reward[t]) and int(dn) == int(done[t]), ("reward / done", t, rew, int(reward[t]), dn, int(done[t]))
        cur["cuts"] += int(dn) == 3
        if dn:
            before = cur["j"]
            assert run.reset() == 0
            cur["opening"] += cur["j"] - before
        assert cur["j"] == int(opp_replies[t]), ("replies", t, cur["j"], int(opp_replies[t]))
    assert np.array_equal(np.asarray(mask[S]).astype(bool), run.get_valid_moves()) and np.array_equal(np.asarray(obs[S]).astype(np.int64), run.get_state(0))
    return run, cur


def replay_windows(wins, T, g, rec0, mt0, pos0, first, pool, move_limit=0):
    """replay() of game g over a list of recorded windows (dicts of numpy arrays, time-major, obs / mask / player with T + 1 slots)."""
    cat = lambda key, sl: np.concatenate([w[key][sl] for w in wins])
    slot = lambda key: np.concatenate([w[key][:T, g] for w in wins] + [wins[-1][key][T:T + 1, g]])
    return replay(rec0, mt0, pos0, first, pool, cat("action", (slice(None), g)), cat("opp_action", (slice(None), slice(None), g)),
                  cat("opp_replies", (slice(None), g)), slot("obs"), slot("mask"), slot("player"), cat("reward", (slice(None), g)),
                  cat("done", (slice(None), g)), move_limit)


# ---- the predictable policy ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def priorities(seed=5):
    """float32[180]: a fixed permutation of 0 .. 179 -- the logits of the predictable policy on every observation."""
    return np.random.RandomState(seed).permutation(180).astype(np.float32)


def priority_policy(seed=5):
    """BatchedActorCritic(136, 180, 180) with every weight zero and actor_linear2.bias = priorities(): hidden = relu(0) = 0, logits = the
    bias exactly, value = 0; with action_selection "Max" the agent plays the legal action of the highest priority."""
    import torch
    from azul_deep_reinforcement_learning_amd.policy import BatchedActorCritic
    net = BatchedActorCritic(136, 180, 180)
    with torch.no_grad():
        for p in net.parameters():
            p.zero_()
        net.actor_linear2.bias.copy_(torch.from_numpy(priorities(seed)))
    return net


def simulate(seed, first, pool, steps, prio=None, move_limit=0):
    """Game `seed` of PolicyRollout(priority_policy(), opponent="greedy", action_selection="Max", seed_base=seed) in the oracle alone.
    -> per agent step: action, replies (opponent moves inside the step, the next episode's openings included), opening (of those, the
    openings), opp (the answers in order), ties (bool per answer: several moves shared the maximum), done."""
    prio = priorities() if prio is None else prio
    log = {"opp": [], "ties": []}

    def opponent(s, m):
        game = run.q.game
        a = sm.greedy_of_game(game)
        tab = sm.table(oz.pack(run.q), sm.PERSP_CURRENT, pool)
        log["opp"].append(a)
        log["ties"].append(int((tab == tab.max()).sum()) >= 2)
        return a

    run = oz.NetRunner(opponent, first, pool, seed=seed)
    assert run.reset() == 0
    rows = []
    for t in range(steps):
        m = run.get_valid_moves()
        a = int(np.argmax(np.where(m, prio, -1.0)))
        log["opp"], log["ties"] = [], []
        rc, rew, dn = run.step(a, move_limit)
        assert rc == 0
        inside = len(log["opp"])
        if dn:
            assert run.reset() == 0
        rows.append({"action": a, "replies": len(log["opp"]), "opening": len(log["opp"]) - inside, "opp": list(log["opp"]),
                     "ties": list(log["ties"]), "reward": rew, "done": int(dn)})
    return rows
