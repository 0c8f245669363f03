"""Batched ``NNRunner.train`` (azulnet/nn_runner.py:49-84) with the on-disk surface either side of the path (row N3):
the CSV training log the reference intends to write, checkpoints, and resumable runs.

One "batch" of the reference is `batch_size` sequential episodes followed by one `Agent.update`; here it is one rollout
window of `window` agent steps for all `n_games` concurrent games (policy vs the RandomAgent opponent inside the env
step) followed by one `A2CLearner.update`: with the default ring of three windows every step of every episode is trained exactly
once, when its episode ends (A2CLearner.update_from_rollout; the reference trains on whole episodes, nn_runner.py:59-76).

CSV (nn_runner.py:51-54, 79-82): header ``batch`` + the five agent statistics keys (agent.py:13) + the ten game statistics
keys (game_runner.py:12); one row per logged batch with the batch's means.  The reference's own writer dereferences
``self.game_statistics``, which NNRunner does not have (it lives on the GameRunner), so that branch raises as soon as a
net name is given; the columns and their order here are the ones that code spells out.
  reward       mean over the batch of the per-episode reward sum (nn_runner.py:63) -- here: the window's total shaped
               reward / episodes finished in the window
  *_loss       the update's loss terms (agent.py:51-57)
  game keys    means over the episodes finished in the window of Azul.get_statistics (azul.py:314-315), accumulated on
               the device by the env step (win_percent etc. are per-episode 0/1 or counts, like the reference's buffers)

Checkpoints (`save_checkpoint` / `load_checkpoint`): the policy's state_dict (the reference's parameter names: loads into
`azulnet.model.ActorCritic` as is), the Adam state, every game's 128-byte record and CPython RNG state, the Philox step
counters, the batch index and (by default) the trajectory ring with the learner's selection books -- a restored run replays the
next window bit for bit and performs the same updates as the uninterrupted run.
"""
import csv
import os

import numpy as np
import torch

from .learner import A2CLearner, PPOLearner, complete_episode_samples
from .records import STAT_KEYS
from .rollout import PolicyRollout

AGENT_STAT_KEYS = ("reward", "actor_loss", "critic_loss", "entropy_loss", "ac_loss")          # agent.py:13


# ---- the league's sampler: host functions of a few numbers per pool member (BatchedTrainer(opponent="league")) ------------------------
def league_probabilities(episodes, win_rate, sampling="uniform", power=2.0):
    """The probability with which a 16-game group is given each pool member.  "uniform": 1 / K each.  "pfsp" (prioritised fictitious
    self-play): proportional to (1 - win_rate_m) ** power, the learner's win rate against member m over the `episodes[m]` episodes finished
    against it -- the members it still loses to are played more; a member without episodes counts as win rate 0.5; weights that are all
    zero (every member beaten every time) fall back to uniform."""
    ep = np.asarray(episodes, dtype=np.float64)
    K = ep.size
    if K < 1:
        raise ValueError("a league has at least one member")
    if sampling not in ("uniform", "pfsp"):
        raise ValueError("league_sampling must be \"uniform\" or \"pfsp\", got %r" % (sampling,))
    if sampling == "uniform":
        return np.full(K, 1.0 / K)
    wr = np.asarray(win_rate, dtype=np.float64)
    wr = np.clip(np.where((ep > 0) & np.isfinite(wr), wr, 0.5), 0.0, 1.0)
    w = (1.0 - wr) ** float(power)
    return w / w.sum() if w.sum() > 0.0 else np.full(K, 1.0 / K)


def league_group_counts(probabilities, groups):
    """How many of `groups` groups each member gets: the largest-remainder apportionment of the probabilities (floor of the quotas, the
    groups left over to the largest fractional parts, ties to the lower member).  A member of probability 0 gets none."""
    q = np.asarray(probabilities, dtype=np.float64) * int(groups)
    counts = np.floor(q).astype(np.int64)
    left = int(groups) - int(counts.sum())
    order = np.argsort(-(q - counts), kind="stable")
    counts[order[:left]] += 1
    return counts


def league_redraw(probabilities, groups, seed):
    """One part's assignment, uint8 [groups]: league_group_counts' members in an order drawn by a NumPy generator seeded with the tuple
    `seed` -- (sample_seed, redraw count, part) in the trainer: a pure function of the checkpointed state."""
    counts = league_group_counts(probabilities, groups)
    members = np.repeat(np.arange(counts.size, dtype=np.uint8), counts)
    return members[np.random.default_rng([int(x) for x in seed]).permutation(int(groups))]


class BatchedTrainer:
    def __init__(self, policy, n_games=4096, window=32, parts=1, learning_rate=3e-4, gamma=0.99, seed_base=0, sample_seed=0x5EED,
                 rules={"first_player": "Random", "tile_pool": "Lid"}, device=None, use_graph=True, persistent=True, results_dir="results",
                 ring=3, opponent="random", opponent_refresh=0, move_limit=0, players=2, fused_wide=False,
                 fused_opponent=False, fused_learner=False, fused_seats=False, gae_lambda=None, bootstrap_tail=False, algorithm="a2c",
                 clip_eps=0.2, value_coeff=0.5, entropy_coeff=0.01, epochs=4, minibatches=4, normalize_advantage=True, league_size=4,
                 league_sampling="uniform", pfsp_power=2.0, opponent_playouts=8, opponent_playout_policy="uniform", opponent_playout_explore=0):
        """ring: trajectory windows kept (persistent rollout with one part): with ring >= 2 every step of every episode is trained
        exactly once (episodes straddle windows; an episode may span ring - 1 window boundaries), like NNRunner.train.
        opponent: "random" (GameRunner's default RandomAgent, the reference's scripts/training.py), a module (GameRunner(opponent=Agent(...)),
        game_runner.py:27-30: a frozen second net inside the rollout kernel), or "self": a frozen COPY of the policy that is replaced by the
        current policy every `opponent_refresh` updates (0: never) -- training against a past self; or "greedy" (two-player reference batches):
        PolicyRollout's scripted one-ply greedy player of the reward, on the per-cut path (no window kernel, ring 1: the learner takes
        update_from_windows; the opponent has no state, so checkpoints carry nothing for it) -- or, with fused_opponent=True (policy
        ActorCritic(136, 180, hidden 180)), inside the two-player window kernel (PolicyRollout(opponent="greedy", fused_opponent=True)): a
        persistent rollout with `ring` windows, the learner on update_from_rollout (every step of every finished episode trained exactly once),
        checkpoints that carry the ring and still nothing for the opponent; or "greedy_margin" (players = 3 / 4 or extended rules): the
        same scripted player for wide batches (PolicyRollout(players=P, opponent="greedy_margin"): every other seat maximises its margin over
        the best other seat), on the per-cut path, the learner on update_from_windows, nothing in the checkpoint for it -- or, with
        fused_wide=True and fused_seats=True (hidden 180), inside the wide window kernel (PolicyRollout(fused_seats=True)): one launch per
        window, the learner as for any fused_wide rollout (fused_learner=True trains whole episodes from the ring), still nothing in the
        checkpoint for the opponent.
        opponent="playout" (two-player reference batches; opponent_playouts=K in 1..256): PolicyRollout's scripted flat Monte-Carlo player -- the
        move with the maximal sum of score differences over K random playouts to the end of the round -- on the per-cut path exactly as
        "greedy" without fused_opponent (no window kernel: fused_opponent / fused_wide raise ValueError; ring 1, update_from_windows).  The
        opponent has no state: its draws are keyed by the Philox step counter a checkpoint already carries; checkpoints carry
        `opponent_playouts` and a file written with another K is refused, so a resumed run replays bit for bit.
        opponent_playout_policy="uniform" | "greedy", opponent_playout_explore=0..255: the playout policy of that player (PolicyRollout has
        the definition); checkpoints carry both, a file without them was written by the uniform player (uniform / 0), and a file written
        with other values is refused like another K.
        opponent="league" (league_size=K in 1..255, opponent_refresh=k, league_sampling="uniform" | "pfsp", pfsp_power): a POOL of K frozen past
        selves (PolicyRollout(opponent=[...]): every 16-game group plays one member, inside the window kernels where a single network opponent
        plays there).  The pool starts as K copies of the initial policy; every k updates the current policy is written into slot
        snapshots % K, that slot's results are zeroed and the assignment is redrawn: member probabilities league_probabilities (uniform, or
        pfsp from the win rates of rollout.league_results()), group counts by largest remainder, their order from a NumPy generator seeded
        with (sample_seed, redraw count, part).  Checkpoints carry the stacked pool, the assignment, the snapshot and redraw counts and the
        results with their marks and the per-game counters the marks refer to: a resumed run equals the uninterrupted one.  Wide batches, algorithm="ppo" and gae_lambda combine with it
        as with any network opponent.
        move_limit > 0: BatchedAzul.set_move_limit (beyond the reference: a game that would never end is cut, done = 3; its steps are trained like an
        episode that ended there, the return chain starts at the cut).
        players = 3 / 4 (or extended-rule keys in `rules`): PolicyRollout(players=...) on MultiplayerAzul parts -- the policy is
        BatchedActorCritic(env.obs_size, env.num_actions, hidden), the rollout runs its per-move PyTorch-GEMM path -- or, with
        fused_wide=True (hidden 180, opponent "random" or None), one window kernel per part (PolicyRollout(fused_wide=True); `persistent` has
        no kernel of its own for wide batches) -- and the learner its PyTorch path (update_from_windows); checkpoints carry the wide records (runner counters included) and the RNG streams as usual.  A module
        opponent or "self" works there too (PolicyRollout's wide network-opponent path; the opponent's weights travel in the checkpoint) --
        with fused_wide=True and fused_opponent=True (opponent hidden 180) its reply rounds run inside the window kernel
        (PolicyRollout(fused_opponent=True)).
        fused_learner=True (wide batches, with fused_wide=True and hidden 180; anything else raises ValueError): the wide batch trains like a
        two-player one -- PolicyRollout(wide_ring=ring) keeps the last `ring` windows, the learner is A2CLearner(fused=True) (gradients and
        Adam on the f32 matrix cores, azul_a2c_gradients / azul_a2c_apply_adam_n) reading the ring through azul_select_episode_samples,
        so every step of every episode is trained once, and rollout and learner share the learner's k-major weight copy.  Checkpoints then
        carry the ring, the learner's books and the fused moments.  Default False: the wide learner stays on its PyTorch path.
        gae_lambda / bootstrap_tail: PolicyRollout's switches of the same names, handed on.  gae_lambda in [0, 1) trains on the TD(lambda)
        return with critic bootstrap (the learner forms returns - V as before, on whichever path it takes); None or 1.0: the Monte-Carlo
        return, the launches of before.  bootstrap_tail=True (needs ring=1): the critic's value of the state after the window flows into its
        newest step and run_batch trains EVERY recorded step that carries an action, open episodes included
        (A2CLearner.update_from_windows(traj, complete_only=False)): n-step A2C.  Both need an opponent; a resumed run replays the next
        window's returns bit for bit (the values are in the ring a checkpoint carries, the tail is recomputed from the restored weights).
        algorithm: "a2c" (default: everything above, launch for launch) or "ppo": the learner is a PPOLearner(clip_eps, value_coeff,
        entropy_coeff, epochs, minibatches, normalize_advantage) -- `fused` decided as for the A2C learner -- and run_batch makes
        epochs x minibatches optimiser steps on the newest window through update_from_windows(traj, complete_only=not bootstrap_tail): the
        clipped surrogate on returns - value (the GAE advantage with gae_lambda), gradients from azul_ppo_gradients on the fused path.  PPO
        trains one window: it needs ring=1 and an opponent other than None (ValueError otherwise, as for an unknown algorithm).  The five
        agent columns of the CSV carry PPOLearner's meanings, averaged over the optimiser steps since the last logged row; checkpoints
        carry the learner's call count, which keys the minibatch permutations."""
        from .batch import parse_ext_rules
        wide = int(players) != 2 or parse_ext_rules(rules, int(players)) != 0
        fused_learner = bool(fused_learner)
        if fused_learner and wide and not fused_wide:
            raise ValueError("fused_learner=True trains a wide batch from the ring of its window kernel: it needs fused_wide=True")
        # (PolicyRollout refuses the same before it allocates; here the learner's buffers would already exist)
        if gae_lambda is not None and not 0.0 <= float(gae_lambda) <= 1.0:
            raise ValueError("gae_lambda must lie in [0, 1] (1: the Monte-Carlo return, 0: the one-step TD target), got %r" % (gae_lambda,))
        if opponent is None and (bootstrap_tail or (gae_lambda is not None and float(gae_lambda) < 1.0)):
            raise ValueError("gae_lambda < 1 and bootstrap_tail need the records of one seat: an opponent other than None")
        if bootstrap_tail and parts == 1 and int(ring) >= 2 and (persistent or (wide and fused_learner)):
            raise ValueError("bootstrap_tail=True gives the open episodes of one window a target: it needs ring=1 (a ring of %d windows "
                             "trains whole episodes, nothing is open there)" % int(ring))
        if algorithm not in ("a2c", "ppo"):
            raise ValueError("algorithm must be \"a2c\" or \"ppo\", got %r" % (algorithm,))
        if algorithm == "ppo" and (int(ring) != 1 or opponent is None):
            raise ValueError("algorithm=\"ppo\" trains the newest window of one seat's records: it needs ring=1 and an opponent other than None")
        if algorithm == "ppo":
            PPOLearner.check_arguments(clip_eps, value_coeff, entropy_coeff, epochs, minibatches)
        if isinstance(opponent, str) and opponent == "league":
            if not 1 <= int(league_size) <= 255:
                raise ValueError("league_size must be in 1..255, got %r" % (league_size,))
            league_probabilities([0], [0.5], league_sampling, pfsp_power)      # (refuses an unknown league_sampling)
        self.algorithm = algorithm
        self.bootstrap_tail = bool(bootstrap_tail)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        policy = policy.to(dev)
        wide_fused = wide and fused_learner
        fused = (True if wide_fused else False) if wide else (True if fused_learner else None)
        if algorithm == "ppo":
            self.learner = PPOLearner(policy, learning_rate=learning_rate, gamma=gamma, clip_eps=clip_eps, value_coeff=value_coeff,
                                      entropy_coeff=entropy_coeff, epochs=epochs, minibatches=minibatches,
                                      normalize_advantage=normalize_advantage, shuffle_seed=sample_seed, fused=fused)
        else:
            self.learner = A2CLearner(policy, learning_rate=learning_rate, gamma=gamma, fused=fused)
        # rollout kernels and learner share ONE k-major copy of the weights (the learner's flat master copy)
        self.opponent_refresh = int(opponent_refresh)
        self._self_opponent = isinstance(opponent, str) and opponent == "self"
        self._league = isinstance(opponent, str) and opponent == "league"
        if self._self_opponent:
            import copy
            opponent = copy.deepcopy(policy)
        if self._league:
            import copy
            opponent = [copy.deepcopy(policy) for _ in range(int(league_size))]
            self.league_sampling, self.pfsp_power, self._sample_seed = league_sampling, float(pfsp_power), int(sample_seed)
            self.snapshots = self.redraws = 0
        self.rollout = PolicyRollout(policy, n_games=n_games, parts=parts, rules=rules, seed_base=seed_base, device=dev, window=window,
                                     use_graph=use_graph, sample_seed=sample_seed, opponent=opponent, persistent=persistent,
                                     kweights=None if (wide and not wide_fused) else self.learner.kweights(dev),
                                     ring=ring if (persistent and parts == 1) else 1,
                                     move_limit=move_limit, players=players, fused_wide=fused_wide,
                                     fused_opponent=fused_opponent, wide_ring=ring if (wide_fused and parts == 1) else 1,
                                     fused_seats=fused_seats, gae_lambda=gae_lambda, bootstrap_tail=bootstrap_tail,
                                     opponent_playouts=opponent_playouts, opponent_playout_policy=opponent_playout_policy,
                                     opponent_playout_explore=opponent_playout_explore)
        self.gamma = gamma
        self.results_dir = results_dir
        self.batch = 0
        self._stat_base = self._stat_totals()
        self.history = {k: [] for k in ("batch",) + AGENT_STAT_KEYS + STAT_KEYS}

    # ---- statistics ----------------------------------------------------------------------------------
    def _stat_totals(self):
        """Finished episodes and the ten get_statistics() sums over all games: reduced ON THE DEVICE (the per-game counters stay
        there; 11 numbers cross PCIe instead of 88 bytes per game), on the stream that ran the games."""
        tot = None
        for p, env in enumerate(self.rollout.envs):
            with torch.cuda.stream(self.rollout.streams[p]):
                c = env.counters_dev()
                t = torch.cat([c["episodes"].sum().to(torch.float64).reshape(1), c["stat_sums"].sum(dim=0)])
            self.rollout.streams[p].synchronize()
            tot = t if tot is None else tot + t
        tot = tot.cpu().numpy()
        return int(tot[0]), tot[1:]

    def _game_statistics(self):
        """Means over the episodes finished since the last call (GameStatistics.get_stats, game_runner.py:17-22)."""
        ep, sums = self._stat_totals()
        ep0, sums0 = self._stat_base
        self._stat_base = (ep, sums)
        n = ep - ep0
        return n, {k: (float(sums[i] - sums0[i]) / n if n else float("nan")) for i, k in enumerate(STAT_KEYS)}

    # ---- one batch -----------------------------------------------------------------------------------
    def run_batch(self, collect_stats=True):
        """One rollout window + one update.  collect_stats=False keeps everything on the device (no host round trip): the
        episode statistics and the reward keep accumulating and are reported by the next collecting call, like the reference's
        GameStatistics buffers between two get_stats() calls (game_runner.py:17-22)."""
        tr = self.rollout.run_window(self.gamma)
        self.rollout.join()                              # device-side dependency: the host keeps enqueueing
        if self.algorithm == "ppo":                      # epochs x minibatches steps on the newest window
            out = self.learner.update_from_windows(tr, complete_only=not self.bootstrap_tail)
        elif self.bootstrap_tail:                        # every recorded step has its target: the open episodes' steps are samples too
            out = self.learner.update_from_windows(tr, complete_only=False)
        else:
            out = self.learner.update_from_rollout(self.rollout)
        self.rollout.refresh_weights()
        self.batch += 1
        if self._self_opponent and self.opponent_refresh and self.batch % self.opponent_refresh == 0:
            self.rollout.set_opponent(self.rollout.policy)         # the frozen past self moves up to the present (weights copied in place)
        if self._league and self.opponent_refresh and self.batch % self.opponent_refresh == 0:
            self._league_refresh()
        r = sum(part["reward"].sum() for part in tr)
        self._reward_acc = r if getattr(self, "_reward_acc", None) is None else self._reward_acc + r
        if not collect_stats:
            return None
        episodes, game = self._game_statistics()
        row = {"batch": self.batch, "reward": float(self._reward_acc) / episodes if episodes else float("nan")}
        self._reward_acc = None
        # the loss terms of every update since the last collecting call, averaged (AgentStatistics.get_stats, agent.py:19-24)
        fresh = min(self.learner.updates - getattr(self, "_loss_mark", 0), len(self.learner.statistics["ac_loss"]))
        for k in AGENT_STAT_KEYS[1:]:
            vals = list(self.learner.statistics[k])[len(self.learner.statistics[k]) - fresh:]
            row[k] = float(torch.stack([torch.as_tensor(v, dtype=torch.float32, device=self.rollout.device) for v in vals]).mean())
        self._loss_mark = self.learner.updates
        row.update(game)
        for k, v in row.items():
            self.history[k].append(v)
        return row

    def _league_refresh(self):
        """The current policy becomes pool member snapshots % K (weights copied in place), that slot's results are zeroed, and the groups are
        dealt anew from the results so far (one host synchronisation per refresh: K x 11 doubles per part)."""
        ro = self.rollout
        res = ro.league_results()                            # booked under the assignment the episodes were played with
        slot = self.snapshots % ro.pool_size
        ro.set_pool_member(slot, ro.policy)
        ro.reset_member_results(slot)
        self.snapshots += 1
        episodes = [0 if m == slot else r["episodes"] for m, r in enumerate(res)]
        probs = league_probabilities(episodes, [r["win_percent"] for r in res], self.league_sampling, self.pfsp_power)
        groups = ro.assignment().shape[1]
        ro.set_assignment(np.stack([league_redraw(probs, groups, (self._sample_seed, self.redraws, p)) for p in range(ro.parts)]))
        self.redraws += 1

    def train(self, net_name=None, batches=1000, log_every=None, checkpoint_every=1000, checkpoint_ring=False):
        """nn_runner.py:49-84: `batches` updates; with a `net_name` the CSV log and the checkpoints go to results_dir.
        checkpoint_ring: whether the periodic checkpoints carry the trajectory ring (~75 KB per game, save_checkpoint) -- off by
        default: a periodic file is a restart point, not a bit-exact continuation; call save_checkpoint(path) for the latter."""
        log_every = max(1, batches // 1000) if log_every is None else log_every             # nn_runner.py:79
        path = None
        if net_name is not None:
            os.makedirs(self.results_dir, exist_ok=True)
            path = os.path.join(self.results_dir, net_name + ".csv")
            if self.batch == 0 or not os.path.exists(path):
                with open(path, mode="w", newline="") as fh:                                # nn_runner.py:51-54
                    csv.writer(fh, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL).writerow(
                        ["batch"] + list(AGENT_STAT_KEYS) + list(STAT_KEYS))
        last = None
        for i in range(batches):
            logging = (self.batch + 1) % log_every == 0 or i == batches - 1
            row = self.run_batch(collect_stats=logging)
            last = row if row is not None else last
            if path is not None and self.batch % log_every == 0:
                with open(path, mode="a+", newline="") as fh:                               # nn_runner.py:80-82
                    csv.writer(fh, delimiter=",", quotechar='"', quoting=csv.QUOTE_MINIMAL).writerow(
                        [last["batch"]] + [last[k] for k in AGENT_STAT_KEYS] + [last[k] for k in STAT_KEYS])
            if net_name is not None and self.batch % checkpoint_every == 0:                # nn_runner.py:83-84
                self.save_checkpoint(os.path.join(self.results_dir, net_name + ".pt"), save_ring=checkpoint_ring)
                self.export_mx(os.path.join(self.results_dir, net_name + ".mx"))            # the reference's file name and content
        return last

    # ---- the reference's own network file ---------------------------------------------------------------
    def export_mx(self, path, module_factory=None):
        """The file the reference writes and reads: NNRunner.train does torch.save(agent.ac_net, "/results/<name>.mx") (nn_runner.py:83-84)
        and Agent(base_net_file=...) torch.load()s that MODULE (agent.py:36).  `module_factory` builds the module to pickle -- pass the
        reference's azulnet.model.ActorCritic to get a file the unchanged reference loads; default: this package's BatchedActorCritic
        (same parameter names, so its state_dict loads into either class).  The weights are copied to the CPU first."""
        from .policy import BatchedActorCritic
        pol = self.rollout.policy
        self.rollout.synchronize()
        mod = (module_factory or (lambda: BatchedActorCritic(pol.critic_linear1.in_features, pol.actor_linear2.out_features,
                                                             pol.critic_linear1.out_features)))()
        mod.load_state_dict({k: v.detach().cpu() for k, v in pol.state_dict().items()})
        torch.save(mod, path)
        return path

    def import_mx(self, path):
        """Continue from a reference network file: a pickled module (anything with state_dict(): the reference's ActorCritic, loadable
        where its class is importable) or a plain state_dict, with the reference's parameter names."""
        obj = torch.load(path, map_location="cpu", weights_only=False)
        sd = obj.state_dict() if hasattr(obj, "state_dict") else obj
        self.rollout.synchronize()
        self.rollout.policy.load_state_dict({k: v.to(self.rollout.device) for k, v in sd.items()})
        self.learner.sync_from_module()                  # the flat k-major master copy the kernels read
        self.rollout.refresh_weights()

    # ---- checkpoints ---------------------------------------------------------------------------------
    def save_checkpoint(self, path, save_ring=True):
        """save_ring=True (default): the trajectory ring (the last `ring` windows: episodes in flight), the rollout's window clock and
        the learner's per-game "first step not trained yet" go into the file, so that a restored run EQUALS the uninterrupted one
        (~75 KB per game with the default ring of 3 x 32 steps).  save_ring=False: a small file; a run restored from it starts its
        books with the first window it plays -- the steps of the episodes in flight at the checkpoint that were recorded before it are
        not trained, and their tails are trained as if they were whole episodes (returns of those tails are still exact)."""
        ro = self.rollout
        ro.synchronize()
        torch.cuda.synchronize(ro.device)
        envs = ro.games_state()                          # records, MT19937 streams, Philox step counters
        for p, e in enumerate(envs):
            e.update({"next_" + k: ro.traj[p][k][ro.T].cpu() for k in ("obs", "mask", "player")})
        ck = {"policy": ro.policy.state_dict(), "optimizer": self.learner.optimizer_state(), "envs": envs,
              "batch": self.batch, "n_games": ro.n, "parts": ro.parts, "window": ro.T, "game_id_base": ro.game_id_base,
              "windows_played": ro.windows_played, "ring": ro.ring, "ring_saved": bool(save_ring and ro.ring > 1)}
        if ro.opponent == "playout":                     # the scripted player's one setting (its draws follow the Philox step counter in `envs`)
            ck["opponent_playouts"] = ro.opponent_playouts
            ck["opponent_playout_policy"], ck["opponent_playout_explore"] = ro.opponent_playout_policy, ro.opponent_playout_explore
        if ro.league:                                    # the assignment, the results and their marks, the snapshot and redraw counts
            ck["league"] = dict(ro.league_state(), snapshots=getattr(self, "snapshots", 0), redraws=getattr(self, "redraws", 0))
        if ro.netopp:                                    # the network opponent's (frozen) weights, a league's stacked: a resumed run plays the same nets
            ck["opponent"] = {"o" + k: getattr(ro, "o" + k).cpu() for k in ro._OPP_ARRAYS}
        if save_ring and ro.ring > 1:
            ck["ring_buffers"] = [{k: v.cpu() for k, v in rg.items()} for rg in ro.rings]
            ck["learner_ring"] = self.learner.ring_state()
        torch.save(ck, path)

    def load_checkpoint(self, path):
        ro = self.rollout
        # (on the CPU first: the ring of a large batch is GBs and every tensor is copied into its resident buffer below, one at a time)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if (ck["n_games"], ck["parts"], ck["window"]) != (ro.n, ro.parts, ro.T):
            raise ValueError("checkpoint was written for n_games=%d parts=%d window=%d" % (ck["n_games"], ck["parts"], ck["window"]))
        if ro.opponent == "playout" and ck.get("opponent_playouts", ro.opponent_playouts) != ro.opponent_playouts:
            raise ValueError("checkpoint was written for opponent_playouts=%d, this trainer plays %d"
                             % (ck["opponent_playouts"], ro.opponent_playouts))
        if ro.opponent == "playout":                     # (a file without the keys was written by the uniform player)
            for key, absent in (("opponent_playout_policy", "uniform"), ("opponent_playout_explore", 0)):
                if ck.get(key, absent) != getattr(ro, key):
                    raise ValueError("checkpoint was written for %s=%r, this trainer plays %r" % (key, ck.get(key, absent), getattr(ro, key)))
        ro.synchronize()
        ro.policy.load_state_dict(ck["policy"])
        self.learner.load_optimizer_state(ck["optimizer"])          # also rebuilds the flat master copy from the module
        ro.refresh_weights()
        new_base = int(ck.get("game_id_base", ro.game_id_base))            # the sampling streams are keyed by the global game id
        if new_base != ro.game_id_base:
            ro.game_id_base = new_base
            if ro.use_graph:                                                # the id base is a launch argument baked into the captured graphs
                ro.graphs = []
                ro._capture(getattr(ro, "gamma", self.gamma))               # (its warm-up window advances the games: they are restored below)
        ro.load_games_state(ck["envs"])
        for p, e in enumerate(ck["envs"]):
            ro.envs[p].set_id_base(ro.game_id_base + p * ro.h)
            for k in ("obs", "mask", "player"):
                ro.traj[p][k][ro.T].copy_(e["next_" + k])
        # the trajectory ring and the books of the ring selection: restored when the file has them (the run then equals the
        # uninterrupted one), otherwise the learner's books restart with the next window (nothing recorded before this call -- by the
        # checkpointed run or by this trainer -- is ever selected: `pending` starts at the next window, whose selection only reads
        # done flags of windows played from now on)
        if "ring_buffers" in ck and ck.get("ring") == ro.ring and ro.ring > 1:
            for rg, saved in zip(ro.rings, ck["ring_buffers"]):
                for k, v in saved.items():
                    rg[k].copy_(v)
            ro.windows_played = int(ck["windows_played"])
            for p in range(ro.parts):
                ro.traj[p] = ro._window_views(ro.rings[p], (ro.windows_played - 1) % ro.ring)
            self.learner.load_ring_state(ro, ck.get("learner_ring"))
        else:
            import warnings
            if "ring_buffers" in ck and ro.ring > 1:
                warnings.warn("checkpoint %s holds a trajectory ring of %s windows, this rollout uses %d: the ring is NOT restored -- the "
                              "resumed run restarts its books with the next window and no longer equals the uninterrupted one"
                              % (path, ck.get("ring"), ro.ring))
            elif ro.ring > 1:
                # a small file (save_ring=False: what train() writes periodically unless checkpoint_ring=True)
                warnings.warn("checkpoint %s carries no trajectory ring (written with save_ring=False): the steps of episodes in flight when it "
                              "was written are not trained, their tails count as whole episodes -- the resumed run does not equal the "
                              "uninterrupted one (save_checkpoint(save_ring=True) / train(checkpoint_ring=True) for an exact resume)" % path)
            self.learner.load_ring_state(ro, None)
        if ro.netopp and "opponent" in ck:
            with torch.no_grad():
                for k, v in ck["opponent"].items():
                    getattr(ro, k).copy_(v.to(ro.device))
        if ro.league and "league" in ck:
            ro.load_league_state(ck["league"])
            self.snapshots, self.redraws = int(ck["league"]["snapshots"]), int(ck["league"]["redraws"])
        torch.cuda.synchronize(ro.device)
        self.batch = int(ck["batch"])
        self._stat_base = self._stat_totals()
        self._reward_acc = None
        self._loss_mark = self.learner.updates
