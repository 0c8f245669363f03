"""An arena: round-robin matches of a pool of networks inside the window kernels, and a rating from their outcomes.

`Arena(nets)` stacks K networks of one shape into one pool and plays every 16-game group (one workgroup of the window kernels) with one
ORDERED pair of them -- the agent seat is pool member a, the opponent seat pool member o -- so that one launch per window plays every
pairing of a tournament side by side (azul_batch_policy_rollout_arena / azul_batch_mp_policy_rollout_arena).  For the games of a group
assigned (a, o) every output is bit-identical to `PolicyRollout(net_a, opponent=net_b)` on its window kernel.  azul_arena_tally books
finished episodes and the sums of the ten game statistics per ordered pair on the device, in one fixed order; `bradley_terry` turns the
win matrix into ratings.  `round_robin_pairs` and `bradley_terry` are host functions and need no device.

A bias of the design, argued and not measured: the arena plays a fixed horizon (windows x window agent steps per slot), and the episode the
cut-off abandons in a slot tends to be a long one (a renewal-reward argument: the horizon's end is more likely to fall into a long episode
than into a short one).  Only finished episodes are booked, so wins / episodes of a cell converges to the per-episode win rate only as
the episodes per slot grow; with few episodes per slot it leans towards the outcomes of short episodes.
"""
import numpy as np
import torch

from . import _lib as L
from .batch import batch_shape, parse_ext_rules
from .pool import checked_seats
from .records import STAT_KEYS
from .rollout import PolicyRollout, _layer_sizes

GROUP = L.LEAGUE_GROUP_GAMES
_WIN = STAT_KEYS.index("win_percent")
_PAIRS = ("pairs are", "[parts][ceil(h / 16)][2]", "pairs name")        # checked_seats' words for an arena's seats


def round_robin_pairs(K, groups, round, mirror=False):
    """The (agent, opponent) pair of every group of schedule round `round`: an int array [groups][2].  The ordered pairs (i, j), i != j,
    of K members are taken in lexicographic order -- mirror=True adds the (i, i) pairs, K = 1 gives the single pair (0, 0) -- and global
    group g of round r plays pair (r * groups + g) mod P, P the number of pairs: consecutive rounds walk the list without a gap, so over
    rounds_per_cycle rounds every pair is played and the pairs' counts differ by at most 1."""
    K, groups, r = int(K), int(groups), int(round)
    if K < 1 or groups < 0 or r < 0:
        raise ValueError("round_robin_pairs: K >= 1, groups >= 0 and round >= 0, got %d, %d, %d" % (K, groups, r))
    pairs = [(i, j) for i in range(K) for j in range(K) if mirror or i != j] or [(0, 0)]
    P = len(pairs)
    return np.asarray([pairs[(r * groups + g) % P] for g in range(groups)], dtype=np.int64).reshape(groups, 2)


def rounds_per_cycle(K, groups, mirror=False):
    """Schedule rounds of `groups` groups after which round_robin_pairs has played every pair (one full cycle): ceil(P / groups)."""
    K = int(K)
    P = max(1, K * K if mirror else K * (K - 1))
    return -(-P // max(1, int(groups)))


def bradley_terry(episodes, wins, prior=1.0, tol=1e-13, max_iter=10000):
    """Bradley-Terry strengths of K members from the arena's matrices: episodes[a][o] finished with a in the agent seat against o, wins[a][o]
    of them won by the agent seat.  For i != j the wins of i over j are wins[i][j] + (episodes[j][i] - wins[j][i]): the reference's
    win_percent is the strict score[0] > score[1] (azul.py:315), so a DRAW goes to the opponent seat -- the two directions cancel when both
    are played equally often, which a round-robin schedule does.  (i, i) games carry no information and are ignored; NaN cells count as
    empty.  `prior` virtual games are split evenly (prior / 2 wins each way) for every pair that has played, so that a member that never
    lost keeps a finite rating.  The update is the MM iteration p_i <- W_i / sum_j n_ij / (p_i + p_j) in float64, normalised to geometric
    mean 1 after every sweep, until the largest relative change is below `tol`.  Returns {"strength", "rating", "iterations"}: rating =
    400 log10 strength (mean 0).  A member without games keeps strength 1."""
    ep = np.nan_to_num(np.asarray(episodes, dtype=np.float64), nan=0.0)
    wn = np.nan_to_num(np.asarray(wins, dtype=np.float64), nan=0.0)
    if ep.ndim != 2 or ep.shape[0] != ep.shape[1] or wn.shape != ep.shape:
        raise ValueError("bradley_terry: episodes and wins are [K][K] matrices, got %s and %s" % (ep.shape, wn.shape))
    K = ep.shape[0]
    w = wn + (ep - wn).T                                     # w[i][j]: games i won against j, whichever seat it sat in
    np.fill_diagonal(w, 0.0)
    n = w + w.T                                              # games between i and j
    played = n > 0
    w = w + np.where(played, 0.5 * float(prior), 0.0)
    n = n + np.where(played, float(prior), 0.0)
    W = w.sum(axis=1)
    p = np.ones(K)
    it = 0
    for it in range(1, int(max_iter) + 1):
        with np.errstate(divide="ignore", invalid="ignore"):
            denom = np.where(played, n / (p[:, None] + p[None, :]), 0.0).sum(axis=1)
        new = np.where(denom > 0, W / np.where(denom > 0, denom, 1.0), p)
        live = new > 0
        if live.any():
            new = new / np.exp(np.log(new[live]).mean())     # geometric mean 1 (a member with no win at prior 0 has strength 0)
        change = np.abs(new - p) / np.where(p > 0, p, 1.0)
        p = new
        if change.max() < tol:
            break
    with np.errstate(divide="ignore"):
        rating = 400.0 * np.log10(p)
    return {"strength": p, "rating": rating, "iterations": it}


class Arena(PolicyRollout):
    """K networks of ONE shape play each other: every 16-game group is one ordered pair (agent member, opponent member) of the pool.

        Arena(nets, n_games=4096, parts=1, rules=..., players=2, window=32, seed_base=0, sample_seed=0x5EED, opponent_seed=None,
              selection="Distribution" | "Max", mirror=False, move_limit=0, device=None, pairs=None)

    Built on PolicyRollout's league: the stacked pool (pool.NetPool: all six arrays of every member; it serves both seats), the openings at
    construction on the per-cut path, the trajectory buffers, the window launch, the parts and their streams.  Window kernels only: two-player batches need
    ActorCritic(136, 180, hidden 180), wide batches (`players` = 3 / 4 or extended rules) ActorCritic(obs_size, num_actions, hidden 180)
    of the batch; anything else raises ValueError before anything is allocated.  `selection` applies to both seats.  `pairs`: the first
    pairing, an int array [parts][G][2] (default: round 0 of round_robin_pairs over the parts' groups, G = ceil(n_games / parts / 16)).
    See the module docstring for the fixed-horizon bias of wins / episodes."""

    def __init__(self, nets, n_games=4096, parts=1, rules={"first_player": "Random", "tile_pool": "Lid"}, players=2, window=32, seed_base=0,
                 sample_seed=0x5EED, opponent_seed=None, selection="Distribution", mirror=False, move_limit=0, device=None, pairs=None):
        nets = list(nets) if isinstance(nets, (list, tuple)) else None
        if nets is None or not 1 <= len(nets) <= 255:
            raise ValueError("an arena is a pool of 1..255 networks (a group's member is one byte), got %s"
                             % ("no list" if nets is None else len(nets)))
        if any(m is None or isinstance(m, str) or not hasattr(m, "critic_linear1") for m in nets):
            raise ValueError("the members of an arena are modules with the reference's four layers")
        if any(_layer_sizes(m) != _layer_sizes(nets[0]) for m in nets):
            raise ValueError("the members of an arena must have ONE shape (their weights are stacked array by array), got %s"
                             % sorted(set(_layer_sizes(m) for m in nets)))
        if selection not in ("Distribution", "Max"):
            raise ValueError("selection is \"Distribution\" or \"Max\" (both seats), got %r" % (selection,))
        if int(n_games) < 1 or int(parts) < 1 or int(n_games) % int(parts):
            raise ValueError("n_games must be a positive multiple of parts, got %r / %r" % (n_games, parts))
        wide = int(players) != 2 or parse_ext_rules(rules, int(players)) != 0
        n_obs, n_act = batch_shape(int(players), rules)
        if _layer_sizes(nets[0]) != (n_obs, n_obs, 180, 180, n_act):
            raise ValueError("the arena runs on the window kernels, compiled for ActorCritic(%d, %d, hidden 180) on this batch; got inputs "
                             "%d / %d, hidden %d / %d and %d actions" % ((n_obs, n_act) + _layer_sizes(nets[0])))
        K, G = len(nets), (int(n_games) // int(parts) + GROUP - 1) // GROUP
        self.mirror = bool(mirror)
        first = round_robin_pairs(K, int(parts) * G, 0, self.mirror).reshape(int(parts), G, 2) if pairs is None else \
            checked_seats(pairs, (int(parts), G, 2), K, *_PAIRS)
        self.schedule_round = 0                                # the next round play_schedule plays
        sw = dict(fused_wide=True, fused_opponent=True) if wide else dict(persistent=True)
        super().__init__(nets[0], n_games=int(n_games), parts=int(parts), rules=rules, seed_base=seed_base, device=device, window=window,
                         use_graph=False, sample_seed=sample_seed, opponent=nets, action_selection=selection, opponent_selection=selection,
                         opponent_seed=opponent_seed, move_limit=move_limit, players=int(players), _pairs=first, **sw)
        self.arena_entry = self.window_entry                   # azul_batch_policy_rollout_arena / azul_batch_mp_policy_rollout_arena

    def _need_league(self):      # PolicyRollout's league methods and set_opponent open with this: an arena's seats are pairs, its results per pair
        raise ValueError("this is an arena: pairs() / set_pairs(), set_member() and results() are its methods")

    # ---- the arena ---------------------------------------------------------------------------------------------------------------------
    def pairs(self):
        """The (agent, opponent) pair of every 16-game group: an int array [parts][G][2] (a host copy)."""
        return self.pool.seats_host.astype(np.int64)

    def set_member(self, i, net_or_state_dict):
        """Install the weights of pool member i in place (both seats read the one pool)."""
        self.pool.set_member(i, net_or_state_dict)

    def set_pairs(self, pairs):
        """Pair the groups anew: an int array [parts][G][2] of pool members (agent, opponent), refused on the host for a wrong shape or a
        member >= K.  The tally runs first, so that the episodes finished so far are booked to the pair that played them; then the pairs
        are installed in place on the parts' streams and EVERY game is restarted -- GameRunner.reset() and the new opponents' openings, on
        the per-cut path of the construction.  Every booked episode is therefore played from its first move to its last by one pair; the
        episodes abandoned in flight are never booked and the restart does not count as an episode."""
        a = checked_seats(pairs, self.pool.seats_host.shape, self.pool.size, *_PAIRS)
        for s in self.streams:
            s.wait_stream(torch.cuda.current_stream(self.device))
        self.pool.install(a)
        for p in range(self.parts):
            with torch.cuda.stream(self.streams[p]):
                self._net_reset(p)
                t = self.traj[p]
                self.envs[p].observe_all(0, t["obs"][self.T], t["mask"][self.T], t["player"][self.T])

    def play(self, windows, gamma=0.99):
        """`windows` windows of every part with the current pairs; returns the trajectory dicts of the last one."""
        for _ in range(int(windows)):
            self.run_window(gamma=gamma)
        return self.traj

    def play_schedule(self, windows_per_round, rounds=None):
        """Round after round: set_pairs(round_robin_pairs(K, groups, r, mirror)) for the next schedule round r, then `windows_per_round`
        windows.  `rounds` defaults to one full cycle (every pair played)."""
        K, G = self.pool.size, self.pool.seats_host.shape[1]
        total = self.parts * G
        n = rounds_per_cycle(K, total, self.mirror) if rounds is None else int(rounds)
        for i in range(n):
            self.set_pairs(round_robin_pairs(K, total, self.schedule_round, self.mirror).reshape(self.parts, G, 2))
            self.schedule_round += 1
            self.play(windows_per_round)

    def results(self, reset=False):
        """Per ordered pair what its groups finished since construction (or the last reset): {"episodes": int [K][K], "wins": [K][K] (the
        win_percent sums: episodes the agent seat won), "mean": {key: [K][K]} for the ten STAT_KEYS}; wins and means of a cell without
        episodes are NaN.  Reduced on the device in a fixed order: K x K x 11 doubles per part cross to the host (parts added in part
        order).  reset=True zeroes the results behind the read."""
        tot = self.pool.totals(reset)
        ep = tot[:, :, 0]
        has = ep > 0
        div = np.where(has, ep, 1.0)
        return {"episodes": ep.astype(np.int64), "wins": np.where(has, tot[:, :, 1 + _WIN], np.nan),
                "mean": {k: np.where(has, tot[:, :, 1 + i] / div, np.nan) for i, k in enumerate(STAT_KEYS)}}

    def ratings(self, prior=1.0):
        """bradley_terry of the results so far."""
        r = self.results()
        return bradley_terry(r["episodes"], r["wins"], prior=prior)

    def state(self):
        """What a checkpoint carries of the arena besides the members' weights (host copies): the pairs, the per-pair results, the marks and
        the per-game counters they refer to (NetPool.state's reasons), the schedule round, and per part the games -- records, MT19937
        streams, the Philox step counter."""
        st = self.pool.state()
        return dict(st, pairs=self.pool.seats_host.copy(), arena_results=st.pop("results"), schedule_round=self.schedule_round,
                    windows_played=self.windows_played, games=self.games_state())

    def load_state(self, st):
        a = checked_seats(st["pairs"], self.pool.seats_host.shape, self.pool.size, *_PAIRS)
        self.pool.load_state(a, st["arena_results"], st["marks"], st["counters"])
        self.schedule_round, self.windows_played = int(st["schedule_round"]), int(st["windows_played"])
        self.load_games_state(st["games"])
        torch.cuda.synchronize(self.device)
