"""Policy-driven self-play on one MI355X (BASELINE configs[2]): the batched counterpart of the reference's
``NNRunner.run_episode`` (azulnet/nn_runner.py:17-47) and of the action sampling in ``Agent.get_ac_output``
(azulnet/agent.py:64-81).

`persistent=True` (what the benches use): ONE launch per window and part -- azul_batch_policy_rollout keeps every game in
registers for the whole window and interleaves network, sampling and env step inside the kernel.  Otherwise, per move and
part of the batch (each part has its own HIP stream) -- two launches:
    azul_policy_forward      the whole ActorCritic forward on the f32 matrix cores (hidden = relu(obs @ [critic_linear1 |
                             actor_linear1]), value, logits) + masked softmax + categorical sample + log-prob + entropy;
                             value / action / log-prob / entropy land straight in trajectory slot t
    azul_batch_policy_step   Azul.step + reward + done + auto-reset + NEXT obs / mask / player, written into slot t+1
                             (opponent="random": azul_batch_agent_step, the reference's training setup)
Nothing is copied.  A window of `T` moves is captured once into a HIP graph per part and replayed (the Philox step counter
lives in device memory and is advanced by the forward launch itself); results are identical with `use_graph=False`.
`fused_mlp=False` runs the network as PyTorch GEMMs (rocBLAS/hipBLASLt) + azul_policy_head (any network shape);
`fused_head=False` keeps the all-PyTorch sampling path (torch.multinomial) for comparison.

Per (move t, game g) the record holds what the reference's run_episode keeps per agent step (C1 in SURVEY.md 8a):
observation, legal mask, action, reward, done, value, log-prob of the action and the entropy term
`-mean(log p over legal actions)` (nn_runner.py:36-40), plus the player who moved and the discounted returns.
"""
import collections
import ctypes as C
import operator

import torch

from . import _lib as L
from .batch import BatchedAzul, batch_shape, parse_ext_rules
from .multiplayer import MultiplayerAzul
from .pool import NetPool, _OPP_ARRAYS, _kmajor, _p, checked_seats


# azul_batch_policy_rollout_returns takes what the two launch structs hold one by one: all weights, and the buffers obs .. returns
_WEIGHT_FIELDS = operator.attrgetter(*[k for k, _ in L.NetWeights._fields_])
_FLAT_BUFFER_FIELDS = operator.attrgetter(*[k for k, _ in L.RolloutBuffers._fields_[:11]])

# The window kernels, one row per (wide batch, opponent kind) that has one: the C entry that plays a whole window of a part in one launch,
# the constructor switch that asks for it, and the hidden size it is compiled for -- the policy must be ActorCritic(obs_size, num_actions,
# hidden) of the batch; opp_hidden: the same for a network opponent whose shape the mode checks vouch for (None: nothing to check there).
# "persistent" is the one switch that gives way quietly: a policy the one-launch forward does not fit plays move by move.
_WindowKernel = collections.namedtuple("_WindowKernel", "entry switch hidden opp_hidden")
_WINDOW_KERNELS = {
    (False, None): _WindowKernel("azul_batch_policy_rollout_returns", "persistent", 180, None),
    (False, "random"): _WindowKernel("azul_batch_policy_rollout_returns", "persistent", 180, None),
    (False, "net"): _WindowKernel("azul_batch_policy_rollout_vs", "persistent", 180, None),
    (False, "league"): _WindowKernel("azul_batch_policy_rollout_league", "persistent", 180, None),
    (False, "greedy"): _WindowKernel("azul_batch_policy_rollout_greedy", "fused_opponent", 180, None),
    (True, None): _WindowKernel("azul_batch_mp_policy_rollout", "fused_wide", 180, None),
    (True, "random"): _WindowKernel("azul_batch_mp_policy_rollout", "fused_wide", 180, None),
    (True, "net"): _WindowKernel("azul_batch_mp_policy_rollout_vs", "fused_opponent", 180, 180),
    (True, "league"): _WindowKernel("azul_batch_mp_policy_rollout_league", "fused_opponent", 180, 180),
    (True, "greedy_margin"): _WindowKernel("azul_batch_mp_policy_rollout_greedy", "fused_seats", 180, None),
}


def _layer_sizes(net):
    """(inputs of the critic / of the actor, hidden of the critic / of the actor, actions) of a module with the reference's four layers."""
    return (net.critic_linear1.in_features, net.actor_linear1.in_features, net.critic_linear1.out_features, net.actor_linear1.out_features,
            net.actor_linear2.out_features)


class PolicyRollout:
    # reply rounds per agent step / opening on the wide path before the loop gives up: a legal opponent ends a step within about two rounds
    # of the game (at most ~45 moves each for four players on nine displays); an opponent that keeps answering illegally would spin
    MAX_REPLY_ROUNDS = 512

    def __init__(self, policy, n_games=4096, parts=1, rules={"first_player": "Random", "tile_pool": "Lid"}, seed_base=0,
                 device=None, window=32, use_graph=True, fused_head=True, sample_seed=0x5EED, opponent=None, fused_mlp=True, persistent=False,
                 action_selection="Distribution", kweights=None, game_id_base=None, ring=1, opponent_selection="Distribution",
                 opponent_seed=None, opponent_trace=0, move_limit=0, players=2, fused_wide=False, fused_opponent=False, wide_ring=1,
                 fused_seats=False, gae_lambda=None, bootstrap_tail=False, opponent_playouts=8, opponent_playout_policy="uniform",
                 opponent_playout_explore=0, _pairs=None):
        """Who answers GameRunner's opponent_move(), and what plays a window.  "window kernel": ONE launch per window and part (_WINDOW_KERNELS),
        asked for by the switch in brackets; "per move" / "per cut": the launches of _window_moves.  Two-player reference batches (players=2, no
        extended-rule key in `rules`) and wide batches (`players` = 3 / 4 or extended rules) admit:

            opponent           two-player reference batch                           wide batch
            None, "random"     per move, HIP graph                                  per move, HIP graph
                               azul_batch_policy_rollout_returns [persistent]       azul_batch_mp_policy_rollout [fused_wide]
            <module>           per cut                                              per cut
                               azul_batch_policy_rollout_vs [persistent]            azul_batch_mp_policy_rollout_vs [fused_wide, fused_opponent]
            [<module>, ...]    per cut                                              per cut
                               azul_batch_policy_rollout_league [persistent]        azul_batch_mp_policy_rollout_league [fused_wide, fused_opponent]
            "greedy"           per cut                                              ValueError
                               azul_batch_policy_rollout_greedy [fused_opponent]
            "greedy_margin"    ValueError                                           per cut
                                                                                    azul_batch_mp_policy_rollout_greedy [fused_wide, fused_seats]
            "playout"          per cut (no window kernel)                           ValueError

        Every other combination of an opponent with fused_wide / fused_opponent / fused_seats raises ValueError, before anything is allocated.
        A window kernel computes what the per-move / per-cut path computes: the same trajectories, records, streams and counters (wide
        kernels add the network's sums in another order: the same bits wherever they are exact).  With an opponent inside, the opening of the
        games at construction stays on the per-cut path (openings after episodes that end inside a window are the kernel's), and a game that
        still owes an opponent_move() after MAX_REPLY_ROUNDS replies of one step (the two-player kernels: 64) ends the step with status AZUL_STUCK
        (unless the step already has a status) instead of raising RuntimeError -- raising would cost a host synchronisation per window.

        The opponents:
        opponent=None: the policy moves for both players / every seat (flat self-play, one record per env move).
        opponent="random": the reference's training setup -- the policy is player 1 of GameRunner, the opponent a RandomAgent inside the env
        step (game_runner.py:43-47); one record per AGENT step, observations from the agent's perspective.
        opponent=<a second BatchedActorCritic / any module with the reference's four layers>: GameRunner(opponent=Agent(...))
        (game_runner.py:27-30; scripts/run_batch.py:6-10) -- every opponent_move(), i.e. the opponent's replies, player 1's FORCED moves (:46)
        and the opening moves of reset() (:84-85), is sampled from that net's forward_actor on the observation from the mover's perspective
        (:38; agent.py:73-81), `opponent_selection` = its action_selection, `opponent_seed` its Philox seed; records as with "random".  Its
        weights are copied at construction; set_opponent() installs new ones (e.g. a frozen past self of the policy being trained).  Per cut:
        one launch per cut of the protocol (BatchedAzul.net_*) and one host synchronisation per reply round, no HIP graph; the window kernel
        runs matrix phases on the second weight set while any game of a workgroup owes a reply.  Two-player: the library's forward,
        ActorCritic(136, 180, hidden 180).  Wide: the module's shape must match the batch (ActorCritic(env.obs_size, env.num_actions), any
        hidden size: anything else raises ValueError); its actor half runs as PyTorch GEMMs + azul_policy_head_n with the two-player path's
        Philox keys, through MultiplayerAzul.net_* (azul_batch_mp_net_*); at most MAX_REPLY_ROUNDS reply rounds per step or opening -- an
        opponent that keeps answering with moves that are not legal raises RuntimeError.
        opponent=[net0, net1, ...] (a list or tuple of 1..255 such modules of ONE shape): a LEAGUE -- a pool of network opponents.  The games
        of a part are taken in groups of 16 (L.LEAGUE_GROUP_GAMES: the games of one workgroup of the window kernels; the last group may be
        ragged) and every group plays one member of the pool: assignment() / set_assignment(), default group i -> member i % pool_size.
        Everything said of a single network opponent holds per member -- the shape refusals, opponent_selection, opponent_seed,
        opponent_trace, the switches (`persistent` two-player; fused_wide with fused_opponent wide), rings, gae_lambda, the fused learner --
        and a game's trajectory is keyed by its global id, so the games of a group assigned to member m play exactly what they would play
        against opponent=<member m> alone.  The window kernels read the member once per workgroup (a base offset into the stacked weights);
        the per-cut path runs the opponent's forward once per member present in the part's assignment and keeps, per game, the answer of
        its group's member.  set_pool_member(i, ...) installs a member's weights in place; league_results() gives per member the episodes
        finished against it and the means of the game statistics over them (azul_league_tally: reduced on the device).
        opponent="greedy": the scripted one-ply greedy player of the reference's own reward on the same per-cut protocol -- every
        opponent_move() is BatchedAzul.greedy_action's answer, the move that maximises the mover's score difference after move + count_score
        (game_runner.py:48-50), one launch per reply round in place of the network's forward; records as with "random"; persistent and
        use_graph resolve to False, ring to 1; at most MAX_REPLY_ROUNDS reply rounds per step or opening (a game with nothing legal would owe
        its move for ever: RuntimeError).
        opponent="playout" (`opponent_playouts` = K in 1 .. L.PLAYOUTS_MAX, default 8): the scripted flat Monte-Carlo player on the same
        per-cut protocol -- every opponent_move() is BatchedAzul.playout_action's answer, the move with the maximal sum of score differences
        over K random playouts to the end of the round (azul_batch_playout_moves), one launch per reply round; reply round j of agent step t
        draws with seed = opponent_seed + j and call = (counter + t) & 0xffffffff, counter the Philox step counter at the start of the
        window (an opening at construction: the counter before the first step, 0xffffffff), so a run restored from games_state() replays bit
        for bit; records, trace, persistent / use_graph / ring and MAX_REPLY_ROUNDS as with "greedy".  It answers per cut only: a wide batch,
        fused_opponent=True and fused_wide=True raise ValueError, and so does opponent_selection="Max" (the player has no distribution to
        take the maximum of).  `opponent_playout_policy` = "uniform" (default) | "greedy" and `opponent_playout_explore` (0 .. 255; 0 with
        "uniform") choose the playout policy (BatchedAzul.playout_moves: with "greedy" both seats of a playout play greedy_action's move,
        a ply in explore / 256 the uniform one); the protocol, the seeds and the calls are the same, and "greedy" with explore 0 draws nothing.
        opponent="greedy_margin": the same scripted player for three / four seats and extended rules -- every other seat answers with
        MultiplayerAzul.greedy_action, the move that maximises the MOVER's margin over the best other seat after move + count_score
        (azul_batch_mp_score_moves; beyond the reference for P > 2, like the wide reward), through MultiplayerAzul.net_* exactly as a network
        opponent's answers: one launch per reply round, no opponent weights, at most MAX_REPLY_ROUNDS rounds.

        The switches:
        `persistent=True` (two-player; the policy must fit the one-launch forward, see fused_mlp -- otherwise it quietly plays per move): the
        window kernel keeps every game in registers for the whole window.  With opponent="greedy" it resolves to False unless fused_opponent.
        `fused_wide=True` (wide batches; ActorCritic(env.obs_size, env.num_actions, hidden 180) and fused_head, anything else raises
        ValueError): env, network on the f32 matrix cores and azul_policy_head_n's draw inside one kernel instead of the per-move GEMMs + head
        + env launches.  opponent=None | "random"; a network opponent needs fused_opponent=True too, greedy_margin seats fused_seats=True.
        `fused_opponent=True`: with fused_wide=True and opponent=<module>, itself of hidden size 180 (other opponents run per cut), the network
        opponent's reply rounds run inside the wide window kernel -- the same keys, counters and answers, opponent_selection, opponent_trace and
        set_opponent() included.  With opponent="greedy" (two-player, ActorCritic(136, 180, hidden 180) with fused_mlp and fused_head; another
        policy raises ValueError) the greedy player answers inside the two-player window kernel: persistent resolves to True.
        `fused_seats=True` (opponent="greedy_margin" with fused_wide=True; anything else, fused_opponent included, raises ValueError): the
        greedy_margin seats answer inside the wide window kernel -- no reply launches, no host synchronisation and no opponent weights.
        `use_graph`: a window of per-move launches is captured once into a HIP graph per part; resolves to False with a window kernel (one
        launch needs no graph) and on the per-cut path (reply rounds are data-dependent).
        `fused_mlp` / `fused_head`: fused_mlp=False, a wide batch, or a policy other than ActorCritic(136, 180, hidden 180) runs the network as
        PyTorch GEMMs + azul_policy_head (azul_policy_head_n on env.num_actions logits; trajectory buffers are env.obs_size / env.num_actions
        wide); fused_head=False keeps the all-PyTorch sampling path (action_selection="Distribution" only).

        The other arguments:
        `opponent_trace` = R > 0 (any opponent but "random") also records the opponent's answers: opp_action / opp_logp [T][R][N] (a scripted
        opponent leaves opp_logp 0; a window kernel fills the slots a step's replies used, the others keep -1), opp_replies [T][N].
        `move_limit` > 0 (beyond the reference, off by default; two-player reference batches only): cut an episode at the first end of a round
        with move_counter >= move_limit (done = 3) -- under the reference's rules some games never end and would keep their slot for ever
        (BatchedAzul.set_move_limit).
        `seed_base` / `game_id_base`: game i of this rollout is global game game_id_base + i (default: seed_base, so that a rank passes the id
        of its first game once); its CPython stream is random.seed(seed_base + i) and its sampling stream is Philox(sample_seed, step, global
        id) -- both independent of how the games are sharded over GPUs or split into parts.
        `ring` (two-player window kernels; rings >= 2 with one part feed A2CLearner.update_from_rollout): the trajectory buffers hold the
        last `ring` windows (a ring of ring * window time slots); run_window fills the next window of the ring and re-chains the discounted returns
        backwards through the older windows (azul_discounted_returns_ring), so that the opening steps of an episode that ends in a LATER window
        get their exact Monte-Carlo return too (A2CLearner.update_from_rollout trains every step of every episode exactly once, like
        NNRunner.train).  `wide_ring` = k >= 2 (wide window kernels, one part) is the same ring for wide batches (`ring` becomes k; the default
        k = 1 keeps it at 1).
        `players` = 3 / 4, or extended-rule keys in `rules` (the wide records): the games are MultiplayerAzul parts (GameRunner for P seats,
        azul_batch_mp_*; the shaped reward is the margin over the best opponent, beyond the reference for P > 2).
        `kweights` (two-player, or a wide window kernel; other wide rollouts ignore it): the k-major weights of a fused A2CLearner of the
        policy's shape (A2CLearner.kweights(): one copy serves rollout and learner).
        `gae_lambda` (any opponent but None; every path): None, or 1.0 without bootstrap_tail, leaves `returns` the reference's Monte-Carlo
        return q[t] = r[t] + gamma * q[t+1] and runs exactly the launches it ran before.  A float in [0, 1): after each window `returns` holds
        the TD(lambda) return G[t] = r[t] + gamma * ((1 - lambda) * V[t+1] + lambda * G[t+1]) (G[t] = r[t] at an episode end), V the recorded
        `value` -- one azul_lambda_returns_ring launch per window and part over the steps the buffers hold (min(ring * window, played); the
        window kernels then write no returns themselves, the move-by-move path launches it in place of azul_discounted_returns); lambda = 0
        is the one-step TD target.  A2CLearner forms returns - V itself, so the learner paths need no change.  Nothing flows into the newest
        step unless bootstrap_tail; the values of a ring's older windows were recorded under older weights and are used as recorded; a step
        recorded without an action (action -1) carries the critic's value of its observation like any other (every path writes it), the scan
        makes no exception.  Flat self-play (opponent=None) raises ValueError: consecutive records there belong to different seats observed
        with PERSP_CURRENT, so V[t+1] would be another seat's value.  Like gamma, lambda is baked into a captured graph.
        `bootstrap_tail=True` (ring 1, any opponent but None; gae_lambda then defaults to 1.0): after the window's moves the critic's value
        of slot T -- the state after the window -- is computed by PyTorch on the part's stream from the weights the kernels read (one GEMM
        pair per window), kept in the trajectory dict as "tail_value" [N] and handed to the scan, where it flows into the newest step: every
        step of the window then has a proper target at once, episodes still open included (n-step A2C:
        A2CLearner.update_from_windows(traj, complete_only=False)).  A ring of two or more windows trains whole episodes, nothing is open
        there: ValueError."""
        self._check_modes(policy, n_games, parts, rules, window, use_graph, fused_head, opponent, fused_mlp, persistent, action_selection, ring,
                          opponent_selection, opponent_trace, move_limit, players, fused_wide, fused_opponent, wide_ring, fused_seats,
                          gae_lambda, bootstrap_tail, opponent_playouts, opponent_playout_policy, opponent_playout_explore)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.policy = policy.to(self.device).eval()
        self.windows_played = 0
        self.sample_seed = L.POLICY_ARGMAX if action_selection == "Max" else int(sample_seed)
        self.game_id_base = int(seed_base if game_id_base is None else game_id_base) & 0xFFFFFFFF
        self.opponent_seed = L.POLICY_ARGMAX if opponent_selection == "Max" else \
            (int(opponent_seed) if opponent_seed is not None else (int(sample_seed) ^ 0x4F50504F4E454E54)) & 0xFFFFFFFFFFFFFFFF
        if _pairs is not None:       # arena.Arena's first seats, checked there: the league's row decided, its entry's _arena twin is launched
            self.window_entry = self.window_entry.replace("_league", "_arena")
        self.envs, self.streams, self.work, self.traj, self.graphs, self.rings = [], [], [], [], [], []
        self._stage_weights(kweights, _pairs)
        for p in range(parts):
            self._alloc_part(p, rules, seed_base, move_limit)
        torch.cuda.synchronize(self.device)
        self.graph_error = None
        if self.use_graph:
            try:
                self._capture()
            except Exception as e:          # capture is a launch-overhead optimisation only
                self.graph_error = repr(e)
                self.graphs = []
                self.use_graph = False
                torch.cuda.synchronize(self.device)

    def _check_modes(self, policy, n_games, parts, rules, window, use_graph, fused_head, opponent, fused_mlp, persistent, action_selection, ring,
                     opponent_selection, opponent_trace, move_limit, players, fused_wide, fused_opponent, wide_ring, fused_seats=False,
                     gae_lambda=None, bootstrap_tail=False, opponent_playouts=8, opponent_playout_policy="uniform", opponent_playout_explore=0):
        """Every refusal of the constructor, then the resolution of the modes -- from the arguments and the modules' shapes alone: no device
        and no library call, so nothing is allocated before a refusal.  Three facts come out: the record family (`wide`), who answers
        opponent_move() (`opponent`, one of the kinds below) and what plays a window (`window_entry`: a row of _WINDOW_KERNELS, or None for
        the move-by-move path); the other flags restate them."""
        assert n_games % parts == 0
        self.n, self.parts, self.h, self.T = n_games, parts, n_games // parts, window
        self.players = int(players)
        self.wide = self.players != 2 or parse_ext_rules(rules, self.players) != 0
        # None | "random" | "net" | "league" | "greedy" | "greedy_margin" | "playout"
        kind = opponent if opponent is None or isinstance(opponent, str) else ("league" if isinstance(opponent, (list, tuple)) else "net")
        members = list(opponent) if kind == "league" else ([opponent] if kind == "net" else [])      # the network opponents, one or a pool
        netopp = kind in ("net", "league")
        n_obs, n_act = batch_shape(self.players, rules)          # azul_batch_obs_size / azul_batch_num_actions
        # (a kind the assert below turns away is checked as self-play until then)
        row = _WINDOW_KERNELS.get((self.wide, kind), _WINDOW_KERNELS[self.wide, None])
        compiled_for = (n_obs, n_obs, row.hidden, row.hidden, n_act)
        # -- the refusals, in the order in which they win
        if kind == "league":
            if not 1 <= len(members) <= 255:
                raise ValueError("a league is a pool of 1..255 network opponents (a group's member is one byte), got %d" % len(members))
            if any(isinstance(m, str) or m is None for m in members):
                raise ValueError("the members of a league are modules with the reference's four layers, not opponent kinds")
            if any(_layer_sizes(m) != _layer_sizes(members[0]) for m in members):
                raise ValueError("the members of a league must have ONE shape (their weights are stacked array by array), got %s"
                                 % sorted(set(_layer_sizes(m) for m in members)))
        for net in (members if self.wide else []):                # (every member of a pool: the refusals of a single network opponent)
            shape = (net.critic_linear1.in_features, net.actor_linear1.in_features, net.actor_linear2.out_features)
            if shape != (n_obs, n_obs, n_act):
                raise ValueError("a network opponent for batches of %d players / extended rules must take the batch's observation and give its "
                                 "actions: ActorCritic(%d, %d, any hidden size), got inputs %d / %d and %d actions"
                                 % (self.players, n_obs, n_act, shape[0], shape[1], shape[2]))
        if kind == "greedy" and self.wide:
            raise ValueError("opponent=\"greedy\" maximises the two-player reward of game_runner.py:48-50: two-player reference batches only, "
                             "not %d players / extended rules (their scripted opponent is opponent=\"greedy_margin\")" % self.players)
        if kind == "greedy_margin" and not self.wide:
            raise ValueError("opponent=\"greedy_margin\" maximises the margin over the best other seat on batches of three / four players or "
                             "extended rules; a two-player reference batch has opponent=\"greedy\"")
        if kind == "playout":
            if self.wide or fused_wide or fused_opponent:
                raise ValueError("opponent=\"playout\" answers per cut (one azul_batch_playout_moves launch per reply round) on two-player "
                                 "reference batches: no wide batch (%d players / extended rules), no fused_wide=True, no fused_opponent=True -- "
                                 "no window kernel plays it" % self.players)
            if opponent_selection == "Max":
                raise ValueError("opponent_selection=\"Max\" has no meaning for opponent=\"playout\": the player takes the maximal playout sum, "
                                 "there is no distribution")
            if not 1 <= int(opponent_playouts) <= L.PLAYOUTS_MAX:
                raise ValueError("opponent_playouts must be in 1 .. %d, got %r" % (L.PLAYOUTS_MAX, opponent_playouts))
            if opponent_playout_policy not in L.PLAYOUT_POLICIES:
                raise ValueError("opponent_playout_policy must be \"uniform\" or \"greedy\", got %r" % (opponent_playout_policy,))
            if isinstance(opponent_playout_explore, bool) or not isinstance(opponent_playout_explore, int) or not 0 <= opponent_playout_explore <= 255:
                raise ValueError("opponent_playout_explore must be an integer in 0 .. 255, got %r" % (opponent_playout_explore,))
            if opponent_playout_explore and opponent_playout_policy == "uniform":
                raise ValueError("opponent_playout_explore=%d has no meaning with opponent_playout_policy=\"uniform\" (every ply of it is "
                                 "uniform): it must be 0" % opponent_playout_explore)
        if fused_seats:
            if kind != "greedy_margin":
                raise ValueError("fused_seats=True plays the greedy_margin seats of a wide batch inside its window kernel: it needs "
                                 "opponent=\"greedy_margin\" (three / four players or extended rules)")
            if fused_opponent:
                raise ValueError("fused_seats=True has no opponent network: fused_opponent=True is the network opponent's switch (or the "
                                 "two-player opponent=\"greedy\")")
            if not fused_wide:
                raise ValueError("fused_seats=True answers inside the wide window kernel: it needs fused_wide=True")
        elif kind == "greedy_margin" and (fused_wide or fused_opponent):
            raise ValueError("opponent=\"greedy_margin\" answers on the per-cut path (one azul_batch_mp_score_moves launch per reply round): "
                             "the wide window kernel does not play it (fused_wide=False, fused_opponent=False) unless fused_seats=True asks "
                             "for it (with fused_wide=True)")
        if self.wide and move_limit:
            raise ValueError("no move limit for batches of three / four players or extended rules")
        if fused_wide:
            if not self.wide:
                raise ValueError("fused_wide=True is the window kernel of batches of three / four players or extended rules; two-player reference "
                                 "batches have persistent=True")
            if netopp and not fused_opponent:
                raise ValueError("fused_wide=True plays opponent=None or \"random\"; a network opponent runs on the per-cut path (fused_wide=False)")
            if not fused_head:
                raise ValueError("fused_wide=True samples with azul_policy_head_n's draw: fused_head=False is the PyTorch sampling path")
            if _layer_sizes(policy) != compiled_for:
                raise ValueError("fused_wide=True is compiled for ActorCritic(%d, %d, hidden 180) on this batch, got inputs %d / %d, hidden %d / %d "
                                 "and %d actions" % ((n_obs, n_act) + _layer_sizes(policy)))
        if int(wide_ring) < 1:
            raise ValueError("wide_ring must be >= 1")
        if int(wide_ring) >= 2 and (not fused_wide or parts != 1):
            raise ValueError("wide_ring >= 2 is the trajectory ring of the wide window kernel: it needs fused_wide=True and parts=1")
        if fused_opponent and kind == "greedy":                  # (wide batches were refused above)
            if _layer_sizes(policy) != compiled_for or not (fused_mlp and fused_head):
                raise ValueError("fused_opponent=True with opponent=\"greedy\" plays inside the two-player window kernel, compiled for "
                                 "ActorCritic(136, 180, hidden 180) -- shape (136, 180, 180) -- with fused_mlp and fused_head; got inputs %d / %d, "
                                 "hidden %d / %d and %d actions; other policies play the greedy opponent on the per-cut path "
                                 "(fused_opponent=False)" % _layer_sizes(policy))
        elif fused_opponent:
            if not fused_wide or not netopp:
                raise ValueError("fused_opponent=True plays a network opponent inside the window kernel of wide batches: it needs fused_wide=True "
                                 "and opponent=<module> (or opponent=\"greedy\" on a two-player reference batch)")
            hidden = [(net.critic_linear1.out_features, net.actor_linear1.out_features) for net in members]
            if any(hd != (row.opp_hidden, row.opp_hidden) for hd in hidden):
                raise ValueError("fused_opponent=True is compiled for an opponent of hidden size 180, got %d / %d; other opponents run on the "
                                 "per-cut path (fused_opponent=False, fused_wide=False)"
                                 % [hd for hd in hidden if hd != (row.opp_hidden, row.opp_hidden)][0])
        lam = None if gae_lambda is None else float(gae_lambda)
        if lam is not None and not 0.0 <= lam <= 1.0:            # (a NaN fails the comparison too)
            raise ValueError("gae_lambda must lie in [0, 1] (1: the Monte-Carlo return, 0: the one-step TD target), got %r" % (gae_lambda,))
        if kind is None and (bootstrap_tail or (lam is not None and lam < 1.0)):
            raise ValueError("gae_lambda < 1 and bootstrap_tail need the records of ONE seat (any opponent but None): consecutive records of "
                             "flat self-play belong to different seats observed with PERSP_CURRENT, so V(s_{t+1}) is another seat's value")
        assert kind in (None, "random", "net", "league", "greedy", "greedy_margin", "playout")
        # -- the resolution
        self.opponent, self.opp_policy = kind, (members[0] if kind == "net" else None)
        self.netopp, self.league = netopp, kind == "league"    # a network answers (one net, or a pool of them: opp_pool)
        self.opp_pool = members if self.league else None
        self.scripted = kind in ("greedy", "greedy_margin", "playout")     # answers are env.greedy_action's / playout_action's: no weights, no log-probabilities
        self.opponent_playouts = int(opponent_playouts) if kind == "playout" else 0
        self.opponent_playout_policy = opponent_playout_policy if kind == "playout" else "uniform"
        self.opponent_playout_explore = int(opponent_playout_explore) if kind == "playout" else 0
        self.cut = netopp or self.scripted                     # GameRunner.step cut at its opponent_move() calls (BatchedAzul.net_*)
        self.fused_head = fused_head
        # the one-launch forward (azul_policy_forward) is compiled for the reference's ActorCritic(136, 180, hidden 180)
        self.fused_mlp = bool(fused_mlp and fused_head and not self.wide and policy.critic_linear1.in_features == L.OBS_SIZE and
                              policy.critic_linear1.out_features == 180 and policy.actor_linear2.out_features == L.NUM_ACTIONS)
        asked = {"persistent": persistent and self.fused_mlp, "fused_wide": fused_wide, "fused_opponent": fused_opponent, "fused_seats": fused_seats}
        # the whole window in ONE launch per part; same results (no window kernel plays the playout opponent)
        self.window_entry = row.entry if asked[row.switch] and kind != "playout" else None
        self.fused_wide, self.fused_opponent, self.fused_seats = bool(fused_wide), bool(fused_opponent), bool(fused_seats)
        self.fused_greedy = self.fused_opponent and kind == "greedy"
        self.persistent = self.window_entry is not None and not self.wide
        self.ring = (int(wide_ring) if self.wide else int(ring)) if self.window_entry else 1
        assert self.ring >= 1
        if bootstrap_tail and self.ring >= 2:                    # (the last refusal: it needs the resolved ring; still nothing allocated)
            raise ValueError("bootstrap_tail=True gives the open episodes of ONE window a target; a ring of %d windows trains whole episodes, "
                             "nothing is open there (ring=1 / wide_ring=1)" % self.ring)
        # None: the Monte-Carlo return and the launches of a rollout without these switches; a float: azul_lambda_returns_ring writes `returns`
        self.bootstrap_tail = bool(bootstrap_tail)
        self.gae_lambda = (1.0 if lam is None else lam) if (self.bootstrap_tail or (lam is not None and lam < 1.0)) else None
        # Agent.get_ac_output's two modes (agent.py:64-72): sample from the masked softmax, or take its first maximum
        assert action_selection in ("Distribution", "Max") and (fused_head or action_selection == "Distribution")
        self.action_selection = action_selection
        assert opponent_selection in ("Distribution", "Max")
        self.opp_slots = int(opponent_trace) if self.cut else 0
        assert not netopp or self.fused_mlp or self.wide, \
            "the network opponent runs on the library's forward (ActorCritic(136, 180, hidden 180))"
        # one launch per window needs no graph; reply rounds are data-dependent (a capture that fails clears the flag again)
        self.use_graph = bool(use_graph and self.window_entry is None and not self.cut)

    def _stage_weights(self, kweights, seats=None):
        """The k-major weight copies the kernels and GEMMs read.  kweights: tensors owned by someone else (A2CLearner.kweights(): views of
        its flat master copy, kept current by the optimiser kernel) -- then nothing is copied here and refresh_weights() has nothing to do.
        A network opponent's pool is seated here, before the parts open their games (`seats`: an arena's first pairs; a league: the default)."""
        if self.wide and self.window_entry is None:
            kweights = None                                # (the PyTorch-GEMM path keeps its own copies)
        self._external_kweights = kweights is not None
        self.H = self.policy.critic_linear1.out_features
        if kweights is not None:
            self.w1t, self.b1, self.w2c, self.w2a_t = kweights["w1t"], kweights["b1"], kweights["w2c"], kweights["w2a_t"]
            self.w2c_t = self.w2c.view(-1, 1)
        self.refresh_weights()
        if self.opponent == "net":
            self.opp_policy = self.opp_policy.to(self.device).eval()
            self.pool = NetPool([self.opp_policy], self.device, self.envs, self.streams)
        elif self.league:
            if seats is None:                                  # the default assignment: group i -> member i % K, for every part
                G = (self.h + L.LEAGUE_GROUP_GAMES - 1) // L.LEAGUE_GROUP_GAMES
                seats = (torch.arange(G, dtype=torch.int64) % len(self.opp_pool)).repeat(self.parts, 1).numpy()
            self.pool = NetPool(self.opp_pool, self.device, self.envs, self.streams, seats, self.h)
            self.opp_pool = None                               # (the weights are copied: the modules are not kept)

    def _alloc_part(self, p, rules, seed_base, move_limit):
        """Part p: its games (opened as GameRunner opens them), its stream, its trajectory ring and work buffers."""
        d, h, T = self.device, self.h, self.T
        env = MultiplayerAzul(h, rules=rules, device=d, players=self.players) if self.wide else BatchedAzul(h, rules=rules, device=d)
        env.seed(seed_base + p * h)                            # seeds follow the global game id
        env.set_id_base(self.game_id_base + p * h)             # ... and so does the sampler's Philox key
        if move_limit:
            env.set_move_limit(move_limit)
        env.runner_init()                                      # GameRunner()
        if self.opponent == "random":
            env.reset()                                        # GameRunner.reset(): the opponent opens when it starts
        elif self.opponent is None:
            env.runner_init()                                  # reset() without pre-moves (flat self-play)
        self.envs.append(env)                                  # (the network opponent opens below, once the work buffers exist)
        self.streams.append(torch.cuda.Stream(device=d))
        R = self.ring * T
        self.obs_size, self.num_actions = env.obs_size, env.num_actions
        rg = {"obs": torch.zeros(R + 1, h, env.obs_size, device=d), "mask": torch.zeros(R + 1, h, env.num_actions, dtype=torch.uint8, device=d),
              "player": torch.zeros(R + 1, h, dtype=torch.uint8, device=d),
              "action": torch.zeros(R, h, dtype=torch.int32, device=d), "reward": torch.zeros(R, h, dtype=torch.int32, device=d),
              "done": torch.zeros(R, h, dtype=torch.uint8, device=d),
              "value": torch.zeros(R, h, 1, device=d), "log_prob": torch.zeros(R, h, device=d), "entropy": torch.zeros(R, h, device=d),
              "returns": torch.zeros(R, h, device=d), "carry": torch.zeros(h, device=d)}
        if self.cut:
            rg["opp_replies"] = torch.zeros(R, h, dtype=torch.uint8, device=d)
            if self.opp_slots:
                rg["opp_action"] = torch.full((R, self.opp_slots, h), -1, dtype=torch.int32, device=d)
                rg["opp_logp"] = torch.zeros(R, self.opp_slots, h, device=d)
        self.rings.append(rg)
        t = self._window_views(rg, self.ring - 1)             # the "previous" window: its slot T seeds the first window
        w = {"hidden": torch.zeros(h, 2 * self.H, device=d), "logits": torch.zeros(h, env.num_actions, device=d),
             "status": torch.zeros(h, dtype=torch.uint8, device=d),
             "counter": torch.tensor([0, 0], dtype=torch.int64, device=d)}     # [0] Philox step counter, [1] launch ticket
        if self.cut:
            w["net"] = env.net_state()
            w["scratch_f"] = torch.zeros(3, h, device=d)       # the opponent forward's value / entropy (not recorded) and untraced log-prob
            if self.wide and self.netopp:                      # the opponent's actor half as PyTorch GEMMs (its own hidden size)
                w["opp_hidden"] = torch.zeros(h, self.ob1.shape[-1] // 2, device=d)
                w["opp_logits"] = torch.zeros(h, env.num_actions, device=d)
            if self.league:                                    # one member's answers before they are taken
                w["lg_action"], w["lg_logp"] = torch.zeros(h, dtype=torch.int32, device=d), torch.zeros(h, device=d)
        if self.bootstrap_tail:                                # the critic's value of slot T, and the hidden layer it is formed from
            w["tail_hidden"], w["tail_value"] = torch.zeros(h, self.H, device=d), torch.zeros(h, 1, device=d)
            t["tail_value"] = w["tail_value"].view(h)
        self.traj.append(t)
        self.work.append(w)
        self.streams[p].wait_stream(torch.cuda.current_stream(d))      # (the buffers above and the pool's seats were written there)
        with torch.cuda.stream(self.streams[p]):
            if self.cut:
                self._net_reset(p)                             # GameRunner.reset(): the network / greedy opponent opens when it starts
            env.observe_all(self._persp(), t["obs"][T], t["mask"][T], t["player"][T])     # becomes slot 0 of the first window

    def _window_views(self, rg, w):
        """Views of window `w` of a ring: T + 1 slots of obs / mask / player (slot T = the state after the window), T of the rest."""
        T = self.T
        lo = w * T
        out = {k: rg[k][lo:lo + T + 1] for k in ("obs", "mask", "player")}
        out.update({k: rg[k][lo:lo + T] for k in ("action", "reward", "done", "value", "log_prob", "entropy", "returns", "opp_replies", "opp_action",
                                                  "opp_logp") if k in rg})
        return out

    def _persp(self):
        return 0 if self.opponent is not None else L.PERSP_CURRENT     # with any opponent NNRunner observes with perspective 0 (game_runner.py:56)

    _OPP_ARRAYS, _kmajor = _OPP_ARRAYS, staticmethod(_kmajor)      # (pool.py's; the opponent's arrays are the attributes o + name, below the class)

    def _stage(self, get, names):
        """The policy's k-major copies `names` as attributes, updated IN PLACE once they exist: captured HIP graphs and whoever shares
        kweights() keep reading the same addresses."""
        with torch.no_grad():
            for k, v in _kmajor(get, names, self.device):
                if hasattr(self, k):
                    getattr(self, k).copy_(v)
                else:
                    setattr(self, k, v.clone())

    def set_opponent(self, policy_or_state_dict):
        """Install the network opponent's weights (k-major copies, updated IN PLACE): a module with the reference's four layers or its
        state_dict -- e.g. `ro.set_opponent(policy)` every so many updates trains against a frozen past self."""
        if self.league:
            self._need_league()                                # (an arena's own refusal)
            raise ValueError("this rollout plays a league: set_pool_member(i, ...) installs the weights of one member")
        if not self.netopp:
            raise ValueError("this rollout has no network opponent (opponent=<module>)")
        self.pool.set_member(0, policy_or_state_dict)

    # ---- the league (opponent=[net0, net1, ...]): a few lines each over the pool, whose seats are the assignment -----------------------
    pool_size = property(lambda self: self.pool.size if self.league else 0, doc="Members of the league's pool (0 without a league).")

    def _need_league(self):
        if not self.league:
            raise ValueError("this rollout plays no league (opponent=[net0, net1, ...])")

    def set_pool_member(self, i, policy_or_state_dict):
        """Install the weights of pool member i (its slice of the stacked k-major copies, updated IN PLACE like set_opponent): a module
        with the reference's four layers, of the pool's shape, or its state_dict."""
        self._need_league()
        self.pool.set_member(i, policy_or_state_dict)

    def assignment(self):
        """The pool member of every 16-game group: a uint8 array [parts][ceil(h / 16)] (a host copy)."""
        self._need_league()
        return self.pool.seats_host.copy()

    def set_assignment(self, members):
        """Assign the groups anew: an int array [parts][ceil(h / 16)] of pool members, refused if any value is >= pool_size.  The tally runs
        first, so that the episodes finished so far are booked to the members they were played against; then the array is copied IN PLACE
        on the parts' streams, behind the windows in flight."""
        self._need_league()
        self.pool.install(checked_seats(members, self.pool.seats_host.shape, self.pool.size, "assignment is", "[parts][ceil(h / 16)]", "assignment names"))

    def league_results(self, reset=False):
        """Per pool member what the games assigned to it finished since construction (or the last reset): a list of pool_size dicts with
        `episodes` and the means over them of the ten STAT_KEYS (win_percent among them; NaN without an episode).  Reduced on the device,
        in a fixed order: pool_size x 11 doubles per part cross to the host.  reset=True zeroes the results behind the read."""
        from .records import STAT_KEYS
        self._need_league()
        return [dict([("episodes", int(row[0]))] + [(k, float(row[1 + i]) / row[0] if row[0] else float("nan")) for i, k in enumerate(STAT_KEYS)])
                for row in self.pool.totals(reset)]

    def reset_member_results(self, i):
        """Zero the results of pool member i (what it finished so far is booked first and dropped with the rest)."""
        self._need_league()
        self.pool.tally()
        for p in range(self.parts):
            with torch.cuda.stream(self.streams[p]):
                self.pool.results[p, int(i)].zero_()

    def league_state(self):
        """What a checkpoint carries of the league besides the stacked weights (host copies): the assignment and NetPool.state()."""
        return dict(assignment=self.assignment(), **self.pool.state())

    def load_league_state(self, st):
        self._need_league()
        self.pool.load_state(st["assignment"], st["results"], st["marks"], st["counters"])

    def games_state(self):
        """Per part the games as a checkpoint carries them (host copies): records, MT19937 streams (`mt`, `pos`), the Philox step counter."""
        return [dict(zip(("mt", "pos"), env.get_rng_range()), records=env.get_records(), counter=w["counter"].cpu().numpy().copy())
                for env, w in zip(self.envs, self.work)]

    def load_games_state(self, games):
        for env, w, g in zip(self.envs, self.work, games):
            env.set_records(g["records"])
            env.set_rng_range(g["mt"], g["pos"])
            w["counter"].copy_(torch.from_numpy(g["counter"]))

    def _opp_forward(self, p, j, logp_out):
        """The opponent's get_a_output (agent.py:73-81) for the games of part p that owe an opponent_move(): forward_actor of its net on
        what net_step_* left in work["net"], reply j of the step sampled with Philox key opponent_seed + j at the step's counter."""
        w = self.work[p]
        net = w["net"]
        if self.opponent == "playout":
            # the flat Monte-Carlo player: reply j of a step draws with seed opponent_seed + j at the step's call (_env_step / _net_reset)
            self.envs[p].playout_action(self.opponent_playouts, (self.opponent_seed + j) & 0xFFFFFFFFFFFFFFFF, w["playout_call"],
                                        active=net["pending"], out=net["action"], policy=self.opponent_playout_policy,
                                        explore=self.opponent_playout_explore)
            return
        if self.scripted:
            # the scripted opponent: the best move of every game that owes one, from the mover's perspective (azul_batch_score_moves /
            # azul_batch_mp_score_moves)
            self.envs[p].greedy_action(active=net["pending"], out=net["action"])
            return
        key = self.opponent_seed if self.opponent_seed == L.POLICY_ARGMAX else (self.opponent_seed + j) & 0xFFFFFFFFFFFFFFFF
        present = self.pool.present(p)
        if len(present) == 1:                                  # a single opponent, or one member for the whole part: its answers are the answers
            return self._opp_forward_net(p, key, self.pool.member(present[0]), net["action"], logp_out)
        # the forward once per member present in the part's seats (all of the part's games through that member's weights), then per game
        # the answer of its group's member: exact, because the head draws per row by the game's global id
        for m in present:
            self._opp_forward_net(p, key, self.pool.member(m), w["lg_action"], w["lg_logp"])
            mine = self.pool.game_member[p] == m
            torch.where(mine, w["lg_action"], net["action"], out=net["action"])
            torch.where(mine, w["lg_logp"], logp_out, out=logp_out)

    def _opp_forward_net(self, p, key, weights, action_out, logp_out):
        """forward_actor + the sampling head of ONE opponent net (`weights`: its six k-major arrays) for all games of part p."""
        w = self.work[p]
        net, sc = w["net"], w["scratch_f"]
        ow1t, ob1, ow2c, ob2c, ow2a_t, ob2a = weights
        if self.wide:
            # forward_actor (model.py:28-41) on the mover-perspective observations net_step_* left; the head samples at the same counter as
            # the two-player path (counter_dev - 1: the value the agent's draw of this step used; before the first step, 2^64 - 1)
            Ho = w["opp_hidden"].shape[1]
            with torch.no_grad():
                torch.addmm(ob1[Ho:], net["obs"], ow1t[:, Ho:], out=w["opp_hidden"])
                w["opp_hidden"].relu_()
                torch.addmm(ob2a, w["opp_hidden"], ow2a_t, out=w["opp_logits"])
            L.check(L.lib.azul_policy_head_n(_p(w["opp_logits"]), _p(net["mask"]), key, 0xFFFFFFFFFFFFFFFF, _p(w["counter"]), self.h, self.num_actions,
                                             self.game_id_base + p * self.h, _p(action_out), _p(logp_out), _p(sc[1]),
                                             C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
            # a forward that is not finite has no distribution to sample (np.random.choice raises on NaN probabilities, agent.py:76):
            # its answer is -1, which the env refuses -- the game keeps owing the move and the bounded reply loop reports it
            action_out.masked_fill_(~torch.isfinite(w["opp_logits"].sum(dim=1)), -1)
            return
        L.check(L.lib.azul_policy_forward(_p(net["obs"]), _p(net["mask"]), _p(ow1t), _p(ob1), _p(ow2c), _p(ob2c), _p(ow2a_t),
                                          _p(ob2a), L.OBS_SIZE, self.H, L.NUM_ACTIONS, key, 0xFFFFFFFFFFFFFFFF, _p(w["counter"]), 0, self.h,
                                          self.game_id_base + p * self.h, _p(sc[0]), _p(action_out), _p(logp_out), _p(sc[1]), None,
                                          C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _net_reset(self, p):
        """GameRunner.reset() with the network opponent for every game of part p (game_runner.py:76-85); its opening moves draw at the
        counter before the first step."""
        w = self.work[p]
        if self.opponent == "playout":
            w["playout_call"] = (int(w["counter"][0].item()) - 1) & 0xFFFFFFFF
        self.envs[p].net_reset_begin(w["net"], w["status"])
        self._reply_rounds(p, "the opening of reset()", None, None)

    def _reply_rounds(self, p, where, reward, done, trace=None):
        """opponent_move() while any game of part p owes one: per round the opponent's answers, one net_step_reply launch and one host
        synchronisation (the loop condition).  `reward` / `done`: the step's slots (None for an opening); `trace`: the step's (opp_action,
        opp_logp) [R][N], whose first opp_slots rounds are recorded.  Wide and scripted opponents give up after MAX_REPLY_ROUNDS rounds."""
        env, w = self.envs[p], self.work[p]
        net = w["net"]
        j = 0
        while int(net["owing"].item()) > 0:
            if (self.wide or self.scripted) and j >= self.MAX_REPLY_ROUNDS:
                self._reply_loop_failed(p, j, where)
            traced = trace is not None and j < self.opp_slots
            self._opp_forward(p, j, trace[1][j] if traced else w["scratch_f"][2])
            if traced:
                trace[0][j].copy_(net["action"])
            env.net_step_reply(net["action"], net, reward, done, w["status"])
            j += 1

    def _reply_loop_failed(self, p, rounds, where):
        net = self.work[p]["net"]
        owing = torch.nonzero(net["pending"]).flatten().cpu().tolist()
        st = self.work[p]["status"].cpu()
        ids = [self.game_id_base + p * self.h + i for i in owing]
        raise RuntimeError("%s opponent: games %s (global ids) still owe an opponent_move() after %d reply rounds of %s (round %d); "
                           "statuses %s -- the opponent keeps answering with moves that are not legal (a forward that is not finite, or a "
                           "state with nothing legal, answers -1)"
                           % (("playout" if self.opponent == "playout" else "greedy") if self.scripted else "network", ids[:16], rounds, where, rounds, [int(st[i]) for i in owing[:16]]))

    def refresh_weights(self):
        """(Re)build the fused first-layer weights from the policy's parameters -- call after every optimiser step.  The
        staging tensors are updated IN PLACE: a captured HIP graph keeps reading the same addresses."""
        if not self._external_kweights:
            self._stage(self.policy.get_parameter, ("w1t", "b1", "w2c_t", "w2a_t", "w2c"))      # (the biases of layer 2 are read in place)

    def kweights(self):
        """The k-major weight copies (refresh_weights keeps them current): the learner's gradient kernel reads the same layouts."""
        return {"w1t": self.w1t, "b1": self.b1, "w2c": self.w2c, "w2a_t": self.w2a_t}

    def _buffers(self, tr, w, returns):
        """azul_rollout_buffers_t of a window's views; the opponent fields only with a network / greedy opponent (the trace only when asked for)."""
        net, trace = self.cut, self.opp_slots > 0           # (a window kernel with a cut protocol plays the opponent itself)
        ptr = lambda k: tr[k].data_ptr()
        return L.RolloutBuffers(ptr("obs"), ptr("mask"), ptr("player"), ptr("action"), ptr("reward"), ptr("done"), ptr("value"), ptr("log_prob"),
                                ptr("entropy"), w["status"].data_ptr(), returns, ptr("opp_action") if trace else None,
                                ptr("opp_logp") if trace else None, ptr("opp_replies") if net else None, self.opp_slots)

    def _head(self, p, t):
        """Masked softmax, draw, log-prob and entropy of move t from work["logits"]: azul_policy_head for the reference's 180 actions,
        azul_policy_head_n for a wide batch's; the step counter moves on behind it."""
        tr, w = self.traj[p], self.work[p]
        head = (_p(w["logits"]), _p(tr["mask"][t]), self.sample_seed, 0, _p(w["counter"]), self.h)
        tail = (self.game_id_base + p * self.h, _p(tr["action"][t]), _p(tr["log_prob"][t]), _p(tr["entropy"][t]),
                C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        L.check(L.lib.azul_policy_head_n(*head, self.num_actions, *tail) if self.wide else L.lib.azul_policy_head(*head, *tail))
        w["counter"][:1].add_(1)

    # one move of one part, enqueued on the current stream
    def _move(self, p, t):
        env, tr, w = self.envs[p], self.traj[p], self.work[p]
        obs, mask, H = tr["obs"][t], tr["mask"][t], self.H
        pol = self.policy
        if self.fused_mlp:                                  # whole forward + head: one launch on the f32 matrix cores
            L.check(L.lib.azul_policy_forward(_p(obs), _p(mask), _p(self.w1t), _p(self.b1), _p(self.w2c), _p(pol.critic_linear2.bias),
                                              _p(self.w2a_t), _p(pol.actor_linear2.bias), L.OBS_SIZE, H, L.NUM_ACTIONS,
                                              self.sample_seed, 0, _p(w["counter"]), 1, self.h, self.game_id_base + p * self.h,
                                              _p(tr["value"][t]), _p(tr["action"][t]),
                                              _p(tr["log_prob"][t]), _p(tr["entropy"][t]), None,
                                              C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
            self._env_step(p, t)
            return
        with torch.no_grad():
            torch.addmm(self.b1, obs, self.w1t, out=w["hidden"])
            w["hidden"].relu_()
            torch.addmm(pol.critic_linear2.bias, w["hidden"][:, :H], self.w2c_t, out=tr["value"][t])          # agent.py:66
            torch.addmm(pol.actor_linear2.bias, w["hidden"][:, H:], self.w2a_t, out=w["logits"])               # agent.py:67
            if self.fused_head:
                self._head(p, t)
            else:
                legal = mask.bool()
                logits = w["logits"].masked_fill(~legal, float("-inf"))
                logp = torch.log_softmax(logits, dim=1)
                any_legal = legal.any(dim=1)
                safe = torch.where(any_legal.unsqueeze(1), logp.exp(), torch.full_like(logp, 1.0 / logp.shape[1]))
                action = torch.multinomial(safe, 1).squeeze(1)                                               # agent.py:69
                tr["log_prob"][t].copy_(logp.gather(1, action.unsqueeze(1)).squeeze(1))                       # nn_runner.py:32
                tr["entropy"][t].copy_(-(torch.where(legal, logp, torch.zeros_like(logp)).sum(dim=1) / legal.sum(dim=1).clamp(min=1)))
                tr["action"][t].copy_(torch.where(any_legal, action, torch.full_like(action, -1)).to(torch.int32))
        self._env_step(p, t)

    def _env_step(self, p, t):
        env, tr, w = self.envs[p], self.traj[p], self.work[p]
        if self.cut:
            # GameRunner.step cut at its opponent_move() calls: the agent's move, then reply rounds while any game owes one (one host
            # synchronisation per round: this is the per-move reference structure, the window kernel is the fast path)
            net = w["net"]
            if self.opponent == "playout":
                w["playout_call"] = (w["playout_counter"] + t) & 0xFFFFFFFF
            env.net_step_begin(tr["action"][t], net, tr["reward"][t], tr["done"][t], w["status"])
            self._reply_rounds(p, "agent step %d of the window" % t, tr["reward"][t], tr["done"][t],
                               (tr["opp_action"][t], tr["opp_logp"][t]) if self.opp_slots else None)
            tr["opp_replies"][t].copy_(net["replies"])
            env.observe_all(0, tr["obs"][t + 1], tr["mask"][t + 1], tr["player"][t + 1])
        elif self.opponent == "random":
            env.agent_step(tr["action"][t], tr["reward"][t], tr["done"][t], w["status"], tr["obs"][t + 1], tr["mask"][t + 1], tr["player"][t + 1])
        else:
            env.policy_step(tr["action"][t], tr["reward"][t], tr["done"][t], w["status"], tr["obs"][t + 1], tr["mask"][t + 1], tr["player"][t + 1])

    def _window(self, p, gamma):
        if self.window_entry:
            self._window_kernel(p, gamma)
        else:
            self._window_moves(p, gamma)

    def _window_kernel(self, p, gamma):
        """The whole window of part p in one launch of `window_entry` (+ the returns scan behind it), the opponent inside.  The only place a
        window kernel is launched from.  The entries share one argument order (include/azul_hip.h); what differs is said where it is added."""
        T, env, w = self.T, self.envs[p], self.work[p]
        if self.ring > 1:
            self.traj[p] = self._window_views(self.rings[p], self.windows_played % self.ring)     # (run_window advances windows_played after all parts)
        tr = self.traj[p]
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        # (a ring, or a lambda-return: the scan below writes the returns)
        out = self._buffers(tr, w, tr["returns"].data_ptr() if self.ring == 1 and self.gae_lambda is None else None)
        vs, flat = self.netopp, self.window_entry == "azul_batch_policy_rollout_returns"
        seats = self.pool.seat_ptrs[p] if self.league else []                         # none: a single opponent; the opponent's: a league; both: an arena
        args = [env._h, T]
        if not self.cut:
            args.append(1 if self.opponent == "random" else 0)                  # opponent_random: the entries without reply rounds play both
        if len(seats) < 2:                                                      # (an arena's agent is a pool member: no weights of its own)
            pol = self.policy                                                   # (the second layer's biases straight from the module)
            wa = L.NetWeights(*[x.data_ptr() for x in (self.w1t, self.b1, self.w2c, pol.critic_linear2.bias, self.w2a_t, pol.actor_linear2.bias)])
            args += _WEIGHT_FIELDS(wa) if flat else [C.byref(wa)]               # (_returns takes the structs' pointers one by one)
        if vs:
            wo = self.pool.weights()
            args.append(C.byref(wo))                                            # the reply rounds run on the opponent's weights
        if seats:
            args += [self.pool.size] + seats                                    # ... of the pool member each 16-game group is seated with
        args += [self.obs_size, self.H, self.num_actions, self.sample_seed]
        if vs:
            args.append(self.opponent_seed)
        args += [0, _p(w["counter"])]
        if self.wide and self.cut:
            args.append(int(self.MAX_REPLY_ROUNDS))                             # max_replies: the wide kernels' bound on one step's reply rounds
        args += _FLAT_BUFFER_FIELDS(out) if flat else [C.byref(out)]
        L.check(getattr(L.lib, self.window_entry)(*args, C.c_float(gamma), st))
        if self.gae_lambda is not None:
            self._lambda_returns(p, gamma)
        elif self.ring > 1:
            # returns of the new window and, chained backwards through the ring, of the older windows: the value flowing out of a
            # window's first step flows into the window before it (nn_runner.py:70-76 across window boundaries) -- one launch
            rg, R, played = self.rings[p], self.ring * T, (self.windows_played + 1) * T
            L.check(L.lib.azul_discounted_returns_ring(_p(rg["reward"]), _p(rg["done"]), _p(rg["returns"]), C.c_float(gamma), R,
                                                       played % (1 << 40), min(R, played), self.h, st))

    def _lambda_returns(self, p, gamma):
        """The TD(lambda) returns of every step part p's buffers hold, on the current stream: one azul_lambda_returns_ring launch from the
        newest step backwards (a single window is a ring of its T slots) -- with bootstrap_tail behind the critic's forward on slot T (the
        two GEMMs of forward_critic, model.py:22-26, on the staged weights the kernels read), whose value flows into the newest step."""
        T, w = self.T, self.work[p]
        rg, R = self.rings[p], self.ring * T
        played = (self.windows_played + 1) * T if self.ring > 1 else T     # (run_window advances windows_played after all parts)
        tail = None
        if self.bootstrap_tail:
            H, tail = self.H, w["tail_value"]
            with torch.no_grad():
                torch.addmm(self.b1[:H], self.traj[p]["obs"][T], self.w1t[:, :H], out=w["tail_hidden"])
                w["tail_hidden"].relu_()
                torch.addmm(self.policy.critic_linear2.bias, w["tail_hidden"], self.w2c_t, out=tail)
        L.check(L.lib.azul_lambda_returns_ring(_p(rg["reward"]), _p(rg["done"]), _p(rg["value"]), None if tail is None else _p(tail),
                                               _p(rg["returns"]), C.c_float(gamma), C.c_float(self.gae_lambda), R, played % (1 << 40),
                                               min(R, played), self.h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _window_moves(self, p, gamma):
        """The window of part p move by move (what a HIP graph captures): slot T of the last window becomes slot 0, T moves, the returns scan."""
        T, tr = self.T, self.traj[p]
        if self.opponent == "playout":                   # the Philox step counter at the start of the window (one read: this path synchronises per reply round)
            self.work[p]["playout_counter"] = int(self.work[p]["counter"][0].item())
        tr["obs"][0].copy_(tr["obs"][T])
        tr["mask"][0].copy_(tr["mask"][T])
        tr["player"][0].copy_(tr["player"][T])
        for t in range(T):
            self._move(p, t)
        if self.gae_lambda is not None:
            return self._lambda_returns(p, gamma)
        L.check(L.lib.azul_discounted_returns(_p(tr["reward"]), _p(tr["done"]), _p(tr["returns"]), None, C.c_float(gamma), T, self.h,
                                              C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _capture(self, gamma=0.99):
        self.gamma = gamma
        for p in range(self.parts):
            s = self.streams[p]
            with torch.cuda.stream(s):
                self._window(p, gamma)                  # warm-up (lazy inits, allocator) outside capture; advances the games
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                self._window(p, gamma)
            self.graphs.append(g)
        torch.cuda.synchronize(self.device)

    def run_window(self, gamma=0.99, gae_lambda=None):
        """Advance every game by `window` moves; returns the per-part trajectory dicts (views into static buffers;
        `obs`, `mask`, `player` have T+1 slots: slot t is what the policy saw at move t).  `gae_lambda` is the constructor's: given here,
        it must name the same returns."""
        if self.use_graph and gamma != getattr(self, "gamma", gamma):
            raise ValueError("gamma is baked into the captured graph")
        if gae_lambda is not None and float(gae_lambda) != (1.0 if self.gae_lambda is None else self.gae_lambda):
            raise ValueError("gae_lambda is the constructor's (and baked into a captured graph): this rollout was built with %r"
                             % (1.0 if self.gae_lambda is None else self.gae_lambda))
        cur = torch.cuda.current_stream(self.device)
        for p in range(self.parts):
            self.streams[p].wait_stream(cur)             # e.g. the optimiser step / refresh_weights enqueued by the caller
            with torch.cuda.stream(self.streams[p]):
                if self.use_graph:
                    self.graphs[p].replay()
                else:
                    self._window(p, gamma)
        self.windows_played += 1
        return self.traj

    def join(self):
        """Make the caller's current stream wait for the window(s) in flight -- on the device, the host does not block."""
        cur = torch.cuda.current_stream(self.device)
        for s in self.streams:
            cur.wait_stream(s)

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def counters(self):
        c = [e.counters() for e in self.envs]
        return {"episodes": sum(int(x["episodes"].sum()) for x in c), "stuck": sum(int(x["stuck"].sum()) for x in c)}


for _k in _OPP_ARRAYS:       # ow1t .. ob2a, array k of the network opponent: member 0's view for a single opponent, the stack [K][...] for a league
    setattr(PolicyRollout, "o" + _k, property(lambda self, k=_k: self.pool.stacks[k] if self.league else self.pool.stacks[k][0]))
