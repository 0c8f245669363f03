"""MultiplayerAzul: GameRunner for batches of three / four players and extended-rule batches (wide records) on one MI355X.

The reference's GameRunner (azulnet/game_runner.py:23-97) on an Azul(players=P): the agent is seat 0 ("player 1"), every other seat
replies with its own RandomAgent draw from the game's stream.  Each method is one launch of azul_x_runner_kernel through the
azul_batch_mp_* entries of the C ABI (include/azul_hip.h).  With a network opponent (GameRunner(opponent=Agent(...)), game_runner.py:27-30)
the net_step_begin / net_step_reply / net_reset_begin cuts (azul_x_net_kernel, azul_batch_mp_net_*) hand every opponent_move() of every
other seat to the caller: PolicyRollout(players=P, opponent=<module>) answers them with the opponent's forward.  The shaped reward is the one departure from the reference, BEYOND THE
REFERENCE for P > 2: phi = s[0] - max_{j>0} s[j] after count_score() on a copy of the game (game_runner.py:48-50), reward = phi - phi_stored;
at P = 2 it is the reference's score[0] - score[1].  Plain BatchedAzul keeps refusing these calls for wide batches.
"""
import torch

from . import _lib as L
from .batch import BatchedAzul, _ptr
from .records import runner_tail


class MultiplayerAzul(BatchedAzul):
    def __init__(self, n_games, rules={"first_player": "Random", "tile_pool": "Lid"}, device=None, seed=None, players=3, ext_rules=None):
        super().__init__(n_games, rules=rules, device=device, seed=seed, players=players, ext_rules=ext_rules)
        if not self.wide:
            raise ValueError("MultiplayerAzul is for batches of three / four players or extended rules: BatchedAzul runs the two-player GameRunner")

    def _status(self):
        return torch.zeros(self.n, dtype=torch.uint8, device=self.device)

    def runner_init(self, active=None):
        """GameRunner.__init__ (game_runner.py:23-36): Azul(players=P, rules) + new_round(), player_score = move_counter = 0."""
        st = self._status()
        L.check(L.lib.azul_batch_mp_runner_init(self._h, _ptr(self._dev(active, torch.uint8)), _ptr(st), self._stream()))
        return st

    def reset(self, active=None):
        """GameRunner.reset (game_runner.py:76-85): a fresh game, then the other seats move while current_player != 1."""
        st = self._status()
        L.check(L.lib.azul_batch_mp_runner_reset(self._h, _ptr(self._dev(active, torch.uint8)), _ptr(st), self._stream()))
        return st

    def step(self, actions, active=None):
        """GameRunner.step (game_runner.py:43-55) for every game -> (reward int32[N], done bool[N], status uint8[N])."""
        a = self._dev(actions, torch.int32)
        reward = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        done = torch.zeros(self.n, dtype=torch.uint8, device=self.device)
        st = self._status()
        L.check(L.lib.azul_batch_mp_runner_step(self._h, _ptr(a), _ptr(self._dev(active, torch.uint8)), _ptr(reward), _ptr(done), _ptr(st),
                                                self._stream()))
        return reward, done.bool(), st

    def score_preview(self):
        """phi of the current state for every game (int32[N])."""
        p = self._new((self.n,), torch.int32)
        L.check(L.lib.azul_batch_mp_score_preview(self._h, _ptr(p), self._stream()))
        return p

    def score_moves(self, perspective=L.PERSP_MOVER, active=None, scores=None, best=None):
        """The one-ply table of the reward above in one launch (azul_batch_mp_score_moves), the games untouched: scores [N][num_actions]
        int32, for every legal action s[p] - max_{j != p} s[j] after move + count_score on a copy of the game (p = `perspective`: a seat
        0 .. P-1, or PERSP_MOVER, the seat to move; at p = 0 phi of the moved copy; beyond the reference for P > 2), L.SCORE_ILLEGAL
        elsewhere; best [N] int32, the first legal action with the maximal score (-1: nothing is legal).  `scores` / `best`: preallocated
        device tensors to write into; rows of games whose `active` is 0 are not written (fresh outputs start as SCORE_ILLEGAL / -1).
        Returns (scores, best)."""
        if scores is None:
            scores = torch.full((self.n, self.num_actions), L.SCORE_ILLEGAL, dtype=torch.int32, device=self.device)
        if best is None:
            best = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
        L.check(L.lib.azul_batch_mp_score_moves(self._h, int(perspective), _ptr(self._dev(active, torch.uint8)), _ptr(scores), _ptr(best),
                                                self._stream()))
        return scores, best

    def greedy_action(self, active=None, out=None):
        """The one-ply greedy seat of that reward: for every game the move that maximises the mover's margin over the best other seat
        after move + count_score (score_moves' `best` from the mover's perspective; -1: nothing is legal).  `out`: a preallocated int32 [N]."""
        best = torch.full((self.n,), -1, dtype=torch.int32, device=self.device) if out is None else out
        L.check(L.lib.azul_batch_mp_score_moves(self._h, L.PERSP_MOVER, _ptr(self._dev(active, torch.uint8)), None, _ptr(best), self._stream()))
        return best

    def observe_all(self, perspective=L.PERSP_MOVER, obs=None, mask=None, player=None):
        return super().observe_all(perspective, obs, mask, player)

    def policy_step(self, actions, reward, done, status, obs_next, mask_next, player_next, perspective=L.PERSP_MOVER, active=None):
        """One env move for the player to move with caller-chosen actions (the policy plays every seat): per-move reward (delta of the
        seat-0 potential), done, statistics and auto-reset, then the next observation (from the mover), mask and player."""
        L.check(L.lib.azul_batch_mp_policy_step(self._h, _ptr(actions), _ptr(self._dev(active, torch.uint8)), _ptr(reward), _ptr(done),
                                                _ptr(status), int(perspective), _ptr(obs_next), _ptr(mask_next), _ptr(player_next),
                                                self._stream()))

    def agent_step(self, actions, reward, done, status, obs_next, mask_next, player_next=None, perspective=0, active=None):
        """One AGENT step of NNRunner.run_episode: GameRunner.step incl. the replies, at the end of an episode its statistics and
        GameRunner.reset() with the opening replies, then the next decision's observation / mask / player (preallocated tensors)."""
        L.check(L.lib.azul_batch_mp_agent_step(self._h, _ptr(actions), _ptr(self._dev(active, torch.uint8)), _ptr(reward), _ptr(done),
                                               _ptr(status), int(perspective), _ptr(obs_next), _ptr(mask_next), _ptr(player_next),
                                               self._stream()))

    # -- GameRunner(opponent=<network>) for P seats, cut at its opponent_move() calls (game_runner.py:27-30, 37-47, 84-85): the protocol of
    # BatchedAzul.net_* on azul_batch_mp_net_*; net_state() sizes obs / mask by obs_size / num_actions.  Every seat other than seat 0 is the
    # opponent; what it is handed is the mover-perspective observation and the legal mask, written for the games that owe a move.
    def net_step_begin(self, actions, net, reward, done, status):
        """The agent's move of GameRunner.step (game_runner.py:44-45) for every game, then the loop condition (:46)."""
        L.check(L.lib.azul_batch_mp_net_step_begin(self._h, _ptr(actions), _ptr(net["pending"]), _ptr(net["replies"]), _ptr(reward), _ptr(done),
                                                   _ptr(status), _ptr(net["obs"]), _ptr(net["mask"]), _ptr(net["owing"]), self._stream()))

    def net_step_reply(self, opp_actions, net, reward, done, status):
        """One opponent_move() (game_runner.py:37-42) with `opp_actions` for every game that owes one, then the loop condition again."""
        L.check(L.lib.azul_batch_mp_net_step_reply(self._h, _ptr(opp_actions), _ptr(net["pending"]), _ptr(net["replies"]), _ptr(reward),
                                                   _ptr(done), _ptr(status), _ptr(net["obs"]), _ptr(net["mask"]), _ptr(net["owing"]),
                                                   self._stream()))

    def net_reset_begin(self, net, status, active=None):
        """GameRunner.reset() (game_runner.py:76-85) up to its first opponent_move()."""
        L.check(L.lib.azul_batch_mp_net_reset_begin(self._h, _ptr(self._dev(active, torch.uint8)), _ptr(net["pending"]), _ptr(status),
                                                    _ptr(net["obs"]), _ptr(net["mask"]), _ptr(net["owing"]), self._stream()))

    def runner_counters(self, first=0, count=None):
        """GameRunner.player_score (the stored potential) and move_counter of every game: (int16[N], uint16[N]) read from the records."""
        return runner_tail(self.get_records(first, count))
