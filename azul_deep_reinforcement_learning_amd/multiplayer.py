"""MultiplayerAzul: GameRunner for batches of three / four players and extended-rule batches (wide records) on one MI355X.

The reference's GameRunner (azulnet/game_runner.py:23-97) on an Azul(players=P): the agent is seat 0 ("player 1"), every other seat
replies with its own RandomAgent draw from the game's stream.  Each method is one launch of azul_x_runner_kernel through the
azul_batch_mp_* entries of the C ABI (include/azul_hip.h).  With a network opponent (GameRunner(opponent=Agent(...)), game_runner.py:27-30)
the net_step_begin / net_step_reply / net_reset_begin cuts (azul_x_net_kernel, azul_batch_mp_net_*) hand every opponent_move() of every
other seat to the caller: PolicyRollout(players=P, opponent=<module>) answers them with the opponent's forward.  The shaped reward is the one departure from the reference, BEYOND THE
REFERENCE for P > 2: phi = s[0] - max_{j>0} s[j] after count_score() on a copy of the game (game_runner.py:48-50), reward = phi - phi_stored;
at P = 2 it is the reference's score[0] - score[1].  Plain BatchedAzul keeps refusing these calls for wide batches.
"""
from . import _lib as L
from .batch import BatchedAzul
from .records import runner_tail


class MultiplayerAzul(BatchedAzul):
    """BatchedAzul's GameRunner and net-protocol methods on the azul_batch_mp_* entries; what the P-seat family means by them:
        runner_init            Azul(players=P, rules) + new_round(), player_score = move_counter = 0
        reset / step           the other seats move while current_player != 1; the reward is the margin above
        score_preview          phi of the current state
        score_moves            for every legal action s[p] - max_{j != p} s[j] after move + count_score on a copy of the game (p = `perspective`:
                               a seat 0 .. P-1, or PERSP_MOVER -- the default -- the seat to move; at p = 0 phi of the moved copy; beyond the
                               reference for P > 2), [N][num_actions]
        greedy_action          the one-ply greedy seat of that reward: the move that maximises the MOVER's margin over the best other seat
        policy_step            the per-move reward is the delta of the seat-0 potential; the next observation is the mover's (PERSP_MOVER)
        net_*                  the protocol of BatchedAzul.net_*; net_state() sizes obs / mask by obs_size / num_actions.  Every seat other than
                               seat 0 is the opponent; what it is handed is the mover-perspective observation and the legal mask, written for
                               the games that owe a move."""
    ENTRY_PREFIX = "azul_batch_mp_"
    PERSP_TO_MOVE = L.PERSP_MOVER

    def __init__(self, n_games, rules={"first_player": "Random", "tile_pool": "Lid"}, device=None, seed=None, players=3, ext_rules=None):
        super().__init__(n_games, rules=rules, device=device, seed=seed, players=players, ext_rules=ext_rules)
        if not self.wide:
            raise ValueError("MultiplayerAzul is for batches of three / four players or extended rules: BatchedAzul runs the two-player GameRunner")

    def runner_counters(self, first=0, count=None):
        """GameRunner.player_score (the stored potential) and move_counter of every game: (int16[N], uint16[N]) read from the records."""
        return runner_tail(self.get_records(first, count))
