"""TEST-ONLY: the P-player GameRunner with an EXTERNAL opponent (azul_batch_mp_net_* / azx::net_body_x), composed from the oracle's primitives
on top of tests/mp_runner_model.MPRunner: the opponents' loop asks for each opponent_move() (game_runner.py:37-42) instead of drawing
oz_random_agent_x, and GameRunner.step / reset are cut at those calls into the device's three-state protocol (azul_env2.hpp NET_*):

    net_begin(a)    the agent's move (:44-45), then the loop condition
    net_reply(a)    one opponent_move() with answer a, for a game that owes one, then the loop condition again
    net_reset()     GameRunner.reset() (:76-85) up to its first opponent_move()

`opp_view()` is what opponent_move() hands the opponent: get_state(perspective = mover) (:38), the legal mask and the player to move.
`step_with(a, answer)` / `reset_with(answer)` run the cuts to the end with a callback answer(obs, mask, player) -> action.  Pinned to the
reference by tests/golden/runner_players_net.npz (tests/test_mp_net_model.py)."""
import numpy as np

from tests.mp_runner_model import BAD_ACTION, GAME_ENDED, ILLEGAL_MOVE, OK, STUCK, MPRunner

READY, REPLY, OPENING, RESET = 0, 1, 2, 3


class MPNetRunner(MPRunner):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.pending, self.replies, self.rew, self.dn, self.closed, self.st = READY, 0, 0, 0, False, OK
        self.closed_game = None          # a copy of the game when the last agent step closed (before the next episode opens)

    def mover(self):
        return (self.g.current_player - 1) % self.P

    def opp_view(self):
        return self.obs(self.mover()).astype(np.float32), self.mask(), int(self.g.current_player)

    def settle(self):
        """az2::net_settle2 for P seats: the loop conditions of opponent_loop (:46 / :84), closing the step, opening the next episode."""
        for _ in range(4):
            if self.pending == RESET:
                st2 = self.restart()
                if not self.st:
                    self.st = st2
                self.pending = READY if st2 else OPENING
                continue
            if self.pending == READY:
                break
            legal = int(self.mask().sum())
            cur = self.g.current_player
            if self.pending == REPLY:
                keep = (cur != 1 or legal < 2) and not self.over()
                if keep and legal:
                    break
                self.closed = True
                if keep:                                     # nobody can move
                    self.stuck += 1
                    self.dn, self.rew = 2, 0
                    if not self.st:
                        self.st = STUCK
                else:
                    phi = self.potential()
                    self.rew = phi - self.phi
                    self.phi = phi
                    self.dn = int(self.over())
                    if self.dn:
                        self.episode_stats()
                self.closed_game = self.g.__class__.from_buffer_copy(bytes(self.g))
                self.pending = RESET if self.dn else READY
                if not self.dn:
                    break
            else:
                if cur != 1 and legal:
                    break
                if cur != 1 and not self.st:
                    self.st = STUCK
                self.pending = READY
                break

    def move(self, a, agent):
        if agent:
            self.pending, self.replies, self.rew, self.dn, self.closed, self.st = READY, 0, 0, int(self.over()), False, OK
        st = self.azul_step(int(a))
        if st == OK:
            self.moves += 1
            if agent:
                self.pending = REPLY
            else:
                self.replies += 1
        else:
            if not self.st:
                self.st = st
            if st in (ILLEGAL_MOVE, BAD_ACTION):             # game and debt untouched
                if agent:
                    self.closed = True
                return st
            in_step = agent or self.pending == REPLY
            self.pending = READY
            if in_step:
                self.closed, self.rew = True, 0
                self.dn = 1 if st == GAME_ENDED else (self.dn if agent else 0)
                if self.dn:
                    self.pending = RESET
        self.settle()
        return st

    def net_begin(self, a):
        return self.move(a, True)

    def net_reply(self, a):
        if self.pending == READY:
            return None
        return self.move(a, False)

    def net_reset(self):
        self.pending, self.replies, self.rew, self.dn, self.closed, self.st = RESET, 0, 0, 0, False, OK
        self.settle()

    def step_with(self, a, answer, rounds=4096):
        """One agent step to its end: (status, reward, done, replies)."""
        self.net_begin(a)
        for _ in range(rounds):
            if self.pending == READY:
                break
            self.net_reply(answer(*self.opp_view()))
        assert self.pending == READY, "the opponent's loop did not end"
        return self.st, self.rew, self.dn, self.replies

    def reset_with(self, answer, rounds=4096):
        self.net_reset()
        for _ in range(rounds):
            if self.pending == READY:
                break
            self.net_reply(answer(*self.opp_view()))
        assert self.pending == READY
        return self.st

