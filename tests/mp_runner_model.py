"""TEST-ONLY: GameRunner for P players (azul_batch_mp_* / azx::runner_body_x) composed from the oracle's primitives -- oz_init_ext + oz_new_round
(Azul(players=P, rules) + new_round()), oz_step (Azul.step), oz_count_score on a STRUCT COPY (deepcopy(game).count_score()),
oz_check_all_valid_x (check_all_valid), oz_random_agent_x (RandomAgent.get_a_output), oz_get_state_x (get_state) -- statement for statement
as azulnet/game_runner.py:23-97 writes GameRunner, with the one departure the device makes BEYOND THE REFERENCE for P > 2: the potential is
phi = s[0] - max_{j>0} s[j] (at P = 2 the reference's s[0] - s[1]).  Pinned to the reference by tests/golden/runner_players.npz and, at P = 2,
to oz_runner_step / oz_runner_reset."""
import ctypes as C

import numpy as np

from oracle import oracle as oz

OK, ILLEGAL_MOVE, GAME_ENDED, STUCK, BAD_ACTION, BOX_EMPTY = 0, 1, 2, 3, 4, 5
GUARD = 4096          # replies per opponent loop before the slot counts as stuck (az2::opponent_loop2's guard)


class MPRunner:
    """One game slot of a wide batch: the game, its CPython stream, the runner's player_score / move_counter and the slot's counters."""

    two = False            # record() packs the wide record

    def __init__(self, players, first_player, tile_pool, ext=0, seed=None, rng=None):
        self.P, self.first, self.pool, self.ext = players, first_player, tile_pool, ext
        self.g = oz.Game()
        if rng is not None:
            self.r = rng
        else:
            self.r = oz.seeded_rng(seed)
        self.L = oz.lib()
        self.phi = 0
        self.moves = 0
        self.episodes = 0
        self.stuck = 0
        self.stat_sum = np.zeros(10)

    @classmethod
    def from_record(cls, rec, cfg, rng, first_player=oz.FIRST_RANDOM):
        """A slot that holds a handed-in record (tests/domain_records.py: cfg = (players, ext, tile_pool); rng: the slot's stream, e.g.
        domain_records.stream_of) instead of a fresh game: the wide 256-byte record (oz.unpack_np; the runner tail from bytes 228..231) or,
        at P = 2, the 128-byte record (oz.unpack(...).game; player_score / move_counter are its tail) -- record() then packs that record."""
        P, ext, pool = cfg
        m = cls(P, first_player, pool, ext, rng=rng)
        raw = np.frombuffer(np.asarray(rec).tobytes(), np.uint8)
        m.two = raw.size == 128
        if m.two:
            assert P == 2 and ext == 0
            q = oz.unpack(raw, pool, first_player)
            m.g = oz.Game.from_buffer_copy(bytes(q.game))
            m.phi, m.moves = int(q.player_score), int(q.move_counter)
        else:
            m.g = oz.unpack_np(raw, pool, ext)
            m.phi, m.moves = int(raw[228:230].view("<i2")[0]), int(raw[230:232].view("<u2")[0])
        return m

    # -- primitives ------------------------------------------------------------------------------------------------
    @property
    def na(self):
        return self.L.oz_num_actions(C.byref(self.g))

    def mask(self):
        return oz.check_all_valid_x(self.g)

    def obs(self, perspective=0):
        return oz.get_state_x(self.g, perspective)

    def over(self):
        return bool(self.L.oz_is_end_of_game(C.byref(self.g)))

    def scores(self):
        return [int(self.g.score[p]) for p in range(self.P)]

    def whatif_scores(self):
        """deepcopy(game).count_score(); .score (game_runner.py:48-49)"""
        copy = oz.Game.from_buffer_copy(bytes(self.g))
        self.L.oz_count_score(C.byref(copy))
        return [int(copy.score[p]) for p in range(self.P)]

    def potential(self):
        s = self.whatif_scores()
        return s[0] - max(s[1:])

    def azul_step(self, a):
        """Azul.step with the device's status order: finished game, action out of range, illegal move (state untouched)."""
        if self.g.end_of_game:
            return GAME_ENDED
        if a < 0 or a >= self.na:
            return BAD_ACTION
        d, c, p = C.c_int(), C.c_int(), C.c_int()
        self.L.oz_deserialize_x(C.byref(self.g), int(a), C.byref(d), C.byref(c), C.byref(p))
        return self.L.oz_step(C.byref(self.g), d.value, c.value, p.value, C.byref(self.r))

    def restart(self):
        """Azul(players=P, rules) + new_round(), player_score = move_counter = 0 (game_runner.py:23-36, 79-82)"""
        self.phi = 0
        self.moves = 0
        st = self.L.oz_init_ext(C.byref(self.g), self.P, self.first, self.pool, self.ext, C.byref(self.r))
        return st if st else self.L.oz_new_round(C.byref(self.g), C.byref(self.r))

    def opponent_loop(self, opening):
        for _ in range(GUARD):
            m = self.mask()
            n = int(m.sum())
            keep = (self.g.current_player != 1) if opening else ((self.g.current_player != 1 or n < 2) and not self.over())
            if not keep:
                return OK
            if n == 0:
                return STUCK
            if self.g.end_of_game:
                return GAME_ENDED
            a = self.L.oz_random_agent_x(m.ctypes.data_as(C.POINTER(C.c_uint8)), len(m), C.byref(self.r))      # :97
            st = self.azul_step(a)
            if st:
                return st
            self.moves += 1                                                                                      # :42
        return STUCK

    def episode_stats(self):
        s = np.zeros(10)
        self.L.oz_get_statistics(C.byref(self.g), s.ctypes.data_as(C.POINTER(C.c_double)))
        self.stat_sum = self.stat_sum + s
        self.episodes += 1

    # -- the runner ---------------------------------------------------------------------------------------------------
    def runner_init(self):
        return self.restart()

    def reset(self):
        st = self.restart()
        return st if st else self.opponent_loop(True)

    def step(self, a):
        """GameRunner.step (game_runner.py:43-55) -> (status, reward, done)"""
        rew, dn = 0, int(self.over())
        st = self.azul_step(a)
        if not st:
            self.moves += 1
            st = self.opponent_loop(False)
            if not st:
                phi = self.potential()
                rew = phi - self.phi
                self.phi = phi
                dn = int(self.over())
        return st, rew, dn

    def runner_step(self, a):
        """azul_batch_mp_runner_step: GameRunner.step, statistics of a finished game, stuck counted"""
        st, rew, dn = self.step(a)
        if not st and dn:
            self.episode_stats()
        if st == STUCK:
            self.stuck += 1
        return st, rew, dn

    def agent_step(self, a):
        st, rew, dn = self.step(a)
        dirty = st not in (ILLEGAL_MOVE, BAD_ACTION)
        if st == STUCK:
            self.stuck += 1
            dn, rew = 2, 0
        elif st == GAME_ENDED:
            dn = 1
        elif st == OK and dn:
            self.episode_stats()
        if dirty and dn:
            st2 = self.reset()
            if st == OK:
                st = st2
        return st, rew, dn

    def policy_step(self, a):
        rew, dn = 0, 0
        stuck = a < 0 and not self.g.end_of_game and int(self.mask().sum()) == 0
        st, restart = OK, False
        if not stuck:
            st = self.azul_step(a)
            if st not in (ILLEGAL_MOVE, GAME_ENDED, BAD_ACTION):
                self.moves += 1
                phi = self.potential()
                rew = phi - self.phi
                self.phi = phi
                dn = int(self.over())
                restart = bool(dn) and st == OK
            elif st == GAME_ENDED:
                dn, restart = 1, True
        if stuck or restart:
            if stuck:
                self.stuck += 1
                dn = 2
            elif st == OK:
                self.episode_stats()
            st0 = self.restart()
            st = (st0 if st0 else STUCK) if stuck else st0
        return st, rew, dn

    # -- what the device holds ------------------------------------------------------------------------------------
    def record(self):
        """The 256-byte wide record + the runner's tail (bytes 228..229 i16 player_score, 230..231 u16 move_counter)."""
        if self.two:       # (from_record on a 128-byte record: oz.pack of a Runner that carries the model's game and tail)
            q = oz.Runner()
            q.game = oz.Game.from_buffer_copy(bytes(self.g))
            q.first_player, q.tile_pool, q.player_score, q.move_counter = self.first, self.pool, self.phi, self.moves & 0xFFFF
            return np.frombuffer(oz.pack(q).tobytes(), np.uint8).copy()
        rec = np.zeros(256, np.uint8)
        assert self.L.oz_pack_np(C.byref(self.g), rec.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        rec[228:230] = np.array([self.phi], "<i2").view(np.uint8)
        rec[230:232] = np.array([self.moves & 0xFFFF], "<u2").view(np.uint8)
        return rec

    def rng_state(self):
        return np.ctypeslib.as_array(self.r.mt).copy(), int(self.r.idx)
