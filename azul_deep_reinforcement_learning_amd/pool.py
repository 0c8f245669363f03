"""`NetPool`: what PolicyRollout holds whenever a network answers opponent_move() -- a single network opponent is a pool of one member
without seats, a league seats the opponent of every 16-game group, an arena both the agent and the opponent.  It hides the stacking layout
(the six k-major arrays of azul_net_weights_t, each [K][...], member m at m * size: include/azul_hip.h), the expansion of a group's byte
to its 16 games, and the book-keeping of finished episodes per member or per ordered pair (marks, results, the tally entries)."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

_OPP_ARRAYS = ("w1t", "b1", "w2c", "b2c", "w2a_t", "b2a")           # azul_net_weights_t, in its order


def _p(t):
    return C.c_void_p(t.data_ptr())


def _kmajor(get, names, device=None):
    """[(name, tensor)]: the k-major copies `names` of the reference's four layers (`get`: parameter name -> tensor), contiguous, on `device`."""
    with torch.no_grad():
        g = lambda k: get(k).detach().to(device=device, dtype=torch.float32)
        build = {"w1t": lambda: torch.cat([g("critic_linear1.weight"), g("actor_linear1.weight")], dim=0).t(),
                 "b1": lambda: torch.cat([g("critic_linear1.bias"), g("actor_linear1.bias")]),
                 "w2c": lambda: g("critic_linear2.weight").reshape(-1), "w2c_t": lambda: g("critic_linear2.weight").t(),
                 "b2c": lambda: g("critic_linear2.bias").reshape(-1),
                 "w2a_t": lambda: g("actor_linear2.weight").t(), "b2a": lambda: g("actor_linear2.bias")}
        return [(k, build[k]().contiguous()) for k in names]


def checked_seats(seats, shape, K, is_, dims, names):
    """The one validator of seats: an int array of exactly `shape` with values in 0..K-1, or ValueError in the caller's words."""
    a = np.asarray(seats)
    if a.shape != tuple(shape) or a.dtype.kind not in "iu":
        raise ValueError("the %s an int array of shape %s = %s, got %s %s" % (is_, dims, tuple(shape), a.dtype, a.shape))
    if a.size and (int(a.min()) < 0 or int(a.max()) >= K):
        raise ValueError("the %s pool members 0..%d, got values in %d..%d" % (names, K - 1, int(a.min()), int(a.max())))
    return a


class NetPool:
    def __init__(self, nets, device, envs, streams, seats=None, h=0):
        """`nets`: K modules of one shape (their weights are copied); `envs`, `streams`: the rollout's lists of parts, which it fills.
        `seats`: None (every game plays member 0), ints [parts][G], the opponent member of every group (a league), or [parts][G][2], agent
        and opponent (an arena), G = ceil(h / 16): on the host in the caller's shape, on the device one byte column [G] per part and role.
        With them: the opponent member of every game, the results [parts][K][11] / [parts][K][K][11] (episodes, ten statistic sums) and
        the marks, the per-game counters at the last tally (zero, like the counters of a new batch)."""
        self.device, self.size, self.envs, self.streams, self.seats_host, self.h = device, len(nets), envs, streams, seats, h
        staged = [dict(_kmajor(m.state_dict().__getitem__, _OPP_ARRAYS, device)) for m in nets]
        self.stacks = {k: torch.stack([st[k] for st in staged]).contiguous() for k in _OPP_ARRAYS}
        if seats is not None:
            self.seats_host = np.ascontiguousarray(seats, dtype=np.uint8)
            self.seats = torch.stack([self._columns(p) for p in range(len(seats))])
            self.game_member = torch.stack([self._games_of(p) for p in range(len(seats))])
            self.seat_ptrs = [[_p(col) for col in part] for part in self.seats]      # per part one pointer per role, as the entries take them
            self.results = torch.zeros((len(seats),) + (self.size,) * self.seats.shape[1] + (1 + L.NUM_STATS,), dtype=torch.float64, device=device)
            self.marks = [{"episodes": torch.zeros(h, dtype=torch.int64, device=device),
                           "stat_sums": torch.zeros(h, L.NUM_STATS, dtype=torch.float64, device=device)} for _ in seats]

    def member(self, m):
        """The six arrays of member m (views of the stacks, in azul_net_weights_t's order)."""
        return [self.stacks[k][m] for k in _OPP_ARRAYS]

    def weights(self):
        """azul_net_weights_t of the stacks: member 0's arrays for a pool of one, the base of every member's for the pool kernels."""
        return L.NetWeights(*[self.stacks[k].data_ptr() for k in _OPP_ARRAYS])

    def set_member(self, i, policy_or_state_dict):
        """Install the weights of member i IN PLACE (the kernels keep reading the same addresses): a module or its state_dict."""
        if not 0 <= int(i) < self.size:
            raise ValueError("pool member %r outside 0..%d" % (i, self.size - 1))
        sd = policy_or_state_dict.state_dict() if hasattr(policy_or_state_dict, "state_dict") else policy_or_state_dict
        with torch.no_grad():
            for k, v in _kmajor(sd.__getitem__, _OPP_ARRAYS, self.device):
                self.stacks[k][int(i)].copy_(v)

    def _columns(self, p):
        """Part p's seats as the entries take them: one contiguous byte column [G] per role, the opponent's last (from the host copy)."""
        return torch.from_numpy(np.ascontiguousarray(self.seats_host[p].reshape(self.seats_host.shape[1], -1).T)).to(self.device)

    def _games_of(self, p):
        """The opponent member of every game of part p: its group's byte, repeated for the group's 16 games, cut to h."""
        return self.seats[p, -1].to(torch.int64).repeat_interleave(L.LEAGUE_GROUP_GAMES)[:self.h]

    def present(self, p):
        """The members that answer in part p, ascending."""
        return [0] if self.seats_host is None else sorted(set(self.seats_host[p].reshape(-1, self.seats.shape[1])[:, -1].tolist()))

    def install(self, seats):
        """Seat the groups anew (checked by the caller).  The tally runs first, so that the episodes finished so far are booked to the
        seats they were played with; then the bytes are copied IN PLACE on the parts' streams, behind the windows in flight."""
        self.tally()
        self.seats_host = np.ascontiguousarray(seats, dtype=np.uint8)
        for p, s in enumerate(self.streams):
            with torch.cuda.stream(s):
                self.seats[p].copy_(self._columns(p))
                self.game_member[p].copy_(self._games_of(p))

    def tally(self):
        """azul_league_tally / azul_arena_tally per part on its stream: what the groups finished since the marks goes to the results; the marks move up."""
        entry = L.lib.azul_league_tally if self.seats.shape[1] == 1 else L.lib.azul_arena_tally
        for p, (env, s) in enumerate(zip(self.envs, self.streams)):
            with torch.cuda.stream(s):
                c, mk = env.counters_dev(), self.marks[p]
                L.check(entry(_p(c["episodes"]), _p(c["stat_sums"]), _p(mk["episodes"]), _p(mk["stat_sums"]), *self.seat_ptrs[p], self.h,
                              self.size, _p(self.results[p]), C.c_void_p(s.cuda_stream)))

    def totals(self, reset=False):
        """The results so far, [K][11] or [K][K][11] float64 on the host (the parts added in part order); reset=True zeroes them behind the read."""
        self.tally()
        torch.cuda.synchronize(self.device)
        tot = self.results.cpu().numpy().sum(axis=0)
        if reset:
            self.results.zero_()
        return tot

    def state(self):
        """Host copies of the results, their marks and the per-game counters the marks refer to (the callers add the seats).  The counters
        travel because percent_first_player is not a whole number: the results are sums of counter - mark, exact only with the same counters."""
        torch.cuda.synchronize(self.device)
        return {"results": self.results.cpu(), "marks": [{k: v.cpu() for k, v in mk.items()} for mk in self.marks],
                "counters": [{k: v.cpu() for k, v in env.counters_dev().items() if k != "keys"} for env in self.envs]}

    def load_state(self, seats, results, marks, counters):
        self.install(seats)                                    # (its tally books into the results and marks that are overwritten below)
        torch.cuda.synchronize(self.device)
        for p, env in enumerate(self.envs):
            for dst, src in ((env.counters_dev(), counters[p]), (self.marks[p], marks[p])):
                for k, v in src.items():
                    dst[k].copy_(v)
        self.results.copy_(results)
        torch.cuda.synchronize(self.device)
