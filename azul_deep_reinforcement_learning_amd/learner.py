"""A2C learner for batched rollouts: the reference's ``Agent.update`` (azulnet/agent.py:39-62) and the batch assembly of
``NNRunner.train`` (azulnet/nn_runner.py:57-79), restated for whole trajectory windows and for data-parallel ranks.

Loss, exactly as the reference writes it (agent.py:45-58), over the n samples of a batch:
    advantage    = qvals - values
    actor_loss   = mean(-log_prob(action) * advantage)          (advantage NOT detached, like the reference)
    critic_loss  = mean(advantage^2)
    entropy_loss = mean(-mean(log p over legal actions))        (nn_runner.py:36-40; coefficient +0.1, sic)
    ac_loss      = 1 * actor_loss + 0.5 * critic_loss + 0.1 * entropy_loss
then one Adam step (lr 3e-4).  The reference evaluates the network once per agent step while it plays and keeps the autograd
graph; here the rollout runs without autograd and the learner re-evaluates the network on the recorded (observation, mask,
action) samples in one batched forward, which yields the same values, log-probabilities and gradients.

Data parallel (one process per GPU): every rank holds the samples of its own games; the loss terms are SUMS over the local
samples divided by the GLOBAL sample count, and gradients are summed over ranks (one flat all-reduce over RCCL), so the
update equals the single-process update on the union of all ranks' samples whatever the per-rank counts are.
"""
import collections

import torch
import torch.distributed as dist
import torch.nn.functional as F

ACTOR_COEFF, CRITIC_COEFF, ENTROPY_COEFF = 1.0, 0.5, 0.1        # agent.py:47-49


def complete_episode_samples(done):
    """[T, N] done flags of a window -> bool [T, N]: the steps whose episode ENDS inside the window, i.e. whose discounted
    return (nn_runner.py:70-76) is exact without bootstrapping.  Steps after a game's last `done` belong to an episode that
    ends in a LATER window: with a single-window rollout they are never trained (the next window overwrites the buffers) --
    A2CLearner.update_from_rollout on a PolicyRollout(ring >= 2) keeps them and trains them when their episode ends."""
    d = done != 0
    return torch.flip(torch.cummax(torch.flip(d, dims=[0]).to(torch.uint8), dim=0).values, dims=[0]).bool()


REFERENCE_SHAPE = (136, 180, 180)                                 # (num_inputs, hidden, num_actions)
# the wide batches' ActorCritic(obs_size, num_actions, hidden 180): three / four players on five displays, three on seven, four on nine
WIDE_SHAPES = ((188, 180, 180), (240, 180, 180), (198, 180, 240), (260, 180, 300))


def flat_layout(num_inputs, hidden, num_actions):
    """Offsets (start, length) of the flat k-major layout of azul_a2c_gradients / azul_a2c_flat_size:
    w1t [IN][2H] | b1 [2H] | w2c [H] | b2c [1] | pad | w2a_t [H][A] | b2a [A]; "size" = the float count (parameters + 1 pad)."""
    h2 = 2 * hidden
    b1 = num_inputs * h2
    w2c = b1 + h2
    b2c = w2c + hidden
    w2a = b2c + 2
    b2a = w2a + hidden * num_actions
    return {"w1t": (0, b1), "b1": (b1, h2), "w2c": (w2c, hidden), "b2c": (b2c, 1), "w2a_t": (w2a, hidden * num_actions),
            "b2a": (b2a, num_actions), "size": b2a + num_actions}


def _policy_shape(pol):
    if not (hasattr(pol, "critic_linear1") and hasattr(pol, "actor_linear1")):
        return None
    return (pol.critic_linear1.in_features, pol.critic_linear1.out_features, pol.actor_linear2.out_features)


class A2CLearner:
    def __init__(self, policy, learning_rate=3e-4, gamma=0.99, process_group=None, distributed=None, fused=None, stat_history=4096):
        """fused=True: gradients from the hand-written kernel azul_a2c_gradients (forward + backward on the f32 matrix cores, one
        launch + a deterministic reduction) and Adam from azul_a2c_apply_adam_n instead of PyTorch autograd and torch.optim; needs CUDA
        tensors and a compiled network shape: the reference's ActorCritic(136, 180, 180) or one of the wide batches' WIDE_SHAPES
        (ActorCritic(obs_size, num_actions, hidden 180) of three / four players on 5 displays, three on 7, four on 9) -- any other shape raises ValueError.
        Default (fused=None): fused for the reference's shape only."""
        self.policy = policy
        self.fused = fused
        shape = _policy_shape(policy)
        if fused is True and shape != REFERENCE_SHAPE and shape not in WIDE_SHAPES:
            raise ValueError("fused=True is compiled for ActorCritic (num_inputs, hidden, num_actions) in %s, got %s"
                             % ((REFERENCE_SHAPE,) + WIDE_SHAPES, shape))
        self.shape = shape
        self.layout = flat_layout(*shape) if shape is not None else None
        self._ws = None
        self.gamma = gamma
        self.optimizer = self._own_adam = torch.optim.Adam(policy.parameters(), lr=learning_rate)        # agent.py:37
        self.fused_apply = True           # the fused path steps with azul_a2c_apply_adam_n while `optimizer` is the learner's own Adam
        self.group = process_group
        self.distributed = (dist.is_available() and dist.is_initialized()) if distributed is None else distributed
        # the last updates' loss terms (device scalars; bounded: the reference keeps one float per logged batch, agent.py:19-24)
        self.statistics = {k: collections.deque(maxlen=stat_history) for k in ("actor_loss", "critic_loss", "entropy_loss", "ac_loss", "samples")}
        self.updates = 0                  # optimiser steps requested so far (statistics entries ever appended)
        self.dropped_steps = None         # device int32[2] of update_from_rollout: [samples of the last update, steps lost from the ring]

    def loss_terms(self, obs, mask, action, qvals, weight=None, n_total=None):
        """obs [n,136] f32, mask [n,180] bool/u8, action [n] int, qvals [n] -> the four loss terms of agent.py:51-57.
        `weight` [n] (0/1) drops samples without changing shapes; `n_total` is the divisor (default: the local count)."""
        legal = mask.bool()
        values, logp = self._values_logp(obs, legal)
        log_prob = logp.gather(1, action.long().clamp(min=0).unsqueeze(1)).squeeze(1)                 # nn_runner.py:32
        entropy = -(torch.where(legal, logp, torch.zeros_like(logp)).sum(dim=1) / legal.sum(dim=1).clamp(min=1))   # :36-40
        advantage = qvals.to(values.dtype) - values
        w = torch.ones_like(values) if weight is None else weight.to(values.dtype)
        n = w.sum() if n_total is None else n_total
        # a window without a finished episode has no sample: the sums are 0, and so are the terms (the fused path's rule), not 0 / 0
        n = n.clamp(min=1.0) if torch.is_tensor(n) else max(float(n), 1.0)
        actor_loss = (-log_prob * advantage * w).sum() / n
        critic_loss = (advantage.pow(2) * w).sum() / n
        entropy_loss = (entropy * w).sum() / n
        ac_loss = ACTOR_COEFF * actor_loss + CRITIC_COEFF * critic_loss + ENTROPY_COEFF * entropy_loss
        return actor_loss, critic_loss, entropy_loss, ac_loss

    def _values_logp(self, obs, legal):
        """The network on a batch with autograd: values [n], masked log-probabilities [n, A] (-inf where illegal)."""
        pol = self.policy
        if hasattr(pol, "critic_linear1") and hasattr(pol, "actor_linear1"):
            # same arithmetic as forward_critic / forward_actor (model.py:22-41) with both first layers in ONE GEMM (and one
            # weight-gradient GEMM in the backward pass): autograd splits the concatenated gradient back onto the two modules
            H = pol.critic_linear1.out_features
            w1 = torch.cat([pol.critic_linear1.weight, pol.actor_linear1.weight], dim=0)
            b1 = torch.cat([pol.critic_linear1.bias, pol.actor_linear1.bias])
            hidden = F.relu(F.linear(obs, w1, b1))
            values = pol.critic_linear2(hidden[:, :H]).squeeze(1)
            logits = pol.actor_linear2(hidden[:, H:]).masked_fill(~legal, float("-inf"))
            logp = F.log_softmax(logits, dim=1)
        else:
            values = pol.forward_critic(obs).squeeze(1)
            _, logp = pol.forward_actor(obs, legal)
        return values, logp

    # ---- hand-written gradient / optimiser path -------------------------------------------------------------------------
    # One flat k-major vector holds the master copy of the parameters (layout of azul_a2c_gradients' gradient; flat_layout()):
    #     w1t [136][360] | b1 [360] | w2c [180] | b2c [1] | pad | w2a_t [180][180] | b2a [180]      (IN inputs / A actions when wide)
    # the policy / rollout kernels read views of it (kweights()), Adam's two moments use the same layout, and
    # azul_a2c_apply_adam_n writes every step into the flat copy AND into the eight nn.Linear tensors of the module.

    def _can_fuse(self, obs):
        pol = self.policy
        return obs.is_cuda and _policy_shape(pol) == REFERENCE_SHAPE and pol.actor_linear1.out_features == REFERENCE_SHAPE[1]

    def _use_fused(self, obs):
        """fused=None: the reference's shape only (today's default); fused=True: any compiled shape (checked at construction)."""
        return self._can_fuse(obs) if self.fused is None else bool(self.fused)

    def _ensure_flat(self, dev):
        if self._ws is None or self._ws["flat"].device != dev:
            n = self.layout["size"]
            self._ws = {"ws": torch.empty(256, n + 4, device=dev), "grad": torch.empty(n + 4, device=dev), "flat": torch.zeros(n, device=dev),
                        "m": torch.zeros(n, device=dev), "v": torch.zeros(n, device=dev),
                        "step": torch.zeros(1, dtype=torch.int32, device=dev)}        # Adam's step counter lives on the device
            self.sync_from_module()
        return self._ws

    def sync_from_module(self):
        """(Re)build the flat k-major master copy from the module's parameters (after load_state_dict or any outside edit)."""
        if self._ws is None:
            return
        pol, f = self.policy, self._ws["flat"]
        v = self._views(f)
        with torch.no_grad():
            v["w1t"].copy_(torch.cat([pol.critic_linear1.weight, pol.actor_linear1.weight], dim=0).t())
            v["b1"].copy_(torch.cat([pol.critic_linear1.bias, pol.actor_linear1.bias]))
            v["w2c"].copy_(pol.critic_linear2.weight.reshape(-1))
            v["b2c"].copy_(pol.critic_linear2.bias)
            v["w2a_t"].copy_(pol.actor_linear2.weight.t())
            v["b2a"].copy_(pol.actor_linear2.bias)

    def _views(self, f):
        """Views of a flat vector (parameters, gradient or moments) in the kernels' layouts."""
        IN, H, A = self.shape
        lay = self.layout
        v = {k: f[on[0]:on[0] + on[1]] for k, on in lay.items() if k != "size"}
        v["w1t"] = v["w1t"].view(IN, 2 * H)
        v["w2a_t"] = v["w2a_t"].view(H, A)
        return v

    def kweights(self, device=None):
        """Views of the flat master copy in the layouts the policy kernels read (None when the fused path is unavailable)."""
        dev = device if device is not None else next(self.policy.parameters()).device
        if torch.device(dev).type != "cuda" or self.fused is False or (self.fused is None and not self._can_fuse(next(self.policy.parameters()))):
            return None
        return self._views(self._ensure_flat(torch.device(dev))["flat"])

    def optimizer_state(self):
        """What a checkpoint needs: torch's Adam state, plus the fused path's moments and step when it is in use."""
        st = {"torch": self.optimizer.state_dict()}
        if self._ws is not None:
            st["fused"] = {"m": self._ws["m"].cpu(), "v": self._ws["v"].cpu(), "step": int(self._ws["step"].item())}
        return st

    def load_optimizer_state(self, st):
        self.optimizer.load_state_dict(st["torch"])
        if "fused" in st:
            ws = self._ensure_flat(next(self.policy.parameters()).device)
            ws["m"].copy_(st["fused"]["m"])
            ws["v"].copy_(st["fused"]["v"])
            ws["step"].fill_(int(st["fused"]["step"]))
        self.sync_from_module()

    def _fused_gradients(self, obs, mask, action, qvals, n_total=None, index=None, count=None, kweights=None, countf=None):
        """The flat gradient from azul_a2c_gradients (summed over the ranks); returns what _finish_fused needs: (n_dev, n_host) -- the
        global sample count as a device float[1] or as a host number.  Either `n_total` (host number; all rows are samples) or
        `index` + `count` (device selection of rows; `countf` = [count, 1 / max(count, 1)] as floats when the selection kernel
        already wrote them: single-process runs then need no arithmetic outside the kernels, no host round trip either way)."""
        import ctypes as C
        from . import _lib as L
        pol, dev = self.policy, obs.device
        ws = self._ensure_flat(dev)
        kw = self.kweights(dev)
        with torch.no_grad():
            obs = obs.contiguous().float()
            mask = mask.contiguous().to(torch.uint8)
            action = action.contiguous().to(torch.int32)
            qvals = qvals.contiguous().float()
            p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
            inv_dev = None
            if index is not None and countf is not None and not self.distributed:
                n_dev, inv_dev, inv_host = countf[0:1], countf[1:2], 1.0
            elif index is not None:
                n_dev = count.to(torch.float32)
                if self.distributed:
                    dist.all_reduce(n_dev, group=self.group)
                inv_dev = (1.0 / n_dev.clamp(min=1.0)).contiguous()
                inv_host = 1.0
            else:
                n_dev = None
                inv_host = 1.0 / float(n_total)
            L.check(L.lib.azul_a2c_gradients(p(obs), p(mask), p(action), p(qvals), int(obs.shape[0]), C.c_float(inv_host),
                                             p(kw["w1t"]), p(kw["b1"]), p(kw["w2c"]), p(kw["b2c"]), p(kw["w2a_t"]), p(kw["b2a"]),
                                             p(pol.actor_linear2.weight), *self.shape, p(ws["ws"]), 256, p(ws["grad"]), p(index), p(count),
                                             p(inv_dev), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            g = ws["grad"]
            if self.distributed:
                dist.all_reduce(g, group=self.group)                       # one flat bucket
        return (n_dev, None) if index is not None else (None, float(n_total))

    def _record(self, out):
        for k2, v in out.items():
            self.statistics[k2].append(v)
        self.updates += 1
        return out

    def _stat_slot(self):
        """Row of the statistics ring that the next update's loss terms go to (written by the optimiser kernel itself)."""
        ws = self._ws
        if "stats" not in ws:
            ws["stats"] = torch.zeros(self.statistics["ac_loss"].maxlen, 5, device=ws["grad"].device)
        return ws["stats"][self.updates % ws["stats"].shape[0]]

    def _finish_fused(self, n_dev, n_host):
        """Optimiser step: azul_a2c_apply_adam_n on the flat copy + module (the learner's own Adam), or -- when the caller installed
        another optimiser -- the flat gradient scattered into the parameters' .grad and that optimiser's step.  The update's loss
        terms (agent.py:51-58) are written by the same kernel into a row of a device-resident ring: no small launches follow."""
        import ctypes as C
        from . import _lib as L
        pol, ws = self.policy, self._ws
        g = ws["grad"]
        dev = g.device
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        row = self._stat_slot()
        if self.optimizer is self._own_adam and self.fused_apply:
            grp = self.optimizer.param_groups[0]
            # the step counter and the "any samples at all?" test stay on the device: an update without samples (a window in which
            # no episode ended) leaves parameters, moments and step untouched
            hp = (C.c_float(grp["lr"]), C.c_float(grp["betas"][0]), C.c_float(grp["betas"][1]), C.c_float(grp["eps"]), 0)
            mod = (p(pol.critic_linear1.weight), p(pol.critic_linear1.bias), p(pol.critic_linear2.weight), p(pol.critic_linear2.bias),
                   p(pol.actor_linear1.weight), p(pol.actor_linear1.bias), p(pol.actor_linear2.weight), p(pol.actor_linear2.bias))
            tail = (p(ws["step"]), p(n_dev), C.c_float(n_host or 0.0), p(row), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            L.check(L.lib.azul_a2c_apply_adam_n(p(g), p(ws["flat"]), p(ws["m"]), p(ws["v"]), *hp, *self.shape, *mod, *tail))
        else:
            with torch.no_grad():
                gv = self._views(g)
                gw1, gb1, H = gv["w1t"], gv["b1"], self.shape[1]
                pairs = [(pol.critic_linear1.weight, gw1[:, :H].t()), (pol.actor_linear1.weight, gw1[:, H:].t()),
                         (pol.critic_linear1.bias, gb1[:H]), (pol.actor_linear1.bias, gb1[H:]),
                         (pol.critic_linear2.weight, gv["w2c"].view(1, H)), (pol.critic_linear2.bias, gv["b2c"]),
                         (pol.actor_linear2.weight, gv["w2a_t"].t()), (pol.actor_linear2.bias, gv["b2a"])]
                for prm, grad in pairs:
                    if prm.grad is None:
                        prm.grad = torch.empty_like(prm)
                    prm.grad.copy_(grad)
                # the loss terms the optimiser kernel would have written (this branch is the uncommon one: a few small launches)
                o = self.layout["size"]
                nn = n_dev.reshape(1).to(torch.float32) if n_dev is not None else torch.full((1,), float(n_host), device=dev)
                row[0:3] = g[o:o + 3] / nn.clamp(min=1.0)
                row[3] = ACTOR_COEFF * row[0] + CRITIC_COEFF * row[1] + ENTROPY_COEFF * row[2]
                row[4] = nn[0]
            self.optimizer.step()
            self.sync_from_module()
        return self._record({"actor_loss": row[0], "critic_loss": row[1], "entropy_loss": row[2], "ac_loss": row[3], "samples": row[4]})

    def update(self, obs, mask, action, qvals, weight=None):
        """One optimiser step on the given samples (this rank's share when distributed).  Returns the loss terms (global means).
        Rows with weight 0 are compacted away first (the network is not evaluated on them)."""
        if weight is not None:
            idx = torch.nonzero(weight > 0).squeeze(1)
            obs, mask, action, qvals = obs.index_select(0, idx), mask.index_select(0, idx), action.index_select(0, idx), qvals.index_select(0, idx)
            weight = None
        n_local = torch.full((1,), float(obs.shape[0]), dtype=torch.float32, device=obs.device)
        n_total = n_local.clone()
        if self.distributed:
            dist.all_reduce(n_total, group=self.group)
        use_fused = self._use_fused(obs)
        if use_fused:
            return self._finish_fused(*self._fused_gradients(obs, mask, action, qvals, n_total=float(n_total)))
        # rows without a legal action (stuck games) carry no sample
        legal_any = mask.bool().any(dim=1)
        w = legal_any.to(torch.float32) if weight is None else weight.to(torch.float32) * legal_any
        a, c, e, loss = self.loss_terms(obs, mask, action, qvals, w, n_total.squeeze(0))
        self.optimizer.zero_grad(set_to_none=False)
        loss.backward()
        stats = torch.stack([a.detach(), c.detach(), e.detach(), loss.detach()])
        if self.distributed:
            params = [p for p in self.policy.parameters() if p.grad is not None]
            flat = torch.cat([p.grad.reshape(-1) for p in params] + [stats])           # one bucket: ~86k floats
            dist.all_reduce(flat, group=self.group)
            o = 0
            for p in params:
                p.grad.copy_(flat[o:o + p.numel()].view_as(p))
                o += p.numel()
            stats = flat[o:]
        self.optimizer.step()
        return self._record({"actor_loss": stats[0], "critic_loss": stats[1], "entropy_loss": stats[2], "ac_loss": stats[3],
                             "samples": n_total.squeeze(0)})

    def update_from_rollout(self, rollout):
        """One update from a PolicyRollout after run_window().  With a ring of >= 2 windows (one part, fused path) EVERY step of
        EVERY episode is trained exactly once, like NNRunner.train (nn_runner.py:59-76): azul_select_episode_samples picks, per game,
        the steps from the first one not trained yet up to its last episode end inside the newest window -- including the opening
        steps recorded in earlier windows, whose returns run_window has chained backwards through the ring -- and
        azul_a2c_gradients reads them through the index list straight from the ring.  Steps whose episode outlives the ring
        (longer than (ring - 1) * window + 1 agent steps) are dropped and counted in `dropped_steps[1]`.
        The same holds for a wide rollout (PolicyRollout(fused_wide=True, wide_ring >= 2)) and a fused learner of its shape.
        Otherwise (ring == 1, several parts, PyTorch path): update_from_windows on the newest window."""
        ro = rollout
        tr0 = ro.traj[0]
        if ro.ring < 2 or ro.parts != 1 or not self._use_fused(tr0["obs"]):
            return self.update_from_windows(ro.traj)
        import ctypes as C
        from . import _lib as L
        rg, T, N, D = ro.rings[0], ro.T, ro.h, ro.ring
        dev = tr0["obs"].device
        R = D * T
        st = getattr(self, "_ring", None)
        if st is None or st["key"] != (id(ro), R, N):
            st = self._ring = {"key": (id(ro), R, N), "index": torch.empty(R * N, dtype=torch.int32, device=dev),
                               "count": torch.zeros(2, dtype=torch.int32, device=dev), "countf": torch.zeros(2, device=dev),
                               "pending": torch.zeros(N, dtype=torch.int32, device=dev),
                               "scratch": torch.empty(3 * N + (N + 3) // 4, dtype=torch.int32, device=dev), "offset": 0}
            # this learner's books start with the window that was just played (earlier windows -- warm-up -- are nobody's samples);
            # the clock is the rollout's own (absolute step s lives in ring slot s % R), shifted down by whole rings when it grows
            st["pending"].fill_((ro.windows_played - 1) * T)
            self.dropped_steps = st["count"]
        played = ro.windows_played * T - st["offset"]
        if played > (1 << 30):                            # keep the absolute step counters inside int32: rebase by whole rings
            shift = (played - R) // R * R
            st["pending"].sub_(shift)
            st["offset"] += shift
            played -= shift
        p = lambda t: C.c_void_p(t.data_ptr())
        L.check(L.lib.azul_select_episode_samples(p(rg["done"]), p(rg["action"]), T, D, N, int(played), p(st["pending"]), p(st["index"]),
                                                  p(st["count"]), p(st["countf"]), p(st["scratch"]),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return self._finish_fused(*self._fused_gradients(
            rg["obs"][:R].reshape(R * N, -1), rg["mask"][:R].reshape(R * N, -1), rg["action"].reshape(-1), rg["returns"].reshape(-1),
            index=st["index"], count=st["count"][:1], countf=st["countf"]))

    def ring_state(self):
        """The books of update_from_rollout's ring selection (for a checkpoint): per game the first absolute step not trained yet, the
        clock offset and the dropped-step counter; None before the first ring update."""
        st = getattr(self, "_ring", None)
        if st is None:
            return None
        return {"pending": st["pending"].cpu(), "offset": int(st["offset"]), "count": st["count"].cpu(), "R": st["key"][1], "N": st["key"][2]}

    def load_ring_state(self, rollout, state):
        """Restore ring_state() for `rollout` (whose ring buffers and windows_played the caller has restored), or -- state None --
        forget the books: the next update_from_rollout starts them with the window played just before it."""
        self._ring = None
        self.dropped_steps = None
        if state is None or rollout.ring < 2 or rollout.parts != 1:
            return
        R, N = rollout.ring * rollout.T, rollout.h
        if (state["R"], state["N"]) != (R, N):
            raise ValueError("ring state was written for %d slots x %d games" % (state["R"], state["N"]))
        dev = rollout.device
        self._ring = {"key": (id(rollout), R, N), "index": torch.empty(R * N, dtype=torch.int32, device=dev),
                      "count": state["count"].to(dev).clone(), "countf": torch.zeros(2, device=dev),
                      "pending": state["pending"].to(dev).clone(),
                      "scratch": torch.empty(3 * N + (N + 3) // 4, dtype=torch.int32, device=dev), "offset": int(state["offset"])}
        self.dropped_steps = self._ring["count"]

    def update_from_windows(self, trajectories, complete_only=True, kweights=None):
        """`trajectories`: the per-part dicts PolicyRollout.run_window returns (opponent="random": every record is one agent
        step).  Uses the steps whose episode finished inside the window (exact Monte-Carlo returns, the reference's qvals).
        With one part on the GPU the whole update stays on the device: azul_select_complete_samples picks the steps,
        azul_a2c_gradients reads them through the index list -- no compaction copies, no host round trip."""
        tr0 = trajectories[0]
        if len(trajectories) == 1 and complete_only and self._use_fused(tr0["obs"]):
            import ctypes as C
            from . import _lib as L
            T, N = tr0["action"].shape
            dev = tr0["obs"].device
            if getattr(self, "_sel", None) is None or self._sel[0].numel() != T * N or self._sel[0].device != dev:
                self._sel = (torch.empty(T * N, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev))
            index, count = self._sel
            L.check(L.lib.azul_select_complete_samples(C.c_void_p(tr0["done"].data_ptr()), C.c_void_p(tr0["action"].data_ptr()), T, N,
                                                       C.c_void_p(index.data_ptr()), C.c_void_p(count.data_ptr()),
                                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            return self._finish_fused(*self._fused_gradients(
                tr0["obs"][:T].reshape(T * N, -1), tr0["mask"][:T].reshape(T * N, -1), tr0["action"].reshape(-1), tr0["returns"].reshape(-1),
                index=index, count=count, kweights=kweights))
        obs, mask, action, ret = [], [], [], []
        for tr in trajectories:
            T = tr["action"].shape[0]
            keep = complete_episode_samples(tr["done"]) if complete_only else torch.ones_like(tr["done"], dtype=torch.bool)
            keep = keep & (tr["action"] >= 0)
            idx = torch.nonzero(keep.reshape(-1)).squeeze(1)               # compact per part: the big buffers are read once
            obs.append(tr["obs"][:T].reshape(-1, tr["obs"].shape[-1]).index_select(0, idx))
            mask.append(tr["mask"][:T].reshape(-1, tr["mask"].shape[-1]).index_select(0, idx))
            action.append(tr["action"].reshape(-1).index_select(0, idx))
            ret.append(tr["returns"].reshape(-1).index_select(0, idx))
        one = len(trajectories) == 1
        return self.update(obs[0] if one else torch.cat(obs), mask[0] if one else torch.cat(mask),
                           action[0] if one else torch.cat(action), ret[0] if one else torch.cat(ret))


class PPOLearner(A2CLearner):
    """PPO on the windows of a PolicyRollout: `epochs` passes of `minibatches` optimiser steps over the steps of ONE window, made safe
    by the clipped importance ratio.  Reuses A2CLearner's flat k-major master copy, kweights(), Adam (_finish_fused) and statistics ring;
    the gradients come from azul_ppo_gradients (the A2C gradient kernels with a second head, csrc/azul_learner.hpp) on the fused path
    and from autograd of loss_terms_ppo otherwise.

    Objective per sample, over the n samples of a minibatch (old_logp = the rollout's recorded log_prob, Adv an input: detached):
        r = exp(logp[a] - old_logp),   L_pi = -min(r Adv, clamp(r, 1 - clip_eps, 1 + clip_eps) Adv),   H = -sum_k p_k logp_k
        loss = mean(L_pi) + value_coeff * mean((returns - V)^2) - entropy_coeff * mean(H)
    Adv = returns - value from the rollout's recorded `value` (with PolicyRollout(gae_lambda=...) that is the GAE advantage), normalised
    over the selected samples of the window when normalize_advantage: (A - mean) / (std + 1e-8), population std, f32.

    Statistics, one entry per OPTIMISER STEP, under A2CLearner's keys with PPO's meaning: actor_loss = mean L_pi, critic_loss =
    mean (returns - V)^2 (without the coefficient), entropy_loss = mean H (the true entropy, which the loss SUBTRACTS), ac_loss = actor +
    value_coeff * critic - entropy_coeff * H, samples = the minibatch size; and two more: clip_fraction = mean(|r - 1| > clip_eps) and
    approx_kl = mean(old_logp - logp[a]), both of the policy BEFORE the step."""

    def __init__(self, policy, learning_rate=3e-4, gamma=0.99, clip_eps=0.2, value_coeff=0.5, entropy_coeff=0.01, epochs=4, minibatches=4,
                 normalize_advantage=True, shuffle_seed=0, fused=None, stat_history=4096, distributed=None):
        self.check_arguments(clip_eps, value_coeff, entropy_coeff, epochs, minibatches, distributed)
        super().__init__(policy, learning_rate=learning_rate, gamma=gamma, distributed=False, fused=fused, stat_history=stat_history)
        self.clip_eps, self.value_coeff, self.entropy_coeff = float(clip_eps), float(value_coeff), float(entropy_coeff)
        self.epochs, self.minibatches = int(epochs), int(minibatches)
        self.normalize_advantage = bool(normalize_advantage)
        self.shuffle_seed = int(shuffle_seed)
        self.u = 0                        # update_from_windows calls so far: with the epoch it keys the minibatch permutation
        for k in ("clip_fraction", "approx_kl"):
            self.statistics[k] = collections.deque(maxlen=stat_history)
        self._step_extras = None

    @staticmethod
    def check_arguments(clip_eps, value_coeff, entropy_coeff, epochs, minibatches, distributed=None):
        """The refusals of the constructor (ValueError), before anything is allocated; BatchedTrainer asks them before it builds anything."""
        if distributed or (distributed is None and dist.is_available() and dist.is_initialized()):
            raise ValueError("PPOLearner is single-process: its minibatch permutations are not sharded over ranks (distributed=True refused)")
        if int(epochs) < 1 or int(minibatches) < 1:
            raise ValueError("epochs and minibatches must be >= 1, got %r and %r" % (epochs, minibatches))
        if not float(clip_eps) > 0.0 or float(clip_eps) == float("inf"):
            raise ValueError("clip_eps must lie in (0, +inf), got %r" % (clip_eps,))
        if not (0.0 <= float(value_coeff) < float("inf") and 0.0 <= float(entropy_coeff) < float("inf")):
            raise ValueError("value_coeff and entropy_coeff must be finite and >= 0, got %r and %r" % (value_coeff, entropy_coeff))

    def loss_terms_ppo(self, obs, mask, action, returns, old_log_prob, advantage, n_total=None):
        """The objective of the class docstring in PyTorch (any shape, CPU or GPU): (actor_loss, critic_loss, entropy, loss, log_prob) with
        actor_loss = sum L_pi / n, critic_loss = sum (returns - V)^2 / n, entropy = sum H / n, loss = actor + value_coeff * critic -
        entropy_coeff * entropy, and log_prob [rows] = logp[a] (attached).  `n_total`: the divisor (default: the number of rows).  Rows
        without a legal action carry no sample but stay in the divisor, as in the kernels."""
        legal = mask.bool()
        live = legal.any(dim=1)
        legal = legal | ~live.unsqueeze(1)               # (a dead row is evaluated as if every action were legal, then weighted out: no NaN)
        values, logp = self._values_logp(obs, legal)
        log_prob = logp.gather(1, action.long().clamp(min=0).unsqueeze(1)).squeeze(1)
        lp0 = torch.where(legal, logp, torch.zeros_like(logp))
        entropy = -(lp0.exp() * legal * lp0).sum(dim=1)
        adv = advantage.to(values.dtype).detach()
        ratio = torch.exp(log_prob - old_log_prob.to(values.dtype).detach())
        surrogate = torch.min(ratio * adv, torch.clamp(ratio, 1.0 - self.clip_eps, 1.0 + self.clip_eps) * adv)
        w = live.to(values.dtype)
        n = float(obs.shape[0]) if n_total is None else n_total
        n = n.clamp(min=1.0) if torch.is_tensor(n) else max(float(n), 1.0)
        actor_loss = (torch.where(live, -surrogate, torch.zeros_like(surrogate))).sum() / n
        critic_loss = ((returns.to(values.dtype) - values).pow(2) * w).sum() / n
        entropy_mean = (entropy * w).sum() / n
        loss = actor_loss + self.value_coeff * critic_loss - self.entropy_coeff * entropy_mean
        return actor_loss, critic_loss, entropy_mean, loss, log_prob

    def optimizer_state(self):
        """A2CLearner's state plus `u`, the count of update_from_windows calls: a resumed run draws the same permutations."""
        st = super().optimizer_state()
        st["ppo"] = {"u": int(self.u)}
        return st

    def load_optimizer_state(self, st):
        super().load_optimizer_state(st)
        if "ppo" in st:
            self.u = int(st["ppo"]["u"])

    def _record(self, out):
        """The entry of one optimiser step: ac_loss from the three terms with PPO's coefficients (the Adam kernel's slot holds the
        reference's 1 / 0.5 / 0.1 combination), plus the ratio diagnostics of the step."""
        clip_fraction, approx_kl = self._step_extras
        out = dict(out, ac_loss=out["actor_loss"] + self.value_coeff * out["critic_loss"] - self.entropy_coeff * out["entropy_loss"],
                   clip_fraction=clip_fraction, approx_kl=approx_kl)
        return super()._record(out)

    def _ratio_stats(self, log_prob, old_log_prob):
        d = old_log_prob - log_prob
        return ((torch.exp(-d) - 1.0).abs() > self.clip_eps).to(torch.float32).mean(), d.mean()

    def _permutations(self, rows, u, device):
        """[epochs, rows] on `device`: row e is the order in which epoch e of call `u` visits the `rows` rows of the window -- a function of
        (shuffle_seed, u, e) only, drawn on the CPU.  A draw of 131072 rows takes the host about 1 ms, so the caller asks BEFORE the
        selection's host synchronisation: the draws then overlap the device's work on the window (pinned staging buffer, asynchronous
        copy; the synchronisation that follows completes the copy before the buffer is written again)."""
        pin = getattr(self, "_perm_pin", None)
        if pin is None or tuple(pin.shape) != (self.epochs, rows) or pin.is_pinned() != (device.type == "cuda"):
            pin = self._perm_pin = torch.empty(self.epochs, rows, dtype=torch.int64, pin_memory=device.type == "cuda")
        g = torch.Generator()
        for e in range(self.epochs):
            g.manual_seed(((self.shuffle_seed * 1000003 + u) * 1000003 + e) % (1 << 63))
            torch.randperm(rows, generator=g, out=pin[e])
        return pin.to(device, non_blocking=True) if device.type == "cuda" else pin.clone()

    def _fused_gradients(self, src, chunk, adv_rows):
        """One azul_ppo_gradients launch on the rows `chunk` (int32, device) of the window's buffers, read in place; the flat gradient and
        the four sums land in the workspace's `grad`, the recomputed logp[a] of the chunk is returned.  -> (None, n_host) for _finish_fused."""
        import ctypes as C
        from . import _lib as L
        pol, dev = self.policy, src["obs"].device
        ws = self._ensure_flat(dev)
        kw = self.kweights(dev)
        n = int(chunk.numel())
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        with torch.no_grad():
            logp = src["log_prob"].index_select(0, chunk)              # (rows without a sample keep the old value: ratio 1 in the diagnostics)
            L.check(L.lib.azul_ppo_gradients(p(src["obs"]), p(src["mask"]), p(src["action"]), p(src["returns"]), p(src["log_prob"]), p(adv_rows),
                                             n, C.c_float(1.0 / n), C.c_float(self.clip_eps), C.c_float(self.value_coeff),
                                             C.c_float(self.entropy_coeff), p(kw["w1t"]), p(kw["b1"]), p(kw["w2c"]), p(kw["b2c"]), p(kw["w2a_t"]),
                                             p(kw["b2a"]), p(pol.actor_linear2.weight), *self.shape, p(ws["ws"]), 256, p(ws["grad"]), p(chunk),
                                             None, None, p(logp), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return (None, float(n)), logp

    def update_from_rollout(self, rollout):
        """PPO trains the newest window (the ring of whole episodes is A2C's): update_from_windows(rollout.traj)."""
        return self.update_from_windows(rollout.traj)

    def update_from_windows(self, trajectories, complete_only=True):
        """epochs x minibatches optimiser steps on the steps of the window(s) that carry an action -- and whose episode ends inside the
        window unless complete_only=False (PolicyRollout(bootstrap_tail=True) gives every recorded step a target).  The selection is ONE
        torch.nonzero, i.e. one host synchronisation per call: the minibatch sizes are host numbers, and the price is paid once per
        epochs x minibatches optimiser steps.  Epoch e of the u-th call visits the selected rows in the order a permutation of the window's
        rows gives them -- a function of (shuffle_seed, u, e) only, drawn on the CPU before that synchronisation -- cut into `minibatches`
        near-equal chunks; on the fused path (one part) every chunk is one azul_ppo_gradients launch reading the window's
        buffers in place through the chunk as index list (no compaction copies) and one Adam step; otherwise the chunks go through
        loss_terms_ppo and optimizer.step().  Several parts are compacted and concatenated first.  An empty selection performs no step and
        records one entry of zeros.  Returns the statistics of the last step."""
        keys = ("obs", "mask", "action", "returns", "log_prob", "value")
        u, one = self.u, len(trajectories) == 1
        self.u += 1
        flat, perms = [], None
        for tr in trajectories:
            T = tr["action"].shape[0]
            keep = complete_episode_samples(tr["done"]) if complete_only else torch.ones_like(tr["done"], dtype=torch.bool)
            keep = (keep & (tr["action"] >= 0)).reshape(-1)
            rows = {"obs": tr["obs"][:T].reshape(-1, tr["obs"].shape[-1]), "mask": tr["mask"][:T].reshape(-1, tr["mask"].shape[-1])}
            rows.update({k: tr[k].reshape(-1) for k in keys[2:]})
            if one:                                      # drawn while the device still works on the window: before the synchronisation
                perms = self._permutations(keep.numel(), u, keep.device)
            flat.append((rows, keep, torch.nonzero(keep).squeeze(1)))
        if one:
            src, keep, sel = flat[0]
        else:
            src = {k: torch.cat([rows[k].index_select(0, idx) for rows, _, idx in flat]) for k in keys}
            keep, sel = None, torch.arange(src["action"].shape[0], device=src["action"].device)
        dev = src["obs"].device
        n = int(sel.numel())
        if n == 0:
            zero = torch.zeros((), device=dev)
            self._step_extras = (zero, zero)
            return self._record({"actor_loss": zero, "critic_loss": zero, "entropy_loss": zero, "ac_loss": zero, "samples": zero})
        if perms is None:
            perms = self._permutations(n, u, dev)
        fused = self._use_fused(src["obs"])
        with torch.no_grad():
            adv = src["returns"].index_select(0, sel).float() - src["value"].index_select(0, sel).float()
            if self.normalize_advantage:
                adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
            adv_rows = torch.zeros(src["action"].shape[0], device=dev).index_copy_(0, sel, adv)      # per source row, like the buffers
            if fused:
                src = {"obs": src["obs"].contiguous().float(), "mask": src["mask"].contiguous().to(torch.uint8),
                       "action": src["action"].contiguous().to(torch.int32), "returns": src["returns"].contiguous().float(),
                       "log_prob": src["log_prob"].contiguous().float()}                  # (the rollout's buffers as they are: no copies)
        out = None
        for e in range(self.epochs):
            order = perms[e]
            if keep is not None:                         # the selected rows in the permutation's order (a stable sort brings them to the
                order = order[torch.argsort((~keep[order]).to(torch.uint8), stable=True)[:n]]       # front: no second host round trip)
            for rows in torch.tensor_split(order, self.minibatches):
                if rows.numel() == 0:
                    continue
                if fused:
                    chunk = rows.to(torch.int32)
                    nn, logp = self._fused_gradients(src, chunk, adv_rows)
                    self._step_extras = self._ratio_stats(logp, src["log_prob"].index_select(0, rows))
                    out = self._finish_fused(*nn)
                else:
                    a, c, h, loss, logp = self.loss_terms_ppo(*(src[k].index_select(0, rows) for k in keys[:5]), adv_rows.index_select(0, rows))
                    self.optimizer.zero_grad(set_to_none=False)
                    loss.backward()
                    self.optimizer.step()
                    with torch.no_grad():
                        old = src["log_prob"].index_select(0, rows).float()
                        live = src["mask"].index_select(0, rows).bool().any(dim=1)         # (a row without a sample: ratio 1, as on the fused path)
                        self._step_extras = self._ratio_stats(torch.where(live, logp.detach(), old), old)
                    out = self._record({"actor_loss": a.detach(), "critic_loss": c.detach(), "entropy_loss": h.detach(),
                                        "ac_loss": loss.detach(), "samples": torch.full((), float(rows.numel()), device=dev)})
        return out
