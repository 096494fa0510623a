# -*- coding: utf-8 -*-
"""Fused Adam over the model's flat parameter buffer (one HIP launch per step).

Drop-in for ``torch.optim.Adam(model.parameters(), lr=..., weight_decay=...)`` as used by the
reference at train.py:457-460: same update rule (L2-in-gradient weight decay, bias correction),
parameters without a gradient are skipped (the dead last ``res_1x1``), and ``state_dict()`` /
``load_state_dict()`` use torch.optim.Adam's format (``{"state": {idx: {"step", "exp_avg",
"exp_avg_sq"}}, "param_groups": [...]}``) so checkpoints written by either optimizer resume with
the other (train.py:315-332,503-513).

Opt-in, both free of host synchronisation:

``max_grad_norm=c``     global-norm clipping, ``torch.nn.utils.clip_grad_norm_(model.parameters(), c)`` in front of the step: the
                        norm of the whole flat gradient is reduced on the device (two launches) and the Adam launch scales the
                        gradient by ``min(1, c / (norm + 1e-6))`` as it reads it.  Unlike torch's in-place clip the gradient
                        buffer -- and so every ``p.grad`` -- KEEPS ITS UNCLIPPED VALUES.
``skip_nonfinite=True`` a step whose gradient holds a NaN or an inf changes nothing (weights, moments, step count) and is
                        counted in ``steps_skipped()``.

``ema_decay=d``          an exponential moving average of the weights, kept in a second flat buffer and updated by
                        the Adam launch itself while the new weight is in a register: ``e += (1 - d_t) (p_new - e)`` with
                        ``d_t = min(d, (1 + t) / (10 + t))`` (``ema_warmup=True``; t = applied steps, this one included) or
                        ``d_t = d``.  A skipped step leaves the average alone and does not advance t.  Weights and moments get
                        the bits they get without it.  ``opt.ema`` is the flat buffer, ``ema_state_dict()`` /
                        ``load_ema_state_dict()`` (de)serialise it under the model's keys, and ``with opt.ema_weights():``
                        runs its body on the averaged weights.  Ranks of a data-parallel run hold identical weights and
                        gradients, hence identical averages, without communication.

Gradient accumulation (``loss_and_backward(micro_step=(i, A))``) needs nothing here: the final micro-step leaves
the sum in the gradient buffer this optimizer reads, so the norm, the guard and the average see the accumulated (and reduced)
gradient and count optimizer steps.  ``step()`` inside an open cycle raises RuntimeError.

Frozen parameters: a live parameter whose ``p.grad`` is None at ``step()`` -- frozen (``requires_grad`` False,
``WaveNet.freeze`` / ``train_only``; ``loss_and_backward`` then leaves its ``grad`` None) or dropped by the caller -- is left alone
exactly: weights, both moments and the average keep their bits, no weight decay is applied, and whatever the gradient buffer holds
in its range (NaN included) reaches neither the norm nor the guard.  The norm and the Adam launch then run over the live ranges
of the flat buffers (``grad_sumsq_live`` / ``adam*_live``: the same number of launches, a live element gets the bits of the
whole-buffer launch); with every live parameter holding a gradient they are the whole-buffer launches with their arguments of
before.  An empty live set issues no launch and counts no step.  ONE STEP COUNT: the optimizer keeps a single count of applied
steps for the bias correction.  With a freeze set that never changes the step is torch's
``Adam(p for p in params if p.requires_grad)``; a tensor unfrozen later continues with the moments it has and the optimizer's
global count, where torch would restart that tensor's own count at 1.  ``state_dict()`` carries an entry for every non-dead
tensor that has been in the live set of at least one APPLIED step (all of them when nothing is frozen; a step the guard skipped
does not count; a change of the set reads the device's step count once on the guarded path); ``load_state_dict`` takes
a missing entry as zero moments.

With all three at their defaults ``step()`` is the one ``adam`` launch with the host's step count, bit for bit as before.
``state_dict()`` never holds the average: it stays in torch.optim.Adam's format.
"""
import contextlib

import torch

from . import _lib


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 skip_nonfinite=False, ema_decay=None, ema_warmup=True):
        if not hasattr(model, "engine"):
            raise TypeError("FusedAdam takes the WaveNet model (it updates the model's flat buffer)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
        self.model = model
        super(FusedAdam, self).__init__(list(model.parameters()), defaults)
        self._step = 0
        self._exp_avg = None
        self._exp_avg_sq = None
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (None = no clipping)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self._opt_state = None     # device WnOptState + the norm's scratch: allocated once, on the first guarded use
        self._norm_scratch = None
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError("ema_decay must lie in [0, 1) (None = no moving average)")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self._trained = [False] * len(model._param_slices)   # per tensor: was in the live set of an APPLIED step (state_dict carries those)
        self._last_set = None      # the TrainableSet of the last step(); folded into _trained when it changes and by state_dict()
        self._set_applied0 = 0     # applied steps when _last_set became the current set
        self._ema = None           # the shadow buffer: a copy of the flat weights at its first use
        self._ema_swapped = False  # inside ema_weights(): the two buffers have changed places

    def _guard_buffers(self):
        eng = self.model.engine
        if self._opt_state is None or self._opt_state.device != eng.flat_params.device:
            old = self._opt_state
            self._opt_state = eng.new_opt_state()
            self._norm_scratch = eng.grad_norm_scratch()
            if old is not None:
                self._opt_state.copy_(old)
            else:
                self._opt_state[3] = self._step
        return self._opt_state, self._norm_scratch

    @property
    def grad_norm(self):
        """0-dim device tensor (a view of the state block): the global gradient norm of the last ``step()`` BEFORE clipping --
        under data parallelism the norm of the reduced, global gradient.  Valid after ``step()``; reading it on the device
        needs no synchronisation.  None on the unguarded path."""
        if not self.guarded:
            return None
        return self.model.engine.opt_state_views(self._guard_buffers()[0])["total_norm"]

    def steps_applied(self):
        """Number of applied steps (synchronises on the guarded path: the count lives on the device)."""
        if not self.guarded:
            return self._step
        return int(self._guard_buffers()[0][3])

    def steps_skipped(self):
        """Number of steps the non-finite guard skipped (synchronises)."""
        if not self.guarded:
            return 0
        return int(self._guard_buffers()[0][4])

    def _buffers(self):
        eng = self.model.engine
        if self._exp_avg is None or self._exp_avg.device != eng.flat_params.device:
            old = (self._exp_avg, self._exp_avg_sq)
            self._exp_avg = torch.zeros_like(eng.flat_params)
            self._exp_avg_sq = torch.zeros_like(eng.flat_params)
            if old[0] is not None:
                self._exp_avg.copy_(old[0])
                self._exp_avg_sq.copy_(old[1])
        return self._exp_avg, self._exp_avg_sq

    def _ema_buffer(self):
        eng = self.model.engine
        if self._ema is None:
            self._ema = eng.flat_params.detach().clone()
        elif self._ema.device != eng.flat_params.device:
            self._ema = self._ema.to(eng.flat_params.device)
        return self._ema

    @property
    def ema(self):
        """The flat moving average (same layout as ``engine.flat_params``), None when ``ema_decay`` is None.  Inside
        ``ema_weights()`` this buffer holds the training weights."""
        return None if self.ema_decay is None else self._ema_buffer()

    def _need_ema(self):
        if self.ema_decay is None:
            raise RuntimeError("this optimizer keeps no moving average (ema_decay=None)")

    def ema_state_dict(self):
        """Clones of the averaged weights under the model's ``state_dict`` keys and shapes (a dict ``load_state_dict`` of a
        model, or the reference's decode tool, takes as it is)."""
        self._need_ema()
        src = self.model.engine.flat_params if self._ema_swapped else self._ema_buffer()
        return {k: src[off:off + n].view(shape).detach().clone()
                for (k, _), (off, n, shape, dead) in zip(self.model.named_parameters(), self.model._param_slices)}

    @torch.no_grad()
    def load_ema_state_dict(self, sd):
        self._need_ema()
        if self._ema_swapped:
            raise RuntimeError("load_ema_state_dict() inside ema_weights()")
        names = [k for k, _ in self.model.named_parameters()]
        if set(sd.keys()) != set(names):
            raise KeyError("the EMA state dict does not have the model's keys: %s" % sorted(set(sd.keys()) ^ set(names)))
        ema = self._ema_buffer()
        for k, (off, n, shape, dead) in zip(names, self.model._param_slices):
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError("%s: shape %s, the model has %s" % (k, tuple(sd[k].shape), tuple(shape)))
            ema[off:off + n].copy_(sd[k].reshape(-1))

    @contextlib.contextmanager
    def ema_weights(self):
        """Run the body on the averaged weights: the weights and the average change places (one ``swap`` launch, no temporary)
        and change back on exit, also when the body raises.  ``step()`` inside and nesting raise RuntimeError.  The parameter
        version changes on entry and on exit, so the block must not sit between a forward and its ``backward()``."""
        self._need_ema()
        if self._ema_swapped:
            raise RuntimeError("ema_weights() is already active")
        eng = self.model.engine
        eng.swap_params(self._ema_buffer())
        self._ema_swapped = True
        try:
            yield self.model
        finally:
            eng.swap_params(self._ema_buffer())
            self._ema_swapped = False

    @torch.no_grad()
    def step(self, closure=None):
        if self._ema_swapped:
            raise RuntimeError("step() inside ema_weights(): the model holds the averaged weights")
        if self.model.engine.accumulation is not None:
            raise RuntimeError("step() inside an accumulation cycle (%d of %d micro-steps done): the gradient buffer holds one "
                               "micro-batch, not the sum -- run the remaining micro-steps first, or call "
                               "model.engine.abandon_accumulation()" % self.model.engine.accumulation)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        eng = self.model.engine
        m, v = self._buffers()
        ema = self.ema
        flat_g = eng.grads()
        # gradients produced by the autograd path live in separate tensors: gather them
        lo = flat_g.data_ptr()
        hi = lo + flat_g.numel() * 4
        has_grad = []   # a parameter without a gradient -- frozen, or dropped by the caller -- is left alone, as torch.optim.Adam does
        for p, (off, n, shape, dead) in zip(self.model.parameters(), self.model._param_slices):
            has_grad.append(p.grad is not None)
            if p.grad is not None and not (lo <= p.grad.data_ptr() < hi):
                flat_g[off:off + n].copy_(p.grad.reshape(-1))
        # every live parameter has one: today's launches over the whole buffer.  Otherwise the same kernels' arithmetic over the
        # live ranges only: what the gradient buffer holds elsewhere is never read, and weights, moments and the
        # average keep their bits there (no weight decay either).
        ts = self.model.trainable(has_grad)
        if ts.empty:
            return loss   # nothing to update: no launch, and no step is counted
        live = {} if ts.full else {"live": ts.table}
        if ts is not self._last_set:
            # a change of the set (rare) reads the count of applied steps, which on the guarded path lives on the device.  The
            # test is the identity of the object model.trainable() caches: should the model drop and rebuild the set of the same
            # flags, this branch runs once more and changes nothing (the fold is idempotent)
            self._fold_trained()
            self._set_applied0 = self._step if self._last_set is None else self.steps_applied()
            self._last_set = ts
        group = self.param_groups[0]
        if self.guarded:
            # the gather above comes first: the norm is the norm of what the Adam launch reads
            state, scratch = self._guard_buffers()
            eng.grad_norm(state, scratch, self.max_grad_norm, self.skip_nonfinite, group["lr"], group["betas"], **live)
            if ema is None:
                eng.adam_step_guarded(m, v, state, group["eps"], group["weight_decay"], **live)
            else:
                eng.adam_step_guarded_ema(m, v, ema, state, group["eps"], group["weight_decay"], self.ema_decay, self.ema_warmup,
                                          **live)
        else:
            self._step += 1
            if ema is None:
                eng.adam_step(m, v, self._step, group["lr"], group["betas"], group["eps"], group["weight_decay"], **live)
            else:
                eng.adam_step_ema(m, v, ema, self._step, group["lr"], group["betas"], group["eps"], group["weight_decay"],
                                  self.ema_decay, self.ema_warmup, **live)
        return loss

    def _fold_trained(self):
        """Mark the tensors of the current set as trained if a step was APPLIED since it became current: a step the non-finite
        guard skipped trains nothing."""
        if self._last_set is not None and self.steps_applied() > self._set_applied0:
            self._trained = [was or (on and not dead) for was, on, (off, n, shape, dead)
                             in zip(self._trained, self._last_set.mask, self.model._param_slices)]

    # ---- torch.optim.Adam compatible (de)serialisation --------------------------------------
    def state_dict(self):
        self._fold_trained()
        m, v = self._buffers()
        state = {}
        step = self.steps_applied()
        if step > 0:
            for idx, (off, n, shape, dead) in enumerate(self.model._param_slices):
                if dead or not self._trained[idx]:   # (a tensor frozen in every step so far has no state, as in torch)
                    continue
                state[idx] = {"step": torch.tensor(float(step)),
                              "exp_avg": m[off:off + n].view(shape).clone(),
                              "exp_avg_sq": v[off:off + n].view(shape).clone()}
        groups = []
        for g in self.param_groups:
            gg = {k: val for k, val in g.items() if k != "params"}
            gg["params"] = list(range(len(self.model._param_slices)))
            groups.append(gg)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        m, v = self._buffers()
        m.zero_()
        v.zero_()
        step = 0
        self._trained = [False] * len(self.model._param_slices)
        self._last_set = None
        for idx, st in sd["state"].items():
            off, n, shape, dead = self.model._param_slices[int(idx)]
            self._trained[int(idx)] = True
            m[off:off + n].copy_(st["exp_avg"].reshape(-1))
            v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            step = max(step, int(float(st["step"])))
        self._step = step
        if self.guarded:
            self._guard_buffers()[0][3] = step
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k in ("lr", "betas", "eps", "weight_decay"):
                if k in sg:
                    g[k] = tuple(sg[k]) if k == "betas" else sg[k]
