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

Parameter groups: ``groups=[(regex, {"lr": .., "weight_decay": .., "eps": .., "decoupled_weight_decay": ..}), ..]``
gives the tensors whose ``named_parameters()`` key ``re.search`` es ``regex`` (the first matching entry wins) their own learning rate,
epsilon and weight decay -- L2 as above, or decoupled as in ``torch.optim.AdamW`` (``p *= 1 - lr wd`` in front of an update whose
gradient carries no decay term).  A missing key inherits the constructor's value; unmatched tensors form the default group,
``param_groups[0]``.  Betas, the step count, the norm with its clip coefficient, the guard and the average stay one per optimizer.
``param_groups`` then holds ``1 + len(groups)`` torch-format entries with the real ``Parameter`` objects, and every ``step()`` reads
the four values from them: ``torch.optim.lr_scheduler`` works on all groups, and because the values travel in the launch
arguments a changing learning rate costs no copy and no synchronisation.  The step stays one launch (three guarded:
``adam*_groups``, a live table whose ranges carry a group index; with nothing frozen the norm is the whole-buffer ``grad_sumsq``).
An L2 group's elements get the bits the single-group launch gives them with that group's values.  The grouped launch is taken
only when more than one group holds a live parameter or the one that does is decoupled.  ``state_dict()`` numbers the tensors as
torch does -- consecutively over the groups in order, model order inside a group -- so a grouped checkpoint loads into
``torch.optim.Adam`` built with the same groups, and back; a different group structure raises ValueError.  ``add_param_group``
after construction raises: a group is a set of ranges of the flat buffer, fixed with the optimizer.

Layer-wise adaptive steps (LAMB): ``layer_adaptation=True`` scales every adapted tensor's step by its trust ratio
``r = ||w|| / ||u||`` (``u`` the bias-corrected Adam direction, plus ``wd w`` in a decoupled group; ``r = 1`` when either norm is
zero; ``max_trust_ratio`` clamps it): ``w -= lr r u``.  Tensors with two or more dimensions adapt, one-dimensional ones (every bias:
``initialize()`` zeroes them, and an adapted bias would get ``r = 1`` once and then steps proportional to its own tiny norm) take
the plain Adam update; a group's ``"layer_adaptation": True | False`` overrides that for its tensors.  The moments are Adam's bit
for bit, so ``state_dict()`` keeps torch.optim.Adam's format and a run may switch between the two on resume.  The step is three
launches (``lamb_moments``, ``lamb_ratios``, ``lamb_apply``) behind the two of the norm on the guarded path, over a table with one
range per live tensor, rebuilt once when the trainable set changes.  ``opt.trust_ratios``, ``opt.weight_norms`` and
``opt.update_norms`` are device tensors in the order of ``opt.tensor_names`` (``named_parameters()`` order), valid after ``step()``
without synchronisation; a step the guard skipped leaves them.  WITHOUT the guard a non-finite gradient poisons every weight of
its tensor through the ratio (plain Adam poisons one element).  ``opt.grad_norms()`` gives the per-tensor gradient norms (two
launches for all tensors) with or without layer adaptation.

With all of these at their defaults ``step()`` is the one ``adam`` launch with the host's step count, bit for bit as before.
``state_dict()`` never holds the average: it stays in torch.optim.Adam's format.
"""
import contextlib
import re

import torch

from . import _lib


GROUP_KEYS = ("lr", "weight_decay", "eps", "decoupled_weight_decay", "layer_adaptation")


def assign_groups(names, groups):
    """Group index per name for ``FusedAdam(groups=)``: 0 for the default group, ``1 + j`` for the first entry ``j`` whose regex
    ``re.search`` es the name.  ValueError for an entry that is no ``(regex, dict)`` pair, an unknown key, a pattern that matches
    no name and more than ``_lib.MAX_PARAM_GROUPS`` groups."""
    groups = list(groups)
    if 1 + len(groups) > _lib.MAX_PARAM_GROUPS:
        raise ValueError("%d parameter groups and the default one: at most %d in all" % (len(groups), _lib.MAX_PARAM_GROUPS))
    rxs = []
    for entry in groups:
        try:
            pattern, values = entry
            values = dict(values)
        except (TypeError, ValueError):
            raise ValueError("groups takes (regex, dict) pairs, got %r" % (entry,))
        for k in values:
            if k == "betas":
                raise ValueError("group %r: betas are per optimizer, not per group (one step count and one bias correction)" % (pattern,))
            if k not in GROUP_KEYS:
                raise ValueError("group %r: unknown key %r (a group sets %s)" % (pattern, k, ", ".join(GROUP_KEYS)))
            if k == "layer_adaptation" and not isinstance(values[k], bool):
                raise ValueError("group %r: layer_adaptation takes True or False, got %r" % (pattern, values[k]))
        rx = re.compile(pattern)
        if not any(rx.search(k) for k in names):
            raise ValueError("group pattern %r matches no parameter of the model (keys look like %r)" % (pattern, names[0]))
        rxs.append(rx)
    return [next((1 + j for j, rx in enumerate(rxs) if rx.search(k)), 0) for k in names]


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 skip_nonfinite=False, ema_decay=None, ema_warmup=True, groups=None, layer_adaptation=False, max_trust_ratio=None):
        if not hasattr(model, "engine"):
            raise TypeError("FusedAdam takes the WaveNet model (it updates the model's flat buffer)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)
        self.model = model
        named = list(model.named_parameters())
        self.layer_adaptation = bool(layer_adaptation)
        if max_trust_ratio is not None and not float(max_trust_ratio) > 0.0:
            raise ValueError("max_trust_ratio must be positive (None = no clamp)")
        self.max_trust_ratio = None if max_trust_ratio is None else float(max_trust_ratio)
        if not self.layer_adaptation:
            if self.max_trust_ratio is not None:
                raise ValueError("max_trust_ratio needs layer_adaptation=True")
            if any("layer_adaptation" in dict(values) for _, values in (groups or ()) if isinstance(values, dict)):
                raise ValueError("a group sets layer_adaptation, the optimizer was built with layer_adaptation=False")
        self._lamb = (None, None)   # (TrainableSet, its tensor-table route): rebuilt when the set changes
        self._built = False
        if groups is None:
            self._group_of = [0] * len(named)
            super(FusedAdam, self).__init__([p for _, p in named], defaults)
        else:
            # torch's own key for the decay mode (torch.optim.Adam(decoupled_weight_decay=)): a grouped checkpoint carries it
            defaults["decoupled_weight_decay"] = False
            self._group_of = assign_groups([k for k, _ in named], groups)
            entries = [{"params": [p for (_, p), g in zip(named, self._group_of) if g == 0]}]
            for j, (_, values) in enumerate(groups):
                entries.append(dict(values, params=[p for (_, p), g in zip(named, self._group_of) if g == 1 + j]))
            super(FusedAdam, self).__init__(entries, defaults)
        self._built = True
        # torch's numbering of the tensors: consecutive over the groups in order, model order inside a group (one group: model order)
        self._order = [i for g in range(len(self.param_groups)) for i, gi in enumerate(self._group_of) if gi == g]
        self._route = (None, None, None)   # (TrainableSet, groups that hold a live tensor, its GroupTable): rebuilt when the set changes
        self._group_scalars = None         # the guarded grouped step's device block of per-group scalars
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

    def add_param_group(self, param_group):
        if getattr(self, "_built", False):
            raise RuntimeError("FusedAdam: parameter groups are fixed at construction (groups=): a group is a set of ranges of "
                               "the model's flat buffer")
        return super(FusedAdam, self).add_param_group(param_group)

    def _group_route(self, ts):
        """``(live groups, GroupTable)`` of a trainable set: the groups that hold a live tensor, and -- built at its first use,
        once per set -- the live ranges split at group boundaries."""
        if self._route[0] is not ts:
            live = tuple(sorted({g for g, on in zip(self._group_of, ts.mask) if on}))
            self._route = (ts, live, None)
        return self._route[1], self._route[2]

    def _group_table(self, ts):
        if self._route[2] is None:
            triples = []   # in buffer order (not the model's), touching tensors of one group merged into one range
            for lo, hi, g in sorted((off, off + n, g) for g, on, (off, n, shape, dead)
                                    in zip(self._group_of, ts.mask, self.model._param_slices) if on and not dead and n > 0):
                if triples and triples[-1][1] == lo and triples[-1][2] == g:
                    triples[-1] = (triples[-1][0], hi, g)
                else:
                    triples.append((lo, hi, g))
            self._route = (ts, self._route[1], self.model.engine.group_table(triples, len(self.param_groups)))
        return self._route[2]

    # ---- per-tensor tables: layer-wise adaptive steps and grad_norms() -----------------------------
    def _tensor_route(self, ts):
        """What the per-tensor calls need for a trainable set, built at its first use and once per set: the ``TensorTable`` with
        one range per live tensor (buffer order), the statistics buffer, and the names of those tensors in
        ``named_parameters()`` order with the device permutation that brings table order into it (None: they agree)."""
        if self._lamb[0] is not ts:
            eng = self.model.engine
            rows = []
            for idx, ((name, _), g, on, (off, n, shape, dead)) in enumerate(zip(self.model.named_parameters(), self._group_of, ts.mask,
                                                                               self.model._param_slices)):
                if on and not dead and n > 0:
                    adapt = self.param_groups[g].get("layer_adaptation")
                    rows.append((off, off + n, g, int(len(shape) >= 2 if adapt is None else adapt), idx, name))
            order = sorted(range(len(rows)), key=lambda i: rows[i][0])                 # table row -> position in model order
            table = eng.tensor_table([rows[i][:4] for i in order], len(self.param_groups))
            row_of = {i: r for r, i in enumerate(order)}
            perm = [row_of[i] for i in range(len(rows))]
            perm_dev = None if perm == list(range(len(rows))) else torch.tensor(perm, dtype=torch.int64, device=eng.flat_params.device)
            stats = torch.zeros(len(rows), 3, dtype=torch.float32, device=eng.flat_params.device)
            stats[:, 2] = 1.0
            self._lamb = (ts, dict(table=table, stats=stats, names=[r[5] for r in rows], adapts=[bool(r[3]) for r in rows], perm=perm_dev,
                                   sumsq=torch.zeros(len(rows), dtype=torch.float64, device=eng.flat_params.device)))
        return self._lamb[1]

    def _stat(self, col):
        if not self.layer_adaptation:
            raise RuntimeError("this optimizer takes plain Adam steps (layer_adaptation=False)")
        route = self._lamb[1]
        if route is None:
            raise RuntimeError("no step() yet: the per-tensor statistics belong to the tensors of the last step")
        view = route["stats"][:, col]
        return view if route["perm"] is None else view[route["perm"]]

    @property
    def tensor_names(self):
        """``named_parameters()`` keys of the tensors the per-tensor statistics speak of (the live, non-dead ones of the last
        ``step()`` or ``grad_norms()``), in their order."""
        return None if self._lamb[1] is None else list(self._lamb[1]["names"])

    @property
    def tensor_adapts(self):
        """One flag per entry of ``tensor_names``: the tensor's step is scaled by its trust ratio (always False without
        ``layer_adaptation``)."""
        if self._lamb[1] is None:
            return None
        return [a and self.layer_adaptation for a in self._lamb[1]["adapts"]]

    @property
    def weight_norms(self):
        """Per tensor ``||w||`` before the last applied step (0 for a tensor that does not adapt)."""
        return self._stat(0)

    @property
    def update_norms(self):
        """Per tensor ``||u||`` of the last applied step (0 for a tensor that does not adapt)."""
        return self._stat(1)

    @property
    def trust_ratios(self):
        """Per tensor the trust ratio of the last applied step (1 for a tensor that does not adapt)."""
        return self._stat(2)

    @torch.no_grad()
    def grad_norms(self):
        """Per-tensor L2 norms of the gradient ``step()`` would read now, a float64 device tensor in the order of
        ``tensor_names``: two launches for all tensors and no synchronisation."""
        ts = self.model.trainable(self._gather_grads())
        if ts.empty:
            return torch.zeros(0, dtype=torch.float64, device=self.model.engine.flat_params.device)
        route = self._tensor_route(ts)
        norms = self.model.engine.tensor_norms(self.model.engine.grads(), route["table"], out=route["sumsq"])
        return norms.clone() if route["perm"] is None else norms[route["perm"]]

    def _gather_grads(self):
        """Bring gradients the autograd path left in tensors of their own into the flat gradient buffer; one flag per parameter:
        it has a gradient (a parameter without one -- frozen, or dropped by the caller -- is left alone, as torch.optim.Adam does)."""
        flat_g = self.model.engine.grads()
        lo = flat_g.data_ptr()
        hi = lo + flat_g.numel() * 4
        has_grad = []
        for p, (off, n, shape, dead) in zip(self.model.parameters(), self.model._param_slices):
            has_grad.append(p.grad is not None)
            if p.grad is not None and not (lo <= p.grad.data_ptr() < hi):
                flat_g[off:off + n].copy_(p.grad.reshape(-1))
        return has_grad

    def _step_lamb(self, ts, m, v, ema):
        """The layer-wise adaptive step: the norm's two launches on the guarded path, then the three of
        ``lamb_step`` over the set's tensor table with the values of every group as ``param_groups`` holds them NOW."""
        eng = self.model.engine
        route = self._tensor_route(ts)
        table = route["table"]
        values = [(g["lr"], g["eps"], g["weight_decay"], g.get("decoupled_weight_decay", False)) for g in self.param_groups]
        betas = self.param_groups[0]["betas"]
        decay = 0.0 if ema is None else self.ema_decay
        state = None
        if self.guarded:
            state, scratch = self._guard_buffers()
            if self._group_scalars is None or self._group_scalars.device != eng.flat_params.device:
                self._group_scalars = eng.new_group_scalars()
            eng.grad_norm_groups(state, scratch, self._group_scalars, table, values, self.max_grad_norm, self.skip_nonfinite, betas,
                                 whole=ts.full)
        else:
            self._step += 1
        eng.lamb_step(m, v, ema, table, route["stats"], values, step=self._step, state=state, betas=betas,
                      max_trust_ratio=self.max_trust_ratio, ema_decay=decay, ema_warmup=self.ema_warmup)

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
        # gradients produced by the autograd path live in separate tensors: gather them
        has_grad = self._gather_grads()
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
        if self.layer_adaptation:
            self._step_lamb(ts, m, v, ema)
            return loss
        live_groups, _ = self._group_route(ts)
        group = self.param_groups[live_groups[0]]
        if len(live_groups) > 1 or group.get("decoupled_weight_decay", False):
            self._step_groups(ts, m, v, ema)
            return loss
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

    def _step_groups(self, ts, m, v, ema):
        """The step over parameter groups: the values of every group as ``param_groups`` holds them NOW, in the
        launch arguments; the table from the set's cache."""
        eng = self.model.engine
        table = self._group_table(ts)
        values = [(g["lr"], g["eps"], g["weight_decay"], g.get("decoupled_weight_decay", False)) for g in self.param_groups]
        betas = self.param_groups[0]["betas"]
        decay = 0.0 if ema is None else self.ema_decay
        if self.guarded:
            state, scratch = self._guard_buffers()
            if self._group_scalars is None or self._group_scalars.device != eng.flat_params.device:
                self._group_scalars = eng.new_group_scalars()
            eng.grad_norm_groups(state, scratch, self._group_scalars, table, values, self.max_grad_norm, self.skip_nonfinite, betas,
                                 whole=ts.full)
            eng.adam_step_guarded_groups(m, v, ema, table, state, self._group_scalars, decay, self.ema_warmup)
        else:
            self._step += 1
            eng.adam_step_groups(m, v, ema, table, self._step, values, betas, decay, self.ema_warmup)

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
        number = {idx: k for k, idx in enumerate(self._order)}
        if step > 0:
            for idx, (off, n, shape, dead) in enumerate(self.model._param_slices):
                if dead or not self._trained[idx]:   # (a tensor frozen in every step so far has no state, as in torch)
                    continue
                state[number[idx]] = {"step": torch.tensor(float(step)),
                              "exp_avg": m[off:off + n].view(shape).clone(),
                              "exp_avg_sq": v[off:off + n].view(shape).clone()}
        groups = []
        first = 0
        for g in self.param_groups:
            gg = {k: val for k, val in g.items() if k != "params"}
            gg["params"] = list(range(first, first + len(g["params"])))
            first += len(g["params"])
            groups.append(gg)
        return {"state": dict(sorted(state.items())), "param_groups": groups}

    def load_state_dict(self, sd):
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups (%d, this optimizer %d)"
                             % (len(sd["param_groups"]), len(self.param_groups)))
        for i, (g, sg) in enumerate(zip(self.param_groups, sd["param_groups"])):
            if len(sg["params"]) != len(g["params"]):
                raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group "
                                 "(group %d: %d tensors, this optimizer %d)" % (i, len(sg["params"]), len(g["params"])))
        m, v = self._buffers()
        m.zero_()
        v.zero_()
        step = 0
        self._trained = [False] * len(self.model._param_slices)
        self._last_set = None
        # the checkpoint's own numbers, group by group, against ours (torch maps them the same way)
        theirs = [k for sg in sd["param_groups"] for k in sg["params"]]
        tensor_of = dict(zip(theirs, self._order))
        for key, st in sd["state"].items():
            idx = tensor_of[int(key)]
            off, n, shape, dead = self.model._param_slices[idx]
            self._trained[idx] = True
            m[off:off + n].copy_(st["exp_avg"].reshape(-1))
            v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1))
            step = max(step, int(float(st["step"])))
        self._step = step
        if self.guarded:
            self._guard_buffers()[0][3] = step
        for g, sg in zip(self.param_groups, sd["param_groups"]):
            for k in ("lr", "betas", "eps", "weight_decay") + tuple(k for k in ("decoupled_weight_decay", "layer_adaptation") if k in g):
                if k in sg:
                    g[k] = tuple(sg[k]) if k == "betas" else sg[k]
