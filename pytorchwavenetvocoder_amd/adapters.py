# -*- coding: utf-8 -*-
"""Low-rank adapters for fine-tuning: ``W = W0 + (alpha / rank) * B @ A`` on chosen weights of a trained WaveNet.

One speaker-independent model and a small file per voice: the model's tensors stay where they are, the adapter owns two thin
factors per adapted tensor, ``A [rank, cols]`` and ``B [rows, rank]`` (a conv weight ``(out, in, K)`` is the matrix
``[out, in * K]``), all of them in ONE flat ``nn.Parameter``.  The kernels of the model never learn of it: they read the flat
weight buffer, which always holds the MERGED weights, and the backward pass leaves the full ``dW`` in the flat gradient buffer.
Two fused operations over those buffers do the rest (``wn_lora_merge`` / ``wn_lora_project``, include/wavenet_hip.h):

``merge()``     writes ``base + scale * B @ A`` into the weight buffer for every adapted tensor: one launch.
``project()``   turns the ``dW`` of every adapted tensor into ``dA = scale * B^T dW`` and ``dB = scale * dW A^T``: two launches.

A training step is ``loss_and_backward`` -> ``project()`` -> ``AdapterAdam.step()`` (which ends with the merge).  Under data
parallelism the projection follows the gradient reduction, so every rank projects the same reduced ``dW`` and the ranks' adapters
stay bit-identical without further communication.
"""
import ctypes
import math
import re
from collections import OrderedDict

import torch
from torch import nn

from . import _lib
from .engine import _ptr, _stream_handle

DEFAULT_TARGETS = r"^(dil_sigmoid|dil_tanh|skip_1x1|res_1x1)\.\d+\.(conv\.)?weight$"
CONFIG_KEYS = ("n_quantize", "n_aux", "n_resch", "n_skipch", "dilation_depth", "dilation_repeat", "kernel_size",
               "upsampling_factor", "n_mixture")


def model_config(model):
    """The constructor arguments that fix the model's tensors, as an adapter file records them."""
    return OrderedDict((k, int(getattr(model, k))) for k in CONFIG_KEYS)


class LowRankAdapters(object):
    """Adapters on the tensors of ``model`` whose ``named_parameters()`` key ``re.search`` es ``targets`` (default: the weights of
    ``dil_sigmoid``, ``dil_tanh``, ``skip_1x1`` and ``res_1x1`` of every layer; the dead last ``res_1x1`` is never a target).

    ``rank``        1 .. 64 and at most ``min(rows, cols)`` of every target.
    ``alpha``       ``scale = alpha / rank``; None: ``alpha = rank``, scale 1.
    ``seed``        ``A`` is drawn on the CPU from ``torch.Generator().manual_seed(seed)``, uniform in ``+- 1 / sqrt(cols)``, and
                    ``B`` starts at zero: the merged weights equal the pretrained ones and data-parallel ranks start identical.

    Construction copies the model's flat weights into ``base`` and makes the model's trainable set exactly the targets
    (``model.train_only``): the backward pass computes their ``dW`` and stops at the lowest adapted layer.  ``flat`` is the one
    ``nn.Parameter`` holding every ``A`` and ``B`` (``A[key]`` / ``B[key]`` are views of it), ``flat.grad`` the adapter's gradient.
    ValueError for a pattern that matches nothing, a match on a bias and a target smaller than the rank, naming the tensor."""

    def __init__(self, model, rank=8, alpha=None, targets=None, seed=0):
        if not hasattr(model, "engine"):
            raise TypeError("LowRankAdapters takes the WaveNet model (it works on the model's flat buffers)")
        rank = int(rank)
        if not 1 <= rank <= _lib.LORA_MAX_RANK:
            raise ValueError("rank %d outside [1, %d]" % (rank, _lib.LORA_MAX_RANK))
        self.model = model
        self.rank = rank
        self.alpha = float(rank if alpha is None else alpha)
        if not math.isfinite(self.alpha):
            raise ValueError("alpha must be finite")
        self.targets = DEFAULT_TARGETS if targets is None else targets
        rx = re.compile(self.targets)
        named = list(model.named_parameters())
        self.entries = []   # (key, index into parameters(), w_off, rows, cols, a_off, b_off, shape)
        off = 0
        for idx, ((key, p), (w_off, n, shape, dead)) in enumerate(zip(named, model._param_slices)):
            if dead or rx.search(key) is None:
                continue
            if len(shape) < 2:
                raise ValueError("targets %r matches %s, a bias: adapters go on weight matrices" % (self.targets, key))
            rows, cols = int(shape[0]), n // int(shape[0])
            if rank > min(rows, cols):
                raise ValueError("targets %r matches %s, a [%d, %d] matrix: smaller than the rank %d" % (self.targets, key, rows, cols, rank))
            self.entries.append((key, idx, w_off, rows, cols, off, off + rank * cols, tuple(shape)))
            off += rank * (rows + cols)
        if not self.entries:
            raise ValueError("targets %r matches no parameter of the model (keys look like %r)" % (self.targets, named[0][0]))
        self.n_adapter = off
        dev = model.engine.flat_params.device
        flat = torch.zeros(off, dtype=torch.float32)
        gen = torch.Generator().manual_seed(int(seed))
        for key, idx, w_off, rows, cols, a_off, b_off, shape in self.entries:
            bound = 1.0 / math.sqrt(cols)
            flat[a_off:a_off + rank * cols] = (torch.rand(rank * cols, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound
        self.flat = nn.Parameter(flat.to(dev))
        self.base = model.engine.flat_params.detach().clone()
        self._scratch = None
        self._folded = False
        self._build_table()
        self._pattern = "^(?:%s)$" % "|".join(re.escape(e[0]) for e in self.entries)
        model.train_only(self._pattern)

    @classmethod
    def from_state_dict(cls, model, sd):
        """The adapters an adapter file describes, attached to ``model`` (the base it was trained on): rank, alpha and the exact
        target keys come from the file.  ValueError when the file does not fit the model.  ``merge()`` applies them."""
        keys = [k for k, _ in sd["targets"]]
        names = set(k for k, _ in model.named_parameters())
        missing = [k for k in keys if k not in names]
        if missing or not keys:
            raise ValueError("the adapters' targets are not tensors of this model: %s" % (missing[:4] or "no targets"))
        ad = cls(model, rank=int(sd["rank"]), alpha=float(sd["alpha"]), targets="^(?:%s)$" % "|".join(re.escape(k) for k in keys))
        ad.load_state_dict(sd)
        return ad

    # ---- layout -------------------------------------------------------------------------------------
    @property
    def scale(self):
        return self.alpha / self.rank

    @property
    def keys(self):
        return [e[0] for e in self.entries]

    def _build_table(self):
        lib = self.model.engine.lib
        arr = (_lib.WnLoraEntry * len(self.entries))()
        for a, (key, idx, w_off, rows, cols, a_off, b_off, shape) in zip(arr, self.entries):
            a.w_off, a.rows, a.cols, a.rank, a.a_off, a.b_off, a.scale = w_off, rows, cols, self.rank, a_off, b_off, self.scale
        args = (ctypes.cast(arr, ctypes.c_void_p), len(self.entries), self.model.engine.n_params, self.n_adapter)
        words = lib.wn_lora_table(*(args + (None, 0)))
        if words < 0:
            raise _lib.WnError("wn_lora_table failed: %s" % lib.wn_last_error().decode())
        host = torch.zeros(int(words), dtype=torch.int64)
        if lib.wn_lora_table(*(args + (ctypes.c_void_p(host.data_ptr()), int(words)))) != words:
            raise _lib.WnError("wn_lora_table failed: %s" % lib.wn_last_error().decode())
        self._table = host
        self._dev_table = host.to(self.flat.device)
        self._scratch_floats = int(lib.wn_lora_scratch_floats(ctypes.c_void_p(host.data_ptr())))
        self._scratch = None

    def _views(self, buf, which):
        out = OrderedDict()
        for key, idx, w_off, rows, cols, a_off, b_off, shape in self.entries:
            if which == "A":
                out[key] = buf[a_off:a_off + self.rank * cols].view(self.rank, cols)
            else:
                out[key] = buf[b_off:b_off + rows * self.rank].view(rows, self.rank)
        return out

    @property
    def A(self):
        """Per target key the ``[rank, cols]`` view of ``flat``."""
        return self._views(self.flat.data, "A")

    @property
    def B(self):
        """Per target key the ``[rows, rank]`` view of ``flat``."""
        return self._views(self.flat.data, "B")

    def grad_views(self, which):
        """The views of ``flat.grad`` for ``which`` = "A" or "B" (after ``project()``)."""
        if self.flat.grad is None:
            raise RuntimeError("no adapter gradient yet: project() writes it")
        return self._views(self.flat.grad, which)

    def _ready(self):
        """The model's flat buffer may have moved (``model.to(device)``): the adapter's buffers follow it."""
        if self._folded:
            raise RuntimeError("these adapters were folded into the model: the model is a plain model now")
        eng = self.model.engine
        dev = eng.flat_params.device
        if self.flat.device != dev:
            grad = self.flat.grad
            self.flat.data = self.flat.data.to(dev)
            self.flat.grad = None if grad is None else grad.to(dev)
            self.base = self.base.to(dev)
            self._dev_table = self._table.to(dev)
            self._scratch = None
        eng._check_device(self.flat, self.base, self._dev_table)
        return eng

    # ---- the two fused operations --------------------------------------------------------------------
    @torch.no_grad()
    def merge(self):
        """``weights = base + scale * B @ A`` on every adapted tensor: one launch.  Bumps the engine's parameter epoch, so
        everything derived from the weights (packed weight sets) follows."""
        eng = self._ready()
        rc = eng.lib.wn_lora_merge(_ptr(self.base), _ptr(eng.flat_params), eng.n_params, _ptr(self.flat), self.n_adapter,
                                   ctypes.c_void_p(self._table.data_ptr()), _ptr(self._dev_table), _stream_handle(eng.device))
        eng.lib.check(rc, "wn_lora_merge")
        eng._params_epoch += 1

    @torch.no_grad()
    def project(self):
        """``flat.grad`` = the adapter's gradient from the ``dW`` the last ``loss_and_backward`` left in the engine's gradient
        buffer (two launches), and ``p.grad = None`` on the adapted parameters, which ``FusedAdam`` then leaves alone.  With
        ``micro_step`` it follows the FINAL micro-step: the operation is linear, so the projection of the sum is what the sum
        of projections would be.  RuntimeError when there is no gradient yet, inside an open accumulation cycle, and when an
        adapted tensor has been frozen."""
        eng = self._ready()
        if eng.accumulation is not None:
            raise RuntimeError("project() inside an accumulation cycle (%d of %d micro-steps done): the gradient buffer holds one "
                               "micro-batch, not the sum -- project after the final micro-step" % eng.accumulation)
        params = list(self.model.parameters())
        for key, idx, w_off, rows, cols, a_off, b_off, shape in self.entries:
            if not params[idx].requires_grad:
                raise RuntimeError("%s carries an adapter and has been frozen: its dW is not computed" % key)
        if eng.flat_grads is None or any(params[e[1]].grad is None for e in self.entries):
            raise RuntimeError("no gradient to project: loss_and_backward comes first (and project() once per gradient)")
        flat_g = eng.grads()
        lo, hi = flat_g.data_ptr(), flat_g.data_ptr() + 4 * flat_g.numel()
        for key, idx, w_off, rows, cols, a_off, b_off, shape in self.entries:   # gradients the autograd path left elsewhere
            g = params[idx].grad
            if not lo <= g.data_ptr() < hi:
                flat_g[w_off:w_off + rows * cols].copy_(g.reshape(-1))
        if self.flat.grad is None:
            self.flat.grad = torch.zeros_like(self.flat.data)
        if self._scratch is None:
            self._scratch = torch.empty(max(self._scratch_floats, 1), dtype=torch.float32, device=self.flat.device)
        rc = eng.lib.wn_lora_project(_ptr(flat_g), eng.n_params, _ptr(self.flat), _ptr(self.flat.grad), self.n_adapter,
                                     ctypes.c_void_p(self._table.data_ptr()), _ptr(self._dev_table), _ptr(self._scratch),
                                     self._scratch.numel(), _stream_handle(eng.device))
        eng.lib.check(rc, "wn_lora_project")
        for e in self.entries:
            params[e[1]].grad = None

    @torch.no_grad()
    def restore(self):
        """The adapted tensors get the bits of ``base`` back (the adapters keep their values: ``merge()`` applies them again)."""
        eng = self._ready()
        for key, idx, w_off, rows, cols, a_off, b_off, shape in self.entries:
            eng.flat_params[w_off:w_off + rows * cols].copy_(self.base[w_off:w_off + rows * cols])
        eng._params_epoch += 1

    @torch.no_grad()
    def fold(self):
        """Keep the merged weights and detach: the model is a plain model afterwards, every parameter trainable, and this
        object refuses further use."""
        self.merge()
        for p in self.model.parameters():
            p.requires_grad_(True)
            p.grad = None
        self._folded = True
        self.base = None
        self._scratch = None

    # ---- the small file per voice ----------------------------------------------------------------------
    def state_dict(self):
        """``A`` and ``B`` per target key (clones), rank, alpha, the target keys with their shapes and the model configuration."""
        return {"rank": self.rank, "alpha": self.alpha, "targets": [(e[0], tuple(e[7])) for e in self.entries],
                "config": dict(model_config(self.model)),
                "A": OrderedDict((k, v.detach().clone()) for k, v in self.A.items()),
                "B": OrderedDict((k, v.detach().clone()) for k, v in self.B.items())}

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Takes what ``state_dict`` gave.  ValueError when the model configuration, the rank, or the target keys and shapes
        differ from this object's.  The weights change at the next ``merge()``."""
        if self._folded:
            raise RuntimeError("these adapters were folded into the model")
        mine = dict(model_config(self.model))
        theirs = dict(sd["config"])
        if theirs != mine:
            diff = sorted(k for k in set(mine) | set(theirs) if mine.get(k) != theirs.get(k))
            raise ValueError("the adapters were made for another model configuration (%s differ)" % ", ".join(diff))
        if int(sd["rank"]) != self.rank:
            raise ValueError("the adapters have rank %d, this object rank %d" % (int(sd["rank"]), self.rank))
        want = [(e[0], tuple(e[7])) for e in self.entries]
        got = [(k, tuple(s)) for k, s in sd["targets"]]
        if got != want:
            raise ValueError("the adapters' targets differ from this object's: %s" % sorted(set(got) ^ set(want))[:4])
        for name, views in (("A", self.A), ("B", self.B)):
            if list(sd[name].keys()) != list(views.keys()):
                raise ValueError("the adapters' %s tensors do not carry the target keys" % name)
            for k, v in views.items():
                if tuple(sd[name][k].shape) != tuple(v.shape):
                    raise ValueError("%s of %s: shape %s, expected %s" % (name, k, tuple(sd[name][k].shape), tuple(v.shape)))
        for name, views in (("A", self.A), ("B", self.B)):
            for k, v in views.items():
                v.copy_(sd[name][k])
        if float(sd["alpha"]) != self.alpha:
            self.alpha = float(sd["alpha"])
            self._build_table()


class AdapterAdam(torch.optim.Optimizer):
    """Adam on the adapter's flat parameter: the library's generic ``wn_adam_step`` (guarded: ``wn_grad_norm`` +
    ``wn_adam_step_guarded``) on the adapter's buffers, then ``adapters.merge()``.  ``max_grad_norm`` / ``skip_nonfinite`` as in
    ``FusedAdam``, the norm being that of the adapter's gradient; a skipped step leaves adapters, moments and weights alone.
    ``state_dict()`` has ``torch.optim.Adam``'s format for the single parameter ``flat``.  The weight average, parameter groups and
    layer adaptation are not defined for adapters and refused."""

    def __init__(self, adapters, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False,
                 ema_decay=None, groups=None, layer_adaptation=False):
        if not isinstance(adapters, LowRankAdapters):
            raise TypeError("AdapterAdam takes a LowRankAdapters object")
        if ema_decay is not None:
            raise ValueError("AdapterAdam keeps no moving average of the weights (ema_decay): not defined for adapters")
        if groups:
            raise ValueError("AdapterAdam has one parameter, the adapter's flat buffer: parameter groups are not defined for adapters")
        if layer_adaptation:
            raise ValueError("layer-wise adaptive steps are not defined for adapters")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (None = no clipping)")
        self.adapters = adapters
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self.ema_decay = None
        self._step = 0
        self._exp_avg = self._exp_avg_sq = None
        self._opt_state = self._norm_scratch = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None)
        super(AdapterAdam, self).__init__([adapters.flat], defaults)

    def _buffers(self):
        flat = self.adapters.flat
        if self._exp_avg is None:
            self._exp_avg, self._exp_avg_sq = torch.zeros_like(flat.data), torch.zeros_like(flat.data)
        elif self._exp_avg.device != flat.device:
            self._exp_avg, self._exp_avg_sq = self._exp_avg.to(flat.device), self._exp_avg_sq.to(flat.device)
        return self._exp_avg, self._exp_avg_sq

    def _guard_buffers(self):
        eng = self.adapters.model.engine
        dev = self.adapters.flat.device
        if self._opt_state is None or self._opt_state.device != dev:
            old = self._opt_state
            self._opt_state = torch.zeros(eng.OPT_STATE_WORDS, dtype=torch.int64, device=dev)
            self._norm_scratch = torch.empty(int(eng.lib.wn_grad_norm_scratch_floats(self.adapters.n_adapter)), dtype=torch.float32,
                                             device=dev)
            if old is not None:
                self._opt_state.copy_(old)
            else:
                self._opt_state[3] = self._step
        return self._opt_state, self._norm_scratch

    @property
    def grad_norm(self):
        """0-dim device tensor: the norm of the adapter's gradient at the last ``step()``, before clipping; None unguarded."""
        if not self.guarded:
            return None
        return self.adapters.model.engine.opt_state_views(self._guard_buffers()[0])["total_norm"]

    def steps_applied(self):
        return self._step if not self.guarded else int(self._guard_buffers()[0][3])

    def steps_skipped(self):
        return 0 if not self.guarded else int(self._guard_buffers()[0][4])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ad = self.adapters
        eng = ad._ready()
        flat = ad.flat
        if flat.grad is None:
            raise RuntimeError("step() without an adapter gradient: loss_and_backward, then adapters.project(), then step()")
        m, v = self._buffers()
        g = self.param_groups[0]
        st = _stream_handle(eng.device)
        n = ad.n_adapter
        if self.guarded:
            state, scratch = self._guard_buffers()
            eng._check_device(m, v, state, scratch)
            rc = eng.lib.wn_grad_norm(_ptr(flat.grad), n, 0, 0, float(self.max_grad_norm) if self.max_grad_norm else 0.0,
                                      int(self.skip_nonfinite), float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                                      _ptr(scratch), _ptr(state), st)
            eng.lib.check(rc, "wn_grad_norm")
            rc = eng.lib.wn_adam_step_guarded(_ptr(flat), _ptr(flat.grad), _ptr(m), _ptr(v), n, float(g["eps"]),
                                              float(g["weight_decay"]), 0, 0, _ptr(state), st)
            eng.lib.check(rc, "wn_adam_step_guarded")
        else:
            eng._check_device(m, v)
            self._step += 1
            rc = eng.lib.wn_adam_step(_ptr(flat), _ptr(flat.grad), _ptr(m), _ptr(v), n, self._step, float(g["lr"]),
                                      float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]), 0, 0, st)
            eng.lib.check(rc, "wn_adam_step")
        ad.merge()
        return loss

    # ---- torch.optim.Adam compatible (de)serialisation --------------------------------------------------
    def state_dict(self):
        m, v = self._buffers()
        step = self.steps_applied()
        state = {}
        if step > 0:
            state[0] = {"step": torch.tensor(float(step)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        group = {k: val for k, val in self.param_groups[0].items() if k != "params"}
        group["params"] = [0]
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        if len(sd["param_groups"]) != 1 or len(sd["param_groups"][0]["params"]) != 1:
            raise ValueError("loaded state dict does not describe one parameter group with the one adapter parameter")
        m, v = self._buffers()
        m.zero_()
        v.zero_()
        step = 0
        for key, st in sd["state"].items():
            if tuple(st["exp_avg"].shape) != tuple(m.shape):
                raise ValueError("loaded moments have shape %s, the adapter's flat parameter %s" % (tuple(st["exp_avg"].shape), tuple(m.shape)))
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            step = int(float(st["step"]))
        self._step = step
        if self.guarded:
            self._guard_buffers()[0][3] = step
        g, sg = self.param_groups[0], sd["param_groups"][0]
        for k in ("lr", "betas", "eps", "weight_decay"):
            if k in sg:
                g[k] = tuple(sg[k]) if k == "betas" else sg[k]
