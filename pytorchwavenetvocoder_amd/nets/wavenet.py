# -*- coding: utf-8 -*-
"""MI355X-native drop-in for ``wavenet_vocoder.nets.wavenet`` (reference wavenet.py).

Same public surface as the reference module -- ``encode_mu_law``, ``decode_mu_law``,
``initialize``, ``OneHot``, ``CausalConv1d``, ``UpSampling``, ``WaveNet`` with the reference's
constructor, ``forward(x, h)`` contract and ``state_dict`` keys/shapes -- but ``WaveNet.forward``
and its backward run in the hand-written HIP kernels of ``libwavenet_hip.so`` (C ABI:
include/wavenet_hip.h).  The ``nn.Conv1d`` / ``nn.ConvTranspose2d`` sub-modules are parameter
containers only (so ``model.apply(initialize)``, ``load_state_dict`` and checkpoints behave like
the reference's, wavenet.py:57-63, train.py:325-331): their tensors are views into ONE flat fp32
buffer that the kernels, the fused Adam and the RCCL all-reduce operate on.

There is no CPU path: calling the model with CPU tensors raises.
"""
import logging
import re
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import _lib
from ..engine import WaveNetEngine, _stream_handle, coalesce_ranges, key_to_kind


class TrainableSet(object):
    """What a tuple of per-parameter flags means for the flat buffers (``WaveNet.trainable``)."""
    __slots__ = ("mask", "ranges", "n_live", "full", "empty", "first_layer", "needs", "_engine", "_table")

    def __init__(self, model, mask):
        slices = model._param_slices
        self.mask = mask
        # what the backward pass has to reach: the lowest layer with a trainable tensor of its own (n_layers: none), pulled down
        # to 0 by a trainable front conv or upsampling layer (both sit below every layer), and one bit per non-layer part
        self.first_layer, self.needs = model._engine.n_layers, 0
        for on, (key, _) in zip(mask, model.named_parameters()):
            if not on:
                continue
            kind, layer = key_to_kind(key)
            if kind in (_lib.P_POST1_W, _lib.P_POST1_B, _lib.P_POST2_W, _lib.P_POST2_B):
                self.needs |= _lib.NEED_POST
            elif kind in (_lib.P_CAUSAL_W, _lib.P_CAUSAL_B):
                self.needs |= _lib.NEED_FRONT
            elif kind in (_lib.P_UP_W, _lib.P_UP_B):
                self.needs |= _lib.NEED_UP
            else:
                self.first_layer = min(self.first_layer, layer)
        if self.needs & (_lib.NEED_FRONT | _lib.NEED_UP):
            self.first_layer = 0
        self.ranges = coalesce_ranges((off, off + n) for on, (off, n, shape, dead) in zip(mask, slices) if on and not dead)
        self.n_live = sum(hi - lo for lo, hi in self.ranges)
        self.full = all(on or dead for on, (off, n, shape, dead) in zip(mask, slices))
        self.empty = not self.ranges
        self._engine, self._table = model._engine, None

    @property
    def table(self):
        """The device ``LiveTable`` of the ranges (None when full or empty), built at its first use: the optimizer needs it,
        the backward pass and the autograd route do not."""
        if self._table is None and not (self.full or self.empty):
            self._table = self._engine.live_table(self.ranges)
        return self._table


def encode_mu_law(x, mu=256):
    """Mu-law encoding (reference wavenet.py:17-30).

    Args:
        x (ndarray): Audio signal with the range from -1 to 1.
        mu (int): Quantized level.

    Returns:
        ndarray: Quantized audio signal with the range from 0 to mu - 1.
    """
    mu = mu - 1
    fx = np.sign(x) * np.log(1 + mu * np.abs(x)) / np.log(1 + mu)
    return np.floor((fx + 1) / 2 * mu + 0.5).astype(np.int64)


def decode_mu_law(y, mu=256):
    """Mu-law decoding (reference wavenet.py:33-47)."""
    mu = mu - 1
    fx = (y - 0.5) / mu * 2 - 1
    x = np.sign(fx) / mu * ((1 + mu) ** np.abs(fx) - 1)
    return x


def truncated_probs(logits, inv_temperature, top_k, top_p):
    """Class probabilities of a temperature / top-k / top-p draw from ``logits`` (Q,): the set rule of the decode kernels
    (csrc/wn_sample.h) in torch.  s = fp32(logits * inv_temperature); A = the classes whose s is at least the
    k-th largest (ties kept; k = 0 or k >= Q: all); B = the classes of A whose s is at least tau, the largest value whose upper
    set holds top_p of A's probability (ties kept); the result is the softmax of s over B and 0 elsewhere."""
    s = logits.float() * torch.tensor(inv_temperature, dtype=torch.float32, device=logits.device)
    keep = torch.ones_like(s, dtype=torch.bool)
    if 0 < top_k < s.numel():
        keep = s >= torch.topk(s, int(top_k)).values[-1]
    e = torch.where(keep, torch.exp((s - s.max()).double()), torch.zeros((), dtype=torch.float64, device=s.device))
    if top_p < 1.0:
        mass = (e[None, :] * (s[None, :] >= s[:, None])).sum(dim=1)   # mass[q] = probability of A's classes with s >= s_q
        ok = keep & (mass >= top_p * e.sum())
        e = torch.where(s >= s[ok].max(), e, torch.zeros_like(e))
    return (e / e.sum()).float()


def initialize(m):
    """Xavier init for Conv1d, ones/zeros for ConvTranspose2d (reference wavenet.py:50-63).

    In-place, so it writes straight through the parameter views into the flat buffer.
    """
    if isinstance(m, nn.Conv1d):
        nn.init.xavier_uniform_(m.weight)
        nn.init.constant_(m.bias, 0.0)
    if isinstance(m, nn.ConvTranspose2d):
        nn.init.constant_(m.weight, 1.0)
        nn.init.constant_(m.bias, 0.0)


class OneHot(nn.Module):
    """One-hot conversion (reference wavenet.py:66-92).  Kept for API compatibility; the WaveNet
    forward never materialises it (the front convolution is a gather, csrc/wn_elem.hip)."""

    def __init__(self, depth):
        super(OneHot, self).__init__()
        self.depth = depth

    def forward(self, x):
        x = x % self.depth
        x = torch.unsqueeze(x, 2)
        x_onehot = x.new_zeros(x.size(0), x.size(1), self.depth).float()
        return x_onehot.scatter_(2, x, 1)


class CausalConv1d(nn.Module):
    """1D dilated causal convolution (reference wavenet.py:95-121).

    Stand-alone ``forward`` runs the HIP causal-conv op (taps as K-segments of one f32-MFMA
    contraction); inside ``WaveNet`` the module only holds the parameters.
    """

    def __init__(self, in_channels, out_channels, kernel_size, dilation=1, bias=True):
        super(CausalConv1d, self).__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.dilation = dilation
        self.padding = (kernel_size - 1) * dilation
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size,
                              padding=self.padding, dilation=dilation, bias=bias)

    def forward(self, x):
        """x (B, C, T) float -> (B, C', T) on the HIP op ``wn_op_causal_conv``.  Differentiable like the reference's module
        (wavenet.py:95-121 is an ordinary ``nn.Module``): when a gradient is asked for -- x or the conv parameters require grad
        under an enabled grad mode -- the call goes through ``_CausalConv1dFunction``, whose backward is the HIP op
        ``wn_op_causal_conv_backward`` (dx with the taps transposed, dW / db as fixed-order sums over time)."""
        if not x.is_cuda:
            raise _lib.WnError("CausalConv1d runs on the GPU HIP path only (no CPU fallback)")
        w, b = self.conv.weight, self.conv.bias
        if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)):
            return _CausalConv1dFunction.apply(x, w, b, self.dilation)
        return _causal_conv_hip(x, w.detach(), None if b is None else b.detach(), self.dilation)


def _causal_conv_hip(x, w, b, dilation):
    import ctypes
    lib = _lib.load_library()
    if x.dtype != torch.float32 or w.dtype != torch.float32:
        raise _lib.WnError("CausalConv1d on the HIP path is fp32 (got %s / %s)" % (x.dtype, w.dtype))
    x = x.contiguous()
    B, C, T = x.shape
    Cout, Cin, K = w.shape
    if C != Cin:
        raise ValueError("expected %d input channels, got %d" % (Cin, C))
    w = w.contiguous()
    b = b.contiguous() if b is not None else torch.zeros(Cout, device=x.device)
    y = torch.empty(B, Cout, T, device=x.device, dtype=torch.float32)
    scratch = torch.empty(w.numel(), device=x.device, dtype=torch.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    rc = lib.wn_op_causal_conv(w.data_ptr(), b.data_ptr(), x.data_ptr(), y.data_ptr(), scratch.data_ptr(),
                               B, T, Cin, Cout, K, int(dilation), st)
    lib.check(rc, "wn_op_causal_conv")
    return y


class _CausalConv1dFunction(torch.autograd.Function):
    """``CausalConv1d.forward`` with a gradient: forward = wn_op_causal_conv, backward = wn_op_causal_conv_backward (autograd of
    the reference's Conv1d + slice, wavenet.py:105-121)."""

    @staticmethod
    def forward(ctx, x, w, b, dilation):
        ctx.save_for_backward(x, w)
        ctx.dilation, ctx.has_bias = int(dilation), b is not None
        return _causal_conv_hip(x.detach(), w.detach(), None if b is None else b.detach(), dilation)

    @staticmethod
    def backward(ctx, dy):
        import ctypes
        x, w = ctx.saved_tensors
        lib = _lib.load_library()
        x = x.detach().contiguous()
        w = w.detach().contiguous()
        dy = dy.contiguous().float()
        B, Cin, T = x.shape
        Cout, _, K = w.shape
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(w) if need_w else None
        db = torch.empty(Cout, device=x.device, dtype=torch.float32) if need_b else None
        n = lib.wn_op_causal_conv_backward_scratch_floats(B, T, Cin, Cout, K)
        scratch = torch.empty(max(int(n), 1), device=x.device, dtype=torch.float32)
        st = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
        rc = lib.wn_op_causal_conv_backward(w.data_ptr(), x.data_ptr(), dy.data_ptr(), dx.data_ptr() if need_x else None,
                                            dw.data_ptr() if need_w else None, db.data_ptr() if need_b else None,
                                            scratch.data_ptr(), B, T, Cin, Cout, K, ctx.dilation, st)
        lib.check(rc, "wn_op_causal_conv_backward")
        return dx, dw, db, None


class UpSampling(nn.Module):
    """Upsampling with a (1, U) transposed convolution (reference wavenet.py:124-154).

    ``out[b, c, f*U + j] = h[b, c, f] * w[j] + bias`` -- inside ``WaveNet`` this is never
    materialised (applied at frame rate inside the gate, csrc/wn_elem.hip / wn_fused.hip).
    """

    def __init__(self, upsampling_factor, bias=True):
        super(UpSampling, self).__init__()
        self.upsampling_factor = upsampling_factor
        self.bias = bias
        self.conv = nn.ConvTranspose2d(1, 1, kernel_size=(1, self.upsampling_factor),
                                       stride=(1, self.upsampling_factor), bias=self.bias)

    def forward(self, x):
        """x (B, C, T) -> (B, C, T * upsampling_factor).  On the GPU: the HIP op ``wn_op_upsampling`` (what ``generate()``
        calls); when a gradient is asked for (x or the conv parameters require grad under an enabled grad mode) through
        ``_UpSamplingFunction``, whose backward is the closed form of the transposed convolution -- the stand-alone module stays
        differentiable as in the reference.  On the CPU the closed form below (shape tests of the reference)."""
        if x.is_cuda:
            w, b = self.conv.weight, self.conv.bias
            if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or (b is not None and b.requires_grad)):
                return _UpSamplingFunction.apply(x, w, b, self.upsampling_factor)
            return _upsampling_hip(x, w.detach(), None if b is None else b.detach(), self.upsampling_factor)
        w = self.conv.weight.view(-1)
        y = x.unsqueeze(-1) * w
        if self.conv.bias is not None:
            y = y + self.conv.bias
        return y.reshape(x.size(0), x.size(1), -1)


def _upsampling_hip(x, w, b, U):
    import ctypes
    lib = _lib.load_library()
    x = x.contiguous().float()
    B, C, F_ = x.shape
    w = w.reshape(-1).contiguous()
    b = b.contiguous() if b is not None else None
    y = torch.empty(B, C, F_ * U, device=x.device, dtype=torch.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    rc = lib.wn_op_upsampling(w.data_ptr(), b.data_ptr() if b is not None else None, x.data_ptr(), y.data_ptr(), B, C, F_, U, st)
    lib.check(rc, "wn_op_upsampling")
    return y


class _UpSamplingFunction(torch.autograd.Function):
    """``UpSampling.forward`` with a gradient: forward = wn_op_upsampling; y[b, c, f U + j] = x[b, c, f] w[j] + bias, so
    dx = sum_j w[j] dy[.., f, j], dw[j] = sum x dy[.., j], dbias = sum dy (three reductions of (B, C, F, U) views)."""

    @staticmethod
    def forward(ctx, x, w, b, U):
        ctx.save_for_backward(x, w)
        ctx.U, ctx.has_bias = U, b is not None
        return _upsampling_hip(x.detach(), w.detach(), None if b is None else b.detach(), U)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy4 = dy.reshape(x.size(0), x.size(1), x.size(2), ctx.U)
        dx = (dy4 * w.reshape(-1)).sum(-1).to(x.dtype) if ctx.needs_input_grad[0] else None
        dw = (dy4 * x.float().unsqueeze(-1)).sum((0, 1, 2)).reshape(w.shape).to(w.dtype) if ctx.needs_input_grad[1] else None
        db = dy.sum().reshape(1).to(w.dtype) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db, None


class _WaveNetFunction(torch.autograd.Function):
    """autograd bridge: forward = wn_forward, backward = wn_backward (one flat gradient buffer); with h requiring a gradient
    wn_backward_dh, which also writes dL/dh (without the weight gradients when no parameter requires one)."""

    @staticmethod
    def forward(ctx, model, x, h, *params):
        eng = model._engine
        logits = eng.forward(x, h)
        model._fwd_serial += 1
        ctx.model = model
        ctx.serial = model._fwd_serial
        ctx.h_dtype = h.dtype
        return logits.transpose(1, 2)

    @staticmethod
    def backward(ctx, grad_out):
        model = ctx.model
        if ctx.serial != model._fwd_serial:
            raise _lib.WnError("WaveNet backward after a newer forward: the HIP path keeps the activations "
                               "of the latest forward only")
        eng = model._engine
        if grad_out.is_contiguous() and grad_out.dtype == torch.float32:   # (B, T, Q) -> the kernels' (B, Q, T) on the HIP op
            B, T, Q = grad_out.shape
            dl = torch.empty((B, Q, T), dtype=torch.float32, device=grad_out.device)
            st = _stream_handle(grad_out.device)
            eng.lib.check(eng.lib.wn_op_transpose_last2(grad_out.data_ptr(), dl.data_ptr(), B, T, Q, st), "wn_op_transpose_last2")
        else:   # a view that already is (B, Q, T) underneath (e.g. the transposed logits themselves), or another dtype
            dl = grad_out.transpose(1, 2).contiguous().float()
        dh = None
        if ctx.needs_input_grad[2]:
            h = eng._last_inputs[1]
            dh = torch.empty(h.shape, dtype=torch.float32, device=h.device)
        if not any(ctx.needs_input_grad[3:]):   # a frozen model: dh alone
            eng.backward(dl, dh=dh, param_grads=False)
            return (None, None, dh.to(ctx.h_dtype)) + (None,) * len(model._param_slices)
        # the same needs loss_and_backward derives from requires_grad, here from what autograd asks for
        ts = model.trainable(ctx.needs_input_grad[3:])
        needs = {} if ts.full else {"first_layer": 0 if dh is not None else ts.first_layer, "needs": ts.needs}
        flat = eng.backward(dl, dh=dh, **needs).clone()
        grads = []
        for on, (off, n, shape, dead) in zip(ts.mask, model._param_slices):
            grads.append(flat[off:off + n].view(shape) if on else None)
        return (None, None, None if dh is None else dh.to(ctx.h_dtype)) + tuple(grads)


class WaveNet(nn.Module):
    """Conditional WaveNet (reference wavenet.py:157-210) on the MI355X HIP path.

    Args:
        n_quantize (int): Number of quantization.
        n_aux (int): Number of aux feature dimension.
        n_resch (int): Number of filter channels for residual block.
        n_skipch (int): Number of filter channels for skip connection.
        dilation_depth (int): Number of dilation depth (e.g. if set 10, max dilation = 2^(10-1)).
        dilation_repeat (int): Number of dilation repeat.
        kernel_size (int): Filter size of dilated causal convolution.
        upsampling_factor (int): Upsampling factor.
        n_mixture (int): NOT a reference argument.  0 (default) = the reference's n_quantize-way softmax head;
            > 0 = mixture-of-logistics head with that many components (BASELINE configs[3]): ``conv_post_2`` then
            has 3 * n_mixture channels (mixture logits, means, log-scales), the input stays the mu-law one-hot
            front end, the loss is ``mol_loss_and_backward`` and generation draws from the mixture.
        log_scale_min (float): mixture head only -- clamp of the predicted log-scales, used by the loss AND by sampling.
    """

    def __init__(self, n_quantize=256, n_aux=28, n_resch=512, n_skipch=256,
                 dilation_depth=10, dilation_repeat=3, kernel_size=2, upsampling_factor=0, n_mixture=0, _library=None,
                 log_scale_min=-7.0):
        super(WaveNet, self).__init__()
        self.n_mixture = n_mixture
        # mixture head: clamp of the predicted log-scales, ONE value for the likelihood (mol_loss_and_backward) and for
        # sampling (the decode kernels), so that training and generation cannot disagree.  A constructor argument, so it
        # lives in the model configuration (train.py writes it into model.conf, decode.py rebuilds the model from it) and
        # state_dict keeps exactly the reference's parameter keys.
        self.log_scale_min = float(log_scale_min)
        self.out_channels = 3 * n_mixture if n_mixture > 0 else n_quantize
        self.n_aux = n_aux
        self.n_quantize = n_quantize
        self.n_resch = n_resch
        self.n_skipch = n_skipch
        self.kernel_size = kernel_size
        self.dilation_depth = dilation_depth
        self.dilation_repeat = dilation_repeat
        self.upsampling_factor = upsampling_factor

        self.dilations = [2 ** i for i in range(self.dilation_depth)] * self.dilation_repeat
        self.receptive_field = (self.kernel_size - 1) * sum(self.dilations) + 1

        # parameter containers, registered in the reference's order (wavenet.py:187-210)
        self.onehot = OneHot(self.n_quantize)
        self.causal = CausalConv1d(self.n_quantize, self.n_resch, self.kernel_size)
        if self.upsampling_factor > 0:
            self.upsampling = UpSampling(self.upsampling_factor)
        self.dil_sigmoid = nn.ModuleList()
        self.dil_tanh = nn.ModuleList()
        self.aux_1x1_sigmoid = nn.ModuleList()
        self.aux_1x1_tanh = nn.ModuleList()
        self.skip_1x1 = nn.ModuleList()
        self.res_1x1 = nn.ModuleList()
        for d in self.dilations:
            self.dil_sigmoid += [CausalConv1d(self.n_resch, self.n_resch, self.kernel_size, d)]
            self.dil_tanh += [CausalConv1d(self.n_resch, self.n_resch, self.kernel_size, d)]
            self.aux_1x1_sigmoid += [nn.Conv1d(self.n_aux, self.n_resch, 1)]
            self.aux_1x1_tanh += [nn.Conv1d(self.n_aux, self.n_resch, 1)]
            self.skip_1x1 += [nn.Conv1d(self.n_resch, self.n_skipch, 1)]
            self.res_1x1 += [nn.Conv1d(self.n_resch, self.n_resch, 1)]
        self.conv_post_1 = nn.Conv1d(self.n_skipch, self.n_skipch, 1)
        self.conv_post_2 = nn.Conv1d(self.n_skipch, self.out_channels, 1)

        # the HIP engine (loads libwavenet_hip.so; raises when the extension is unavailable)
        object.__setattr__(self, "_engine", WaveNetEngine(
            n_quantize, n_aux, n_resch, n_skipch, dilation_depth, dilation_repeat, kernel_size,
            upsampling_factor, device="cpu", library=_library, out_channels=3 * n_mixture))
        assert self._engine.receptive_field == self.receptive_field
        self._fwd_serial = 0
        self.distill_parts = None   # (total, ce, kl) means of the last distillation step, a device tensor
        self.criterion_parts = None   # (criterion, plain ce mean, divisor) of the last step with class / position weights or smoothing
        self._param_slices = []
        self._trainable_cache = {}   # trainable(): flags as given -> TrainableSet
        self._flatten()

    # ---- flat storage -------------------------------------------------------------------------
    def _flatten(self):
        """(Re)build the flat parameter buffer on the parameters' device and point every
        nn.Parameter at its slice."""
        eng = self._engine
        named = list(self.named_parameters())
        device = named[0][1].device
        for _, p in named:
            if p.dtype != torch.float32:
                raise _lib.WnError("the HIP WaveNet path is fp32 (parity gate 1e-4); got %s" % p.dtype)
            if p.device != device:
                raise _lib.WnError("all WaveNet parameters must live on one device")
        flat = torch.empty(eng.n_params, dtype=torch.float32, device=device)
        slices = []
        with torch.no_grad():
            for k, p in named:
                kind, layer = key_to_kind(k)
                off, n = eng.param_slice(kind, layer)
                assert n == p.numel(), k
                flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + n].view(p.shape)
                dead = (eng.dead_range[0] <= off < eng.dead_range[1])
                slices.append((off, n, tuple(p.shape), dead))
        eng.device = device
        eng.flat_params = flat
        eng.flat_grads = None
        eng.release_accumulation()
        eng._ws = None
        eng._ws_key = None
        eng.release_eval_workspace()
        eng._version_sources = tuple(p for _, p in named)
        eng._fwd_version = None
        self._param_slices = slices

    def _apply(self, fn, *args, **kwargs):
        out = super(WaveNet, self)._apply(fn, *args, **kwargs)
        self._flatten()
        return out

    @property
    def engine(self):
        return self._engine

    # ---- forward ------------------------------------------------------------------------------
    def forward(self, x, h):
        """Forward calculation (reference wavenet.py:212-241).

        Args:
            x (Tensor): Long tensor variable with the shape (B, T).
            h (Tensor): Float tensor variable with the shape (B, n_aux, T)
                (or (B, n_aux, T / upsampling_factor) with the upsampling layer).

        Returns:
            Tensor: Float tensor variable with the shape (B, T, n_quantize)
                (a transposed view of a (B, n_quantize, T) buffer, like the reference's result).
        """
        params = tuple(self.parameters())
        return _WaveNetFunction.apply(self, x, h, *params)

    def loss_and_backward(self, x, h, t, t_start=None, grad_scale=1.0, events=None, layers_per_bucket=0, aux_grad=False,
                          lengths=None, micro_step=None, _accumulate=True, teacher_logits=None, distill_alpha=0.5,
                          distill_temperature=1.0, class_weights=None, label_smoothing=0.0, position_weights=None,
                          normalize="weights"):
        """Fused training half-step: forward -> CrossEntropy on ``[:, t_start:]`` -> backward
        (reference train.py:533-538) without an autograd graph.

        Leaves the gradients in the flat buffer (``p.grad`` of every parameter is a view of it;
        ``None`` for the dead last ``res_1x1`` and for every frozen parameter, ``requires_grad`` False:
        its range of the buffer holds unspecified values that neither ``FusedAdam`` nor its norm reads;
        with nothing trainable and no ``aux_grad`` the call is forward and loss, no backward launch)
        and returns the mean loss as a 1-element device
        tensor (no host sync).  ``grad_scale`` multiplies the gradients (1/world_size for DP).
        ``aux_grad=True``: returns ``(loss, dh)`` with dh = d(loss)/dh (scaled by ``grad_scale`` as well).

        ``lengths``: a padded batch of sequences of unequal length -- B host integers (a sequence of ints or a CPU integer
        tensor), ``1 <= lengths[b] <= T``.  The loss is the mean over the positions ``[t_start, lengths[b])`` of every
        sequence, i.e. ``nn.CrossEntropyLoss()`` with the targets behind each end set to -100; x, h and t may hold anything
        finite on the padding.  Only the loss knows the lengths: the network is causal, so the padding reaches no valid
        position, its ``dlogits`` is exactly zero and so is ``dh`` on every frame wholly behind a sequence's end.  The
        residual stack still computes the whole (B, T) rectangle.  None: every sequence runs to T.

        ``micro_step=(i, A)``, ``0 <= i < A``: gradient accumulation -- this call is micro-batch i of A whose gradients are
        summed in front of ONE ``optimizer.step()``.  One ``grad_accumulate`` launch follows the backward launches on the
        caller's stream (nothing synchronises): i = 0 opens a cycle and sets the engine's accumulator (``engine.grad_accum``,
        allocated by the first cycle) to this gradient, 0 < i < A - 1 adds to it, i = A - 1 adds the accumulator INTO the gradient
        buffer and closes the cycle.  So after a non-final micro-step ``p.grad`` (the flat buffer) holds that micro-batch's own
        gradient, after the final one the sum ((g0 + g1) + g2) + ... in plain fp32 -- the bits torch's ``p.grad += g`` gives.
        ``grad_scale`` keeps its meaning, it multiplies this micro-batch's gradient: ``grad_scale_i = N_i / sum_j N_j`` (N: loss
        positions) makes the sum the gradient of the mean over all loss positions of the cycle.  The micro-batches may differ in
        B, T, ``lengths`` and ``aux_grad`` (``dh`` belongs to its micro-batch and is never accumulated).  ``None`` or A = 1:
        the plain call, no launch, no accumulator.  Out of order, a changed A, a plain call or ``optimizer.step()`` inside a
        cycle raise; ``engine.abandon_accumulation()`` drops a cycle.

        ``teacher_logits``: knowledge distillation -- a (B, Q, T) fp32 device tensor in the physical layout ``engine.forward``
        returns (``teacher.teacher_logits(x, h)``), a constant.  The loss per position becomes
        ``(1 - distill_alpha) * ce + distill_alpha * distill_temperature^2 * KL(softmax(teacher / temperature) ||
        softmax(student / temperature))`` (``engine.distill_loss``): the step is ``engine.forward`` -> ``distill_loss`` ->
        ``engine.backward``, the logits reach memory.  Returns the mean of that loss; its parts (total, ce, unweighted kl) stay
        in ``self.distill_parts``, a 3-element device tensor.  Everything else composes unchanged.  ``None``, or
        ``distill_alpha == 0`` (the teacher then has no say): the fused cross-entropy step.

        ``class_weights`` ((Q,) fp32), ``label_smoothing`` (in [0, 1)), ``position_weights`` ((B, T) fp32): the criterion becomes
        torch's ``CrossEntropyLoss(weight=class_weights, label_smoothing=label_smoothing)`` with one more weight per position
        (``engine.weighted_loss``, where the formulas are): the step is ``engine.forward`` -> ``weighted_loss`` ->
        ``engine.backward``, the logits reach memory.  ``normalize="weights"`` divides by the sum of the weights of the targets
        (torch's mean), ``"positions"`` by the number of loss positions: with shares ``N_k / sum N`` as ``grad_scale`` over ranks
        and micro-batches ``"positions"`` pools exactly, ``"weights"`` gives the share-weighted mean of per-call weighted means
        (what torch DDP gives).  Weights must be finite and >= 0 (checked on host tensors, once per tensor).  Returns the
        criterion; (criterion, plain unweighted cross-entropy mean, divisor) stay in ``self.criterion_parts``, a 3-element device
        tensor.  Everything else composes unchanged; not together with ``teacher_logits``.  With the three options at their
        defaults the step is the fused one, launch for launch."""
        weighted = class_weights is not None or float(label_smoothing) != 0.0 or position_weights is not None
        if weighted or normalize != "weights":
            if self.n_mixture > 0:
                raise ValueError("the weighted cross-entropy is defined for the softmax head (n_mixture = 0)")
            if teacher_logits is not None:
                raise ValueError("class_weights / label_smoothing / position_weights cannot go with teacher_logits")
            eps, class_weights, position_weights = self._engine.weighted_loss_args(
                class_weights, label_smoothing, position_weights, normalize, x.shape[0], self.n_quantize, x.shape[1])
        if teacher_logits is not None:
            if self.n_mixture > 0:
                raise ValueError("distillation is defined for the softmax head (n_mixture = 0)")
            if not 0.0 <= float(distill_alpha) <= 1.0:
                raise ValueError("distill_alpha = %r outside [0, 1]" % (distill_alpha,))
            if not (float(distill_temperature) > 0.0 and float(distill_temperature) < float("inf")):
                raise ValueError("distill_temperature = %r must be positive and finite" % (distill_temperature,))
        eng = self._engine
        mode = eng.begin_micro_step(micro_step)
        if t_start is None:
            t_start = eng.receptive_field
        distilling = teacher_logits is not None and float(distill_alpha) != 0.0
        if distilling or weighted:   # another loss head beside the fused epilogue: the logits reach memory
            ragged = {} if lengths is None else {"lengths": lengths}
            ts = self.trainable()
            nothing = ts.empty and not aux_grad   # forward and loss only: no backward launch
            logits = eng.forward(x, h)
            self._fwd_serial += 1
            if distilling:
                loss3, dlogits = eng.distill_loss(logits, teacher_logits, t, distill_alpha, distill_temperature, t_start=t_start,
                                                  grad_scale=grad_scale, want_grad=not nothing, **ragged)
                self.distill_parts = loss3
            else:
                loss3, dlogits = eng.weighted_loss(logits, t, class_weights, eps, position_weights, normalize, t_start=t_start,
                                                   grad_scale=grad_scale, want_grad=not nothing, **ragged)
                self.criterion_parts = loss3
            loss = loss3[0:1]
            if nothing:
                return self._nothing_to_train(loss, events, micro_step, mode)
            dh = self._aux_grad_buffer(h) if aux_grad else None
            flat = eng.backward(dlogits, events=events, layers_per_bucket=layers_per_bucket, t_first=t_start, dh=dh,
                                **self._backward_needs(ts, aux_grad, events))
            self._finish_micro_step(micro_step, mode, _accumulate)
            self._point_grads(flat)
            return (loss, dh) if aux_grad else loss
        # forward + loss in one call: the cross-entropy is the epilogue of conv_post_2 where the model allows it (the logits
        # never reach memory), and the backward pass runs its post-net part over the loss window only
        ragged = {} if lengths is None else {"lengths": lengths}
        ts = self.trainable()
        nothing = ts.empty and not aux_grad   # forward and loss only: no backward launch
        loss, dlogits = eng.forward_loss(x, h, t, t_start=t_start, grad_scale=grad_scale, want_grad=not nothing, **ragged)
        self._fwd_serial += 1
        if nothing:
            return self._nothing_to_train(loss, events, micro_step, mode)
        dh = self._aux_grad_buffer(h) if aux_grad else None
        flat = eng.backward(dlogits, events=events, layers_per_bucket=layers_per_bucket, t_first=t_start, dh=dh,
                            **self._backward_needs(ts, aux_grad, events))
        self._finish_micro_step(micro_step, mode, _accumulate)
        self._point_grads(flat)
        return (loss, dh) if aux_grad else loss

    def teacher_logits(self, x, h):
        """This model as a distillation teacher: its logits for ``loss_and_backward(teacher_logits=...)`` of a student --
        ``engine.forward`` without an autograd graph, the physical (B, Q, T) fp32 tensor."""
        with torch.no_grad():
            return self._engine.forward(x, h)

    def _backward_needs(self, ts, aux_grad, events=None):
        """What ``engine.backward`` has to compute for the model's trainable set: nothing extra when every parameter trains (the
        full pass through the entry points of before), ``first_layer`` / ``needs`` otherwise -- ``first_layer`` 0 with ``dh``,
        which needs every layer -- and ``param_grads=False`` for ``dh`` alone."""
        if ts.full:
            return {}
        if ts.empty:
            if events:
                raise ValueError("bucket events with nothing trainable: there is no gradient to reduce")
            return {"param_grads": False}
        return {"first_layer": 0 if aux_grad else ts.first_layer, "needs": ts.needs}

    def _point_grads(self, flat):
        """``p.grad`` of every trainable parameter = its view of the flat gradient; None for the dead last ``res_1x1`` and for
        frozen parameters (``requires_grad`` False), whose ranges of the buffer hold unspecified values nobody reads."""
        for p, (off, n, shape, dead) in zip(self.parameters(), self._param_slices):
            p.grad = None if (dead or flat is None or not p.requires_grad) else flat[off:off + n].view(shape)

    def _nothing_to_train(self, loss, events, micro_step, mode):
        """Every parameter frozen and no ``dh`` asked for: the call was forward and loss.  An accumulation cycle still advances
        and every ``p.grad`` is None.  Bucket events cannot be served (no backward call records them): an error."""
        if events:
            raise ValueError("bucket events with nothing trainable: no backward pass runs, so there is no gradient to reduce")
        if mode is not None:
            self._engine.end_micro_step(micro_step)
        for p in self.parameters():
            p.grad = None
        return loss

    # ---- frozen parameters ---------------------------------------------------------------------------------
    def trainable(self, mask=None):
        """The trainable set derived from ``mask`` -- one bool per parameter in ``parameters()`` order; default: the
        parameters' own ``requires_grad``, THE interface for freezing (it may change between steps).  Returns a
        ``TrainableSet``: ``mask``, ``ranges`` (live ranges of the flat buffers: trainable and not the dead last ``res_1x1``,
        coalesced into maximal sorted ``[lo, hi)`` runs), ``n_live``, ``full`` (every non-dead parameter: the whole-buffer
        launches of a model without frozen parameters apply, nothing else is built), ``empty``, and ``table`` (the device
        ``LiveTable`` of the ranges; None when full or empty).  Rebuilt only when the tuple of flags (or the flat buffer) changes."""
        # this runs in front of the first launch of every training call, so a hit costs the parameter tuple the engine keeps (no
        # walk over the module tree) and one dictionary lookup by the flags as given; the rest runs once per tuple of flags
        raw = tuple(p.requires_grad for p in self._engine._version_sources) if mask is None else tuple(bool(on) for on in mask)
        key = (raw, self._engine.flat_params.data_ptr(), str(self._engine.device))
        ts = self._trainable_cache.get(key)
        if ts is None:
            if len(raw) != len(self._param_slices):
                raise ValueError("the mask has %d entries, the model %d parameters" % (len(raw), len(self._param_slices)))
            if len(self._trainable_cache) >= 8:   # of sets that came and went the oldest goes
                self._trainable_cache.pop(next(iter(self._trainable_cache)))
            # (the dead tensors never count: the flags and an optimizer's "has a gradient" then describe the same set)
            ts = TrainableSet(self, tuple(on and not dead for on, (off, n, shape, dead) in zip(raw, self._param_slices)))
            self._trainable_cache[key] = ts
        return ts

    def _set_requires_grad(self, pattern, matched_value, others_value):
        rx = re.compile(pattern)
        named = list(self.named_parameters())
        hits = [rx.search(k) is not None for k, _ in named]
        if not any(hits):
            raise ValueError("pattern %r matches no parameter of the model (keys look like %r)" % (pattern, named[0][0]))
        changed = 0
        for (k, p), hit in zip(named, hits):
            want = matched_value if hit else others_value
            if want is not None and p.requires_grad != want:
                p.requires_grad_(want)
                changed += 1
        return changed

    def freeze(self, pattern):
        """Freeze (``requires_grad_(False)``) every parameter whose ``named_parameters()`` key ``re.search`` es ``pattern``; the
        others stay as they are.  Returns the number of tensors changed; ValueError when the pattern matches nothing.  A frozen
        parameter gets no gradient (``p.grad`` None) and ``FusedAdam`` leaves its weights, moments and average bit for bit."""
        return self._set_requires_grad(pattern, False, None)

    def train_only(self, pattern):
        """Train exactly the parameters whose key matches ``pattern``: those become trainable, every other one frozen.
        Returns the number of tensors changed; ValueError when the pattern matches nothing."""
        return self._set_requires_grad(pattern, True, False)

    def _finish_micro_step(self, micro_step, mode, accumulate):
        """The ``grad_accumulate`` launch of a micro-step behind its backward launches, and the cycle's next state.
        ``accumulate=False`` (GradientReducer on the final micro-step): the caller issues the launch itself, bucket by bucket."""
        if mode is None:
            return
        if accumulate:
            self._engine.accumulate_grads(mode)
        self._engine.end_micro_step(micro_step)

    def _aux_grad_buffer(self, h):
        return torch.empty(h.shape, dtype=torch.float32, device=self._engine.device)

    def mol_loss_and_backward(self, x, h, y, t_start=None, grad_scale=1.0, num_classes=65536, log_scale_min=None,
                              events=None, layers_per_bucket=0, aux_grad=False, lengths=None, micro_step=None, _accumulate=True):
        """Training half-step of the mixture-of-logistics head (``n_mixture > 0``): forward -> mean negative
        log-likelihood of the waveform ``y`` (B, T) in [-1, 1] (the value of the NEXT sample at every position,
        like ``t`` of the softmax head) on ``[:, t_start:]`` -> backward.  Gradients land as in
        ``loss_and_backward``; ``aux_grad=True`` returns ``(loss, dh)``, ``lengths`` masks the padding and ``micro_step=(i, A)``
        accumulates the gradient over micro-batches as there."""
        if self.n_mixture <= 0:
            raise ValueError("this model has the softmax head (n_mixture = 0)")
        # ONE clamp for the likelihood and for sampling: the constructor's value (it travels in model.conf; a per-call
        # value would be lost with the checkpoint and generation would clamp differently from training)
        if log_scale_min is not None and float(log_scale_min) != self.log_scale_min:
            raise ValueError("log_scale_min=%g differs from the model's %g: pass it to the constructor "
                             "(train.py --log_scale_min), it is part of the model configuration"
                             % (float(log_scale_min), self.log_scale_min))
        log_scale_min = self.log_scale_min
        eng = self._engine
        mode = eng.begin_micro_step(micro_step)
        out = eng.forward(x, h)
        self._fwd_serial += 1
        if t_start is None:
            t_start = eng.receptive_field
        ragged = {} if lengths is None else {"lengths": lengths}
        ts = self.trainable()
        nothing = ts.empty and not aux_grad   # forward and loss only: no backward launch
        loss, dout = eng.mol_loss(out, y, t_start=t_start, grad_scale=grad_scale, num_classes=num_classes,
                                  log_scale_min=log_scale_min, want_grad=not nothing, **ragged)
        if nothing:
            return self._nothing_to_train(loss, events, micro_step, mode)
        dh = self._aux_grad_buffer(h) if aux_grad else None
        flat = eng.backward(dout, events=events, layers_per_bucket=layers_per_bucket, t_first=t_start, dh=dh,
                            **self._backward_needs(ts, aux_grad, events))
        self._finish_micro_step(micro_step, mode, _accumulate)
        self._point_grads(flat)
        return (loss, dh) if aux_grad else loss

    def evaluate(self, x, h, t=None, y=None, t_start=None, lengths=None, acc=None, num_classes=65536):
        """Score held-out data: ``(row_nll, counts)`` -- per sequence the SUM of the negative log-likelihoods over the positions
        ``[t_start, lengths[b])`` (device tensor (B,), no host sync) and the number of those positions (host ints), see
        ``WaveNetEngine.forward_nll``.  Softmax head: the class targets ``t``; mixture head: the waveform ``y``.  ``acc``:
        a 1-element float64 device tensor the batch total is added to.  No gradient exists afterwards and none is touched:
        ``p.grad``, the training workspace and a pending ``backward`` of an earlier forward stay valid, in ``train()`` and
        ``eval()`` mode alike (the network has no mode-dependent layer)."""
        if (t is None) == (y is None):
            raise ValueError("evaluate takes exactly one of t (softmax head) and y (mixture-of-logistics head)")
        if self.n_mixture > 0:
            if y is None:
                raise ValueError("this model has the mixture-of-logistics head (n_mixture = %d): pass the waveform y"
                                 % self.n_mixture)
            return self._engine.forward_nll(x, h, y=y, t_start=t_start, lengths=lengths, acc=acc, num_classes=num_classes,
                                            log_scale_min=self.log_scale_min)
        if t is None:
            raise ValueError("this model has the softmax head (n_mixture = 0): pass the class targets t")
        return self._engine.forward_nll(x, h, target=t, t_start=t_start, lengths=lengths, acc=acc)

    # ---- generation (reference wavenet.py:243-511) --------------------------------------------
    def _window_logits(self, x, h_up):
        """Logits (T, Q) for ONE window with the aux features already at sample rate."""
        eng = self._gen_engine()
        logits = eng.forward(x, h_up)
        return logits[0].transpose(0, 1)

    def _gen_engine(self):
        """Engine that treats h as already up-sampled (the reference bypasses the upsampling layer
        inside generate(), wavenet.py:258-259,273-283).  The flat layout keeps the upsampling
        tensors at the very end, so the U=0 layout is a prefix of this model's buffer."""
        if self.upsampling_factor == 0:
            return self._engine
        eng = getattr(self, "_gen_eng", None)
        if eng is None or eng.device != self._engine.device or \
                eng.flat_params.data_ptr() != self._engine.flat_params.data_ptr():
            eng = WaveNetEngine(self.n_quantize, self.n_aux, self.n_resch, self.n_skipch, self.dilation_depth,
                                self.dilation_repeat, self.kernel_size, 0, device=self._engine.device,
                                library=self._engine.lib, out_channels=3 * self.n_mixture)
            eng.flat_params = self._engine.flat_params[:eng.n_params]
            object.__setattr__(self, "_gen_eng", eng)
        return eng

    def generate(self, x, h, n_samples, intervals=None, mode="sampling", temperature=1.0, top_k=None, top_p=None):
        """Naive generation (reference wavenet.py:243-307): every new sample is the last output of
        a full forward over the newest ``receptive_field`` samples (activations left of the window
        count as zero, which is what distinguishes it from ``fast_generate``).  Every window runs
        through the HIP forward; the token buffer stays on the device.

        Args:
            x (Tensor): Long tensor variable with the shape (1, T).
            h (Tensor): Float tensor variable with the shape (1, n_aux, n_samples + T).
            n_samples (int): Number of samples to be generated.
            intervals (int): Log interval.
            mode (str): "sampling" or "argmax".
            temperature, top_k, top_p: as in ``fast_generate``; the same set rule, applied in torch before the draw.

        Returns:
            ndarray: Generated quantized waveform (n_samples,).
        """
        if mode not in ("sampling", "argmax"):
            logging.error("mode should be sampling or argmax")
            sys.exit(1)
        setting = self._sampling_setting(mode, temperature, top_k, top_p)
        if self.n_mixture > 0:
            # the 3 * n_mixture outputs are mixture parameters, not class logits: a softmax / argmax over them would
            # return meaningless tokens.  The queue-based generators draw from the mixture on the device.
            raise ValueError("generate() is the reference's softmax-head generator; a model with the mixture-of-logistics "
                             "head (n_mixture = %d) generates with fast_generate / batch_fast_generate" % self.n_mixture)
        rf = self.receptive_field
        with torch.no_grad():
            if self.upsampling_factor > 0:
                h = self.upsampling(h)
            n_pad = max(rf - x.size(1), 0)
            n_ctx = x.size(1) + n_pad
            tokens = torch.full((1, n_ctx + n_samples), self.n_quantize // 2, dtype=torch.long, device=h.device)
            tokens[:, n_pad:n_ctx] = x
            if n_pad > 0:
                h = F.pad(h, (n_pad, 0), "replicate")
            tick, done_at_tick = time.time(), 0
            for i in range(n_samples):
                end = n_ctx + i
                logits = self._window_logits(tokens[:, end - rf:end].contiguous(), h[:, :, end - rf:end].contiguous())[-1]
                if mode == "argmax":
                    tokens[0, end] = logits.argmax()
                else:
                    probs = F.softmax(logits, dim=0) if setting is None else truncated_probs(logits, *setting)
                    tokens[0, end] = torch.distributions.Categorical(probs).sample()
                if intervals is not None and (i + 1) % intervals == 0:
                    per = (time.time() - tick) / (i + 1 - done_at_tick)
                    logging.info("%d/%d estimated time = %.3f sec (%.3f sec / sample)" % (
                        i + 1, n_samples, (n_samples - i - 1) * per, per))
                    tick, done_at_tick = time.time(), i + 1
            return tokens[0, n_ctx:].cpu().numpy()

    def _sampling_setting(self, mode, temperature, top_k, top_p):
        """(inverse temperature, top_k, top_p) of a generation call, None for the identity; ValueError for values out of range,
        for parameters other than the identity with mode "argmax" and with the mixture-of-logistics head."""
        if self.n_mixture > 0:
            try:
                s = self.engine.sampling_setting("argmax", temperature, top_k, top_p)
            except ValueError:
                raise ValueError("temperature / top_k / top_p should be a valid setting, and are not defined for the "
                                 "mixture-of-logistics head (n_mixture = %d)" % self.n_mixture)
            return None
        s = self.engine.sampling_setting(mode, temperature, top_k, top_p)
        return None if s is None else (s.inv_temperature, s.top_k, s.top_p)

    def _decode(self, x, h, n_samples_list, intervals, mode, temperature=1.0, top_k=None, top_p=None):
        """Run the HIP decode kernel (csrc/wn_decode.hip); returns per-utterance LongTensors."""
        if mode not in ("sampling", "argmax"):
            logging.error("mode should be sampling or argmax")
            sys.exit(1)
        self._sampling_setting(mode, temperature, top_k, top_p)
        if self.n_mixture > 0:  # the mixture head has no argmax: both modes draw from the mixture
            mode = "mol"
        start = [time.time(), 0]

        def progress(done, total):
            if intervals is not None and done > start[1]:
                dt = (time.time() - start[0]) / (done - start[1])
                logging.info("%d/%d estimated time = %.3f sec (%.3f sec / sample)" % (
                    done, total, (total - done) * dt, dt))
                start[0], start[1] = time.time(), done

        with torch.no_grad():
            return self.engine.decode(x, h, list(n_samples_list), mode=mode,
                                      chunk=intervals if intervals else 4096, progress=progress,
                                      log_scale_min=self.log_scale_min, temperature=temperature, top_k=top_k, top_p=top_p)

    def fast_generate(self, x, h, n_samples, intervals=None, mode="sampling", temperature=1.0, top_k=None, top_p=None):
        """Generate a waveform with the queue algorithm (reference wavenet.py:309-395) on the HIP
        decode path: one persistent workgroup per utterance for the model sizes the decode kernel
        covers, layer-wise launches on [channels x batch] operands for any other size; the context
        walk fills the dilation queues, then ``n_samples`` tokens are emitted; nothing but the result
        leaves the GPU.

        Args:
            x (tensor): Long tensor variable with the shape  (1, T).
            h (tensor): Float tensor variable with the shape  (1, n_aux, n_samples + T)
                (frames if the model up-samples).
            n_samples (int): Number of samples to be generated.
            intervals (int): Log interval.
            mode (str): "sampling" or "argmax".
            temperature (float): sampling temperature T > 0: the logits are multiplied by 1 / T (mode "sampling").
            top_k (int): keep the k most probable classes (ties at the k-th kept); 0 or None: off.
            top_p (float): keep the smallest set of most probable classes holding this probability mass (ties kept), taken
                after top_k; 1 or None: off.  The defaults are the reference's plain draw; the choice is made inside the
                decode kernels (csrc/wn_sample.h).

        Returns:
            ndarray: Generated quantized waveform (n_samples,).
        """
        return self._decode(x, h, [n_samples], intervals, mode, temperature, top_k, top_p)[0].cpu().numpy()

    def batch_fast_generate(self, x, h, n_samples_list, intervals=None, mode="sampling", temperature=1.0, top_k=None, top_p=None):
        """Batched queue-algorithm generation (reference wavenet.py:397-511): one workgroup per
        utterance, each stops at its own length.  Returns the list of generated waveforms in order
        of completion (shortest first), like the reference.

        Args:
            x (tensor): Long tensor variable with the shape (B, T).
            h (tensor): Float tensor variable with the shape (B, n_aux, max(n_samples_list) + T).
            n_samples_list (list): List of number of samples to be generated (B,).
            intervals (int): Log interval.
            mode (str): "sampling" or "argmax".
            temperature, top_k, top_p: as in ``fast_generate``, one setting for the whole batch.
        """
        order = sorted(range(len(n_samples_list)), key=lambda i: (n_samples_list[i], i))
        toks = self._decode(x, h, n_samples_list, intervals, mode, temperature, top_k, top_p)
        return [toks[i].cpu().numpy() for i in order]
