# -*- coding: utf-8 -*-
"""Device-side state of one WaveNet replica: flat parameter / gradient / Adam buffers and the
workspace the HIP library needs, plus thin wrappers around the C-ABI calls.

PyTorch is used here only for device memory, streams and (in ``DataParallelReducer``)
``torch.distributed``; every FLOP of the path runs in libwavenet_hip.so.
"""
import ctypes
import os
import warnings
import weakref

import torch

from . import _lib

# Launch modes every engine starts with: everything on the caller's stream, and the aux-path gradients as partial sums
# inside the gate kernel (WN_FLAG_AUX_FUSED: -3.4 % step time, profiles/r01/aux_fused_probe.txt; it applies to the fused
# split kernels with U % 16 == 0 and is ignored elsewhere).  The opt-in overlap modes (_lib.FLAG_BWD_OVERLAP /
# FLAG_FWD_OVERLAP) measured no faster on MI355X (profiles/r01/overlap_probe.txt).
# Round 5: WN_FLAG_DW_3PRODUCT (opt-in, NOT in the defaults): the weight-gradient contractions -- LEAF results, sums over every
# position of the minibatch that nothing else consumes -- with three of the six products of the operand split.  It meets the
# gradient gates with room (worst gradient tensor against the oracle at the three timed sizes 6.3e-6 / 6.3e-6 / 1.5e-5 of its
# maximum; six products 4.9e-6 / 6.3e-6 / 1.5e-5) and buys 3 - 4 % (headline step 9.84 -> 9.46 ms, recipe size 126 -> 117 ms, same
# box, profiles/r05/), but NOT the golden after-Adam gate (weights after one Adam step within 1e-2 lr of the reference's): on the
# small golden cases elements whose gradient is ~1e-8 -- where Adam's update lr g / (|g| + eps) is sign-like -- move by up to
# 2e-2 lr (tests/test_gpu_parity.py, r64_k2_up).  Parity first: every default-mode contraction stays fp32-equivalent; the flag is
# for callers who accept that (engine.flags |= _lib.FLAG_DW_3PRODUCT, or WN_ENGINE_FLAGS=262176), bench.py reports its step time
# beside the headline (extras.dw_3product), tests/test_gpu_fullsize.py keeps its 3e-5 gradient gate.
# WN_FLAG_DW_F16PAIR (round 5, DEFAULT): the same contractions with TWO FP16 pieces per operand (11 + 11 significand bits) and the
# three products h h + h l + l h on v_mfma_f32_32x32x16_f16 -- 2^-22 per product instead of the 2^-16 of two bf16 pieces, below
# the rounding of an fp32 running sum over a minibatch's positions -- at the three-bf16-product mode's speed (headline step 9.54 ->
# 9.08 ms, recipe size 119.0 -> 104.9 ms, configs[3] geometry 12.70 -> 12.17 ms, same box, profiles/r05/abk_f16pair_headline.txt,
# dw3_probe_f16pair.txt).  It meets EVERY gate of the six-product mode: golden gradients and the golden weights after Adam
# (tests/test_gpu_dw_f16pair.py), the full-size gradient gates with the six-product mode's own worst tensor (4.87e-6 / 1.49e-5,
# tests/test_gpu_fullsize.py).  fp16's 5 exponent bits need the size of the gradient: backward() passes the bound of the
# tensor its own loss call returned (a mean cross-entropy: |dlogits| <= grad_scale / positions), the kernels scale the gradient
# operand by 2^(e + 8), and a gradient that still leaves fp16's range is DETECTED (non-finite block result) and redone by the
# six-product launch issued behind every fp16 launch (an empty launch otherwise: 0.04 ms per step).  Any other gradient (autograd's
# grad_output, the mixture-of-logistics head) keeps the six bf16 products unless the caller gives backward(dlogits_bound=...).
# WN_FLAG_MM_F16PAIR (round 6, DEFAULT): the weights x activations contractions on the split matrix-core kernel k_gemm6 -- skip sum,
# post-net with the cross-entropy epilogue, their data gradients, the all-layer skip gradient; the per-layer contractions of wide
# models -- take the same fp16 pair split (three products, ~2^-22 each: the rounding of an fp32 running sum over >= 64 terms), each
# launch followed by a conditional six-product redo (an operand outside fp16's range raises a workspace word).  Same box: headline
# step 9.21 -> 8.72 ms (fwd_skip_sum 0.68 -> 0.43, bwd_dz_skip_all 0.80 -> 0.62; profiles/r06/abk_mm_f16.txt).  Gates on the
# benchmark's own instance against the reference module (tests/test_gpu_fullsize.py, bench.py `parity`): logits 4.9e-6 (six
# products 5.5e-6), worst gradient 8.3e-6 (8.2e-6); against the fp64 evaluation of the same step the worst gradient is 6.2e-6 --
# closer than the reference's own fp32 step (8.3e-6; profiles/r06/adam_gate_study.txt).
# WN_FLAG_FUSED_F16PAIR (round 6, DEFAULT): the fused 64-channel FORWARD block (taps, gate, res 1x1: k_resblock_fwd<K, FwdF16x2>) on the same
# split, block-scaled -- every weight image and every 64 x 32 operand tile by the power of two that puts its maximum at 2^12 /
# 2^14, so no magnitude leaves fp16's range and no redo exists.  Same box: 8.64 -> 8.43 ms per step (forward blocks 1.79 -> 1.55 ms,
# profiles/r06/abk_fused_f16.txt).  The backward data chain (k_chain64s) keeps six bf16 products.
DEFAULT_FLAGS = _lib.FLAG_AUX_FUSED | _lib.FLAG_DW_F16PAIR | _lib.FLAG_MM_F16PAIR | _lib.FLAG_FUSED_F16PAIR
SIX_PRODUCT_FLAGS = DEFAULT_FLAGS & ~_lib.NARROW_FLAGS   # every contraction fp32-equivalent (six bf16 products)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream_handle(device):
    if device.type == "cuda":
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    return None


class LiveTable(object):
    """The live ranges of a flat buffer for the ``*_live`` calls (include/wavenet_hip.h, ABI v16): ``ranges`` the sorted, disjoint
    ``(lo, hi)`` pairs, ``n_live`` their number of elements, ``table`` the int64 device tensor the kernels read (``lo``, ``hi``
    and the live elements in front of each range, as ``wn_live_table`` wrote them).  Built by ``WaveNetEngine.live_table``."""
    __slots__ = ("ranges", "n_ranges", "n_live", "n", "table")

    def __init__(self, ranges, n_live, n, table):
        self.ranges, self.n_ranges, self.n_live, self.n, self.table = ranges, len(ranges), int(n_live), int(n), table


class GroupTable(LiveTable):
    """A ``LiveTable`` whose ranges carry a parameter-group index (include/wavenet_hip.h, ABI v17): ``groups`` one index per
    range, ``n_groups`` the number of groups the indices refer to; ``table`` holds a fourth row, the indices, behind the three of
    a ``LiveTable`` (the ``*_live`` calls read it as it is).  Built by ``WaveNetEngine.group_table``."""
    __slots__ = ("groups", "n_groups")

    def __init__(self, ranges, groups, n_groups, n_live, n, table):
        LiveTable.__init__(self, ranges, n_live, n, table)
        self.groups, self.n_groups = groups, int(n_groups)


class TensorTable(GroupTable):
    """A ``GroupTable`` with ONE range per tensor (never coalesced) for ``lamb_step`` and ``tensor_norms`` (include/wavenet_hip.h,
    ABI v20): ``adapt`` one flag per range, ``n_blocks`` the blocks the ranges own (``ceil(len / _lib.TENSOR_CHUNK)`` each),
    ``scratch`` the per-block partial sums the calls write.  ``table`` holds the rows of a ``GroupTable`` first, so the
    ``*_live`` and ``*_groups`` norm calls read it as it is.  Built by ``WaveNetEngine.tensor_table``."""
    __slots__ = ("adapt", "n_blocks", "scratch")

    def __init__(self, ranges, groups, n_groups, n_live, n, table, adapt, n_blocks, scratch):
        GroupTable.__init__(self, ranges, groups, n_groups, n_live, n, table)
        self.adapt, self.n_blocks, self.scratch = adapt, int(n_blocks), scratch


def group_array(groups):
    """Host array of ``WnAdamGroup`` from ``(lr, eps, weight_decay, decoupled)`` tuples: what the ``*_groups`` calls take (the values
    travel in the launch arguments)."""
    arr = (_lib.WnAdamGroup * max(len(groups), 1))()
    for a, (lr, eps, wd, decoupled) in zip(arr, groups):
        a.lr, a.eps, a.weight_decay, a.decoupled = float(lr), float(eps), float(wd), int(bool(decoupled))
    return arr


def coalesce_ranges(ranges):
    """Sorted ``(lo, hi)`` pairs with empty ones dropped and touching or overlapping neighbours merged into maximal runs."""
    out = []
    for lo, hi in sorted((int(a), int(b)) for a, b in ranges if int(b) > int(a)):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


class WaveNetEngine(object):
    """Owns the flat buffers of one model replica.

    Args mirror ``WaveNet.__init__`` (reference wavenet.py:172-173).
    """

    def __init__(self, n_quantize=256, n_aux=28, n_resch=512, n_skipch=256, dilation_depth=10,
                 dilation_repeat=3, kernel_size=2, upsampling_factor=0, device="cpu", library=None, out_channels=0):
        self.lib = library if library is not None else _lib.load_library()
        self.cfg = _lib.WnConfig(n_quantize, n_aux, n_resch, n_skipch, dilation_depth, dilation_repeat,
                                 kernel_size, upsampling_factor, out_channels)
        self.out_channels = out_channels if out_channels > 0 else n_quantize
        self.device = torch.device(device)
        n = self.lib.wn_param_count(ctypes.byref(self.cfg))
        if n <= 0:
            raise _lib.WnError("invalid WaveNet configuration: %s" % self.lib.wn_last_error().decode())
        self.n_params = int(n)
        self.n_layers = self.lib.wn_num_layers(ctypes.byref(self.cfg))
        self.receptive_field = self.lib.wn_receptive_field(ctypes.byref(self.cfg))
        self.flat_params = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.flat_grads = None
        self.grad_accum = None    # the sum over the micro-batches of an accumulation cycle (layout of grads()); allocated by the first cycle
        self._accum = None        # an open cycle: (micro-steps done, A)
        self._ws = None
        self._ws_key = None
        self._eval_ws = None      # forward_nll's own workspace slot: scoring never evicts or rewrites the training one
        self._eval_ws_key = None
        self._lengths_key = None  # (lengths, device) of the int32 array _lengths_arg uploaded last
        self._lengths_dev = None
        self._eval_lengths = (None, None)  # the same pair for forward_nll
        self._distill_scratch = None  # partial sums of distill_loss (grown on demand; the call reads nothing it did not write)
        self._cew_scratch = None  # divisor and partial sums of weighted_loss (likewise)
        self._weights_seen = {}   # weighted_loss: name -> (weak reference, version, device copy) of the weight tensor checked last
        self._last_shape = None
        self._fwd_window = 0      # first loss position of the last forward_loss (0: a full forward)
        self._fwd_version = None  # parameter version the last forward packed its weight sets from
        self._fwd_flags = 0       # launch-mode flags of the last forward
        self._dlogits_bound = None  # (weak reference, version, max |dlogits|) of the gradient tensor the last loss call of this engine made
        self._params_epoch = 0    # bumped by every in-library parameter update (adam_step): torch cannot see those
        self._version_sources = ()  # tensors aliasing flat_params whose in-place version counters count as well
        self.ws_finite = True     # workspace() allocates zero-filled memory -> WN_FLAG_WS_FINITE (tests clear it)
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        self.lib.check(self.lib.wn_dead_param_range(ctypes.byref(self.cfg), ctypes.byref(lo), ctypes.byref(hi)),
                       "wn_dead_param_range")
        self.dead_range = (lo.value, hi.value)
        # launch-mode flags of wn_forward / wn_backward (include/wavenet_hip.h WN_FLAG_*); WN_ENGINE_FLAGS overrides
        # the default for A/B measurements (tools/overlap_probe.py)
        self.flags = int(os.environ.get("WN_ENGINE_FLAGS", str(DEFAULT_FLAGS)), 0)

    # ---- layout ---------------------------------------------------------------------------
    def param_slice(self, kind, layer=0):
        off, n = ctypes.c_int64(), ctypes.c_int64()
        self.lib.check(self.lib.wn_param_offset(ctypes.byref(self.cfg), kind, layer, ctypes.byref(off), ctypes.byref(n)),
                       "wn_param_offset")
        return off.value, n.value

    def bucket_ranges(self, layers_per_bucket):
        nb = self.lib.wn_num_buckets(ctypes.byref(self.cfg), layers_per_bucket)
        out = []
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        for i in range(nb):
            self.lib.check(self.lib.wn_bucket_range(ctypes.byref(self.cfg), layers_per_bucket, i, ctypes.byref(lo),
                                                    ctypes.byref(hi)), "wn_bucket_range")
            out.append((lo.value, hi.value))
        return out

    def live_table(self, ranges, n=None, device=None):
        """``LiveTable`` of the given ``(lo, hi)`` ranges of a buffer of ``n`` elements (default: the flat buffers) on ``device``
        (default: the engine's).  The ranges are taken as given -- non-empty, sorted, disjoint, inside ``[0, n)``;
        ``wn_live_table`` checks that and raises through ``wn_last_error`` (``coalesce_ranges`` tidies a list first).  One small
        host-to-device copy: build it once per freeze set, not per step."""
        n = self.n_params if n is None else int(n)
        ranges = [(int(a), int(b)) for a, b in ranges]
        nr = len(ranges)
        flat = (ctypes.c_int64 * max(2 * nr, 1))(*[x for r in ranges for x in r])
        host = torch.zeros(max(3 * nr, 1), dtype=torch.int64)
        n_live = self.lib.wn_live_table(ctypes.cast(flat, ctypes.c_void_p), nr, n, ctypes.c_void_p(host.data_ptr()))
        if n_live < 0:
            raise _lib.WnError("wn_live_table failed: %s" % self.lib.wn_last_error().decode())
        return LiveTable(ranges, n_live, n, host.to(self.device if device is None else device))

    def group_table(self, triples, n_groups, n=None, device=None):
        """``GroupTable`` of the given ``(lo, hi, group)`` triples -- ranges as for ``live_table``, ``group`` in
        ``[0, n_groups)``, ``n_groups`` at most ``_lib.MAX_PARAM_GROUPS``; ``wn_group_table`` checks all of it.  One small
        host-to-device copy: build it once per set of live ranges, not per step."""
        n = self.n_params if n is None else int(n)
        triples = [(int(a), int(b), int(c)) for a, b, c in triples]
        nr = len(triples)
        flat = (ctypes.c_int64 * max(3 * nr, 1))(*[x for r in triples for x in r])
        host = torch.zeros(max(4 * nr, 1), dtype=torch.int64)
        n_live = self.lib.wn_group_table(ctypes.cast(flat, ctypes.c_void_p), nr, n, int(n_groups), ctypes.c_void_p(host.data_ptr()))
        if n_live < 0:
            raise _lib.WnError("wn_group_table failed: %s" % self.lib.wn_last_error().decode())
        return GroupTable([(a, b) for a, b, _ in triples], [c for _, _, c in triples], n_groups, n_live, n,
                          host.to(self.device if device is None else device))

    def _live_args(self, live):
        self._check_device(live.table)
        if live.n != self.n_params:
            raise ValueError("the live table was built for a buffer of %d elements, the flat buffers hold %d" % (live.n, self.n_params))
        return _ptr(live.table), live.n_ranges, live.n_live

    # ---- device management ----------------------------------------------------------------
    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            self.flat_params = self.flat_params.to(device)
            self.flat_grads = None if self.flat_grads is None else self.flat_grads.to(device)
            self.release_accumulation()
            self._ws = None
            self._ws_key = None
            self.release_eval_workspace()
            self.device = device
        return self

    def _check_device(self, *tensors):
        if self.lib.is_emulator:
            for t in tensors:
                if t is not None and t.device.type != "cpu":
                    raise _lib.WnError("emulator binding takes CPU tensors")
            return
        if self.device.type != "cuda":
            raise _lib.WnError("the WaveNet HIP path runs on an MI355X: move the model to a GPU "
                               "(model.cuda()); there is no CPU fallback")
        for t in tensors:
            if t is not None and t.device != self.device:
                raise _lib.WnError("tensor on %s but the model lives on %s" % (t.device, self.device))

    def workspace(self, B, T):
        key = (B, T)
        if self._ws_key != key:
            nbytes = self.lib.wn_workspace_bytes(ctypes.byref(self.cfg), B, T)
            if nbytes == 0:
                raise _lib.WnError("wn_workspace_bytes: %s" % self.lib.wn_last_error().decode())
            self._ws = None  # free first
            # zero-filled: wn_forward_loss (FLAG_WS_FINITE) leaves the post-net columns in front of the loss window
            # untouched, and whatever is there must be finite (include/wavenet_hip.h)
            self._ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
            self._ws_key = key
        return self._ws

    def eval_workspace(self, B, T):
        """The workspace of ``forward_nll``: a slot of its own beside ``workspace()``, zero-filled on allocation like it."""
        key = (B, T)
        if self._eval_ws_key != key:
            nbytes = self.lib.wn_workspace_bytes(ctypes.byref(self.cfg), B, T)
            if nbytes == 0:
                raise _lib.WnError("wn_workspace_bytes: %s" % self.lib.wn_last_error().decode())
            self._eval_ws = None  # free first
            self._eval_ws = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=self.device)
            self._eval_ws_key = key
        return self._eval_ws

    def release_eval_workspace(self):
        """Drop the scoring workspace (and the lengths uploaded for it); the next ``forward_nll`` allocates again."""
        self._eval_ws = None
        self._eval_ws_key = None
        self._eval_lengths = (None, None)

    def params_version(self):
        """Changes whenever the flat parameter buffer is written: torch's in-place version counter (optimizers working
        on the nn.Parameter views, load_state_dict, ...) plus the engine's count of in-library updates."""
        v = self.flat_params._version
        for t in self._version_sources:   # nn.Parameter views keep their own counters (nets.WaveNet registers them)
            v += t._version
        return (self.flat_params.data_ptr(), v, self._params_epoch)

    def saved(self, kind):
        """View of a tensor the last forward / backward left in the workspace (``_lib.WS_*``; parity tests only)."""
        if self._last_shape is None:
            raise _lib.WnError("saved() without a preceding forward()")
        B, T = self._last_shape
        off, n = ctypes.c_int64(), ctypes.c_int64()
        self.lib.check(self.lib.wn_workspace_region(ctypes.byref(self.cfg), B, T, int(kind), ctypes.byref(off),
                                                    ctypes.byref(n)), "wn_workspace_region")
        R, S, L = self.cfg.n_resch, self.cfg.n_skipch, self.n_layers
        shape = {_lib.WS_RELU_SKIP: (B, S, T), _lib.WS_RELU_POST1: (B, S, T), _lib.WS_DSKIP: (B, S, T),
                 _lib.WS_DP: (L, B, 2 * R, T)}.get(int(kind), (L, B, R, T))
        return self.workspace(B, T)[off.value:off.value + n.value].view(shape)

    def grads(self):
        if self.flat_grads is None:
            self.flat_grads = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        return self.flat_grads

    # ---- gradient accumulation over micro-batches (include/wavenet_hip.h, ABI v15) -----------------
    @property
    def accumulation(self):
        """None, or ``(micro-steps done, A)`` of the open cycle."""
        return self._accum

    def abandon_accumulation(self):
        """Forget an open cycle (after an error, or to drop the micro-batches seen so far).  The accumulator stays allocated; the
        next cycle's first micro-step overwrites it, so nothing of the abandoned one leaks."""
        self._accum = None

    def release_accumulation(self):
        """``abandon_accumulation`` and drop the accumulator itself (a move to another device, a re-built flat buffer)."""
        self._accum = None
        self.grad_accum = None

    def accumulate_grads(self, mode, lo=0, hi=None):
        """One ``grad_accumulate`` launch on the current stream over ``[lo, hi)`` of the two flat buffers (default: all of them):
        ``_lib.ACCUM_SET`` accumulator = gradient, ``ACCUM_ADD`` accumulator += gradient, ``ACCUM_FINISH`` gradient = accumulator +
        gradient.  The thin call: it knows nothing of cycles (``begin_micro_step`` / ``end_micro_step`` keep that state)."""
        hi = self.n_params if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo < hi <= self.n_params:
            raise ValueError("accumulate_grads: [%d, %d) is not a range of the %d parameters" % (lo, hi, self.n_params))
        g = self.grads()
        if self.grad_accum is None:
            self.grad_accum = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        rc = self.lib.wn_op_accumulate(ctypes.c_void_p(self.grad_accum.data_ptr() + 4 * lo), ctypes.c_void_p(g.data_ptr() + 4 * lo),
                                       hi - lo, int(mode), _stream_handle(self.device))
        self.lib.check(rc, "wn_op_accumulate")

    def begin_micro_step(self, micro_step):
        """Check ``micro_step`` against the state of the cycle.  Returns None for a plain call (``None`` or ``A == 1``) and the
        mode of this micro-step's ``accumulate_grads`` otherwise; changes nothing (``end_micro_step`` does, once the launches are
        issued, so a call that raises half-way leaves the cycle where it was)."""
        if micro_step is not None:
            try:
                i, A = micro_step
                ok = int(i) == i and int(A) == A and not isinstance(i, bool) and not isinstance(A, bool)
            except (TypeError, ValueError):
                ok = False
            if not ok or not 0 <= int(i) < int(A):
                raise ValueError("micro_step must be (i, A) with integers 0 <= i < A, got %r" % (micro_step,))
            i, A = int(i), int(A)
        if micro_step is None or A == 1:
            if self._accum is not None:
                raise RuntimeError("an accumulation cycle is open (%d of %d micro-steps done): pass micro_step=(%d, %d), or call "
                                   "engine.abandon_accumulation() to drop it" % (self._accum + self._accum))
            return None
        if self._accum is None:
            if i != 0:
                raise RuntimeError("micro_step=(%d, %d) but no accumulation cycle is open: a cycle starts with micro_step=(0, %d)"
                                   % (i, A, A))
            return _lib.ACCUM_SET
        done, A0 = self._accum
        if A != A0:
            raise RuntimeError("micro_step=(%d, %d) inside a cycle of %d micro-steps (%d done): A must not change inside a cycle -- "
                               "finish it with micro_step=(%d, %d) ..., or call engine.abandon_accumulation()"
                               % (i, A, A0, done, done, A0))
        if i == 0:
            raise RuntimeError("micro_step=(0, %d) while a cycle is open (%d of %d micro-steps done): finish it, or call "
                               "engine.abandon_accumulation() to start over" % (A, done, A0))
        if i != done:
            raise RuntimeError("micro_step=(%d, %d) is not the next micro-step: the cycle expects micro_step=(%d, %d) (call "
                               "engine.abandon_accumulation() to drop it)" % (i, A, done, A0))
        return _lib.ACCUM_FINISH if i == A - 1 else _lib.ACCUM_ADD

    def end_micro_step(self, micro_step):
        """Advance the cycle after the launches of ``micro_step`` (one ``begin_micro_step`` accepted) have been issued."""
        i, A = int(micro_step[0]), int(micro_step[1])
        self._accum = None if i == A - 1 else (i + 1, A)

    # ---- C-ABI calls ------------------------------------------------------------------------
    def forward(self, x, h):
        """x (B,T) int64, h (B,A,T/U | T) fp32 -> logits (B,Q,T) fp32 (physical layout)."""
        self._check_device(x, h)
        if x.dtype != torch.int64 or x.dim() != 2:
            raise ValueError("x must be a LongTensor of shape (B, T)")
        B, T = x.shape
        U = self.cfg.upsampling_factor
        want = (B, self.cfg.n_aux, T // U if U > 0 else T)
        if U > 0 and T % U != 0:
            raise ValueError("T=%d is not a multiple of upsampling_factor=%d" % (T, U))
        if tuple(h.shape) != want:
            raise ValueError("h must have shape %s, got %s" % (want, tuple(h.shape)))
        x = x.contiguous()
        h = h.contiguous().float()
        ws = self.workspace(B, T)
        logits = torch.empty((B, self.out_channels, T), dtype=torch.float32, device=self.device)
        rc = self.lib.wn_forward(ctypes.byref(self.cfg), B, T, _ptr(self.flat_params), _ptr(x), _ptr(h), _ptr(logits),
                                 _ptr(ws), ws.numel() * 4, self.flags, _stream_handle(self.device))
        self.lib.check(rc, "wn_forward")
        self._last_shape = (B, T)
        self._last_inputs = (x, h)
        self._fwd_window = 0
        self._fwd_version = self.params_version()
        self._fwd_flags = self.flags
        return logits

    def forward_loss(self, x, h, target, t_start=None, grad_scale=1.0, loss_scale=1.0, want_grad=True, lengths=None):
        """``forward`` + ``loss`` of a training step in one call (reference train.py:533-536).  Softmax head with at most
        256 classes on the split contractions: the cross-entropy is the EPILOGUE of the conv_post_2 contraction, the
        (B, Q, T) logits never reach memory (``wn_forward_loss``); otherwise the two calls back to back.
        Returns (loss, dlogits) exactly as ``loss`` does.

        ``lengths`` (B host integers, see ``_lengths_arg``): a padded batch of sequences of unequal length -- the loss is the
        mean over the positions [t_start, lengths[b]) of every sequence, nn.CrossEntropyLoss() with the targets behind each
        end set to -100; ``dlogits`` is exactly zero on the padding, whatever finite values x, h and target hold there.  The
        fused form is kept (``wn_forward_loss_ragged``).  None: every sequence runs to T, the dense call."""
        self._check_device(x, h, target)
        if x.dtype != torch.int64 or x.dim() != 2:
            raise ValueError("x must be a LongTensor (B, T)")
        B, T = x.shape
        if t_start is None:
            t_start = self.receptive_field
        flen = T // self.cfg.upsampling_factor if self.cfg.upsampling_factor > 0 else T
        if h.dim() != 3 or h.size(0) != B or h.size(1) != self.cfg.n_aux or h.size(2) != flen:
            raise ValueError("h must be (B, n_aux, %d)" % flen)
        if self.cfg.upsampling_factor > 0 and T % self.cfg.upsampling_factor != 0:
            raise ValueError("T must be a multiple of the upsampling factor")
        x, h, target = x.contiguous(), h.contiguous().float(), target.contiguous()
        cfg = ctypes.byref(self.cfg)
        fused = bool(self.lib.wn_forward_loss_fused(cfg, B, T, self.flags))
        ws = self.workspace(B, T)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        dlogits = torch.empty((B, self.out_channels, T), dtype=torch.float32, device=self.device) if want_grad else None
        scratch = None if fused else torch.empty((B, self.out_channels, T), dtype=torch.float32, device=self.device)
        call_flags = self.flags | (_lib.FLAG_WS_FINITE if self.ws_finite else 0)
        count = B * (T - int(t_start))
        if lengths is None:
            rc = self.lib.wn_forward_loss(cfg, B, T, _ptr(self.flat_params), _ptr(x), _ptr(h), _ptr(target), int(t_start),
                                          float(grad_scale), float(loss_scale), _ptr(loss), _ptr(dlogits), _ptr(scratch),
                                          _ptr(ws), ws.numel() * 4, call_flags, _stream_handle(self.device))
            self.lib.check(rc, "wn_forward_loss")
        else:
            t_end, count = self._lengths_arg(lengths, B, T, t_start)
            rc = self.lib.wn_forward_loss_ragged(cfg, B, T, _ptr(self.flat_params), _ptr(x), _ptr(h), _ptr(target),
                                                 int(t_start), _ptr(t_end), count, float(grad_scale), float(loss_scale),
                                                 _ptr(loss), _ptr(dlogits), _ptr(scratch), _ptr(ws), ws.numel() * 4,
                                                 call_flags, _stream_handle(self.device))
            self.lib.check(rc, "wn_forward_loss_ragged")
        self._last_shape = (B, T)
        self._last_inputs = (x, h)
        # the fused form ran the skip sum / post-net over the loss window only (saved(WS_RELU_*) is valid from
        # t_start rounded down to a multiple of 128 on); backward() defaults its window to it
        self._fwd_window = int(t_start) if fused else 0
        self._fwd_version = self.params_version()
        self._fwd_flags = self.flags
        self._note_bound(dlogits, grad_scale, count)
        return loss, dlogits

    def _lengths_arg(self, lengths, B, T, t_start, scoring=False):
        """``lengths`` of a padded batch -> (device int32 array for the ragged C entry points, N).  ``lengths[b]`` is the number of
        valid positions of sequence b, 1 <= lengths[b] <= T; the loss positions of b are [t_start, lengths[b]) and
        N = sum_b max(lengths[b] - t_start, 0) is their count -- known here, on the host, because the lengths are host
        integers (a sequence of ints or a CPU integer tensor): the step gains no device-to-host synchronisation.
        ``scoring`` (``forward_nll``): N == 0 is allowed -- there is no divisor -- and the uploaded array is kept in a slot of its
        own, so the training step's stays where it is."""
        if isinstance(lengths, torch.Tensor):
            if lengths.device.type != "cpu":
                raise ValueError("lengths must be host integers (a sequence of ints or a CPU integer tensor), got a tensor on "
                                 "%s: the loss divisor N is computed on the host" % lengths.device)
            if lengths.dtype.is_floating_point or lengths.dtype.is_complex or lengths.dtype == torch.bool:
                raise ValueError("lengths must be integers, got %s" % lengths.dtype)
            lens = [int(v) for v in lengths.reshape(-1).tolist()] if lengths.dim() == 1 else None
        else:
            try:
                lens = list(lengths)
            except TypeError:
                lens = None
            if lens is not None:
                for v in lens:
                    if isinstance(v, bool) or int(v) != v:
                        raise ValueError("lengths must be integers, got %r" % (v,))
                lens = [int(v) for v in lens]
        if lens is None or len(lens) != B:
            raise ValueError("lengths must have one entry per sequence (B = %d), got %s"
                             % (B, "%d" % len(lens) if lens is not None else "shape %s" % (tuple(getattr(lengths, "shape", ())),)))
        for b, v in enumerate(lens):
            if v < 1 or v > T:
                raise ValueError("lengths[%d] = %d outside [1, T = %d]" % (b, v, T))
        n = sum(max(v - int(t_start), 0) for v in lens)
        if n == 0 and not scoring:
            raise ValueError("lengths %s leave no loss position behind t_start = %d (N == 0)" % (lens, int(t_start)))
        key = (tuple(lens), str(self.device))
        if scoring:
            if self._eval_lengths[0] != key:
                self._eval_lengths = (key, torch.tensor(lens, dtype=torch.int32).to(self.device, non_blocking=True))
            return self._eval_lengths[1], n
        if self._lengths_key != key:   # an upload of B integers, not a launch; the same lengths step after step upload once
            self._lengths_dev = torch.tensor(lens, dtype=torch.int32).to(self.device, non_blocking=True)
            self._lengths_key = key
        return self._lengths_dev, n

    def _note_bound(self, dlogits, grad_scale, count):
        # The loss calls leave max |dlogits| of the tensor they wrote in the workspace (measured in their epilogue); backward() may
        # tell the library to use it (WN_FLAG_DW_F16_AMAX_WS) only for exactly that tensor in exactly that state, so the tensor
        # OBJECT is remembered, weakly (an address could be handed out again by the caching allocator), with its version counter.
        self._dlogits_bound = None
        if dlogits is not None and count > 0 and grad_scale != 0.0:
            self._dlogits_bound = (weakref.ref(dlogits), dlogits._version, self._ws_key)

    def _dw_mode_flags(self, flags, dlogits, dlogits_bound=None):
        """FLAG_DW_F16PAIR scales the gradient operand by max |dlogits| (include/wavenet_hip.h).  Where it comes from:
          * ``dlogits_bound`` given: the caller's promise, taken as given (a loose bound costs precision -- prefer None);
          * ``dlogits`` is the unmodified tensor the last loss call of this engine returned, same workspace: the maximum that call
            measured (| FLAG_DW_F16_AMAX_WS: free);
          * anything else (autograd's grad_output, a tensor modified in place, the mixture-of-logistics head): the library
            scans the tensor for its maximum first (the flag alone: one pass over the loss window).
        Never a silent default: an a-priori bound that is merely safe would underflow fp16's range."""
        if not (flags & _lib.FLAG_DW_F16PAIR):
            return flags
        flags &= ~((63 << _lib.DW_F16_EXP_SHIFT) | _lib.FLAG_DW_F16_EXP_VALID | _lib.FLAG_DW_F16_AMAX_WS)
        if dlogits_bound is not None:
            return flags | _lib.dw_f16_exp(float(dlogits_bound))
        nb = self._dlogits_bound
        if nb is not None and nb[0]() is dlogits and nb[1] == dlogits._version and nb[2] == self._ws_key:
            return flags | _lib.FLAG_DW_F16_AMAX_WS
        return flags

    def loss(self, logits, target, t_start=None, grad_scale=1.0, loss_scale=1.0, want_grad=True, lengths=None):
        """Softmax-CE over positions >= t_start (default: receptive field).  Returns (loss, dlogits).  ``lengths``: as
        ``forward_loss`` (positions [t_start, lengths[b]) of every sequence; ``dlogits`` exactly zero elsewhere)."""
        self._check_device(logits, target)
        B, Q, T = logits.shape
        if t_start is None:
            t_start = self.receptive_field
        target = target.contiguous()
        ws = self.workspace(B, T)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        dlogits = torch.empty_like(logits) if want_grad else None
        count = B * (T - int(t_start))
        if lengths is None:
            rc = self.lib.wn_softmax_ce_loss(ctypes.byref(self.cfg), B, T, _ptr(logits), _ptr(target), int(t_start),
                                             float(grad_scale), float(loss_scale), _ptr(loss), _ptr(dlogits), _ptr(ws),
                                             ws.numel() * 4, _stream_handle(self.device))
            self.lib.check(rc, "wn_softmax_ce_loss")
        else:
            t_end, count = self._lengths_arg(lengths, B, T, t_start)
            rc = self.lib.wn_softmax_ce_loss_ragged(ctypes.byref(self.cfg), B, T, _ptr(logits), _ptr(target), int(t_start),
                                                    _ptr(t_end), count, float(grad_scale), float(loss_scale), _ptr(loss),
                                                    _ptr(dlogits), _ptr(ws), ws.numel() * 4, _stream_handle(self.device))
            self.lib.check(rc, "wn_softmax_ce_loss_ragged")
        self._note_bound(dlogits, grad_scale, count)
        return loss, dlogits

    def distill_loss(self, logits, teacher_logits, target, alpha, temperature, t_start=None, grad_scale=1.0, loss_scale=1.0,
                     want_grad=True, lengths=None, want_pos=False):
        """Soft-target loss of the softmax head (knowledge distillation, ``wn_softmax_distill_loss``): per loss position
        ``l = (1 - alpha) * ce + alpha * temperature^2 * kl`` with ``ce`` the cross-entropy against ``target`` and ``kl`` the
        divergence of ``softmax(logits / temperature)`` from ``softmax(teacher_logits / temperature)``.  ``logits`` and
        ``teacher_logits``: (B, Q, T) fp32 in the physical layout ``forward`` returns; the teacher is a constant.  ``target`` may
        be None with ``alpha == 1``.  Returns ``(loss3, dlogits[, pos_loss])``: ``loss3`` a 3-element device tensor, the means of
        ``l``, ``ce`` and the unweighted ``kl``; ``dlogits`` for ``backward`` (None without ``want_grad``; exactly zero off the loss
        positions); ``pos_loss`` (B, T), ``l`` per position and 0 elsewhere, with ``want_pos``.  ``t_start`` / ``lengths`` /
        ``grad_scale`` / ``loss_scale`` as ``loss``."""
        self._check_device(logits, teacher_logits, target)
        if self.cfg.out_channels > 0:
            raise ValueError("the soft-target loss is defined for the softmax head (n_mixture = 0)")
        if logits.dim() != 3 or logits.dtype != torch.float32 or not logits.is_contiguous():
            raise ValueError("logits must be a contiguous float32 (B, Q, T) tensor")
        B, Q, T = logits.shape
        if tuple(teacher_logits.shape) != (B, Q, T) or teacher_logits.dtype != torch.float32 or not teacher_logits.is_contiguous():
            raise ValueError("teacher_logits must be a contiguous float32 tensor of the logits' shape %s, got %s %s"
                             % ((B, Q, T), tuple(teacher_logits.shape), teacher_logits.dtype))
        if target is None:
            if float(alpha) != 1.0:
                raise ValueError("target may be None with alpha == 1 only")
        else:
            if tuple(target.shape) != (B, T) or target.dtype != torch.int64:
                raise ValueError("target must be a (B, T) LongTensor")
            target = target.contiguous()
        if t_start is None:
            t_start = self.receptive_field
        ws = self.workspace(B, T)
        n_scratch = int(self.lib.wn_softmax_distill_scratch_floats(B, T))
        if self._distill_scratch is None or self._distill_scratch.numel() < n_scratch or self._distill_scratch.device != logits.device:
            self._distill_scratch = torch.empty(n_scratch, dtype=torch.float32, device=self.device)
        loss3 = torch.empty(3, dtype=torch.float32, device=self.device)
        dlogits = torch.empty_like(logits) if want_grad else None
        pos = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_pos else None
        if lengths is None:
            t_end, count = None, B * (T - int(t_start))
        else:
            t_end, count = self._lengths_arg(lengths, B, T, t_start)
        rc = self.lib.wn_softmax_distill_loss(ctypes.byref(self.cfg), B, T, _ptr(logits), _ptr(teacher_logits), _ptr(target),
                                              int(t_start), _ptr(t_end), count, float(alpha), float(temperature),
                                              float(grad_scale), float(loss_scale), _ptr(loss3), _ptr(dlogits), _ptr(pos),
                                              _ptr(self._distill_scratch), _ptr(ws), ws.numel() * 4, _stream_handle(self.device))
        self.lib.check(rc, "wn_softmax_distill_loss")
        self._note_bound(dlogits, grad_scale, count)
        return (loss3, dlogits, pos) if want_pos else (loss3, dlogits)

    NORMALIZE = {"weights": 0, "positions": 1}

    def _weight_arg(self, w, shape, name):
        """A weight tensor of ``weighted_loss`` -> its float32 copy on the engine's device.  Shape and dtype are checked, and on a
        host tensor that every entry is finite and >= 0 -- once per tensor object and version, not once per step (a tensor that is
        already on the device is the caller's contract: checking it would synchronise)."""
        if w is None:
            return None
        if not isinstance(w, torch.Tensor):
            w = torch.as_tensor(w, dtype=torch.float32)
        seen = self._weights_seen.get(name)
        if seen is not None and seen[2] is w:   # the copy this method made (loss_and_backward checks before it launches)
            return w
        if seen is not None and seen[0]() is w and seen[1] == w._version and seen[2].device == self.device:
            return seen[2]
        if tuple(w.shape) != tuple(shape) or w.dtype != torch.float32:
            raise ValueError("%s must be a float32 tensor of shape %s, got %s %s" % (name, tuple(shape), tuple(w.shape), w.dtype))
        if w.device.type == "cpu" and (not bool(torch.isfinite(w).all()) or bool((w < 0).any())):
            raise ValueError("%s must be finite and >= 0 everywhere" % name)
        dev = w.detach().contiguous().to(self.device)
        self._weights_seen[name] = (weakref.ref(w), w._version, dev)
        return dev

    def weighted_loss_args(self, class_weights, label_smoothing, position_weights, normalize, B, Q, T):
        """The refusals of ``weighted_loss``'s options, made before anything is launched; returns (eps, class weights, position
        weights) with the weights on the device."""
        if self.cfg.out_channels > 0:
            raise ValueError("the weighted cross-entropy is defined for the softmax head (n_mixture = 0)")
        eps = float(label_smoothing)
        if not 0.0 <= eps < 1.0:
            raise ValueError("label_smoothing = %r outside [0, 1)" % (label_smoothing,))
        if normalize not in self.NORMALIZE:
            raise ValueError("normalize = %r: \"weights\" or \"positions\"" % (normalize,))
        return (eps, self._weight_arg(class_weights, (Q,), "class_weights"),
                self._weight_arg(position_weights, (B, T), "position_weights"))

    def weighted_loss(self, logits, target, class_weights=None, label_smoothing=0.0, position_weights=None, normalize="weights",
                      t_start=None, grad_scale=1.0, loss_scale=1.0, want_grad=True, lengths=None, want_pos=False):
        """Weighted cross-entropy of the softmax head (``wn_softmax_cew_loss``): torch's ``CrossEntropyLoss(weight=class_weights,
        label_smoothing=label_smoothing)`` with one more weight per position.  Per loss position, with ``p = softmax(logits)``,
        ``y`` the target, ``w`` the (Q,) ``class_weights`` and ``r`` the (B, T) ``position_weights`` (None: ones),
        ``l = (1 - eps) w_y (-log p_y) + eps / Q sum_q w_q (-log p_q)``; the criterion is ``sum r l / D`` with
        ``D = sum r w_y`` (``normalize="weights"``: torch's mean; with ``r`` None exactly ``F.cross_entropy(weight=,
        label_smoothing=)``) or ``D = N``, the number of loss positions (``normalize="positions"``).  ``"positions"`` is the
        choice for several ranks or micro-batches: with the per-call shares ``N_k / sum N`` as ``grad_scale`` the pooled
        objective is exact; with ``"weights"`` it is the share-weighted mean of the per-call weighted means, which is what torch
        DDP gives.  ``D == 0`` gives a loss and a gradient of exactly 0 (torch: NaN); a position with ``r == 0`` is off.

        ``logits``: (B, Q, T) fp32 in the physical layout ``forward`` returns.  Weights must be finite and >= 0: checked on host
        tensors, once per tensor.  Returns ``(loss3, dlogits[, pos_loss])``: ``loss3`` a 3-element device tensor -- the
        criterion, the plain unweighted cross-entropy mean over the same positions, and ``D``; ``dlogits`` for ``backward``
        (None without ``want_grad``; exactly zero off the loss positions and where ``r == 0``); ``pos_loss`` (B, T), ``r l`` per
        position, with ``want_pos``.  ``t_start`` / ``lengths`` / ``grad_scale`` / ``loss_scale`` as ``loss``."""
        self._check_device(logits, target)
        if self.cfg.out_channels > 0:
            raise ValueError("the weighted cross-entropy is defined for the softmax head (n_mixture = 0)")
        if logits.dim() != 3 or logits.dtype != torch.float32 or not logits.is_contiguous():
            raise ValueError("logits must be a contiguous float32 (B, Q, T) tensor")
        B, Q, T = logits.shape
        if tuple(target.shape) != (B, T) or target.dtype != torch.int64:
            raise ValueError("target must be a (B, T) LongTensor")
        target = target.contiguous()
        eps, cw, pw = self.weighted_loss_args(class_weights, label_smoothing, position_weights, normalize, B, Q, T)
        if t_start is None:
            t_start = self.receptive_field
        ws = self.workspace(B, T)
        n_scratch = int(self.lib.wn_softmax_cew_scratch_floats(B, T))
        if self._cew_scratch is None or self._cew_scratch.numel() < n_scratch or self._cew_scratch.device != logits.device:
            self._cew_scratch = torch.empty(n_scratch, dtype=torch.float32, device=self.device)
        loss3 = torch.empty(3, dtype=torch.float32, device=self.device)
        dlogits = torch.empty_like(logits) if want_grad else None
        pos = torch.empty((B, T), dtype=torch.float32, device=self.device) if want_pos else None
        if lengths is None:
            t_end, count = None, B * (T - int(t_start))
        else:
            t_end, count = self._lengths_arg(lengths, B, T, t_start)
        rc = self.lib.wn_softmax_cew_loss(ctypes.byref(self.cfg), B, T, _ptr(logits), _ptr(target), int(t_start), _ptr(t_end), count,
                                          _ptr(cw), _ptr(pw), eps, self.NORMALIZE[normalize], float(grad_scale), float(loss_scale),
                                          _ptr(loss3), _ptr(dlogits), _ptr(pos), _ptr(self._cew_scratch), _ptr(ws), ws.numel() * 4,
                                          _stream_handle(self.device))
        self.lib.check(rc, "wn_softmax_cew_loss")
        self._note_bound(dlogits, grad_scale, count)
        return (loss3, dlogits, pos) if want_pos else (loss3, dlogits)

    def mol_loss(self, out, y, t_start=None, grad_scale=1.0, loss_scale=1.0, want_grad=True, num_classes=65536,
                 log_scale_min=-7.0, lengths=None):
        """Mixture-of-logistics head: mean NLL of the waveform ``y`` (B,T) in [-1,1] under ``out`` (B, 3*n_mix, T)
        over positions >= t_start, and d(loss)/d(out) for ``backward``.  Not in the reference (see include/).
        ``lengths``: the same mask and the same divisor as ``forward_loss`` gives the softmax head."""
        self._check_device(out, y)
        B, C, T = out.shape
        if C != self.out_channels or C % 3 != 0:
            raise ValueError("out must be (B, 3*n_mix = %d, T)" % self.out_channels)
        if t_start is None:
            t_start = self.receptive_field
        y = y.contiguous().float()
        ws = self.workspace(B, T)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        dout = torch.empty_like(out) if want_grad else None
        if lengths is None:
            rc = self.lib.wn_mol_loss(ctypes.byref(self.cfg), B, T, _ptr(out), _ptr(y), int(t_start), float(grad_scale),
                                      float(loss_scale), int(num_classes), float(log_scale_min), _ptr(loss), _ptr(dout),
                                      _ptr(ws), ws.numel() * 4, _stream_handle(self.device))
            self.lib.check(rc, "wn_mol_loss")
        else:
            t_end, count = self._lengths_arg(lengths, B, T, t_start)
            rc = self.lib.wn_mol_loss_ragged(ctypes.byref(self.cfg), B, T, _ptr(out), _ptr(y), int(t_start), _ptr(t_end), count,
                                             float(grad_scale), float(loss_scale), int(num_classes), float(log_scale_min),
                                             _ptr(loss), _ptr(dout), _ptr(ws), ws.numel() * 4, _stream_handle(self.device))
            self.lib.check(rc, "wn_mol_loss_ragged")
        self._dlogits_bound = None   # (the mixture head's loss call measures no maximum: backward scans its gradient)
        return loss, dout

    def forward_nll(self, x, h, target=None, y=None, t_start=None, lengths=None, acc=None, num_classes=65536, log_scale_min=-7.0):
        """Score a batch: the negative log-likelihood of every sequence, no gradient.  Returns ``(row_nll, counts)``:
        ``row_nll`` (B,) fp32 on the device, the SUM over the positions [t_start, min(lengths[b], T)) of sequence b (exactly 0.0
        where there is none), and ``counts``, B host ints ``max(min(lengths[b], T) - t_start, 0)`` -- sums and counts pool
        exactly over batches of any size, a mean is one division away.  Softmax head: ``target`` (B, T) int64; mixture head:
        ``y`` (B, T) waveform in [-1, 1], ``num_classes`` / ``log_scale_min`` as ``mol_loss``.  ``lengths``: as ``forward_loss``,
        except that a batch without any loss position is fine.  ``acc``: a 1-element float64 tensor on the model's device;
        the batch's total -- the fp64 sum of ``row_nll`` as returned -- is ADDED to it on the device, so a pass over many batches
        reads the host once.

        The call runs in a workspace of its own (``eval_workspace``) and touches nothing a later ``backward()`` reads: the
        training workspace, the shapes / inputs / parameter version of the last forward and the gradient buffer stay as
        they are, so it may sit between ``forward_loss`` and ``backward``."""
        mixture = self.cfg.out_channels > 0
        if (target is None) == (y is None):
            raise ValueError("forward_nll takes exactly one of target (softmax head) and y (mixture-of-logistics head)")
        if mixture and y is None:
            raise ValueError("this model has the mixture-of-logistics head: pass the waveform y, not class targets")
        if not mixture and target is None:
            raise ValueError("this model has the softmax head: pass the class targets, not a waveform y")
        ref = target if target is not None else y
        self._check_device(x, h, ref, acc)
        if x.dtype != torch.int64 or x.dim() != 2:
            raise ValueError("x must be a LongTensor (B, T)")
        B, T = x.shape
        U = self.cfg.upsampling_factor
        if U > 0 and T % U != 0:
            raise ValueError("T must be a multiple of the upsampling factor")
        flen = T // U if U > 0 else T
        if h.dim() != 3 or h.size(0) != B or h.size(1) != self.cfg.n_aux or h.size(2) != flen:
            raise ValueError("h must be (B, n_aux, %d)" % flen)
        if tuple(ref.shape) != (B, T) or (target is not None and target.dtype != torch.int64):
            raise ValueError("%s must be a (B, T) %s" % (("target", "LongTensor") if target is not None else ("y", "tensor")))
        if acc is not None:
            if not isinstance(acc, torch.Tensor) or acc.dtype != torch.float64 or acc.numel() != 1 or not acc.is_contiguous():
                raise ValueError("acc must be a 1-element float64 tensor on the model's device, got %s"
                                 % ("%s %s" % (tuple(acc.shape), acc.dtype) if isinstance(acc, torch.Tensor) else type(acc)))
        if t_start is None:
            t_start = self.receptive_field
        t_start = int(t_start)
        if t_start < 0:
            raise ValueError("t_start must not be negative")
        if lengths is None:
            t_end, counts = None, [max(T - t_start, 0)] * B
        else:
            t_end, _ = self._lengths_arg(lengths, B, T, t_start, scoring=True)
            counts = [max(min(int(v), T) - t_start, 0) for v in self._eval_lengths[0][0]]
        x, h = x.contiguous(), h.contiguous().float()
        cfg = ctypes.byref(self.cfg)
        ws = self.eval_workspace(B, T)
        st = _stream_handle(self.device)
        row_nll = torch.empty(B, dtype=torch.float32, device=self.device)
        if mixture:
            if self.out_channels % 3 != 0:
                raise ValueError("out_channels = %d is not 3 * n_mix" % self.out_channels)
            y = y.contiguous().float()
            out = torch.empty((B, self.out_channels, T), dtype=torch.float32, device=self.device)
            self.lib.check(self.lib.wn_forward(cfg, B, T, _ptr(self.flat_params), _ptr(x), _ptr(h), _ptr(out), _ptr(ws),
                                               ws.numel() * 4, self.flags, st), "wn_forward")
            rc = self.lib.wn_mol_nll_rows(cfg, B, T, _ptr(out), _ptr(y), t_start, _ptr(t_end), int(num_classes),
                                          float(log_scale_min), _ptr(row_nll), _ptr(acc), _ptr(ws), ws.numel() * 4, st)
            self.lib.check(rc, "wn_mol_nll_rows")
        else:
            target = target.contiguous()
            fused = bool(self.lib.wn_forward_loss_fused(cfg, B, T, self.flags))
            scratch = None if fused else torch.empty((B, self.out_channels, T), dtype=torch.float32, device=self.device)
            rc = self.lib.wn_forward_nll(cfg, B, T, _ptr(self.flat_params), _ptr(x), _ptr(h), _ptr(target), t_start, _ptr(t_end),
                                         _ptr(row_nll), _ptr(acc), _ptr(scratch), _ptr(ws), ws.numel() * 4, self.flags, st)
            self.lib.check(rc, "wn_forward_nll")
        return row_nll, counts

    def backward(self, dlogits, events=None, layers_per_bucket=0, t_first=None, repack=False, dlogits_bound=None, dh=None,
                 param_grads=True, first_layer=0, needs=_lib.NEED_ALL):
        """Backward of the last ``forward`` / ``forward_loss`` call; fills ``self.grads()`` completely.  ``t_first``: the
        caller guarantees ``dlogits[:, :, :t_first] == 0`` (the training loss covers ``[:, receptive_field:]``,
        train.py:534-536): the post-net / skip part of the backward pass then runs over the loss window only
        (``wn_backward_window``).  Default: the window of the forward call (0 after ``forward``, its ``t_start`` after
        ``forward_loss``, whose ``dlogits`` is zero in front of it by construction).

        The parameters must not have changed since the forward call -- the workspace holds the weight sets that call
        packed from them next to its activations.  Like torch.autograd for a tensor modified in place between forward
        and backward this raises; ``repack=True`` instead rebuilds the weight sets from the current parameters
        (``WN_FLAG_REPACK``) and back-propagates through those.

        ``dlogits_bound``: with ``FLAG_DW_F16PAIR`` in ``self.flags`` the weight gradients take the fp16 pair split
        (include/wavenet_hip.h), scaled by max |dlogits|.  Default (None): MEASURED -- by the loss call for the unmodified
        tensor ``forward_loss`` / ``loss`` returned (free), by one pass over any other gradient (autograd's grad_output, the
        mixture-of-logistics head).  A number: the caller's own promise ``max |dlogits| <= dlogits_bound``, taken as given.

        ``dh``: a contiguous fp32 tensor shaped like the forward call's ``h`` (B, n_aux, T / upsampling_factor or T) on the
        model's device; it receives dL/dh (``wn_backward_dh``).  ``param_grads=False`` (with ``dh``): no weight gradient is
        computed (a frozen model), ``self.grads()`` is left as it is and the call returns None.

        ``first_layer`` / ``needs`` (``wn_backward_needs``; ``WaveNet`` derives them from ``requires_grad``): the lowest layer
        with a trainable tensor of its own (``n_layers``: none) and ``_lib.NEED_POST | NEED_FRONT | NEED_UP`` for the post-net,
        the front conv and the upsampling layer.  The pass stops below ``first_layer`` and leaves out the launches only frozen
        tensors need; the ranges of those tensors in ``self.grads()`` then hold unspecified values.  ``first_layer`` must be 0
        with ``dh``, ``NEED_FRONT`` or ``NEED_UP``.  The defaults are the full pass, through the entry points of before."""
        if self._last_shape is None:
            raise _lib.WnError("backward() without a preceding forward()")
        if t_first is None:
            t_first = self._fwd_window
        flags = self.flags
        # NO_FUSED / EXACT_MFMA: the kernel families save different ACTIVATIONS (the fused forward saves no Gt, the layered
        # backward reads it) -- nothing rebuilds those, so a change always raises.  MM_F16PAIR / CHAIN_F16PAIR change only the
        # weight images, which repack=True rebuilds from the parameters.
        changed = flags ^ self._fwd_flags
        if changed & (_lib.FLAG_NO_FUSED | _lib.FLAG_EXACT_MFMA) or (changed & (_lib.FLAG_MM_F16PAIR | _lib.FLAG_CHAIN_F16PAIR)
                                                                      and not repack):
            raise _lib.WnError("engine.flags changed the kernel family (NO_FUSED / EXACT_MFMA / MM_F16PAIR / CHAIN_F16PAIR) since the "
                               "forward call: the families save different activations and weight sets -- run forward again "
                               "(repack=True rebuilds the weight sets of MM_F16PAIR / CHAIN_F16PAIR, not the activations)")
        flags = self._dw_mode_flags(flags, dlogits, dlogits_bound)
        if repack:
            flags |= _lib.FLAG_REPACK
        elif self._fwd_version is not None and self._fwd_version != self.params_version():
            raise _lib.WnError("the WaveNet parameters were modified between forward and backward (in-place update, "
                               "optimizer step or load_state_dict): the gradient of the forward pass is no longer "
                               "defined -- run forward again, or pass repack=True to back-propagate through the "
                               "current weights")
        B, T = self._last_shape
        x, h = self._last_inputs
        self._check_device(dlogits)
        if tuple(dlogits.shape) != (B, self.out_channels, T) or not dlogits.is_contiguous():
            raise ValueError("dlogits must be a contiguous (B,Q,T) tensor")
        if dh is not None:
            self._check_device(dh)
            want = (B, self.cfg.n_aux, T // self.cfg.upsampling_factor if self.cfg.upsampling_factor > 0 else T)
            if tuple(dh.shape) != want or dh.dtype != torch.float32 or not dh.is_contiguous():
                raise ValueError("dh must be a contiguous float32 tensor of shape %s, got %s %s%s"
                                 % (want, tuple(dh.shape), dh.dtype, "" if dh.is_contiguous() else " (not contiguous)"))
        elif not param_grads:
            raise ValueError("param_grads=False needs dh: the call would compute nothing")
        if not param_grads and events:
            raise ValueError("bucket events need the weight gradients (param_grads=True)")
        g = self.grads() if param_grads else None
        ws = self.workspace(B, T)
        if events:
            arr = (ctypes.c_void_p * len(events))(*[ctypes.c_void_p(e) for e in events])
            n_ev = len(events)
        else:
            arr, n_ev = None, 0
        if int(first_layer) != 0 or int(needs) != _lib.NEED_ALL:
            rc = self.lib.wn_backward_needs(ctypes.byref(self.cfg), B, T, _ptr(self.flat_params), _ptr(x), _ptr(h), _ptr(dlogits),
                                            int(t_first), _ptr(g), _ptr(dh), _ptr(ws), ws.numel() * 4, arr, n_ev,
                                            int(layers_per_bucket), flags, _stream_handle(self.device), int(first_layer),
                                            int(needs))
            self.lib.check(rc, "wn_backward_needs")
            return g
        if dh is not None or not param_grads:
            rc = self.lib.wn_backward_dh(ctypes.byref(self.cfg), B, T, _ptr(self.flat_params), _ptr(x), _ptr(h), _ptr(dlogits),
                                         int(t_first), _ptr(g), _ptr(dh), _ptr(ws), ws.numel() * 4, arr, n_ev,
                                         int(layers_per_bucket), flags, _stream_handle(self.device))
            self.lib.check(rc, "wn_backward_dh")
            return g
        rc = self.lib.wn_backward_window(ctypes.byref(self.cfg), B, T, _ptr(self.flat_params), _ptr(x), _ptr(h),
                                         _ptr(dlogits), int(t_first), _ptr(g), _ptr(ws), ws.numel() * 4, arr, n_ev,
                                         int(layers_per_bucket), flags, _stream_handle(self.device))
        self.lib.check(rc, "wn_backward_window")
        return g

    def adam_step(self, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, live=None):
        """One Adam step over the flat buffers without the dead range.  ``live`` (a ``LiveTable``; here and in the three variants
        below, ``ema`` None or the average): over those ranges only -- everything outside keeps its bits in every buffer,
        whatever the gradient buffer holds there (``wn_adam_step_live`` / ``wn_adam_step_guarded_live``)."""
        self._check_device(exp_avg, exp_avg_sq)
        if live is not None:
            return self._adam_step_live(exp_avg, exp_avg_sq, None, live, step, lr, betas, eps, weight_decay, 0.0, False)
        rc = self.lib.wn_adam_step(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq),
                                   self.n_params, int(step), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                   float(weight_decay), self.dead_range[0], self.dead_range[1],
                                   _stream_handle(self.device))
        self.lib.check(rc, "wn_adam_step")
        self._params_epoch += 1

    # ---- global-norm clipping / non-finite-step guard (include/wavenet_hip.h, ABI v12) ---------------
    OPT_STATE_WORDS = ctypes.sizeof(_lib.WnOptState) // 8   # the state block as int64 words (8-byte aligned)

    def new_opt_state(self):
        """A zeroed ``WnOptState`` on the engine's device (an int64 tensor; ``opt_state_views`` names its fields).  Allocate it,
        and the scratch of ``grad_norm_scratch``, once per optimizer -- not per step."""
        return torch.zeros(self.OPT_STATE_WORDS, dtype=torch.int64, device=self.device)

    @staticmethod
    def opt_state_views(state):
        """0-dim views of the fields of a state block: no copies, no synchronisation."""
        f, i32 = state.view(torch.float32), state.view(torch.int32)
        return {"sumsq": state.view(torch.float64)[0], "total_norm": f[2], "clip_coef": f[3], "apply": i32[4],
                "steps_applied": state[3], "steps_skipped": state[4], "lr_over_bc1": f[10], "sqrt_bc2": f[11]}

    def grad_norm_scratch(self, n=None):
        n = self.n_params if n is None else int(n)
        return torch.empty(int(self.lib.wn_grad_norm_scratch_floats(n)), dtype=torch.float32, device=self.device)

    def _adam_step_live(self, exp_avg, exp_avg_sq, ema, live, step, lr, betas, eps, weight_decay, ema_decay, ema_warmup):
        table, nr, n_live = self._live_args(live)
        rc = self.lib.wn_adam_step_live(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(ema),
                                        self.n_params, table, nr, n_live, int(step), float(lr), float(betas[0]), float(betas[1]),
                                        float(eps), float(weight_decay), float(ema_decay), int(bool(ema_warmup)),
                                        _stream_handle(self.device))
        self.lib.check(rc, "wn_adam_step_live")
        self._params_epoch += 1

    def _adam_step_guarded_live(self, exp_avg, exp_avg_sq, ema, live, state, eps, weight_decay, ema_decay, ema_warmup):
        table, nr, n_live = self._live_args(live)
        rc = self.lib.wn_adam_step_guarded_live(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq),
                                                _ptr(ema), self.n_params, table, nr, n_live, float(eps), float(weight_decay),
                                                _ptr(state), float(ema_decay), int(bool(ema_warmup)), _stream_handle(self.device))
        self.lib.check(rc, "wn_adam_step_guarded_live")
        self._params_epoch += 1

    def grad_norm(self, state, scratch, max_norm=0.0, guard=False, lr=1e-3, betas=(0.9, 0.999), grads=None, skip=None, live=None):
        """Global L2 norm of the flat gradient (without the dead range) into ``state``, together with everything the guarded
        Adam launch reads: two launches, no host synchronisation.  ``max_norm`` None / <= 0 / inf: measure only.  ``live`` (a
        ``LiveTable``): the norm over those ranges of the flat gradient only (``wn_grad_norm_live``)."""
        g = self.grads() if grads is None else grads
        self._check_device(g, scratch, state)
        if live is not None:
            if grads is not None or skip is not None:
                raise ValueError("grad_norm: live ranges belong to the engine's flat gradient (no grads=, no skip=)")
            table, nr, n_live = self._live_args(live)
            rc = self.lib.wn_grad_norm_live(_ptr(g), g.numel(), table, nr, n_live, float(max_norm) if max_norm else 0.0,
                                            int(bool(guard)), float(lr), float(betas[0]), float(betas[1]), _ptr(scratch),
                                            _ptr(state), _stream_handle(self.device))
            self.lib.check(rc, "wn_grad_norm_live")
            return
        lo, hi = self.dead_range if skip is None else skip
        if grads is not None and skip is None:
            lo = hi = 0
        rc = self.lib.wn_grad_norm(_ptr(g), g.numel(), int(lo), int(hi), float(max_norm) if max_norm else 0.0, int(bool(guard)),
                                   float(lr), float(betas[0]), float(betas[1]), _ptr(scratch), _ptr(state),
                                   _stream_handle(self.device))
        self.lib.check(rc, "wn_grad_norm")

    def adam_step_guarded(self, exp_avg, exp_avg_sq, state, eps=1e-8, weight_decay=0.0, live=None):
        """``adam_step`` with its scalars (lr / bc1, sqrt(bc2), clip coefficient, apply flag) read from ``state`` as the
        preceding ``grad_norm`` on the same stream left them.  The gradient buffer keeps its unclipped values."""
        self._check_device(exp_avg, exp_avg_sq, state)
        if live is not None:
            return self._adam_step_guarded_live(exp_avg, exp_avg_sq, None, live, state, eps, weight_decay, 0.0, False)
        rc = self.lib.wn_adam_step_guarded(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq),
                                           self.n_params, float(eps), float(weight_decay), self.dead_range[0],
                                           self.dead_range[1], _ptr(state), _stream_handle(self.device))
        self.lib.check(rc, "wn_adam_step_guarded")
        self._params_epoch += 1

    # ---- exponential moving average of the weights (include/wavenet_hip.h, ABI v14) -----------------
    def adam_step_ema(self, exp_avg, exp_avg_sq, ema, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, ema_decay=0.999,
                      ema_warmup=True, live=None):
        """``adam_step`` that also moves the flat buffer ``ema`` towards the new weights in the same launch:
        ``ema += (1 - d_t) (p_new - ema)``, ``d_t = min(ema_decay, (1 + step) / (10 + step))`` with the warm-up."""
        self._check_device(exp_avg, exp_avg_sq, ema)
        if live is not None:
            return self._adam_step_live(exp_avg, exp_avg_sq, ema, live, step, lr, betas, eps, weight_decay, ema_decay, ema_warmup)
        rc = self.lib.wn_adam_step_ema(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(ema),
                                       self.n_params, int(step), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                       float(weight_decay), self.dead_range[0], self.dead_range[1], float(ema_decay),
                                       int(bool(ema_warmup)), _stream_handle(self.device))
        self.lib.check(rc, "wn_adam_step_ema")
        self._params_epoch += 1

    def adam_step_guarded_ema(self, exp_avg, exp_avg_sq, ema, state, eps=1e-8, weight_decay=0.0, ema_decay=0.999,
                              ema_warmup=True, live=None):
        """``adam_step_guarded`` with the moving average: the warm-up index is the device's count of applied steps, and a step
        that does not apply leaves ``ema`` alone like everything else."""
        self._check_device(exp_avg, exp_avg_sq, ema, state)
        if live is not None:
            return self._adam_step_guarded_live(exp_avg, exp_avg_sq, ema, live, state, eps, weight_decay, ema_decay, ema_warmup)
        rc = self.lib.wn_adam_step_guarded_ema(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq),
                                               _ptr(ema), self.n_params, float(eps), float(weight_decay), self.dead_range[0],
                                               self.dead_range[1], _ptr(state), float(ema_decay), int(bool(ema_warmup)),
                                               _stream_handle(self.device))
        self.lib.check(rc, "wn_adam_step_guarded_ema")
        self._params_epoch += 1

    # ---- parameter groups (include/wavenet_hip.h, ABI v17) -----------------------------------------
    def new_group_scalars(self):
        """The device block of per-group scalars ``grad_norm_groups`` writes and ``adam_step_guarded_groups`` reads (256 bytes;
        allocate it once per optimizer)."""
        return torch.zeros(_lib.MAX_PARAM_GROUPS * ctypes.sizeof(_lib.WnGroupScalars) // 4, dtype=torch.float32, device=self.device)

    def _group_args(self, table, groups):
        if not isinstance(table, GroupTable):
            raise TypeError("the *_groups calls take a GroupTable (WaveNetEngine.group_table)")
        if len(groups) != table.n_groups:
            raise ValueError("%d groups given, the table was built for %d" % (len(groups), table.n_groups))
        return group_array(groups), len(groups)

    def adam_step_groups(self, exp_avg, exp_avg_sq, ema, table, step, groups, betas=(0.9, 0.999), ema_decay=0.0, ema_warmup=False):
        """One Adam step over the ranges of ``table`` (a ``GroupTable``), each with the ``(lr, eps, weight_decay, decoupled)`` of
        its group: one launch (``wn_adam_step_groups``).  ``ema`` None or the average."""
        self._check_device(exp_avg, exp_avg_sq, ema)
        tab, nr, n_live = self._live_args(table)
        arr, ng = self._group_args(table, groups)
        rc = self.lib.wn_adam_step_groups(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(ema),
                                          self.n_params, tab, nr, n_live, int(step), ctypes.cast(arr, ctypes.c_void_p), ng,
                                          float(betas[0]), float(betas[1]), float(ema_decay), int(bool(ema_warmup)),
                                          _stream_handle(self.device))
        self.lib.check(rc, "wn_adam_step_groups")
        self._params_epoch += 1

    def grad_norm_groups(self, state, scratch, group_scalars, table, groups, max_norm=0.0, guard=False, betas=(0.9, 0.999),
                         whole=False):
        """``grad_norm`` for a grouped step: ``state`` as ``grad_norm`` fills it with group 0's lr, and every group's scalars in
        ``group_scalars``.  ``whole``: the ranges of ``table`` are all of the buffer but the dead range (nothing frozen), and
        the sum of squares is the whole-buffer launch of ``grad_norm``; otherwise that of ``grad_norm(live=)`` over the table."""
        g = self.grads()
        self._check_device(g, scratch, state, group_scalars)
        tab, nr, n_live = self._live_args(table)
        arr, ng = self._group_args(table, groups)
        lo, hi = self.dead_range if whole else (0, 0)
        rc = self.lib.wn_grad_norm_groups(_ptr(g), g.numel(), None if whole else tab, nr, n_live, int(lo), int(hi),
                                          float(max_norm) if max_norm else 0.0, int(bool(guard)),
                                          ctypes.cast(arr, ctypes.c_void_p), ng, float(betas[0]), float(betas[1]), _ptr(scratch),
                                          _ptr(state), _ptr(group_scalars), _stream_handle(self.device))
        self.lib.check(rc, "wn_grad_norm_groups")

    def adam_step_guarded_groups(self, exp_avg, exp_avg_sq, ema, table, state, group_scalars, ema_decay=0.0, ema_warmup=False):
        """``adam_step_groups`` with its scalars read from ``state`` and ``group_scalars`` as the preceding ``grad_norm_groups``
        on the same stream left them."""
        self._check_device(exp_avg, exp_avg_sq, ema, state, group_scalars)
        tab, nr, n_live = self._live_args(table)
        rc = self.lib.wn_adam_step_guarded_groups(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq),
                                                  _ptr(ema), self.n_params, tab, nr, n_live, _ptr(group_scalars), _ptr(state),
                                                  float(ema_decay), int(bool(ema_warmup)), _stream_handle(self.device))
        self.lib.check(rc, "wn_adam_step_guarded_groups")
        self._params_epoch += 1

    # ---- layer-wise adaptive steps and per-tensor norms (include/wavenet_hip.h, ABI v20) ------------
    def tensor_table(self, quads, n_groups=1, n=None, device=None):
        """``TensorTable`` of ``(lo, hi, group, adapt)`` quadruples, ONE range per tensor (``wn_tensor_table`` checks them as
        ``wn_group_table`` does, and the adapt flags).  It carries the scratch of the calls that walk it.  One small
        host-to-device copy: build it once per set of live tensors, not per step."""
        n = self.n_params if n is None else int(n)
        quads = [(int(a), int(b), int(c), int(d)) for a, b, c, d in quads]
        nr = len(quads)
        flat = (ctypes.c_int64 * max(4 * nr, 1))(*[x for q in quads for x in q])
        host = torch.zeros(7 * nr + 1 + n // _lib.TENSOR_CHUNK, dtype=torch.int64)
        n_live = self.lib.wn_tensor_table(ctypes.cast(flat, ctypes.c_void_p), nr, n, int(n_groups), ctypes.c_void_p(host.data_ptr()))
        if n_live < 0:
            raise _lib.WnError("wn_tensor_table failed: %s" % self.lib.wn_last_error().decode())
        n_blocks = int(self.lib.wn_tensor_blocks(ctypes.c_void_p(host.data_ptr()), nr))
        host = host[:6 * nr + 1 + n_blocks]
        device = self.device if device is None else device
        scratch = torch.empty(int(self.lib.wn_lamb_scratch_floats(n_blocks)), dtype=torch.float32, device=device)
        return TensorTable([(a, b) for a, b, _, _ in quads], [c for _, _, c, _ in quads], n_groups, n_live, n, host.to(device),
                           [bool(d) for _, _, _, d in quads], n_blocks, scratch)

    def _tensor_args(self, table):
        if not isinstance(table, TensorTable):
            raise TypeError("this call takes a TensorTable (WaveNetEngine.tensor_table)")
        self._check_device(table.table, table.scratch)
        return _ptr(table.table), table.n_ranges, table.n_live

    def lamb_step(self, exp_avg, exp_avg_sq, ema, table, stats, groups, step=0, state=None, betas=(0.9, 0.999), max_trust_ratio=None,
                  ema_decay=0.0, ema_warmup=False):
        """One layer-wise adaptive step over the tensors of ``table`` (a ``TensorTable``), each with the
        ``(lr, eps, weight_decay, decoupled)`` of its group: three launches (``wn_lamb_step``).  ``state`` None: unguarded, with
        the host's ``step``; otherwise the state block as the preceding ``grad_norm*`` call left it.  ``stats``: ``3 * n_ranges``
        floats on the device, per tensor the weight norm, the update norm and the trust ratio."""
        self._check_device(exp_avg, exp_avg_sq, ema, stats, state)
        if table.n != self.n_params:
            raise ValueError("the tensor table was built for a buffer of %d elements, the flat buffers hold %d" % (table.n, self.n_params))
        tab, nr, n_live = self._tensor_args(table)
        if stats.dtype != torch.float32 or stats.numel() < 3 * nr:
            raise ValueError("stats takes 3 * n_ranges floats")
        arr, ng = self._group_args(table, groups)
        rc = self.lib.wn_lamb_step(_ptr(self.flat_params), _ptr(self.grads()), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(ema), self.n_params,
                                   tab, nr, n_live, int(step), ctypes.cast(arr, ctypes.c_void_p), ng, float(betas[0]), float(betas[1]),
                                   float(max_trust_ratio) if max_trust_ratio else 0.0, _ptr(state), float(ema_decay),
                                   int(bool(ema_warmup)), _ptr(table.scratch), _ptr(stats), _stream_handle(self.device))
        self.lib.check(rc, "wn_lamb_step")
        self._params_epoch += 1

    def tensor_norms(self, buf, table, out=None):
        """Per-tensor L2 norms of the flat fp32 buffer ``buf`` over the ranges of ``table`` (a ``TensorTable`` built for
        ``buf.numel()`` elements): a float64 device tensor of ``n_ranges`` elements, two launches and one ``sqrt``, whatever the
        number of tensors.  ``out``: a float64 tensor to take the sums of squares (it is returned square-rooted in place)."""
        tab, nr, n_live = self._tensor_args(table)
        self._check_device(buf)
        if buf.dtype != torch.float32 or not buf.is_contiguous() or buf.numel() != table.n:
            raise ValueError("tensor_norms takes a contiguous fp32 buffer of the %d elements the table was built for" % table.n)
        out = torch.empty(nr, dtype=torch.float64, device=buf.device) if out is None else out
        rc = self.lib.wn_tensor_sumsq(_ptr(buf), buf.numel(), tab, nr, n_live, _ptr(table.scratch), _ptr(out),
                                      _stream_handle(self.device))
        self.lib.check(rc, "wn_tensor_sumsq")
        return out.sqrt_()

    def swap_params(self, other):
        """Exchange the flat parameter buffer with ``other`` (same length, same device) element by element: one launch, no
        temporary.  The parameter version changes, so everything derived from the weights (packed weight sets) follows."""
        self._check_device(other)
        if other.dtype != torch.float32 or other.numel() != self.n_params or not other.is_contiguous():
            raise ValueError("swap_params takes a contiguous fp32 tensor of n_params elements")
        rc = self.lib.wn_op_swap(_ptr(self.flat_params), _ptr(other), self.n_params, _stream_handle(self.device))
        self.lib.check(rc, "wn_op_swap")
        self._params_epoch += 1

    # ---- autoregressive decode (reference wavenet.py:309-511) ---------------------------------
    def decode_supported(self):
        return bool(self.lib.wn_decode_supported(ctypes.byref(self.cfg)))

    def sampling_setting(self, mode, temperature=1.0, top_k=None, top_p=None):
        """``WnSampling`` of a decode with these parameters, or None for the identity (temperature 1, no top-k, top-p 1: the plain
        call).  ValueError for a temperature that is not positive and finite, top_k < 0, top_p outside (0, 1], and for parameters
        other than the identity with anything but mode "sampling" on the softmax head."""
        T = float(temperature)
        k = 0 if top_k is None else int(top_k)
        pp = 1.0 if top_p is None else float(top_p)
        if not (T > 0.0) or T == float("inf") or 1.0 / T > 3.0e38:
            raise ValueError("temperature should be positive and finite, got %r" % (temperature,))
        if k < 0:
            raise ValueError("top_k should be >= 0 (0 or None: off), got %r" % (top_k,))
        if not (0.0 < pp <= 1.0):
            raise ValueError("top_p should be in (0, 1] (1 or None: off), got %r" % (top_p,))
        if T == 1.0 and k == 0 and pp == 1.0:
            return None
        if mode != "sampling":
            raise ValueError("temperature / top_k / top_p apply to mode sampling only, got mode %s" % mode)
        if self.out_channels != self.cfg.n_quantize:
            raise ValueError("temperature / top_k / top_p are not defined for the mixture-of-logistics head")
        return _lib.WnSampling(1.0 / T, k, pp)   # (1.0 / T in double, rounded to float by the structure)

    def decode(self, x, h, n_samples_list, mode="argmax", chunk=4096, return_logits=False, progress=None, layered=None,
               prefill="parallel", prefill_batch=32, log_scale_min=-7.0, temperature=1.0, top_k=None, top_p=None):
        """See ``_decode``.  ``layered="granules"``: the any-size path with its persistent launches handing their vectors over
        as 8-byte granules everywhere (csrc/wn_dlp.hip, wn_dlpm.hip) instead of plain vectors + flags where csrc/wn_dlpf.hip
        covers the model -- an A/B and test knob (the mode bit WN_DECODE_GRANULES of every library call of this decode).

        A persistent launch that gives up waiting between its workgroups (they were not all resident: another kernel held
        compute units) raises ``WnDecodeTimeout`` inside; the decode is then done again by layer-wise launches (HIP kernels
        as well; a warning says so) -- context, aux features and, in the sampling mode, the uniform draws are the same, so
        the tokens are those the persistent launch would have produced.

        ``temperature``, ``top_k``, ``top_p`` (mode "sampling", softmax head): the logits are multiplied by 1 / temperature, cut to
        the top_k largest (ties kept), then to the smallest set of largest classes holding top_p of the probability (ties kept),
        and the draw is made among what is left -- inside the decode kernels (csrc/wn_sample.h); one setting per
        call, carried through the groups of a large batch and the fall-back.  The defaults are the plain sampling decode."""
        sampling = self.sampling_setting(mode, temperature, top_k, top_p)
        granules = layered == "granules"
        lay = True if granules else layered
        mbits = _lib.DECODE_GRANULES if granules else 0
        draws = None
        if mode == "sampling":   # drawn once for the whole batch: neither the grouping nor a fall-back changes the tokens
            n_pad = max(self.receptive_field - x.size(1), 0)
            draws = torch.rand((x.size(0), x.size(1) + n_pad + int(max(n_samples_list))), dtype=torch.float32, device=self.device)
        try:
            return self._decode_groups(x, h, n_samples_list, mode, chunk, return_logits, progress, lay, prefill, prefill_batch,
                                       log_scale_min, mbits, draws, sampling)
        except _lib.WnDecodeTimeout as e:
            warnings.warn("%s -- decoding again by layer-wise launches" % e, RuntimeWarning)
            return self._decode_groups(x, h, n_samples_list, mode, chunk, return_logits, progress, "launches", prefill,
                                       prefill_batch, log_scale_min, 0, draws, sampling)

    def _decode_groups(self, x, h, n_samples_list, mode, chunk, return_logits, progress, lay, prefill, prefill_batch, log_scale_min,
                       mbits, draws, sampling=None):
        groups = self._persistent_groups(x.size(0), lay, mode, mbits)
        if groups is None:
            return self._decode(x, h, n_samples_list, mode, chunk, return_logits, progress, lay, prefill, prefill_batch,
                                log_scale_min, _uniforms=draws, _mbits=mbits, _sampling=sampling)
        # More utterances than ONE persistent launch takes (64 with the flag hand-off: four column blocks = 256 workgroups), up to
        # two launches' worth: the batch goes through it in two groups -- the utterances are independent.
        T0 = x.size(1)
        n_pad = max(self.receptive_field - T0, 0)
        toks, lgs = [], []
        total = sum(int(max(n_samples_list[g0:g1])) for g0, g1 in groups)
        done = 0
        for g0, g1 in groups:
            ns = list(n_samples_list[g0:g1])
            u = None if draws is None else draws[g0:g1, :T0 + n_pad + int(max(ns))].contiguous()
            prog = None if progress is None else (lambda d, n, base=done: progress(base + d, total))   # steps over all groups
            r = self._decode(x[g0:g1].contiguous(), h[g0:g1].contiguous(), ns, mode, chunk, return_logits, prog, lay, prefill,
                             prefill_batch, log_scale_min, _uniforms=u, _mbits=mbits, _sampling=sampling)
            done += int(max(ns))
            toks += r[0] if return_logits else r
            if return_logits:
                lgs += r[1]
        self.last_uniforms = draws
        return (toks, lgs) if return_logits else toks

    def decode_residency(self, B, layered=None):
        """(persistent, workgroups, capacity) of the any-size decode of B utterances on this device: whether it runs as ONE
        persistent launch, the workgroups that launch needs resident at once and how many the device keeps
        (``wn_decode_layered_residency``)."""
        wg, cap = ctypes.c_int(0), ctypes.c_int(0)
        rc = self.lib.wn_decode_layered_residency(ctypes.byref(self.cfg), int(B), _lib.DECODE_GRANULES if layered == "granules" else 0,
                                                  ctypes.byref(wg), ctypes.byref(cap))
        if rc < 0:
            raise _lib.WnError("wn_decode_layered_residency: %s" % self.lib.wn_last_error().decode())
        return bool(rc), wg.value, cap.value

    def _persistent_groups(self, B, layered, mode, mbits=0):
        """[(begin, end)] when a batch of B utterances should go through the persistent any-size launch in groups, else None: the
        any-size path is asked for (or chosen because the one-workgroup kernel does not cover the model), B is more than one
        launch takes, and a launch of the group size exists."""
        if layered == "launches" or mode not in ("argmax", "sampling") or B <= 1:
            return None
        if layered is None and self.decode_supported():
            return None
        if layered is not None and not layered:
            return None
        cfg = ctypes.byref(self.cfg)
        if self.lib.wn_decode_layered_error_offset(cfg, B, mbits) >= 0:
            return None   # one launch takes the whole batch
        gs = 0
        for cand in (64, 48, 32, 16, 8, 4, 2):   # whole column blocks of 16 first; what the device keeps resident decides (wn_dlp.h)
            if self.lib.wn_decode_layered_error_offset(cfg, cand, mbits) >= 0:
                gs = cand
                break
        if gs <= 1 or B <= gs or B > 2 * gs:
            return None   # (three groups and more: the layer-wise launches on the whole batch are as fast or faster -- n_resch 512:
                          # 777 against 751 us per step at 128 utterances, 1575 against 837 at 256; 509 against 710 at 64)
        return [(g0, min(g0 + gs, B)) for g0 in range(0, B, gs)]

    def _decode(self, x, h, n_samples_list, mode="argmax", chunk=4096, return_logits=False, progress=None, layered=None,
                prefill="parallel", prefill_batch=32, log_scale_min=-7.0, _uniforms=None, _mbits=0, _sampling=None):
        """Queue-based sample-by-sample generation on the HIP decode kernel.

        x (B,T0) int64 context, h (B, n_aux, frames | samples) aux features covering T0 + max(n)
        samples, n_samples_list: samples to generate per utterance.  Follows the reference's prologue
        (wavenet.py:328-336, 417-425): the context is left-padded with n_quantize//2 up to the
        receptive field and the aux features by replicating their first column.  Returns the
        generated tokens as a list of LongTensors (utterance order) [and the per-step logits].

        Two kernels implement it: the persistent one-workgroup-per-utterance kernel (model sizes covered by
        ``decode_supported()``) and the any-size path (``layered=True``; chosen automatically when the first does not
        apply, e.g. the n_resch = 512 recipe default).  The any-size path is itself ONE persistent launch per chunk of
        steps where csrc/wn_dlp.hip / wn_dlpm.hip / wn_dlpf.hip cover the model and the batch (up to 64 utterances: workgroups
        handing their vectors to each other) and layer-wise launches otherwise; ``layered="launches"`` forces the launches (independent check, A/B).

        ``prefill``: how the dilation queues of the context are built.  "parallel" (default) does what the
        reference does (wavenet.py:338-349): one forward of the residual stack over the whole padded context
        (``prefill_batch`` utterances at a time), then decoding starts at the last context position.  "walk"
        steps the decode kernel through the context sample by sample (teacher forced; receptive-field steps
        before the first new sample) -- kept as the independent check of the former.
        ``log_scale_min`` (mode "mol"): clamp of the mixture log-scales, the value the model was trained with.
        """
        self._check_device(x, h)
        if x.dtype != torch.int64 or x.dim() != 2 or h.dim() != 3:
            raise ValueError("x must be a LongTensor (B, T) and h a FloatTensor (B, n_aux, F)")
        if mode not in ("argmax", "sampling", "mol"):
            raise ValueError("mode should be sampling, argmax or mol")
        if mode == "mol" and (self.out_channels % 3 != 0 or self.out_channels == self.cfg.n_quantize):
            raise ValueError("mode mol needs a model with the mixture-of-logistics head (n_mixture)")
        n_mix = self.out_channels // 3 if mode == "mol" else 0
        cfg = ctypes.byref(self.cfg)
        B, T0 = x.shape
        if len(n_samples_list) != B or h.size(0) != B or h.size(1) != self.cfg.n_aux:
            raise ValueError("batch mismatch between x, h and n_samples_list")
        U = self.cfg.upsampling_factor
        n_max = int(max(n_samples_list))
        need = T0 + n_max - 1   # last aux column read: sample index T0 + n_max - 2
        F = h.size(2)
        if (F * U if U > 0 else F) < need:
            raise ValueError("h covers %d samples, %d needed" % (F * U if U > 0 else F, need))
        n_pad = max(self.receptive_field - T0, 0)
        Tctx = T0 + n_pad
        Ttot = Tctx + n_max
        if layered is None:
            layered = not self.decode_supported()
        mbits = (_lib.DECODE_BY_LAUNCHES if layered == "launches" else 0) | int(_mbits)   # the same bits to every call of this decode
        layered = bool(layered)
        if prefill not in ("parallel", "walk"):
            raise ValueError("prefill should be parallel or walk")
        st = _stream_handle(self.device)
        dev = self.device
        h = h.contiguous().float()
        nG = self.n_layers * 2 * self.cfg.n_resch
        # Aux projections G (B, columns, L*2R).  With the upsampling layer the columns are frames (small): all of them
        # up front.  Without it (U = 0, decode.py's extend_time path) a column is a SAMPLE -- 5 s at 16 kHz with the
        # recipe-size model would be 9.8 GB per utterance -- so G only ever holds the columns of the chunk of steps
        # being decoded (at most ~1 GiB), recomputed per chunk from the matching slice of h.
        windowed = (U == 0)
        if windowed:
            chunk = max(1, min(int(chunk), (1 << 30) // (4 * nG * B)))
        wpack = None
        if layered:
            nst = self.lib.wn_decode_layered_state_floats(cfg, B, mbits)
            if nst <= 0:
                raise _lib.WnError("wn_decode_layered_state_floats: %s" % self.lib.wn_last_error().decode())
            state = torch.zeros(nst, dtype=torch.float32, device=dev)
        else:
            npk = self.lib.wn_decode_pack_floats(cfg)
            if npk <= 0:
                raise _lib.WnError("wn_decode_pack_floats: %s" % self.lib.wn_last_error().decode())
            wpack = torch.empty(npk, dtype=torch.float32, device=dev)
            self.lib.check(self.lib.wn_decode_pack(cfg, _ptr(self.flat_params), _ptr(wpack), st), "wn_decode_pack")
            state = torch.zeros((B, self.lib.wn_decode_state_floats(cfg)), dtype=torch.float32, device=dev)

        packed = [False]

        def aux_columns(c0, c1):
            """G of aux columns [c0, c1).  The layered variant packs the weights into its state on the first call only
            (params = NULL afterwards: a windowed decode comes here once per chunk of steps)."""
            hw = h if (c0 == 0 and c1 == F) else h[:, :, c0:c1].contiguous()
            Gw = torch.empty((B, c1 - c0, nG), dtype=torch.float32, device=dev)
            if layered:
                self.lib.check(self.lib.wn_decode_layered_prepare(cfg, B, c1 - c0, None if packed[0] else _ptr(self.flat_params),
                                                                  _ptr(hw), _ptr(Gw), _ptr(state), nst, mbits, st),
                               "wn_decode_layered_prepare")
                packed[0] = True
            else:
                self.lib.check(self.lib.wn_decode_aux(cfg, B, c1 - c0, _ptr(wpack), _ptr(hw), _ptr(Gw), st), "wn_decode_aux")
            return Gw

        G = None if windowed else aux_columns(0, F)
        samples = torch.full((B, Ttot), self.cfg.n_quantize // 2, dtype=torch.int64, device=dev)
        samples[:, n_pad:Tctx] = x
        t_forced = torch.full((B,), Tctx, dtype=torch.int32, device=dev)
        t_end = torch.tensor([Tctx + int(n) for n in n_samples_list], dtype=torch.int32, device=dev)
        if mode == "mol":   # n_mix Gumbel draws + one logistic draw per position, kept away from 0 and 1
            uniforms = torch.rand((B, Ttot, n_mix + 1), dtype=torch.float32, device=dev).clamp_(1e-5, 1.0 - 1e-5)
            wave = torch.zeros((B, Ttot), dtype=torch.float32, device=dev)
        else:
            uniforms = None
            if mode == "sampling":   # (a group of a larger batch brings its rows of the whole batch's draws)
                uniforms = _uniforms if _uniforms is not None else torch.rand((B, Ttot), dtype=torch.float32, device=dev)
                if tuple(uniforms.shape) != (B, Ttot):
                    raise ValueError("uniforms must be (B, Ttot)")
            wave = None
        logits = torch.zeros((B, Ttot, self.out_channels), dtype=torch.float32, device=dev) if return_logits else None
        eoff = -1   # float offset of the persistent launch's error word in the state (-1: layer-wise launches / other kernel)
        if layered and not (mbits & _lib.DECODE_BY_LAUNCHES) and mode != "mol":
            eoff = self.lib.wn_decode_layered_error_offset(cfg, B, mbits)
        p = 0
        if prefill == "parallel" and Tctx >= 2:
            self._decode_prefill(samples, h, F, Tctx, n_pad, state, (1 | int(_mbits)) if layered else 0, int(prefill_batch), st)
            p = Tctx - 1
        while p < Ttot - 1:
            p1 = min(p + chunk, Ttot - 1)
            if windowed:
                # steps [p, p1) read the aux columns max(q - n_pad, 0) for q in [p, p1): compute that window and shift
                # the kernel's padding origin by its first column (a position left of it can only be inside the left
                # padding, which replicates column 0 = the window's first column then)
                c0 = min(max(p - n_pad, 0), F - 1)
                c1 = min(max(p1 - 1 - n_pad, 0), F - 1) + 1
                G = None  # release the previous window first
                G = aux_columns(c0, c1)
                Fw, pad_w = c1 - c0, n_pad + c0
            else:
                Fw, pad_w = F, n_pad
            if layered:
                largs = (cfg, B, _ptr(self.flat_params), _ptr(G), Fw, pad_w, _ptr(samples), Ttot, _ptr(t_forced), _ptr(t_end), p, p1,
                         _ptr(state), state.numel(), _ptr(uniforms), _ptr(logits), {"argmax": 0, "sampling": 1, "mol": 2}[mode] | mbits,
                         _ptr(wave), float(log_scale_min))
                if _sampling is None:   # the identity setting IS the plain call
                    rc = self.lib.wn_decode_layered_steps(*(largs + (st,)))
                else:
                    rc = self.lib.wn_decode_layered_steps_filtered(*(largs + (ctypes.byref(_sampling), st)))
                if rc == 4 and eoff >= 0:   # the persistent grid would not be resident at once (the device changed under a cached
                    # layout, a partitioned GPU): the same fall-back as a time-out
                    raise _lib.WnDecodeTimeout("the persistent decode launch was refused: its %s" % self.lib.wn_last_error().decode())
                self.lib.check(rc, "wn_decode_layered_steps")
                # the persistent launch bounds every wait between its workgroups and reports a time-out in the state; a launch
                # that finds the word set returns at once, so it is looked at after every chunk (one word, once per chunk)
                if eoff >= 0 and int(state[eoff:eoff + 1].view(torch.int32).item()) != 0:
                    raise _lib.WnDecodeTimeout("the persistent decode launch timed out waiting between its workgroups (not all "
                                               "of them were resident at once: another kernel on the device?)")
            else:
                sargs = (cfg, B, _ptr(self.flat_params), _ptr(wpack), _ptr(G), Fw, pad_w, _ptr(samples), Ttot, _ptr(t_forced),
                         _ptr(t_end), p, p1, _ptr(state), _ptr(uniforms), _ptr(logits), {"argmax": 0, "sampling": 1, "mol": 2}[mode],
                         _ptr(wave), float(log_scale_min))
                if _sampling is None:
                    rc = self.lib.wn_decode_steps(*(sargs + (st,)))
                else:
                    rc = self.lib.wn_decode_steps_filtered(*(sargs + (ctypes.byref(_sampling), st)))
                self.lib.check(rc, "wn_decode_steps")
            p = p1
            if progress is not None:
                progress(max(p + 1 - Tctx, 0), n_max)
        self.last_decode_state = state if layered else None   # (tools/dlp_timing.py reads a timing build's stamps from it)
        out = [samples[b, Tctx:Tctx + int(n)] for b, n in enumerate(n_samples_list)]
        self.last_wave = None if wave is None else [wave[b, Tctx:Tctx + int(n)] for b, n in enumerate(n_samples_list)]
        self.last_uniforms = uniforms
        if return_logits:   # row Tctx-1+i holds the logits that chose generated sample i
            return out, [logits[b, Tctx - 1:Tctx - 1 + int(n)] for b, n in enumerate(n_samples_list)]
        return out

    def _decode_prefill(self, samples, h, F, Tctx, n_pad, state, layered, nbatch, st):
        """Dilation queues of the context from one forward of the residual stack (wn_decode_prefill)."""
        cfg = ctypes.byref(self.cfg)
        B = samples.size(0)
        dev = self.device
        # Only the newest rf + K - 1 positions reach the queues (rf - 1 through the dilated stack, K - 1 more
        # through the causal front conv): a longer context is passed as its tail.
        pos0 = max(0, Tctx - (self.receptive_field + self.cfg.kernel_size - 1))
        Tpre = Tctx - pos0
        # groups of utterances with a bounded workspace (the training workspace of nb x Tpre inputs)
        per_utt = self.lib.wn_decode_prefill_workspace_bytes(cfg, 1, Tpre)
        if per_utt == 0:
            raise _lib.WnError("wn_decode_prefill_workspace_bytes: %s" % self.lib.wn_last_error().decode())
        nbatch = max(1, min(nbatch, (8 << 30) // per_utt))
        ws = None
        for b0 in range(0, B, nbatch):
            nb = min(nbatch, B - b0)
            x_ctx = samples[b0:b0 + nb, pos0:Tctx].contiguous()
            h_ctx = torch.empty((nb, self.cfg.n_aux, Tpre), dtype=torch.float32, device=dev)
            self.lib.check(self.lib.wn_decode_ctx_aux(cfg, nb, F, Tpre, n_pad, pos0, _ptr(self.flat_params),
                                                      _ptr(h[b0:b0 + nb]), _ptr(h_ctx), st), "wn_decode_ctx_aux")
            nbytes = self.lib.wn_decode_prefill_workspace_bytes(cfg, nb, Tpre)
            if ws is None or ws.numel() * 4 < nbytes:
                ws = None
                ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
            rc = self.lib.wn_decode_prefill(cfg, nb, Tpre, pos0, _ptr(self.flat_params), _ptr(x_ctx), _ptr(h_ctx), _ptr(ws),
                                            ws.numel() * 4, _ptr(state), state.numel(), B, b0, int(layered), self.flags,
                                            st)
            self.lib.check(rc, "wn_decode_prefill")



# ---- reference state_dict keys <-> flat buffer ------------------------------------------------
_LIST_KINDS = {
    "dil_sigmoid": (_lib.P_DSIG_W, _lib.P_DSIG_B, True),
    "dil_tanh": (_lib.P_DTANH_W, _lib.P_DTANH_B, True),
    "aux_1x1_sigmoid": (_lib.P_ASIG_W, _lib.P_ASIG_B, False),
    "aux_1x1_tanh": (_lib.P_ATANH_W, _lib.P_ATANH_B, False),
    "skip_1x1": (_lib.P_SKIP_W, _lib.P_SKIP_B, False),
    "res_1x1": (_lib.P_RES_W, _lib.P_RES_B, False),
}
_SINGLE_KINDS = {
    "causal.conv.weight": _lib.P_CAUSAL_W, "causal.conv.bias": _lib.P_CAUSAL_B,
    "upsampling.conv.weight": _lib.P_UP_W, "upsampling.conv.bias": _lib.P_UP_B,
    "conv_post_1.weight": _lib.P_POST1_W, "conv_post_1.bias": _lib.P_POST1_B,
    "conv_post_2.weight": _lib.P_POST2_W, "conv_post_2.bias": _lib.P_POST2_B,
}


def key_to_kind(key):
    """Reference state_dict key (wavenet.py:187-210) -> (tensor kind, layer)."""
    if key in _SINGLE_KINDS:
        return _SINGLE_KINDS[key], 0
    parts = key.split(".")
    name, layer = parts[0], int(parts[1])
    wk, bk, has_conv = _LIST_KINDS[name]
    expect = 4 if has_conv else 3
    if len(parts) != expect or (has_conv and parts[2] != "conv"):
        raise KeyError(key)
    return (wk if parts[-1] == "weight" else bk), layer


def state_keys(cfg):
    """All state_dict keys in the reference's registration order."""
    L = cfg.dilation_depth * cfg.dilation_repeat
    keys = ["causal.conv.weight", "causal.conv.bias"]
    if cfg.upsampling_factor > 0:
        keys += ["upsampling.conv.weight", "upsampling.conv.bias"]
    for name in ("dil_sigmoid", "dil_tanh"):
        for l in range(L):
            keys += ["%s.%d.conv.weight" % (name, l), "%s.%d.conv.bias" % (name, l)]
    for name in ("aux_1x1_sigmoid", "aux_1x1_tanh", "skip_1x1", "res_1x1"):
        for l in range(L):
            keys += ["%s.%d.weight" % (name, l), "%s.%d.bias" % (name, l)]
    keys += ["conv_post_1.weight", "conv_post_1.bias", "conv_post_2.weight", "conv_post_2.bias"]
    return keys


def load_state_into_flat(engine, state):
    """Copy a reference-layout state dict {key: tensor} into the engine's flat parameter buffer."""
    for k in state_keys(engine.cfg):
        kind, layer = key_to_kind(k)
        off, n = engine.param_slice(kind, layer)
        v = state[k]
        if v.numel() != n:
            raise ValueError("%s: expected %d elements, got %s" % (k, n, tuple(v.shape)))
        engine.flat_params[off:off + n].copy_(v.reshape(-1).to(engine.flat_params.dtype))


def flat_to_state(engine, flat, shapes):
    """Views of a flat buffer keyed like the reference state dict (shapes: {key: shape})."""
    out = {}
    for k in state_keys(engine.cfg):
        kind, layer = key_to_kind(k)
        off, n = engine.param_slice(kind, layer)
        out[k] = flat[off:off + n].view(shapes[k])
    return out
