# -*- coding: utf-8 -*-
"""No result depends on what the workspace held before the call: checks shared by tests/test_emu_workspace.py (host emulator)
and tests/test_gpu_workspace.py (MI355X).

The C ABI says the caller owns the workspace and the library keeps no state between calls (include/wavenet_hip.h).  The
workspace is one buffer carved into more than forty regions (make_ws, csrc/wn_api.hip); which launch writes a region and which
reads it depends on the kernel family, the arithmetic flags and the launch plan.  ``WaveNetEngine.workspace()`` allocates it
zero-filled, and zero is the neutral element of a split-K sum, of a ReLU mask product and of an abs-max -- so a word that is read
before it is written passes every oracle gate of the other test files.  In training the same buffer serves step after step and
such a word holds the previous minibatch's value instead.

``probe_step`` runs one training step the way a user of the engine does (a ROUTE) and returns everything the step hands its
caller, each buffer NaN before the call that writes it.  ``check_workspace_independence`` runs it on a fresh zero-filled
workspace (the BASELINE: asserted bit-identical run to run and held to the oracle's gates) and then again after a PRE-STATE was
given to the workspace; every returned tensor must be bit-identical (``torch.equal``) to the baseline's -- the same launches
on the same inputs in the same order give the same bits, so there is no tolerance to choose.

The one input a backward call takes from the workspace of an EARLIER call by contract is max |dlogits| of the last loss call
(WN_FLAG_DW_F16_AMAX_WS); the engine sets that flag only for the tensor that very call returned on that very workspace, so no
route needs an exception for it."""
import contextlib
import ctypes
import functools
from unittest import mock

import numpy as np
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS, WaveNetEngine, flat_to_state, load_state_into_flat
from tests import parity_common as PC
from tests import plan_common as PL
from tests import ragged_common as RG
from tests.golden_util import rel_to_max

NM = 4   # mixture components of the "mol" route: the engine gets out_channels = 3 * NM

# id -> (cfg, B, T): the smallest shapes that still take each path (PATH_TAGS)
SHAPES = dict(PL.SHAPES)
SHAPES["N3"] = ((32, 4, 64, 128, 3, 1, 2, 0), 1, 150)     # fused, no upsampling layer, T % 32 != 0: tile tails, dh from dP
SHAPES["W1"] = ((32, 4, 128, 128, 2, 1, 2, 8), 1, 64)     # wide any-size path (n_resch % 128 == 0): apk_wide / apk_wide16
SHAPES["T1"] = ((256, 4, 64, 256, 7, 1, 3, 16), 1, 288)   # 256 classes: the loss as the epilogue of conv_post_2 over the window
#                                                           [t0 = 128, T); receptive field 255, so columns lie in front of t0;
#                                                           256 skip channels: the fused skip + res launch reads dSkip there
MIDSIZE = ((256, 80, 64, 256, 10, 3, 2, 80), 2, 3120)

# launches of one training step (forward_loss + backward with dh) under DEFAULT_FLAGS: (must appear, must not appear)
PATH_TAGS = dict((k, (v[0], tuple(t for t in v[1] if t != "aux_bwd"))) for k, v in PL.PATH_TAGS.items())
PATH_TAGS["N3"] = (("fused_bwd_chain", "aux_dh", "dw_aux"), ("aux_finish", "aux_bwd", "bwd_dx_dilated"))
PATH_TAGS["W1"] = (("fwd_dilated_gate", "bwd_dx_dilated", "bwd_dz_res_gate"), ("fused_bwd_chain", "dw_skip_res"))
PATH_TAGS["T1"] = (("fwd_post2_ce", "fused_bwd_chain", "fill_cols", "dw_skip_res"), ("softmax_ce", "dw_skip"))

# the other (B, T) pairs of the stale-shape sequence on ONE buffer sized for the largest: (2, 2 T) first, then (1, T / 2 rounded
# to the upsampling factor), then the probe step at the shape's own (B, T)
def companions(cfg, B, T):
    U = max(cfg[7], 1)
    rf = O.OracleConfig(*cfg).receptive_field
    half = max((T // 2 + U - 1) // U * U, (rf + 1 + U - 1) // U * U)   # (a step needs a loss position: T > receptive field)
    return (2, 2 * T), (1, half)


ARITH = {
    "default": DEFAULT_FLAGS,
    "six": SIX_PRODUCT_FLAGS,
    "default+chain16": DEFAULT_FLAGS | _lib.FLAG_CHAIN_F16PAIR,
    "exact": DEFAULT_FLAGS | _lib.FLAG_EXACT_MFMA,
    "nofused": DEFAULT_FLAGS | _lib.FLAG_NO_FUSED,
    "default-auxfused": DEFAULT_FLAGS & ~_lib.FLAG_AUX_FUSED,
}
# stale-arith: the arithmetic of the step that used the buffer before the probe step.  The 16-bit weight images, the amaxP
# maxima and the overflow words of one mode must not be read by the other.
STALE_ARITH = {
    "default": SIX_PRODUCT_FLAGS,
    "six": DEFAULT_FLAGS,
    "default+chain16": SIX_PRODUCT_FLAGS,
    "exact": DEFAULT_FLAGS,
    "nofused": DEFAULT_FLAGS,
    "default-auxfused": SIX_PRODUCT_FLAGS | _lib.FLAG_CHAIN_F16PAIR | _lib.FLAG_MM_F16PAIR,
}
CHAIN_MM = SIX_PRODUCT_FLAGS | _lib.FLAG_CHAIN_F16PAIR | _lib.FLAG_MM_F16PAIR   # ... and this one before the default, per shape
STATES = ("nan", "garbage", "stale-data", "stale-shape", "stale-arith")
ROUTES = ("train", "train0", "full", "ragged", "frozen", "mol", "scan", "promise")
AXES = (("state", STATES), ("route", ROUTES), ("arith", tuple(ARITH)))


def rows():
    """Pairwise covering of (pre-state, route, arithmetic) -- tests/plan_common.pairwise_rows -- used for every shape."""
    return PL.pairwise_rows(AXES, ())


def row_id(r):
    return "%s-%s-%s" % (r["state"], r["route"], r["arith"].replace("+", "_"))


def ragged_lengths(B, T, rf):
    """Sequence 0 ends early -- 57 positions (a third of T where T < 114), or half way through the loss positions where that
    would leave it none: inside a 128-column block of the loss launches, never on its edge -- and the others run to T."""
    n0 = T - (57 if T >= 114 else T // 3)
    if n0 <= rf:
        n0 = rf + max((T - rf) // 2, 1)
    return tuple(n0 if b == 0 else T for b in range(B))


def _cfg(cfg_t, route):
    return O.OracleConfig(*cfg_t, out_channels=3 * NM) if route == "mol" else O.OracleConfig(*cfg_t)


MIDSIZE_SEED, MIDSIZE_SCALE = 41, 0.05   # the instance of test_gpu_launch_plans' mid-size test: one oracle step for both files


@functools.lru_cache(maxsize=64)
def instance(cfg_t, B, T, mol):
    """Seeded model and minibatch (ReLU kink margin >= PC.KINK_MARGIN): (params, x, h, t, y); ``y`` is the waveform of the
    mixture head."""
    if (cfg_t, B, T) == MIDSIZE and not mol:
        params, x, h, t = PL.reference(cfg_t, B, T, MIDSIZE_SEED, scale=MIDSIZE_SCALE)[:4]
        sd = MIDSIZE_SEED
    else:
        params, x, h, t, margin, sd = PC.pick_instance(_cfg(cfg_t, "mol" if mol else ""), B, T, PL.SEED, 0.1)
    y = torch.from_numpy(np.random.RandomState(sd + 2).uniform(-1, 1, (B, T)).astype(np.float32))
    return params, x, h, t, y


def other_batch(cfg_t, B, T, seed, h_scale=1.0):
    """Another minibatch (x, h, t, y) for the steps that use the workspace BEFORE the probe step (no kink margin needed:
    nothing is compared with the oracle)."""
    x, h, t = O.synthetic_batch(O.OracleConfig(*cfg_t), B, T, seed)
    y = torch.from_numpy(np.random.RandomState(seed + 2).uniform(-1, 1, (B, T)).astype(np.float32))
    return x, (h * h_scale).contiguous(), t, y


@functools.lru_cache(maxsize=64)
def reference(cfg_t, B, T, kind):
    """The oracle's step on ``instance``, computed once per (shape, kind) and left unchanged: (loss, {name: gradient}, dh,
    logits or None, fp32 error of the mixture formula or None).  kind "dense" / "ragged": the fp64 evaluation of the softmax step
    (tests/ragged_common.oracle_ragged); "mol": the restatement of the mixture likelihood in fp64, and how far its own fp32
    evaluation is from that (tests/mol_common.py: the gate allows for it)."""
    params, x, h, t, y = instance(cfg_t, B, T, kind == "mol")
    if (cfg_t, B, T) == MIDSIZE and kind == "dense":   # (loss and weight gradients; dh is compared bit for bit only at this size)
        _, _, _, _, loss_ref, _, grads_ref = PL.reference(cfg_t, B, T, MIDSIZE_SEED, scale=MIDSIZE_SCALE)
        return float(loss_ref), grads_ref, None, None, None
    if kind == "mol":
        cfg = _cfg(cfg_t, "mol")
        l64, g64, dh64 = RG.mol_oracle(cfg, params, x, h, y, (T,) * B, torch.float64)
        l32, g32, dh32 = RG.mol_oracle(cfg, params, x, h, y, (T,) * B, torch.float32)
        eo = {k: (0.0 if g64[k] is None else rel_to_max(g32[k], g64[k])) for k in g64}
        eo["dh"] = rel_to_max(dh32, dh64)
        return l64, g64, dh64, None, eo
    lengths = ragged_lengths(B, T, O.OracleConfig(*cfg_t).receptive_field) if kind == "ragged" else (T,) * B
    loss, grads, dh, logits = RG.oracle_ragged(cfg_t, params, x, h, t, lengths)
    return loss, grads, dh, logits, None


@contextlib.contextmanager
def poisoned_outputs():
    """Every floating-point buffer the engine allocates for a result (torch.empty / torch.empty_like: loss, logits, dlogits)
    is NaN before the library call that writes it -- a caching allocator hands back the block that held the previous step's
    values, which would hide an element that no launch writes."""
    empty, empty_like = torch.empty, torch.empty_like

    def nan_empty(*a, **kw):
        t = empty(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t

    def nan_empty_like(*a, **kw):
        t = empty_like(*a, **kw)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    with mock.patch.object(torch, "empty", nan_empty), mock.patch.object(torch, "empty_like", nan_empty_like):
        yield


def probe_step(eng, route, data, lpb=0):
    """One step of ``route`` on ``eng``; ``data`` = (x, h, t, y) on the engine's device.  Returns {name: CPU tensor} of everything
    the step hands its caller.  Routes (each calls the engine the way its users do, nets/wavenet.py):
      train    forward_loss -> backward(dh=...) over the loss window          (loss_and_backward(aux_grad=True))
      train0   forward_loss -> backward(dh=..., t_first=0): the backward window starts left of the forward's, so the columns of
               relu(skip) / relu(post1) that the windowed forward left untouched are contracted with dlogits == 0 -- what
               WN_FLAG_WS_FINITE vouches for (finite garbage there contributes exactly nothing)
      full     forward -> loss -> backward(t_first=0)                         (the C ABI's wn_forward / wn_backward pair)
      ragged   forward_loss(lengths=...) -> backward(dh=...)
      frozen   forward_loss -> backward(dh=..., param_grads=False)
      mol      forward -> mol_loss -> backward(dh=...): the unfused loss; the library scans dout for the fp16 scale
      scan     train with a copy of dlogits: the library scans it
      promise  train with dlogits_bound = 8 x the true maximum"""
    x, h, t, y = data
    B, T = x.shape
    rf = eng.receptive_field
    out = {}
    with poisoned_outputs():
        if route == "full":
            logits = eng.forward(x, h)
            out["logits"] = logits
            loss, dl = eng.loss(logits, t)
            tf = 0
        elif route == "mol":
            logits = eng.forward(x, h)
            out["logits"] = logits
            loss, dl = eng.mol_loss(logits, y)
            tf = rf
        elif route == "ragged":
            loss, dl = eng.forward_loss(x, h, t, lengths=ragged_lengths(B, T, rf))
            tf = rf
        else:
            loss, dl = eng.forward_loss(x, h, t)
            tf = 0 if route == "train0" else rf
    out["loss"], out["dlogits"] = loss, dl
    kw = {}
    if route == "scan":
        dl = dl.clone()
    elif route == "promise":
        kw["dlogits_bound"] = float(dl.abs().max()) * 8.0
    eng.grads().fill_(float("nan"))
    if route != "full":
        kw["dh"] = out["dh"] = torch.full(h.shape, float("nan"), dtype=torch.float32, device=h.device)
    if route == "frozen":
        eng.backward(dl, layers_per_bucket=lpb, t_first=tf, param_grads=False, **kw)
    else:
        out["grads"] = eng.backward(dl, layers_per_bucket=lpb, t_first=tf, **kw)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def garbage_(ws, seed=1234):
    """Finite garbage in every word: seeded normal values x 1e3, every 97th word +-3e38, every 89th -0.0 (WN_FLAG_WS_FINITE
    stays set: the caller vouches for finite values, nothing more; route "train0" is the one that reads what the flag leaves).  (One block of 2^20 + 7 words, repeated: a large workspace is filled on its device.)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((1 << 20) + 7, generator=g) * 1e3
    v[::97] = 3e38
    v[48::194] = -3e38
    v[::89] = -0.0
    v = v.to(ws.device)
    n = ws.numel()
    ws.copy_(v.repeat((n + v.numel() - 1) // v.numel())[:n])


def _engine(cfg_t, route, params, lib, device, flags):
    eng = WaveNetEngine(*cfg_t, device=device, library=lib, out_channels=3 * NM if route == "mol" else 0)
    eng.flags = flags
    load_state_into_flat(eng, params)
    return eng


def _on(data, device):
    return tuple(v.to(device) for v in data)


def check_oracle(eng, cfg_t, B, T, route, res, what):
    """The baseline against the oracle: loss within PC.TOL_LOSS, logits within PC.TOL_LOGITS, every gradient tensor and dh
    within PC.TOL_GRAD of its maximum (plan_common.check_grads).  The mixture head: the loss within 1e-4 of its value and the
    gradients within PC.TOL_GRAD plus the error of the fp32 evaluation of the published formula, the gates of
    tests/mol_common.py and tests/ragged_common.check_mol (the formula takes a bin's mass as the difference of two sigmoids one
    part in 1e5 apart)."""
    kind = "mol" if route == "mol" else "ragged" if route == "ragged" else "dense"
    loss_ref, grads_ref, dh_ref, logits_ref, eo = reference(cfg_t, B, T, kind)
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), "%s: %d elements of %s not finite (never written?)" % (what, int((~torch.isfinite(v)).sum()), k)
    if kind == "mol":
        assert abs(float(res["loss"]) - loss_ref) <= 1e-4 * abs(loss_ref), (what, float(res["loss"]), loss_ref)
        grads = flat_to_state(eng, res["grads"], O.param_shapes(_cfg(cfg_t, "mol")))
        for k, ref in grads_ref.items():
            if ref is None or float(ref.abs().max()) == 0.0:
                assert float(grads[k].abs().max()) == 0.0, (what, k)
            else:
                e = rel_to_max(grads[k], ref)
                assert e <= PC.TOL_GRAD + eo[k], "%s: %s grad rel err %g (fp32 formula %g)" % (what, k, e, eo[k])
        e = rel_to_max(res["dh"], dh_ref)
        assert e <= PC.TOL_GRAD + eo["dh"], "%s: dh rel err %g" % (what, e)
        return
    assert abs(float(res["loss"]) - loss_ref) <= PC.TOL_LOSS, (what, float(res["loss"]), loss_ref)
    if "logits" in res:
        e = float((res["logits"].transpose(1, 2) - logits_ref).abs().max())
        assert e <= PC.TOL_LOGITS, "%s: logits max-abs err %g" % (what, e)
    if "grads" in res:
        PL.check_grads(eng, res["grads"], cfg_t, grads_ref, what)
    if "dh" in res and dh_ref is not None:
        e = rel_to_max(res["dh"], dh_ref)
        assert e <= PC.TOL_GRAD, "%s: dh rel err %g" % (what, e)


_BASELINES = {}


def baseline(cfg_t, B, T, route, flags, lib, device):
    """The probe step on a fresh engine (zero-filled workspace of exactly wn_workspace_bytes): asserted bit-identical run to run
    and held to the oracle.  Computed once per (shape, route, flags)."""
    key = (cfg_t, B, T, route, flags, id(lib), str(device))
    if key not in _BASELINES:
        params, x, h, t, y = instance(cfg_t, B, T, route == "mol")
        eng = _engine(cfg_t, route, params, lib, device, flags)
        data = _on((x, h, t, y), device)
        a = probe_step(eng, route, data)
        b = probe_step(eng, route, data)
        for k in a:
            assert torch.equal(a[k], b[k]), "baseline %s differs run to run (route %s, flags %#x)" % (k, route, flags)
        check_oracle(eng, cfg_t, B, T, route, a, "baseline route %s flags %#x" % (route, flags))
        _BASELINES[key] = a
    return _BASELINES[key]


def _install(eng, buf, B, T):
    """``buf`` as the engine's workspace for calls at (B, T): make_ctx accepts ws_bytes >= the need."""
    eng._ws, eng._ws_key = buf, (B, T)


def run_state(cfg_t, B, T, route, flags, state, lib, device, stale_flags=None):
    """The probe step after ``state`` was given to the workspace; returns its results.
      nan          every word NaN and eng.ws_finite = False: the caller vouches for nothing
      garbage      every word finite garbage (garbage_), ws_finite kept True
      stale-data   the same engine first runs the same route on ANOTHER minibatch (another seed, h x 50: stale activations and
                   maxima orders of magnitude away) under another launch plan: layers_per_bucket = 1, WN_FLAG_DW_FLUSH(1)
      stale-shape  one buffer of wn_workspace_bytes of the largest (B, T) of ``companions`` serves a step at (2, 2 T), a step at
                   (1, T / 2) and then the probe step, no re-allocation in between (the regions of one shape overlay other
                   regions of the next)
      stale-arith  the same engine first runs the route on the same minibatch under ``stale_flags``"""
    mol = route == "mol"
    params, x, h, t, y = instance(cfg_t, B, T, mol)
    eng = _engine(cfg_t, route, params, lib, device, flags)
    data = _on((x, h, t, y), device)
    if state == "nan":
        eng.workspace(B, T).fill_(float("nan"))
        eng.ws_finite = False
    elif state == "garbage":
        garbage_(eng.workspace(B, T))
    elif state == "stale-data":
        other = other_batch(cfg_t, B, T, PL.SEED + 77, h_scale=50.0)
        eng.flags = flags | _lib.flag_dw_flush(1)
        probe_step(eng, route, _on(other, device), lpb=1)
        eng.flags = flags
    elif state == "stale-shape":
        comp = companions(cfg_t, B, T)
        need = max(lib.wn_workspace_bytes(ctypes.byref(eng.cfg), b, tt) for b, tt in comp + ((B, T),))
        buf = torch.zeros((need + 3) // 4, dtype=torch.float32, device=device)
        for i, (b, tt) in enumerate(comp):
            other = other_batch(cfg_t, b, tt, PL.SEED + 31 + i)
            _install(eng, buf, b, tt)
            probe_step(eng, route, _on(other, device))
        _install(eng, buf, B, T)
    elif state == "stale-arith":
        eng.flags = stale_flags
        probe_step(eng, route, data)
        eng.flags = flags
    else:
        raise ValueError(state)
    return probe_step(eng, route, data)


def check_workspace_independence(shape, route, arith, state, lib, device, stale_flags=None, cfg_bt=None):
    """Baseline on a fresh zero-filled workspace (twice, oracle gates), then ``torch.equal`` on every tensor the probe step
    returns after the pre-state ``state``.

    One comparison is narrower, by two documented contracts together: route "train0" after "garbage".  WN_FLAG_WS_FINITE
    (include/wavenet_hip.h): in front of the loss window relu(skip) / relu(post1) hold "whatever finite values were there" and a
    backward pass with an earlier window start "contracts them with dlogits == 0: any FINITE value there contributes exactly
    nothing" -- to the VALUE.  WN_FLAG_DW_F16PAIR / WN_FLAG_MM_F16PAIR: an operand outside fp16's range (the +-3e38 words) raises
    the overflow word and "the six-product launch issued behind every fp16 launch" redoes the contraction -- the same gradient in
    the six-product rounding, not the fp16 pair's bits (seen on the MI355X: T1 under the default arithmetic, 5e-8 of values of
    0.14).  There loss and dlogits (the forward never reads those columns) stay bit-identical, and the gradients and dh must be
    finite, meet the oracle's gates themselves and lie within 1e-5 of each tensor's maximum of the baseline -- the bound
    tests/test_gpu_launch_plans.py holds two correct roundings of one gradient to (different launch-group sizes)."""
    cfg_t, B, T = cfg_bt if cfg_bt is not None else SHAPES[shape]
    flags = ARITH[arith]
    if state == "stale-arith" and stale_flags is None:
        stale_flags = STALE_ARITH[arith]
    base = baseline(cfg_t, B, T, route, flags, lib, device)
    got = run_state(cfg_t, B, T, route, flags, state, lib, device, stale_flags)
    assert set(got) == set(base)
    bad = []
    rounding = ("grads", "dh") if (route == "train0" and state == "garbage") else ()
    if rounding:
        params = instance(cfg_t, B, T, False)[0]
        check_oracle(_engine(cfg_t, route, params, lib, device, flags), cfg_t, B, T, route, got, "%s train0 after garbage" % shape)
    for k in sorted(base):
        if k in rounding:
            d = float((got[k] - base[k]).abs().max())
            if not d <= 1e-5 * float(base[k].abs().max()):
                bad.append("%s: %g from the baseline (max |baseline| %g)" % (k, d, float(base[k].abs().max())))
            continue
        if not torch.equal(got[k], base[k]):
            d = (got[k] - base[k]).abs()
            n = int((~(got[k] == base[k])).sum())
            bad.append("%s: %d of %d elements differ, max |diff| %g (max |baseline| %g), first at flat index %d" % (
                k, n, base[k].numel(), float(torch.nan_to_num(d, nan=float("inf")).max()), float(base[k].abs().max()),
                int((~(got[k] == base[k])).reshape(-1).nonzero()[0])))
    assert not bad, "%s route %s arith %s after %s:\n  %s" % (shape, route, arith, state, "\n  ".join(bad))


def check_path(shape, lib, device):
    """Under DEFAULT_FLAGS the training step of a shape launches what the shape is here for."""
    cfg_t, B, T = SHAPES[shape]
    params, x, h, t, y = instance(cfg_t, B, T, False)
    eng = _engine(cfg_t, "train", params, lib, device, DEFAULT_FLAGS)
    if shape == "T1":
        eng.workspace(B, T)
        eng.ws_finite = False   # (the fill launches of the columns in front of the window)
    data = _on((x, h, t, y), device)
    if shape == "T1":   # without WN_FLAG_WS_FINITE the windowed forward itself fills relu(skip), relu(post1) and dlogits in front of t0
        fwd = PC.launch_log(lib, lambda: eng.forward_loss(data[0], data[1], data[2]))
        assert fwd.get("fill_cols") == 3 and fwd.get("fwd_post2_ce") == 1, fwd
    log = PC.launch_log(lib, lambda: probe_step(eng, "train", data))
    need, never = PATH_TAGS[shape]
    for tag in need:
        assert log.get(tag, 0) >= 1, (shape, tag, log)
    for tag in never:
        assert tag not in log, (shape, tag, log)
    return log


PREFILL_TAG = "decode_fill_queues"   # the launch that moves the prefill forward's layer inputs into the dilation queues


def check_decode_prefill(name, lib, device, layered=(False, True)):
    """wn_decode_prefill takes its workspace uninitialised (engine._decode_prefill: torch.empty): with NaN in every word of it,
    tokens and logits are bit-identical to those of a zero-filled one.  (``state`` is documented as zero before step 0 and is
    left alone.)  ``layered``: the decode paths to run (the one-workgroup kernel, the any-size path); each has its own layout of
    the queues the prefill fills."""
    from pytorchwavenetvocoder_amd.nets import WaveNet
    from tests.decode_common import DecodeCase
    g = DecodeCase(name)
    model = WaveNet(*g.cfg.as_tuple(), _library=lib)
    model.load_state_dict(g.params)
    model.to(device)
    x, h = g.x.to(device), g.h.to(device)
    empty = torch.empty
    res = {}
    for fill in (0.0, float("nan")):
        def filled(*a, **kw):
            t = empty(*a, **kw)
            return t.fill_(fill) if t.is_floating_point() else t
        for lay in layered:
            out = {}

            def run():
                with mock.patch.object(torch, "empty", filled):
                    out["r"] = model.engine.decode(x, h, g.n_list, mode="argmax", chunk=7, return_logits=True, layered=lay)
            log = PC.launch_log(lib, run)
            assert log.get(PREFILL_TAG, 0) >= 1, (name, lay, log)   # the prefill ran (parallel prefill, context of >= 2 samples)
            toks, lg = out["r"]
            res[(fill == 0.0, lay)] = ([v.cpu().clone() for v in toks], [v.cpu().clone() for v in lg])
    for lay in layered:
        (t0, l0), (t1, l1) = res[(True, lay)], res[(False, lay)]
        for b in range(len(g.n_list)):
            assert (t0[b].numpy() == g.fast[b]).all(), (name, lay, b)
            assert torch.equal(t0[b], t1[b]), (name, lay, b)
            assert torch.equal(l0[b], l1[b]), (name, lay, b)
