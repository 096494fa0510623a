# -*- coding: utf-8 -*-
"""The exponential moving average of the weights inside the Adam launch (wn_adam_step_ema, wn_adam_step_guarded_ema, wn_op_swap,
FusedAdam(ema_decay=, ema_warmup=)): the cases tests/test_emu_ema.py runs on the host-compiled kernels and tests/test_gpu_ema.py on
the MI355X.

The reference of every numeric check is numpy in fp64 or torch on the CPU -- never the code under test.

Tolerances
  one step  |e - (e0 + (1 - d_t)(p - e0))| <= 4 * 2^-24 * max(|e0|, |p|) against fp64: the kernel rounds w = (float)(1 - d_t) once
            (2^-24 relative of an increment of at most 2 max), the subtraction p - e0 once (2^-24 of at most 2 max) and the fused
            multiply-add once (2^-24 of at most max): under 4 units together.
  k steps   4 * k * 2^-24 * M, M the largest magnitude among e0 and every p: the recurrence is a contraction (an error already in
            e is multiplied by d_t <= 1), so the per-step budgets add at most.
  module    the weights stay inside the project's after-Adam gate TOL_ADAM_REL_LR * lr (tests/parity_common.py); the average is a
            convex combination of iterates that are each inside it, plus the k-step budget above.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import _ptr, _stream_handle
from pytorchwavenetvocoder_amd.nets import WaveNet
from pytorchwavenetvocoder_amd.optim import FusedAdam
from tests import clip_common as CC
from tests import parity_common as PC
from tests.golden_util import GoldenCase

U24 = 2.0 ** -24
TINY = CC.TINY
SWAP_SIZES = [1, 3, 4, 5, 255, 256, 257, 4097, 512 * 256 * 4 + 4099]   # the last: past one sweep of the swap's grid, scalar tail
SWAP_MISALIGN = [(0, 0), (1, 1), (0, 1)]                                 # floats behind a 16-byte boundary: (a, b)
N, LO, HI = 5003, 1021, 1290
# (ema_decay, warm-up, t): the warm-up's crossover (1 + t) / (10 + t) = 0.5 sits exactly at t = 8, t = 9 is capped
RECURRENCE_CASES = [(0.5, True, 1), (0.5, True, 7), (0.5, True, 8), (0.5, True, 9), (0.999, False, 3), (0.9999, True, 10 ** 6)]
# bit patterns a float copy might mangle: quiet and signalling NaNs with payloads, both infinities, a denormal, -0
SPECIAL_BITS = [0x7fc12345, 0xffc00001, 0x7f800001, 0xff8abcde, 0x7f800000, 0xff800000, 0x00000001, 0x80000000]


def decay_at(ema_decay, warmup, t):
    return min(ema_decay, (1.0 + t) / (10.0 + t)) if warmup else ema_decay


def ema_ref(e, p, ema_decay, warmup, t):
    """One step of the recurrence in fp64."""
    e, p = np.asarray(e, np.float64), np.asarray(p, np.float64)
    return e + (1.0 - decay_at(ema_decay, warmup, t)) * (p - e)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def adam_ema(lib, dev, p, g, m, v, e, step, lr, wd, lo, hi, ema_decay, warmup, betas=(0.9, 0.999), eps=1e-8):
    lib.check(lib.wn_adam_step_ema(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), p.numel(), int(step), float(lr), float(betas[0]),
                                   float(betas[1]), float(eps), float(wd), lo, hi, float(ema_decay), int(warmup),
                                   _stream_handle(torch.device(dev))), "wn_adam_step_ema")


def adam_plain(lib, dev, p, g, m, v, step, lr, wd, lo, hi, betas=(0.9, 0.999), eps=1e-8):
    lib.check(lib.wn_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), int(step), float(lr), float(betas[0]),
                               float(betas[1]), float(eps), float(wd), lo, hi, _stream_handle(torch.device(dev))), "wn_adam_step")


def adam_guarded_ema(lib, dev, p, g, m, v, e, state, wd, lo, hi, ema_decay, warmup, eps=1e-8):
    lib.check(lib.wn_adam_step_guarded_ema(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), p.numel(), float(eps), float(wd), lo, hi,
                                           _ptr(state), float(ema_decay), int(warmup), _stream_handle(torch.device(dev))),
              "wn_adam_step_guarded_ema")


# ---- 1. swap, op level ---------------------------------------------------------------------------------------------------------
def _swap_buffer(n, misalign, dev, seed):
    """(whole allocation, view of n elements) of int32 bit patterns: the view starts `misalign` floats behind a 16-byte boundary
    and has at least one guard element on each side."""
    rs = np.random.RandomState(seed + n)
    raw = rs.randint(-2 ** 31, 2 ** 31, size=n + 12, dtype=np.int64).astype(np.int32)
    for k, b in enumerate(SPECIAL_BITS):
        raw[4 + (k * 37) % (n + 4)] = np.array(b, np.uint32).view(np.int32)
    whole = torch.from_numpy(raw).to(dev)
    assert whole.data_ptr() % 16 == 0
    view = whole[4 + misalign:4 + misalign + n]
    assert view.data_ptr() % 16 == 4 * misalign
    return whole, view


def check_swap(lib, dev, n, misalign):
    st = _stream_handle(torch.device(dev))
    wa, a = _swap_buffer(n, misalign[0], dev, 1)
    wb, b = _swap_buffer(n, misalign[1], dev, 2)
    wa0, wb0 = wa.cpu().clone(), wb.cpu().clone()
    a0, b0 = a.cpu().clone(), b.cpu().clone()
    lib.check(lib.wn_op_swap(a.data_ptr(), b.data_ptr(), n, st), "wn_op_swap")
    assert torch.equal(a.cpu(), b0) and torch.equal(b.cpu(), a0), (n, misalign)
    for whole, whole0, mis in ((wa, wa0, misalign[0]), (wb, wb0, misalign[1])):   # everything around the views is untouched
        got = whole.cpu()
        assert torch.equal(got[:4 + mis], whole0[:4 + mis]) and torch.equal(got[4 + mis + n:], whole0[4 + mis + n:]), (n, misalign)
    lib.check(lib.wn_op_swap(a.data_ptr(), b.data_ptr(), n, st), "wn_op_swap")
    assert torch.equal(wa.cpu(), wa0) and torch.equal(wb.cpu(), wb0), (n, misalign)


def check_swap_errors(lib, dev):
    st = _stream_handle(torch.device(dev))
    buf = torch.zeros(64, dtype=torch.float32, device=dev)
    p = buf.data_ptr()
    for a, b, n in ((p, p, 8), (p, p + 4 * 7, 8), (p + 4 * 7, p, 8)):
        assert lib.wn_op_swap(a, b, n, st) != 0
        assert b"overlap" in lib.wn_last_error()
    assert lib.wn_op_swap(p, p + 4 * 8, 8, st) == 0        # adjacent ranges are fine
    assert lib.wn_op_swap(None, p, 8, st) != 0 and lib.wn_op_swap(p, p + 32, 0, st) != 0
    assert not bool(buf.cpu().any())


# ---- 2. the recurrence in isolation (lr = 0) ---------------------------------------------------------------------------------
def _random_buffers(dev, seed=11):
    rs = np.random.RandomState(seed)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))   # noqa: E731
    p0, e0 = f32(rs.standard_normal(N)), f32(rs.standard_normal(N))
    m0, v0 = f32(0.1 * rs.standard_normal(N)), f32(0.01 * rs.uniform(size=N) + 1e-4)
    return rs, f32, p0, e0, m0, v0


def check_recurrence(lib, dev, ema_decay, warmup, t):
    rs, f32, p0, e0, m0, v0 = _random_buffers(dev)
    g0 = f32(rs.standard_normal(N))
    # unguarded: the host forms w from step = t
    p, e, m, v, g = (x.clone().to(dev) for x in (p0, e0, m0, v0, g0))
    adam_ema(lib, dev, p, g, m, v, e, t, 0.0, 0.0, LO, HI, ema_decay, warmup)
    # guarded: every thread forms w from the state block's count, t - 1 before the norm call
    p2, e2, m2, v2 = (x.clone().to(dev) for x in (p0, e0, m0, v0))
    state = CC.new_state(dev)
    state[3] = t - 1
    CC.run_norm(lib, dev, g, LO, HI, guard=True, state=state, lr=0.0)
    adam_guarded_ema(lib, dev, p2, g, m2, v2, e2, state, 0.0, LO, HI, ema_decay, warmup)
    st = CC.read_state(state)
    assert st.apply == 1 and st.steps_applied == t
    for pp, ee in ((p, e), (p2, e2)):
        assert same_bits(pp, p0)                                   # lr = 0: the weights do not move, on either path
        assert same_bits(ee[LO:HI], e0[LO:HI])                     # the skip range is never written
    want = ema_ref(e0.numpy(), p0.numpy(), ema_decay, warmup, t)
    tol = 4.0 * U24 * np.maximum(np.abs(f64(e0)), np.abs(f64(p0)))
    err = np.abs(f64(e) - want)
    live = np.ones(N, bool)
    live[LO:HI] = False
    print("ema_decay %g warm-up %d t %d: max err / tol = %.3f" % (ema_decay, warmup, t, float((err[live] / tol[live]).max())))
    assert bool((err[live] <= tol[live]).all())
    assert not same_bits(e, e0)                                    # (the case moves the average at all)
    assert same_bits(e, e2), "host-formed and device-formed averaging weight differ"


# ---- 3. EMA on changes nothing else ----------------------------------------------------------------------------------------------
def check_ema_changes_nothing_else(lib, dev, weight_decay, guarded):
    lr, k, ema_decay, warmup = 1e-3, 3, 0.999, True
    rs, f32, p0, e0, m0, v0 = _random_buffers(dev, seed=13)
    p, m, v, e = (x.clone().to(dev) for x in (p0, m0, v0, e0))
    q, qm, qv = (x.clone().to(dev) for x in (p0, m0, v0))          # twin buffers: the plain launches
    state, qstate, scratch = CC.new_state(dev), CC.new_state(dev), CC.new_scratch(lib, N, dev)
    ps = []
    for step in range(1, k + 1):
        g0 = f32(rs.standard_normal(N) * step)
        g = g0.to(dev)
        if guarded:
            max_norm = 0.5 * CC.ref_norm(g0, LO, HI)               # the clip is active
            CC.run_norm(lib, dev, g, LO, HI, max_norm=max_norm, guard=True, state=state, scratch=scratch, lr=lr)
            adam_guarded_ema(lib, dev, p, g, m, v, e, state, weight_decay, LO, HI, ema_decay, warmup)
            CC.run_norm(lib, dev, g, LO, HI, max_norm=max_norm, guard=True, state=qstate, scratch=scratch, lr=lr)
            CC.run_adam(lib, dev, q, g, qm, qv, qstate, wd=weight_decay, lo=LO, hi=HI)
            assert CC.read_state(state).clip_coef < 1.0 and CC.read_state(state).steps_applied == step
        else:
            adam_ema(lib, dev, p, g, m, v, e, step, lr, weight_decay, LO, HI, ema_decay, warmup)
            adam_plain(lib, dev, q, g, qm, qv, step, lr, weight_decay, LO, HI)
        for ours, plain in ((p, q), (m, qm), (v, qv)):
            assert same_bits(ours, plain), step
        assert not same_bits(p, p0)
        ps.append(f64(p))
    want, big = f64(e0), float(np.abs(f64(e0)).max())
    for step, pk in enumerate(ps, 1):
        want = ema_ref(want, pk, ema_decay, warmup, step)
        big = max(big, float(np.abs(pk).max()))
    live = np.ones(N, bool)
    live[LO:HI] = False
    err = float(np.abs(f64(e) - want)[live].max())
    print("wd %g guarded %d: ema err %.3e, bound %.3e" % (weight_decay, guarded, err, 4.0 * k * U24 * big))
    assert err <= 4.0 * k * U24 * big
    assert same_bits(e[LO:HI], e0[LO:HI])


# ---- 4. module level against torch -------------------------------------------------------------------------------------------
def check_module_ema_training(name, lib, dev):
    g = GoldenCase(name)
    ema_decay = 0.5
    model = WaveNet(*g.cfg.as_tuple(), _library=lib)
    model.load_state_dict(g.params)
    model.to(dev)
    opt = FusedAdam(model, lr=g.adam_lr, weight_decay=g.wd, ema_decay=ema_decay)
    ref = {k: torch.nn.Parameter(v.clone()) for k, v in g.params.items()}
    ropt = torch.optim.Adam(list(ref.values()), lr=g.adam_lr, weight_decay=g.wd)
    rema = {k: f64(v) for k, v in g.params.items()}
    big = max(float(np.abs(v).max()) for v in rema.values())
    x, h, t = g.x.to(dev), g.h.to(dev), g.t.to(dev)
    for step in range(1, g.adam_steps + 1):
        _, _, og = O.train_step(g.cfg, {k: v.detach() for k, v in ref.items()}, None, g.x, g.h, g.t)
        for k, p in ref.items():
            p.grad = None if og[k] is None else og[k].clone()
        ropt.step()
        for k, p in ref.items():
            rema[k] = ema_ref(rema[k], f64(p), ema_decay, True, step)
            big = max(big, float(p.detach().abs().max()))
        model.loss_and_backward(x, h, t)
        opt.step()
    gate = PC.TOL_ADAM_REL_LR * g.adam_lr
    ema = opt.ema_state_dict()
    assert list(ema.keys()) == list(model.state_dict().keys())
    for k, v in model.state_dict().items():
        err = float((v.cpu() - ref[k].detach()).abs().max())
        assert err <= gate, "%s: |dw| err %g (lr %g)" % (k, err, g.adam_lr)
        err = float(np.abs(f64(ema[k]) - rema[k]).max())
        assert err <= gate + 4.0 * g.adam_steps * U24 * big, "%s: ema err %g" % (k, err)
    moved = max(float((ema[k].cpu() - v.cpu()).abs().max()) for k, v in model.state_dict().items())
    assert moved > 0.0, "the average equals the weights: the case shows nothing"


# ---- 5. guard --------------------------------------------------------------------------------------------------------------------
def _slice_of(model, key):
    for (k, _), (off, n, shape, dead) in zip(model.named_parameters(), model._param_slices):
        if k == key:
            assert not dead
            return slice(off, off + n)
    raise KeyError(key)


def check_guard(lib, dev):
    lr, ema_decay = 1e-3, 0.5
    model, x, h, t = CC._tiny_model(lib, dev)
    eng = model.engine
    lo, hi = eng.dead_range
    opt = FusedAdam(model, lr=lr, skip_nonfinite=True, ema_decay=ema_decay)
    e0 = opt.ema.cpu().clone()
    assert same_bits(e0, eng.flat_params)                          # the shadow starts as a copy of the weights
    live = np.ones(eng.n_params, bool)
    live[lo:hi] = False

    def one_step_check(e_before, t_applied):
        want = ema_ref(f64(e_before), f64(eng.flat_params), ema_decay, True, t_applied)
        tol = 4.0 * U24 * np.maximum(np.abs(f64(e_before)), np.abs(f64(eng.flat_params)))
        err = np.abs(f64(opt.ema) - want)
        assert bool((err[live] <= tol[live]).all()), t_applied
        assert same_bits(opt.ema[lo:hi], e_before[lo:hi])

    model.loss_and_backward(x, h, t)
    opt.step()                                                     # applied: t = 1
    one_step_check(e0, 1)
    e1 = opt.ema.cpu().clone()
    assert not same_bits(e1, e0) and not same_bits(e1, eng.flat_params)
    model.loss_and_backward(x, h, t)
    eng.grads()[CC._live_index(eng)] = float("nan")
    p1 = eng.flat_params.cpu().clone()
    opt.step()                                                     # skipped: nothing moves, t stays
    assert same_bits(opt.ema, e1) and same_bits(eng.flat_params, p1)
    assert (opt.steps_applied(), opt.steps_skipped()) == (1, 1)
    model.loss_and_backward(x, h, t)
    opt.step()                                                     # applied: t = 2, d_2 = min(0.5, 3 / 12)
    assert (opt.steps_applied(), opt.steps_skipped()) == (2, 1)
    assert decay_at(ema_decay, True, 2) == 0.25
    one_step_check(e1, 2)
    # a live parameter without a gradient keeps its slice of the average, as it keeps its weights and moments
    e2 = opt.ema.cpu().clone()
    model.loss_and_backward(x, h, t)
    sl = _slice_of(model, "conv_post_1.weight")
    dict(model.named_parameters())["conv_post_1.weight"].grad = None
    p2 = eng.flat_params.cpu().clone()
    opt.step()
    assert same_bits(opt.ema[sl], e2[sl]) and same_bits(eng.flat_params[sl], p2[sl])
    assert not same_bits(opt.ema, e2) and opt.steps_applied() == 3


# ---- 6. launches -------------------------------------------------------------------------------------------------------------------
def check_launches(lib, dev):
    for kw, want in ((dict(ema_decay=0.999), {"adam_ema": 1}),
                     (dict(ema_decay=0.999, max_grad_norm=0.05, skip_nonfinite=True),
                      {"grad_sumsq": 1, "grad_norm_finalize": 1, "adam_guarded_ema": 1}),
                     (dict(), {"adam": 1}),
                     (dict(ema_decay=None, skip_nonfinite=True), {"grad_sumsq": 1, "grad_norm_finalize": 1, "adam_guarded": 1})):
        model, x, h, t = CC._tiny_model(lib, dev)
        opt = FusedAdam(model, lr=1e-3, **kw)
        model.loss_and_backward(x, h, t)
        assert (opt.ema is None) == (kw.get("ema_decay") is None)
        for _ in range(2):
            log = PC.launch_log(lib, opt.step)
            assert log == want, (kw, log)
    model, x, h, t = CC._tiny_model(lib, dev)
    opt = FusedAdam(model, lr=1e-3, ema_decay=0.9)
    opt.ema

    def block():
        with opt.ema_weights():
            pass
    assert PC.launch_log(lib, block) == {"swap": 2}
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            FusedAdam(model, ema_decay=bad)


# ---- 7. ema_weights() --------------------------------------------------------------------------------------------------------------
def check_ema_weights(lib, dev):
    model, x, h, t = CC._tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, lr=1e-2, ema_decay=0.9)
    for _ in range(2):
        model.loss_and_backward(x, h, t)
        opt.step()
    p0, e0 = eng.flat_params.cpu().clone(), opt.ema.cpu().clone()
    assert not same_bits(p0, e0)
    sd = opt.ema_state_dict()
    other = WaveNet(*TINY, _library=lib)
    other.load_state_dict(sd)
    other.to(dev)
    want_nll, _ = other.evaluate(x, h, t)
    plain_nll, _ = model.evaluate(x, h, t)
    v_before = eng.params_version()
    with opt.ema_weights() as inside:
        assert inside is model
        v_inside = eng.params_version()
        for (k, a), (k2, b) in zip(model.state_dict().items(), opt.ema_state_dict().items()):
            assert k == k2 and same_bits(a, b) and same_bits(a, sd[k]), k
        got_nll, _ = model.evaluate(x, h, t)
        assert same_bits(got_nll, want_nll)
        assert not same_bits(got_nll, plain_nll)                   # (the two weight sets score differently: the check means something)
        with pytest.raises(RuntimeError):
            opt.step()
        with pytest.raises(RuntimeError):
            with opt.ema_weights():
                pass
    v_after = eng.params_version()
    assert v_inside != v_before and v_after != v_inside and v_after != v_before
    assert same_bits(eng.flat_params, p0) and same_bits(opt.ema, e0)
    assert same_bits(model.evaluate(x, h, t)[0], plain_nll)       # the packed weight sets followed the weights back
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("from the body")
    assert same_bits(eng.flat_params, p0) and same_bits(opt.ema, e0)
    model.loss_and_backward(x, h, t)
    opt.step()                                                     # usable again after the block
    off = FusedAdam(model, lr=1e-2)
    for call in (off.ema_state_dict, lambda: off.load_ema_state_dict(sd), lambda: off.ema_weights().__enter__()):
        with pytest.raises(RuntimeError):
            call()


# ---- 8. checkpoint ---------------------------------------------------------------------------------------------------------------
def check_checkpoint(lib, dev, tmp_path):
    kw = dict(lr=1e-3, weight_decay=1e-2, ema_decay=0.99)
    model, x, h, t = CC._tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, **kw)
    model.loss_and_backward(x, h, t)
    g0 = eng.grads().clone()
    for step in range(3):
        eng.grads().copy_(g0 * (1.0 + step))
        opt.step()
    esd, msd, osd = opt.ema_state_dict(), model.state_dict(), opt.state_dict()
    assert list(esd.keys()) == list(msd.keys())
    for k, v in msd.items():
        assert esd[k].shape == v.shape and esd[k].dtype == v.dtype and esd[k].data_ptr() != v.data_ptr(), k
    assert set(osd.keys()) == {"state", "param_groups"}
    assert all(set(s.keys()) == {"step", "exp_avg", "exp_avg_sq"} for s in osd["state"].values())
    path = str(tmp_path / "ck.pkl")
    torch.save({"model": msd, "optimizer": osd, "ema": esd}, path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    resumed = WaveNet(*TINY, _library=lib)
    resumed.load_state_dict(ck["model"])
    ropt = FusedAdam(resumed, **kw)
    ropt.load_state_dict(ck["optimizer"])
    ropt.load_ema_state_dict(ck["ema"])                             # before the move: the average follows the model
    resumed.to(dev)
    assert same_bits(ropt.ema, opt.ema) and ropt.ema.device == resumed.engine.flat_params.device
    resumed.loss_and_backward(x, h, t)   # (gives the resumed model's parameters their gradient views)
    for mdl, o in ((model, opt), (resumed, ropt)):
        mdl.engine.grads().copy_(g0 * 0.5)
        o.step()
    assert same_bits(eng.flat_params, resumed.engine.flat_params)
    for a, b in zip(opt._buffers(), ropt._buffers()):
        assert same_bits(a, b)
    assert same_bits(opt.ema, ropt.ema) and not same_bits(opt.ema, eng.flat_params)
    with pytest.raises(KeyError):
        ropt.load_ema_state_dict({k: v for k, v in list(esd.items())[1:]})


# ---- argument errors of the two entry points -------------------------------------------------------------------------------------
def check_api_errors(lib, dev):
    n = 64
    p, g, m, v, e = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(5))
    v.fill_(1.0)
    state = CC.new_state(dev)
    st = _stream_handle(torch.device(dev))
    P = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def plain(ema, decay):
        return lib.wn_adam_step_ema(P(p), P(g), P(m), P(v), ema, n, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0, decay, 1, st)

    def guarded(ema, decay):
        return lib.wn_adam_step_guarded_ema(P(p), P(g), P(m), P(v), ema, n, 1e-8, 0.0, 0, 0, P(state), decay, 1, st)
    for call in (plain, guarded):
        for ema, decay, word in ((None, 0.5, b"NULL"), (P(e), 1.0, b"[0, 1)"), (P(e), -0.01, b"[0, 1)"), (P(e), float("nan"), b"[0, 1)"),
                                 (P(p), 0.5, b"overlaps"), (P(p) + 4 * (n - 1), 0.5, b"overlaps")):
            assert call(ema, decay) != 0
            assert word in lib.wn_last_error(), (word, lib.wn_last_error())
    for t in (p, m, e):
        assert not bool(t.cpu().any())
    assert ctypes.sizeof(_lib.WnOptState) == 56
