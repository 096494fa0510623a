# -*- coding: utf-8 -*-
"""Global-norm clipping and the non-finite-step guard (wn_grad_norm, wn_adam_step_guarded, FusedAdam(max_grad_norm=,
skip_nonfinite=)): the cases tests/test_emu_clip.py runs on the host-compiled kernels and tests/test_gpu_clip.py on the MI355X.

The reference of every numeric check is numpy in fp64 or torch on the CPU (``torch.nn.utils.clip_grad_norm_`` followed by
``torch.optim.Adam`` on the same numbers) -- never the code under test.

Tolerances
  norm      |norm - ref| <= 4 * 2^-24 * ref against the fp64 norm: the kernel accumulates exact squares in double (error about
            n * 2^-53 relative, far below) and rounds ONCE, in the cast of the root to float (2^-24 relative).
  weights   |p - p_torch| <= TOL_ADAM_REL_LR * lr (tests/parity_common.py, the project's after-Adam gate).
  moments   1e-4 of the tensor's maximum.  The kernel (like the unguarded one) takes beta as an fp32 number and forms 1 - beta in
            fp32; torch forms it in double.  fp32 beta2 = 0.999 is off by up to 2^-25, which is 2^-25 / (1 - beta2) = 3e-5 of the
            weight (1 - beta2) every new g^2 enters exp_avg_sq with -- per step, so 9e-5 over the three steps of the op-level
            case (exp_avg: 3e-7 per step).  The fp32 roundings of the update itself and of the clip coefficient (rounded once
            from double here, computed in fp32 by torch) are a few 2^-23.  Far inside the 1e-2 relative of the weight gate.
"""
import ctypes

import numpy as np
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import WaveNetEngine, _ptr, _stream_handle
from pytorchwavenetvocoder_amd.nets import WaveNet
from pytorchwavenetvocoder_amd.optim import FusedAdam
from tests import parity_common as PC
from tests.golden_util import GoldenCase

NORM_TOL = 4.0 * 2.0 ** -24
MOMENT_TOL = 1e-4
# One sweep of the norm's grid is 512 blocks x 256 threads x 4 floats; N_BIG needs a second, partial sweep (the test asserts that
# the grid has stopped growing there), with a scalar tail.
SWEEP = 512 * 256 * 4
N_BIG = SWEEP + 4099
SIZES = [1, 3, 4, 5, 7, 255, 256, 257, 1023, 4097, N_BIG]
BLOCK_FLOATS = 256 * 4   # floats of one block in one sweep
NEW_TAGS = ("grad_sumsq", "grad_norm_finalize", "adam_guarded")
TINY = (32, 6, 8, 12, 3, 2, 2, 4)


def _not_multiple_of_4(i, n):
    while i % 4 == 0 and i < n:
        i += 1
    return i


def skip_ranges(n):
    """Named skip ranges that exist for a buffer of n elements: empty; at the start; at the end; in the middle with both bounds
    no multiples of 4 (n >= 3); straddling the boundary of two blocks' shares (n > 1030) and of two sweeps (n > SWEEP)."""
    third = max(1, n // 3)
    out = [("empty", 0, 0), ("start", 0, third), ("end", n - third, n)]
    lo, hi = _not_multiple_of_4(third, n), _not_multiple_of_4(max(2 * n // 3, third + 1), n)
    if 0 < lo < hi < n and lo % 4 and hi % 4:
        out.append(("middle_unaligned", lo, hi))
    if n > BLOCK_FLOATS + 6:
        out.append(("block_boundary", BLOCK_FLOATS - 5, BLOCK_FLOATS + 6))
    if n > SWEEP + 5:
        out.append(("sweep_boundary", SWEEP - 3, SWEEP + 5))
    return out


def ref_norm(g, lo, hi):
    a = np.asarray(g.detach().cpu().numpy(), dtype=np.float64)
    return float(np.sqrt(np.sum(a[:lo] ** 2) + np.sum(a[hi:] ** 2)))


def new_state(dev):
    return torch.zeros(ctypes.sizeof(_lib.WnOptState) // 8, dtype=torch.int64, device=dev)


def new_scratch(lib, n, dev):
    return torch.empty(int(lib.wn_grad_norm_scratch_floats(n)), dtype=torch.float32, device=dev)


def read_state(state):
    s = _lib.WnOptState.from_buffer_copy(state.cpu().numpy().tobytes())
    return s


def state_bits(state):
    """The words of a state block that a call writes from scratch (everything except the two counters), as integers."""
    w = state.cpu().clone()
    w[3] = 0
    w[4] = 0
    return w.tolist()


def poison(state, scratch):
    """NaN bit patterns in the scratch and in every non-counter word of the state."""
    scratch.fill_(float("nan"))
    keep = state[3:5].clone()
    state.view(torch.float32).fill_(float("nan"))
    state[3:5] = keep


def run_norm(lib, dev, g, lo=0, hi=0, max_norm=0.0, guard=False, state=None, scratch=None, lr=1e-3, betas=(0.9, 0.999)):
    state = new_state(dev) if state is None else state
    scratch = new_scratch(lib, g.numel(), dev) if scratch is None else scratch
    lib.check(lib.wn_grad_norm(_ptr(g), g.numel(), lo, hi, float(max_norm), int(guard), float(lr), float(betas[0]), float(betas[1]),
                               _ptr(scratch), _ptr(state), _stream_handle(torch.device(dev))), "wn_grad_norm")
    return state


def run_adam(lib, dev, p, g, m, v, state, eps=1e-8, wd=0.0, lo=0, hi=0):
    lib.check(lib.wn_adam_step_guarded(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), float(eps), float(wd), lo, hi, _ptr(state),
                                       _stream_handle(torch.device(dev))), "wn_adam_step_guarded")


def buffer(n, misalign, dev, seed=0):
    """n standard-normal floats whose base pointer is 16-byte aligned (misalign 0) or one float behind such an address."""
    base = torch.from_numpy(np.random.RandomState(seed + n).standard_normal(n + 4).astype(np.float32)).to(dev)
    assert base.data_ptr() % 16 == 0
    g = base[misalign:misalign + n]
    assert g.data_ptr() % 16 == 4 * misalign
    return g


# ---- 1. the norm, op level -------------------------------------------------------------------------------------------------
def check_norm(lib, dev, n, misalign):
    g = buffer(n, misalign, dev)
    if n == N_BIG:
        assert lib.wn_grad_norm_scratch_floats(n) == lib.wn_grad_norm_scratch_floats(4 * n)   # the grid no longer grows: a second sweep
    other = buffer(777, 0, dev, seed=5)
    ranges = skip_ranges(n)
    for name, lo, hi in ranges:
        ref = ref_norm(g, lo, hi)
        st = read_state(run_norm(lib, dev, g, lo, hi))
        assert abs(st.total_norm - ref) <= NORM_TOL * ref, (n, misalign, name, st.total_norm, ref)
        assert abs(st.sumsq - ref * ref) <= 1e-12 * ref * ref and st.clip_coef == 1.0 and st.apply == 1
    # bit-level checks (on every range for the small sizes, on the one that cuts quads across two sweeps for the large one)
    for name, lo, hi in (ranges if n != N_BIG else ranges[-1:]):
        first = state_bits(run_norm(lib, dev, g, lo, hi, max_norm=0.25))
        assert state_bits(run_norm(lib, dev, g, lo, hi, max_norm=0.25)) == first, (n, misalign, name, "two calls")
        state, scratch = new_state(dev), torch.empty(max(int(lib.wn_grad_norm_scratch_floats(n)), int(lib.wn_grad_norm_scratch_floats(777))),
                                                     dtype=torch.float32, device=dev)
        poison(state, scratch)
        assert state_bits(run_norm(lib, dev, g, lo, hi, max_norm=0.25, state=state, scratch=scratch)) == first, (n, misalign, name, "NaN")
        run_norm(lib, dev, other, 3, 50, max_norm=7.0, guard=True, state=state, scratch=scratch, lr=0.5, betas=(0.5, 0.7))
        assert read_state(state).steps_applied == 2   # the counters ARE state (lr / bc1 and sqrt(bc2) follow the applied count) ...
        state[3:5] = 0                                 # ... so the compared call starts from the count the first one started from
        assert state_bits(run_norm(lib, dev, g, lo, hi, max_norm=0.25, state=state, scratch=scratch)) == first, (n, misalign, name, "stale")


# ---- 2. range --------------------------------------------------------------------------------------------------------------
def check_range(lib, dev):
    n = 1001
    a = np.where(np.arange(n) % 2 == 0, 1e30, 1e-30).astype(np.float32)
    a[::3] *= -1
    st = read_state(run_norm(lib, dev, torch.from_numpy(a).to(dev), guard=True))
    ref = float(np.sqrt(np.sum(a.astype(np.float64) ** 2)))
    assert st.apply == 1 and st.steps_skipped == 0 and abs(st.total_norm - ref) <= NORM_TOL * ref
    a = np.full(n, 1e-30, np.float32)
    st = read_state(run_norm(lib, dev, torch.from_numpy(a).to(dev), guard=True))
    ref = float(np.sqrt(np.sum(a.astype(np.float64) ** 2)))
    assert st.apply == 1 and st.total_norm > 0.0 and abs(st.total_norm - ref) <= NORM_TOL * ref
    # finite elements at the edge of fp32: the sum of squares is finite in double, so the step is never called non-finite (the
    # norm itself no longer fits a float and is reported as inf; the double sum holds the value)
    a = np.array([3e38, -3e38, 3e38, -3e38, 3e38, 1.0, -3e38], np.float32)
    st = read_state(run_norm(lib, dev, torch.from_numpy(a).to(dev), guard=True, max_norm=1.0))
    ref2 = float(np.sum(a.astype(np.float64) ** 2))
    assert st.apply == 1 and st.steps_skipped == 0 and abs(st.sumsq - ref2) <= 1e-12 * ref2
    assert abs(st.clip_coef - 1.0 / np.sqrt(ref2)) <= NORM_TOL / np.sqrt(ref2)


# ---- 3. non-finite detection -------------------------------------------------------------------------------------------------
def check_nonfinite(lib, dev, misalign):
    n, lo, hi = 4097, 1021, 2055   # skip bounds that are no multiples of 4, one block boundary inside
    for bad in (float("nan"), float("inf"), -float("inf")):
        for idx in (0, n - 1, lo - 1, hi):
            g = buffer(n, misalign, dev)
            g[idx] = bad
            st = read_state(run_norm(lib, dev, g, lo, hi, guard=True, max_norm=1.0))
            assert st.apply == 0 and st.steps_skipped == 1 and st.steps_applied == 0, (bad, idx)
            assert st.lr_over_bc1 == 0.0 and st.sqrt_bc2 == 0.0
            st = read_state(run_norm(lib, dev, g, lo, hi, guard=False))   # guard off: the step applies
            assert st.apply == 1 and st.steps_skipped == 0 and st.steps_applied == 1 and st.clip_coef == 1.0
            assert not np.isfinite(st.total_norm)
        for idx in (lo, hi - 1, (lo + hi) // 2):
            g = buffer(n, misalign, dev)
            ref = ref_norm(g, lo, hi)
            g[idx] = bad
            st = read_state(run_norm(lib, dev, g, lo, hi, guard=True))
            assert st.apply == 1 and st.steps_skipped == 0 and abs(st.total_norm - ref) <= NORM_TOL * ref, (bad, idx)


# ---- 4. clipped step against torch, op level -----------------------------------------------------------------------------------
def check_clipped_step(lib, dev, weight_decay, factor):
    """max_norm = factor * ||g|| per step (0.5: clip active, 2: inactive), three steps with fresh gradients, random p / m / v."""
    n, lo, hi, lr = 5003, 1021, 1290, 1e-3
    rs = np.random.RandomState(11)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))   # noqa: E731
    p0, m0, v0 = f32(rs.standard_normal(n)), f32(0.1 * rs.standard_normal(n)), f32(0.01 * rs.uniform(size=n))
    keep = torch.cat([torch.arange(0, lo), torch.arange(hi, n)])
    q = torch.nn.Parameter(p0[keep].clone())
    ropt = torch.optim.Adam([q], lr=lr, weight_decay=weight_decay)
    ropt.state[q] = {"step": torch.tensor(0.0), "exp_avg": m0[keep].clone(), "exp_avg_sq": v0[keep].clone()}
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    state, scratch = new_state(dev), new_scratch(lib, n, dev)
    for step in range(3):
        g0 = f32(rs.standard_normal(n) * (1.0 + step))
        norm64 = ref_norm(g0, lo, hi)
        max_norm = factor * norm64
        q.grad = g0[keep].clone()
        tnorm = float(torch.nn.utils.clip_grad_norm_([q], max_norm))
        ropt.step()
        g = g0.to(dev)
        run_norm(lib, dev, g, lo, hi, max_norm=max_norm, guard=True, state=state, scratch=scratch, lr=lr)
        run_adam(lib, dev, p, g, m, v, state, wd=weight_decay, lo=lo, hi=hi)
        st = read_state(state)
        assert st.apply == 1 and st.steps_applied == step + 1
        assert (st.clip_coef < 1.0) == (factor < 1.0)
        assert abs(st.total_norm - norm64) <= NORM_TOL * norm64 and abs(st.total_norm - tnorm) <= NORM_TOL * norm64
        assert torch.equal(g.cpu(), g0)   # the gradient buffer keeps its unclipped values
        rst = ropt.state[q]
        assert float((p.cpu()[keep] - q.detach()).abs().max()) <= PC.TOL_ADAM_REL_LR * lr, step
        for ours, theirs in ((m, rst["exp_avg"]), (v, rst["exp_avg_sq"])):
            assert float((ours.cpu()[keep] - theirs).abs().max()) <= MOMENT_TOL * float(theirs.abs().max()), step
        for ours, start in ((p, p0), (m, m0), (v, v0)):   # the skip range is left alone
            assert torch.equal(ours.cpu()[lo:hi], start[lo:hi])


# ---- 5. module level ---------------------------------------------------------------------------------------------------------
def _flat_norm(grads):
    return float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values() if g is not None)))


def check_module_clipped_training(name, lib, dev):
    g = GoldenCase(name)
    max_norm = 0.5 * _flat_norm(g.grads)
    model = WaveNet(*g.cfg.as_tuple(), _library=lib)
    model.load_state_dict(g.params)
    model.to(dev)
    opt = FusedAdam(model, lr=g.adam_lr, weight_decay=g.wd, max_grad_norm=max_norm)
    ref = {k: torch.nn.Parameter(v.clone()) for k, v in g.params.items()}
    ropt = torch.optim.Adam(list(ref.values()), lr=g.adam_lr, weight_decay=g.wd)
    x, h, t = g.x.to(dev), g.h.to(dev), g.t.to(dev)
    active = 0
    for step in range(g.adam_steps):
        _, _, og = O.train_step(g.cfg, {k: v.detach() for k, v in ref.items()}, None, g.x, g.h, g.t)
        for k, p in ref.items():
            p.grad = None if og[k] is None else og[k].clone()
        tnorm = float(torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm))
        ropt.step()
        model.loss_and_backward(x, h, t)
        opt.step()
        norm = float(opt.grad_norm)
        # the HIP gradient is held to TOL_GRAD of each tensor's maximum: | ||g|| - ||g_ref|| | <= ||g - g_ref|| <= that bound
        bound = PC.TOL_GRAD * float(np.sqrt(sum(v.numel() * float(v.abs().max()) ** 2 for v in og.values() if v is not None)))
        assert abs(norm - tnorm) <= bound + NORM_TOL * tnorm, (norm, tnorm, bound)
        active += norm > max_norm
        assert opt.steps_applied() == step + 1 and opt.steps_skipped() == 0
    assert active >= 1, "the clip was never active: the case shows nothing"
    for k, v in model.state_dict().items():
        e = float((v.cpu() - ref[k].detach()).abs().max())
        assert e <= PC.TOL_ADAM_REL_LR * g.adam_lr, "%s: |dw| err %g (lr %g)" % (k, e, g.adam_lr)


# ---- 6. skip -------------------------------------------------------------------------------------------------------------------
def _tiny_model(lib, dev, seed=3):
    cfg = O.OracleConfig(*TINY)
    model = WaveNet(*TINY, _library=lib)
    model.load_state_dict(O.random_params(cfg, seed))
    model.to(dev)
    x, h, t = O.synthetic_batch(cfg, 2, 48, seed + 1)
    return model, x.to(dev), h.to(dev), t.to(dev)


def _live_index(eng):
    i = eng.n_params // 2
    assert not (eng.dead_range[0] <= i < eng.dead_range[1])
    return i


def _torch_adam_on_flat(eng, p0, g, lr, max_norm=None, weight_decay=0.0):
    """One torch.optim.Adam step (after clip_grad_norm_) on the live part of a flat buffer, on the CPU; returns the new buffer."""
    lo, hi = eng.dead_range
    keep = torch.cat([torch.arange(0, lo), torch.arange(hi, eng.n_params)])
    q = torch.nn.Parameter(p0.cpu()[keep].clone())
    q.grad = g.cpu()[keep].clone()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_([q], max_norm)
    torch.optim.Adam([q], lr=lr, weight_decay=weight_decay).step()
    out = p0.cpu().clone()
    out[keep] = q.detach()
    return out


def check_skip(lib, dev):
    lr = 1e-3
    model, x, h, t = _tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, lr=lr, skip_nonfinite=True)
    m, v = opt._buffers()
    m.normal_()
    v.uniform_()
    model.loss_and_backward(x, h, t)
    eng.grads()[_live_index(eng)] = float("nan")
    before = [b.cpu().clone() for b in (eng.flat_params, m, v)]
    opt.step()
    for b, b0 in zip((eng.flat_params, m, v), before):
        assert torch.equal(b.cpu().view(torch.int32), b0.view(torch.int32))
    assert opt.steps_skipped() == 1 and opt.steps_applied() == 0 and not np.isfinite(float(opt.grad_norm))
    assert opt.state_dict()["state"] == {}   # no applied step yet
    # the next finite step is Adam's FIRST step (bias correction at step 1)
    m.zero_()
    v.zero_()
    model.loss_and_backward(x, h, t)
    want = _torch_adam_on_flat(eng, eng.flat_params, eng.grads(), lr)
    opt.step()
    assert opt.steps_skipped() == 1 and opt.steps_applied() == 1
    assert float((eng.flat_params.cpu() - want).abs().max()) <= PC.TOL_ADAM_REL_LR * lr


def check_guard_off_nan_reaches_the_weights(lib, dev):
    lr = 1e-3
    model, x, h, t = _tiny_model(lib, dev)
    eng = model.engine
    lo, hi = eng.dead_range
    live = torch.ones(eng.n_params, dtype=torch.bool)
    live[lo:hi] = False
    # clipping on: torch's coefficient is NaN, every clipped gradient and so every weight becomes NaN
    opt = FusedAdam(model, lr=lr, max_grad_norm=1.0, skip_nonfinite=False)
    model.loss_and_backward(x, h, t)
    eng.grads()[_live_index(eng)] = float("nan")
    p0 = eng.flat_params.cpu().clone()
    want = _torch_adam_on_flat(eng, p0, eng.grads(), lr, max_norm=1.0)
    opt.step()
    got = eng.flat_params.cpu()
    assert bool(torch.isnan(want[live]).all()) and bool(torch.isnan(got[live]).all())
    assert torch.equal(got[lo:hi], p0[lo:hi]) and opt.steps_applied() == 1 and opt.steps_skipped() == 0


# ---- 7. defaults untouched ---------------------------------------------------------------------------------------------------
def check_defaults(lib, dev):
    lr = 1e-3
    model, x, h, t = _tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, lr=lr, weight_decay=1e-2)
    assert opt.grad_norm is None and not opt.guarded
    twin = WaveNetEngine(*TINY, device=dev, library=lib)   # wn_adam_step driven directly
    twin.flat_params.copy_(eng.flat_params)
    tm, tv = torch.zeros_like(twin.flat_params), torch.zeros_like(twin.flat_params)
    model.loss_and_backward(x, h, t)
    g0 = eng.grads().clone()
    for step in range(2):
        eng.grads().copy_(g0 * (1.0 + step))   # a fresh gradient per step (the backward pass is not what is under test)
        twin.grads().copy_(eng.grads())
        log = PC.launch_log(lib, opt.step)
        assert log == {"adam": 1}, log
        twin.adam_step(tm, tv, step + 1, lr, weight_decay=1e-2)
        assert torch.equal(eng.flat_params.cpu().view(torch.int32), twin.flat_params.cpu().view(torch.int32))
    assert opt.steps_applied() == 2 and opt.steps_skipped() == 0


def check_guarded_launches_and_plain_agreement(lib, dev):
    """max_grad_norm=None, skip_nonfinite=True on finite gradients against the plain path, per step (both start every step from
    the same weights and moments): the moments are bit-identical (clip_coef is exactly 1), the weights within 2^-23 |p| + 1e-6 lr
    -- the prepared lr / bc1, sqrt(bc2) may differ from the host's by one float ulp, which moves an update of at most ~3.2 lr by
    at most ~8e-7 lr and may flip the rounding of p by one ulp."""
    lr = 1e-3
    model, x, h, t = _tiny_model(lib, dev)
    plain, _, _, _ = _tiny_model(lib, dev)
    opt = FusedAdam(model, lr=lr, weight_decay=1e-2, skip_nonfinite=True)
    popt = FusedAdam(plain, lr=lr, weight_decay=1e-2)
    model.loss_and_backward(x, h, t)
    plain.loss_and_backward(x, h, t)
    g0 = model.engine.grads().clone()
    for step in range(3):
        for mdl in (model, plain):
            mdl.engine.grads().copy_(g0 * (1.0 + step))   # a fresh gradient per step (the backward pass is not under test)
        log = PC.launch_log(lib, opt.step)
        assert log == {"grad_sumsq": 1, "grad_norm_finalize": 1, "adam_guarded": 1}, log
        popt.step()
        p, q = model.engine.flat_params.cpu(), plain.engine.flat_params.cpu()
        assert bool(((p - q).abs() <= 2.0 ** -23 * q.abs() + 1e-6 * lr).all()), float((p - q).abs().max())
        for a, b in zip(opt._buffers(), popt._buffers()):
            assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))
        model.engine.flat_params.copy_(plain.engine.flat_params)
        st = read_state(opt._guard_buffers()[0])
        assert st.clip_coef == 1.0 and st.apply == 1 and st.steps_applied == step + 1


# ---- 8. checkpoint ------------------------------------------------------------------------------------------------------------
def check_checkpoint(lib, dev):
    lr = 1e-3
    kw = dict(lr=lr, weight_decay=1e-2, max_grad_norm=0.05, skip_nonfinite=True)
    model, x, h, t = _tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, **kw)
    model.loss_and_backward(x, h, t)
    g0 = eng.grads().clone()
    for step in range(3):   # apply, skip, apply
        eng.grads().copy_(g0 * (1.0 + step))
        if step == 1:
            eng.grads()[_live_index(eng)] = float("inf")
        opt.step()
    assert (opt.steps_applied(), opt.steps_skipped()) == (2, 1)
    sd = opt.state_dict()
    assert set(sd.keys()) == {"state", "param_groups"}
    assert all(set(s.keys()) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 2.0 for s in sd["state"].values())
    # ... loads into torch.optim.Adam over the same parameters, and back
    topt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-2)
    topt.load_state_dict(sd)
    assert all(float(s["step"]) == 2.0 for s in topt.state_dict()["state"].values())
    resumed = WaveNet(*TINY, _library=lib)
    resumed.load_state_dict(model.state_dict())
    resumed.to(dev)
    ropt = FusedAdam(resumed, **kw)
    ropt.load_state_dict(topt.state_dict())
    assert (ropt.steps_applied(), ropt.steps_skipped()) == (2, 0)
    resumed.loss_and_backward(x, h, t)   # (gives the resumed model's parameters their gradient views)
    for mdl, o in ((model, opt), (resumed, ropt)):
        mdl.engine.grads().copy_(g0 * 0.5)
        o.step()
    assert torch.equal(eng.flat_params.cpu().view(torch.int32), resumed.engine.flat_params.cpu().view(torch.int32))
    for a, b in zip(opt._buffers(), ropt._buffers()):
        assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))
    assert opt.steps_applied() == 3 and ropt.steps_applied() == 3


# ---- the autograd route and live parameters without a gradient ----------------------------------------------------------------
def check_autograd_route_and_missing_gradients(lib, dev):
    """Gradients that live outside the flat buffer (the autograd route) are gathered BEFORE the norm; a live parameter without a
    gradient is left alone and adds nothing to the norm -- torch's clip_grad_norm_ + Adam leave it out the same way."""
    lr, max_norm = 1e-2, 0.05
    model, x, h, t = _tiny_model(lib, dev)
    opt = FusedAdam(model, lr=lr, weight_decay=1e-3, max_grad_norm=max_norm)
    ref = {k: torch.nn.Parameter(v.cpu().clone()) for k, v in model.state_dict().items()}
    ropt = torch.optim.Adam(list(ref.values()), lr=lr, weight_decay=1e-3)
    drop = {"conv_post_1.weight", "dil_tanh.1.conv.bias"}
    for step in range(2):
        model.loss_and_backward(x, h, t)
        for k, p in model.named_parameters():
            if p.grad is None or (step == 1 and k in drop):
                p.grad = None
                ref[k].grad = None
            else:
                p.grad = p.grad.clone()   # a tensor of its own, as autograd would leave it
                ref[k].grad = p.grad.cpu().clone()
        tnorm = float(torch.nn.utils.clip_grad_norm_([p for p in ref.values() if p.grad is not None], max_norm))
        ropt.step()
        opt.step()
        # the same numbers on both sides; torch rounds every tensor's norm and the norm of those to fp32 (3 * 2^-24 with ours)
        assert tnorm > max_norm and abs(float(opt.grad_norm) - tnorm) <= NORM_TOL * tnorm
    for k, v in model.state_dict().items():
        assert float((v.cpu() - ref[k].detach()).abs().max()) <= PC.TOL_ADAM_REL_LR * lr, k
