# -*- coding: utf-8 -*-
"""Gradient accumulation over micro-batches (wn_op_accumulate, WaveNet.loss_and_backward(micro_step=(i, A)), FusedAdam behind a
cycle): the cases tests/test_emu_accum.py runs on the host-compiled kernels and tests/test_gpu_accum.py on the MI355X.

The reference of every numeric check is torch on the CPU, numpy in fp64 or the oracle -- never the code under test.

Tolerances
  op level  none: one fp32 add per element is what torch's CPU ``a + b`` does, so the written buffer has torch's bits wherever the
            result is not a NaN (a NaN's payload is not part of the contract) and is a NaN exactly where torch's is.
  sums      none: the chain SET, ADD, ..., FINISH adds in the order ((g0 + g1) + g2) + ..., torch's ``p.grad += g``.
  oracle    PC.TOL_GRAD of each tensor's maximum / PC.TOL_LOSS, the project's gates for one step: with shares N_i / N the sum of
            the micro-batch gradients IS the gradient of the mean over all loss positions, and the A - 1 extra fp32 roundings of
            the sum (2^-24 of the largest term each) are far inside 1e-4.
  norm      CC.NORM_TOL against the fp64 norm of the summed buffer (tests/clip_common.py).
"""
import numpy as np
import pytest
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import _stream_handle, flat_to_state
from pytorchwavenetvocoder_amd.nets import WaveNet
from pytorchwavenetvocoder_amd.optim import FusedAdam
from tests import clip_common as CC
from tests import ema_common as EC
from tests import mol_common as MC
from tests import parity_common as PC
from tests import ragged_common as RC

SET, ADD, FINISH = _lib.ACCUM_SET, _lib.ACCUM_ADD, _lib.ACCUM_FINISH
MODES = {"set": SET, "add": ADD, "finish": FINISH}
TINY = CC.TINY
# One sweep of the kernel's grid: 1024 blocks x 256 threads x 4 floats x 2 quads in flight -- more than CC.SWEEP, so the last size of
# CC.SIZES is replaced by one that passes a whole sweep, starts a second one and leaves a scalar tail of 3.
ACCUM_SWEEP = 1024 * 256 * 4 * 2
SIZES = CC.SIZES[:-1] + [ACCUM_SWEEP + 4099]
MISALIGN = [(0, 0), (1, 1), (3, 3), (0, 1), (2, 3)]   # floats behind a 16-byte boundary: (acc, grad)
GUARD = 4
SEED = 5

same_bits, bits, f64 = EC.same_bits, EC.bits, EC.f64


# ---- 1. op level -------------------------------------------------------------------------------------------------------------------
def _bit_buffer(n, seed):
    """int32 bit patterns for a whole allocation (n elements, up to 3 floats of misalignment, GUARD or more floats on each side):
    random, made finite; _plant adds the special values."""
    rs = np.random.RandomState(seed + n)
    raw = rs.randint(-2 ** 31, 2 ** 31, size=n + 2 * GUARD + 4, dtype=np.int64).astype(np.int32)
    nonfinite = ~np.isfinite(raw.view(np.float32))
    raw[nonfinite] &= np.int32(~0x40000000)            # clear an exponent bit: the pattern becomes a finite number
    assert bool(np.isfinite(raw.view(np.float32)).all())
    return raw


def _plant(ra, rg, mis, n):
    """The special values, at the same index of both views: every pattern of EC.SPECIAL_BITS against a finite partner (both
    ways), +-3e38 pairs that overflow to +-inf, inf + -inf (a NaN from two non-NaNs), +0 + -0."""
    fa, fg = ra.view(np.float32), rg.view(np.float32)
    k = 0

    def put(a_bits=None, g_bits=None, a=None, g=None):
        nonlocal k
        i = (k * 37 + 1) % n
        k += 1
        ia, ig = GUARD + mis[0] + i, GUARD + mis[1] + i
        if a_bits is not None:
            ra[ia] = np.array(a_bits, np.uint32).view(np.int32)
        if g_bits is not None:
            rg[ig] = np.array(g_bits, np.uint32).view(np.int32)
        if a is not None:
            fa[ia] = a
        if g is not None:
            fg[ig] = g
    for b in EC.SPECIAL_BITS:
        put(a_bits=b)
        put(g_bits=b)
    put(a=3e38, g=3e38)
    put(a=-3e38, g=-3e38)
    put(a_bits=0x7f800000, g_bits=0xff800000)
    put(a_bits=0x00000000, g_bits=0x80000000)
    put(a_bits=0x80000000, g_bits=0x80000000)


def _views(n, misalign, dev):
    ra, rg = _bit_buffer(n, 1), _bit_buffer(n, 2)
    _plant(ra, rg, misalign, n)
    out = []
    for raw, mis in ((ra, misalign[0]), (rg, misalign[1])):
        whole = torch.from_numpy(raw.copy()).to(dev)
        assert whole.data_ptr() % 16 == 0
        view = whole[GUARD + mis:GUARD + mis + n]
        assert view.data_ptr() % 16 == 4 * mis and whole.numel() - (GUARD + mis + n) >= GUARD
        out.append((whole, view, torch.from_numpy(raw.copy())))
    return out


def _assert_sum(got, want, what):
    """`got` has `want`'s bits wherever want is not a NaN, and is a NaN exactly where want is."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(bits(got)[~nan], bits(want)[~nan]), what


def check_op(lib, dev, n, misalign, mode_name):
    mode = MODES[mode_name]
    st = _stream_handle(torch.device(dev))
    (wa, a, wa0), (wg, g, wg0) = _views(n, misalign, dev)
    sa = slice(GUARD + misalign[0], GUARD + misalign[0] + n)
    sg = slice(GUARD + misalign[1], GUARD + misalign[1] + n)
    a0, g0 = wa0[sa].view(torch.float32), wg0[sg].view(torch.float32)
    want = g0.clone() if mode == SET else a0 + g0                     # torch on the CPU
    if n > 64:
        assert bool(torch.isinf(want).any()) and bool(torch.isnan(want).any())   # (the planted cases are there)
    lib.check(lib.wn_op_accumulate(a.data_ptr(), g.data_ptr(), n, mode, st), "wn_op_accumulate")
    ga, gg = wa.cpu(), wg.cpu()
    written, w_slice, w0 = (gg, sg, wg0) if mode == FINISH else (ga, sa, wa0)
    other, o0 = (ga, wa0) if mode == FINISH else (gg, wg0)
    _assert_sum(written[w_slice].view(torch.float32), want, (n, misalign, mode_name))
    assert torch.equal(other, o0), (n, misalign, mode_name, "the buffer this mode only reads was written")
    assert torch.equal(written[:w_slice.start], w0[:w_slice.start]) and torch.equal(written[w_slice.stop:], w0[w_slice.stop:]), \
        (n, misalign, mode_name, "guard floats")


def check_chain(lib, dev, n, misalign):
    """SET, ADD, ADD, FINISH over four arrays: the gradient buffer ends as ((g0 + g1) + g2) + g3."""
    st = _stream_handle(torch.device(dev))
    rs = np.random.RandomState(n)
    gs = [torch.from_numpy((rs.standard_normal(n) * 10.0 ** rs.randint(-3, 4, size=n)).astype(np.float32)) for _ in range(4)]
    wa = torch.full((n + 12,), float("nan"), dtype=torch.float32, device=dev)     # SET overwrites whatever the accumulator held
    wg = torch.zeros(n + 12, dtype=torch.float32, device=dev)
    a, g = wa[GUARD + misalign[0]:GUARD + misalign[0] + n], wg[GUARD + misalign[1]:GUARD + misalign[1] + n]
    for k, mode in enumerate((SET, ADD, ADD, FINISH)):
        g.copy_(gs[k])
        lib.check(lib.wn_op_accumulate(a.data_ptr(), g.data_ptr(), n, mode, st), "wn_op_accumulate")
        if mode != FINISH:
            assert same_bits(g, gs[k])                                            # the gradient buffer keeps its micro-batch
    want = ((gs[0] + gs[1]) + gs[2]) + gs[3]
    assert same_bits(g, want)
    assert same_bits(a, (gs[0] + gs[1]) + gs[2])                                  # FINISH left the accumulator alone


def check_op_errors(lib, dev):
    st = _stream_handle(torch.device(dev))
    buf = torch.zeros(64, dtype=torch.float32, device=dev)
    p = buf.data_ptr()
    for a, b, n in ((p, p, 8), (p, p + 4 * 7, 8), (p + 4 * 7, p, 8)):
        for mode in (SET, ADD, FINISH):
            assert lib.wn_op_accumulate(a, b, n, mode, st) != 0
            assert b"overlap" in lib.wn_last_error()
    assert lib.wn_op_accumulate(p, p + 4 * 8, 8, ADD, st) == 0        # adjacent ranges are fine
    assert lib.wn_op_accumulate(None, p, 8, ADD, st) != 0 and b"wn_op_accumulate" in lib.wn_last_error()
    assert lib.wn_op_accumulate(p, None, 8, ADD, st) != 0
    assert lib.wn_op_accumulate(p, p + 32, 0, ADD, st) != 0 and lib.wn_op_accumulate(p, p + 32, -1, ADD, st) != 0
    for mode in (3, -1):
        assert lib.wn_op_accumulate(p, p + 32, 8, mode, st) != 0
        assert b"mode" in lib.wn_last_error()
    assert not bool(buf.cpu().any())


# ---- 2. module level, dense ----------------------------------------------------------------------------------------------------
_DENSE = {}


def dense_instance():
    """Kink-free instance of TINY, B = 4, T = 48, and the fp64 oracle's step on the four rows as one batch (computed once)."""
    if not _DENSE:
        cfg = O.OracleConfig(*TINY)
        params, x, h, t, margin, sd = PC.pick_instance(cfg, 4, 48, SEED, 0.1)
        _DENSE["v"] = (params, x, h, t, RC.oracle_ragged(TINY, params, x, h, t, [48] * 4))
    return _DENSE["v"]


def new_model(cfg_t, params, lib, dev, **kw):
    model = WaveNet(*cfg_t, _library=lib, **kw)
    model.load_state_dict(params)
    model.to(dev)
    return model


def _rows(x, h, t, lo, hi, T=None, U=TINY[7]):
    T = x.size(1) if T is None else T
    return x[lo:hi, :T].contiguous(), h[lo:hi, :, :T // U].contiguous(), t[lo:hi, :T].contiguous()


def run_cycle(model, dev, batches, shares, lengths=None):
    """One cycle through model.loss_and_backward; returns (losses, the flat buffer cloned after each micro-step (CPU))."""
    losses, grads = [], []
    A = len(batches)
    for i, (xb, hb, tb) in enumerate(batches):
        kw = {} if lengths is None else {"lengths": lengths[i]}
        loss = model.loss_and_backward(xb.to(dev), hb.to(dev), tb.to(dev), grad_scale=shares[i], micro_step=(i, A), **kw)
        assert model.engine.accumulation == (None if i == A - 1 else (i + 1, A))
        losses.append(float(loss.cpu()))
        grads.append(model.engine.grads().cpu().clone())
    return losses, grads


def torch_sum(grads):
    """((g0 + g1) + g2) + ... on the CPU."""
    acc = grads[0].clone()
    for g in grads[1:]:
        acc = acc + g
    return acc


def _oracle_gates(tag, cfg_t, eng, flat, loss, ref):
    loss_ref, grads_ref = ref[0], ref[1]
    grads = flat_to_state(eng, flat, O.param_shapes(O.OracleConfig(*cfg_t)))
    worst, worst_k = 0.0, None
    for k, r in grads_ref.items():
        if r is None:
            assert float(grads[k].abs().max()) == 0.0, (tag, k)
            continue
        e = PC.rel_to_max(grads[k], r)
        if e > worst:
            worst, worst_k = e, k
    e_loss = abs(loss - loss_ref)
    print("%s: loss err %.3g, worst gradient %.3g of its maximum (%s)" % (tag, e_loss, worst, worst_k))
    return e_loss, worst, worst_k


def check_dense(lib, dev, split):
    params, x, h, t, ref = dense_instance()
    bounds = np.cumsum([0] + list(split))
    batches = [_rows(x, h, t, int(lo), int(hi)) for lo, hi in zip(bounds[:-1], bounds[1:])]
    shares = [r / 4.0 for r in split]
    model = new_model(TINY, params, lib, dev)
    eng = model.engine
    assert eng.grad_accum is None
    losses, grads = run_cycle(model, dev, batches, shares)
    # (a) the bits of torch's sum of the buffers captured after each micro-step, in order
    own = grads[:-1]
    total = grads[-1]
    # the last micro-batch's own gradient is not in any buffer afterwards: run it alone on a twin for the reference sum
    twin = new_model(TINY, params, lib, dev)
    xb, hb, tb = batches[-1]
    twin.loss_and_backward(xb.to(dev), hb.to(dev), tb.to(dev), grad_scale=shares[-1])
    last_own = twin.engine.grads().cpu().clone()
    want = torch_sum(own + [last_own])
    assert same_bits(total, want), "the accumulated buffer is not torch's sum in order"
    assert same_bits(eng.grad_accum, torch_sum(own))
    for p, (off, n, shape, dead) in zip(model.parameters(), model._param_slices):   # p.grad is a view of the summed buffer
        assert (p.grad is None) == dead
        if not dead:
            assert same_bits(p.grad, want[off:off + n].view(shape))
    # (b) against the fp64 oracle's step on the four rows as one batch; the one-call B = 4 step beside it for the record
    loss = sum(s * l for s, l in zip(shares, losses))
    e_loss, worst, worst_k = _oracle_gates("A = %d, rows %s" % (len(split), "+".join(map(str, split))), TINY, eng, total, loss, ref)
    one = new_model(TINY, params, lib, dev)
    l1 = float(one.loss_and_backward(x.to(dev), h.to(dev), t.to(dev)).cpu())
    _oracle_gates("one call, B = 4", TINY, one.engine, one.engine.grads().cpu(), l1, ref)
    assert e_loss <= PC.TOL_LOSS and worst <= PC.TOL_GRAD, (e_loss, worst, worst_k)
    # (c) the optimizer step behind the cycle == the step of a twin whose gradient buffer holds that torch sum
    opt, topt = FusedAdam(model, lr=1e-3), FusedAdam(twin, lr=1e-3)
    twin.engine.grads().copy_(want)
    opt.step()
    topt.step()
    assert same_bits(eng.flat_params, twin.engine.flat_params) and not same_bits(eng.flat_params, one.engine.flat_params)
    for ours, theirs in zip(opt._buffers(), topt._buffers()):
        assert same_bits(ours, theirs)


# ---- 3. ragged ---------------------------------------------------------------------------------------------------------------------
RAGGED_T, RAGGED_LENGTHS = 64, [64, 40, 52, 33]


def check_ragged(lib, dev):
    cfg = O.OracleConfig(*TINY)
    rf = cfg.receptive_field
    params, x, h, t, margin, sd = PC.pick_instance(cfg, 4, RAGGED_T, SEED + 1, 0.1)
    ref = RC.oracle_ragged(TINY, params, x, h, t, RAGGED_LENGTHS)
    batches = [_rows(x, h, t, 0, 2), _rows(x, h, t, 2, 4, T=52)]
    lengths = [RAGGED_LENGTHS[:2], RAGGED_LENGTHS[2:]]
    counts = [sum(max(v - rf, 0) for v in ls) for ls in lengths]
    shares = [c / float(sum(counts)) for c in counts]
    model = new_model(TINY, params, lib, dev)
    losses, grads = run_cycle(model, dev, batches, shares, lengths=lengths)      # (the workspace changes inside the cycle)
    loss = sum(s * l for s, l in zip(shares, losses))
    e_loss, worst, worst_k = _oracle_gates("ragged, T = 64 then 52", TINY, model.engine, grads[-1], loss, ref)
    assert e_loss <= PC.TOL_LOSS and worst <= PC.TOL_GRAD, (e_loss, worst, worst_k)


# ---- 4. mixture head -----------------------------------------------------------------------------------------------------------
def check_mol(lib, dev):
    cfg = O.OracleConfig(*MC.CFG, out_channels=3 * MC.NM)
    B, T = 2, 48
    params, x, h, seed = MC._kink_free_instance(cfg, B, T)
    y = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (B, T)).astype(np.float32))
    model = new_model(MC.CFG, params, lib, dev, n_mixture=MC.NM)
    eng = model.engine
    rows = [(x[b:b + 1].contiguous().to(dev), h[b:b + 1].contiguous().to(dev), y[b:b + 1].contiguous().to(dev)) for b in range(B)]
    own = []
    model.mol_loss_and_backward(*rows[0], grad_scale=0.5)   # each micro-batch alone first: its own gradient, and dh of the plain call
    own.append(eng.grads().cpu().clone())
    _, dh_plain = model.mol_loss_and_backward(*rows[1], grad_scale=0.5, aux_grad=True)
    own.append(eng.grads().cpu().clone())
    assert eng.grad_accum is None
    model.mol_loss_and_backward(*rows[0], grad_scale=0.5, micro_step=(0, 2))
    assert same_bits(eng.grads(), own[0]) and eng.accumulation == (1, 2)
    _, dh = model.mol_loss_and_backward(*rows[1], grad_scale=0.5, micro_step=(1, 2), aux_grad=True)
    assert eng.accumulation is None
    assert same_bits(eng.grads(), own[0] + own[1])
    assert same_bits(dh, dh_plain) and tuple(dh.shape) == tuple(rows[1][1].shape)   # dh belongs to its micro-batch: never accumulated
    assert not same_bits(own[0] + own[1], own[1])


# ---- 5. off means off --------------------------------------------------------------------------------------------------------------
def check_off_means_off(lib, dev):
    model, x, h, t = CC._tiny_model(lib, dev)
    eng = model.engine
    model.loss_and_backward(x, h, t)                     # (first call: packs the weight sets)
    plain = PC.launch_sequence(lib, lambda: model.loss_and_backward(x, h, t))
    l0 = model.loss_and_backward(x, h, t)
    g0 = eng.grads().cpu().clone()
    assert "grad_accumulate" not in plain and len(plain) > 3
    for ms in (None, (0, 1)):
        assert PC.launch_sequence(lib, lambda: model.loss_and_backward(x, h, t, micro_step=ms)) == plain, ms
        l1 = model.loss_and_backward(x, h, t, micro_step=ms)
        assert same_bits(l1, l0) and same_bits(eng.grads(), g0)
        assert eng.grad_accum is None and eng.accumulation is None
    for i in range(3):
        seq = PC.launch_sequence(lib, lambda: model.loss_and_backward(x, h, t, micro_step=(i, 3)))
        assert seq == plain + ["grad_accumulate"], (i, seq)
    assert eng.grad_accum is not None and eng.accumulation is None
    assert same_bits(eng.grads(), (g0 + g0) + g0)


# ---- 6. optimizer interplay ------------------------------------------------------------------------------------------------------
def _three(x, h, t):
    return [(x[0:1].contiguous(), h[0:1].contiguous(), t[0:1].contiguous()), (x[1:2].contiguous(), h[1:2].contiguous(), t[1:2].contiguous()),
            (x.contiguous(), h.contiguous(), t.contiguous())]


def _cycle(model, batches, shares):
    for i, (xb, hb, tb) in enumerate(batches):
        model.loss_and_backward(xb, hb, tb, grad_scale=shares[i], micro_step=(i, len(batches)))


def check_norm(lib, dev):
    model, x, h, t = CC._tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, lr=1e-3, max_grad_norm=1e9)
    _cycle(model, _three(x, h, t), [0.25, 0.25, 0.5])
    lo, hi = eng.dead_range
    ref = CC.ref_norm(eng.grads(), lo, hi)
    opt.step()
    got = float(opt.grad_norm)
    print("norm of the accumulated gradient %.9g, fp64 %.9g" % (got, ref))
    assert abs(got - ref) <= CC.NORM_TOL * ref and ref > 0.0


def check_guard(lib, dev):
    kw = dict(lr=1e-3, skip_nonfinite=True, ema_decay=0.9)
    shares = [0.25, 0.25, 0.5]
    model, x, h, t = CC._tiny_model(lib, dev)
    twin, _, _, _ = CC._tiny_model(lib, dev)
    opt, topt = FusedAdam(model, **kw), FusedAdam(twin, **kw)
    clean = _three(x, h, t)
    for m, o in ((model, opt), (twin, topt)):                # one applied step first: moments and average have moved
        _cycle(m, clean, shares)
        o.step()
    eng = model.engine
    assert same_bits(eng.flat_params, twin.engine.flat_params)
    bad = [list(b) for b in clean]
    bad[1][1] = bad[1][1].clone()
    bad[1][1][0, 0, 2] = float("nan")                        # NaN in h of the middle micro-batch
    before = [b.cpu().clone() for b in (eng.flat_params, opt.ema) + tuple(opt._buffers())]
    _cycle(model, bad, shares)
    assert not bool(torch.isfinite(eng.grads()).all())       # the sum carries the bad micro-batch
    opt.step()
    for b, b0 in zip((eng.flat_params, opt.ema) + tuple(opt._buffers()), before):
        assert same_bits(b, b0)
    assert (opt.steps_applied(), opt.steps_skipped()) == (1, 1)
    for m, o in ((model, opt), (twin, topt)):                # SET overwrites: nothing of the bad cycle is left
        _cycle(m, clean, shares)
        o.step()
    assert (opt.steps_applied(), opt.steps_skipped()) == (2, 1) and (topt.steps_applied(), topt.steps_skipped()) == (2, 0)
    assert same_bits(eng.grads(), twin.engine.grads())
    for ours, theirs in zip((eng.flat_params, opt.ema) + tuple(opt._buffers()), (twin.engine.flat_params, topt.ema) + tuple(topt._buffers())):
        assert same_bits(ours, theirs)
    assert not same_bits(eng.flat_params, before[0])


def check_ema_counts_optimizer_steps(lib, dev):
    ema_decay, shares = 0.9, [0.25, 0.25, 0.5]
    model, x, h, t = CC._tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, lr=1e-2, ema_decay=ema_decay, ema_warmup=True)
    want = f64(opt.ema)
    big = float(np.abs(want).max())
    for step in range(1, 4):
        _cycle(model, _three(x, h, t), shares)
        opt.step()
        assert opt.steps_applied() == step                   # optimizer steps, not micro-steps
        want = EC.ema_ref(want, f64(eng.flat_params), ema_decay, True, step)
        big = max(big, float(eng.flat_params.abs().max()))
    lo, hi = eng.dead_range
    live = np.ones(eng.n_params, bool)
    live[lo:hi] = False
    err = float(np.abs(f64(opt.ema) - want)[live].max())
    # the same three weight snapshots with the warm-up index counted per micro-step would give another average
    assert EC.decay_at(ema_decay, True, 3) != EC.decay_at(ema_decay, True, 9)
    assert err <= 4.0 * 3 * EC.U24 * big, err
    assert opt.state_dict()["state"][0]["step"] == 3.0


# ---- 7. misuse ---------------------------------------------------------------------------------------------------------------------
def check_misuse(lib, dev):
    model, x, h, t = CC._tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, lr=1e-3)
    call = lambda **kw: model.loss_and_backward(x, h, t, **kw)   # noqa: E731

    def open_cycle():
        eng.abandon_accumulation()
        call(micro_step=(0, 3))
        assert eng.accumulation == (1, 3)

    def usable(full=False):
        eng.abandon_accumulation()
        assert eng.accumulation is None
        call()                                                   # a plain call is accepted again
        if full:
            _cycle(model, [(x, h, t)] * 2, [0.5, 0.5])
            opt.step()
    with pytest.raises(RuntimeError, match="starts with micro_step=\\(0, 3\\)"):
        call(micro_step=(1, 3))                                  # no cycle open
    usable()
    for bad, word in (((2, 3), "not the next micro-step"), ((1, 4), "A must not change"), (None, "a cycle is open|cycle is open"),
                      ((0, 1), "cycle is open"), ((0, 3), "while a cycle is open")):
        open_cycle()
        with pytest.raises(RuntimeError, match=word):
            call(micro_step=bad)
        assert eng.accumulation == (1, 3)                        # a refused call leaves the cycle where it was
        usable()
    open_cycle()
    with pytest.raises(RuntimeError, match="abandon_accumulation"):
        opt.step()
    usable(full=True)
    for bad in ((3, 3), (-1, 3), (0, 0), (0.5, 2), "ab", (1,)):
        with pytest.raises(ValueError):
            call(micro_step=bad)
    # to() and _flatten() abandon a cycle and drop the accumulator
    for move in (lambda: model.to(dev), model._flatten):
        open_cycle()
        assert eng.grad_accum is not None
        move()
        assert model.engine.accumulation is None and model.engine.grad_accum is None
        usable()
    with pytest.raises(ValueError):
        eng.accumulate_grads(SET, 5, 5)
    with pytest.raises(ValueError):
        eng.accumulate_grads(SET, 0, eng.n_params + 1)


def check_bucket_ranges_tile(lib, dev):
    from pytorchwavenetvocoder_amd.distributed import GradientReducer
    model, x, h, t = CC._tiny_model(lib, dev)
    for lpb in (None, 1, 2, 4):
        red = GradientReducer(model, layers_per_bucket=lpb)
        assert red.ranges[0][0] == 0 and red.ranges[-1][1] == model.engine.n_params and red._gaps == []
        for (a0, a1), (b0, b1) in zip(red.ranges[:-1], red.ranges[1:]):
            assert a0 < a1 == b0
    # one rank, no process group: the reducer's cycle is the model's (same bits), the share passed through
    red = GradientReducer(model, layers_per_bucket=2)
    twin, _, _, _ = CC._tiny_model(lib, dev)
    for i in range(2):
        red.loss_and_backward(x, h, t, grad_scale=0.5, micro_step=(i, 2))
        twin.loss_and_backward(x, h, t, grad_scale=0.5, micro_step=(i, 2), layers_per_bucket=2)
    assert same_bits(model.engine.grads(), twin.engine.grads()) and model.engine.accumulation is None
