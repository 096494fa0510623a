# -*- coding: utf-8 -*-
"""Training with frozen parameters (``WaveNet.freeze`` / ``train_only``, ``FusedAdam`` over live ranges,
wn_live_table / wn_grad_norm_live / wn_adam_step_live / wn_adam_step_guarded_live): the cases tests/test_emu_freeze.py runs on the
host-compiled kernels and tests/test_gpu_freeze.py on the MI355X.

Every reference is numpy in fp64, torch on the CPU, the oracle (``O.train_step``; the gradient of a trainable tensor does not
depend on what else is frozen, so the oracle's full gradient restricted to the trainable tensors is the reference), or the
library's own whole-buffer entry points where the claim IS bit-identity with them.  Tolerances are the project's:
``PC.TOL_ADAM_REL_LR``, ``PC.TOL_GRAD``, ``PC.TOL_LOSS`` (tests/parity_common.py), ``NORM_TOL`` and ``MOMENT_TOL``
(tests/clip_common.py).
"""
import ctypes
import re

import numpy as np
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import WaveNetEngine, _ptr, _stream_handle
from pytorchwavenetvocoder_amd.nets import WaveNet
from pytorchwavenetvocoder_amd.optim import FusedAdam
from tests import clip_common as CC
from tests import parity_common as PC

TINY = CC.TINY            # L = 6
TINY_LAYERS = 6
LDS_RANGES = 1024         # tables up to this many ranges are staged in LDS, longer ones are read from global memory


# ---- freeze sets ---------------------------------------------------------------------------------------------------------------
def layer_of(key):
    """Layer index of a per-layer tensor's key, None for the front conv, the upsampling layer and the post-net."""
    m = re.match(r"(?:dil_sigmoid|dil_tanh|aux_1x1_sigmoid|aux_1x1_tanh|skip_1x1|res_1x1)\.(\d+)\.", key)
    return int(m.group(1)) if m else None


def frozen_keys(name, keys, n_layers):
    """The keys a named freeze set freezes.  ``bottom:k``: front conv, upsampling and the layers below k."""
    keys = list(keys)
    if name == "none":
        return set()
    if name == "all":
        return set(keys)
    if name.startswith("bottom:"):
        k = int(name.split(":")[1])
        return {key for key in keys if key.startswith(("causal.", "upsampling.")) or (layer_of(key) is not None and layer_of(key) < k)}
    if name == "post_frozen":
        return {key for key in keys if key.startswith("conv_post_")}
    if name == "aux_only":
        return {key for key in keys if not key.startswith(("aux_1x1_", "upsampling."))}
    if name == "scatter":
        return {key for i, key in enumerate(keys) if i % 3 == 0}
    raise KeyError(name)


def apply_freeze(model, name, n_layers):
    frozen = frozen_keys(name, [k for k, _ in model.named_parameters()], n_layers)
    for k, p in model.named_parameters():
        p.requires_grad_(k not in frozen)
    return frozen


def tiny_model(lib, dev, seed=3):
    cfg = O.OracleConfig(*TINY)
    params = O.random_params(cfg, seed)
    model = WaveNet(*TINY, _library=lib)
    model.load_state_dict(params)
    model.to(dev)
    x, h, t = O.synthetic_batch(cfg, 2, 48, seed + 1)
    return cfg, model, (x, h, t), (x.to(dev), h.to(dev), t.to(dev))


def bits(t):
    return t.detach().cpu().clone().contiguous().view(torch.int32)   # a snapshot (on the CPU .cpu() alone would alias the buffer)


def frozen_mask(model):
    """Bool tensor over the flat buffer: True outside the live ranges of the model's own flags (frozen tensors and the dead one)."""
    m = torch.ones(model.engine.n_params, dtype=torch.bool)
    for lo, hi in model.trainable().ranges:
        m[lo:hi] = False
    return m


def live_norm64(flat, ranges):
    a = flat.detach().cpu().numpy().astype(np.float64)
    return float(np.sqrt(sum(float(np.sum(a[lo:hi] ** 2)) for lo, hi in ranges)))


# ---- 1. frozen parameters stay, trainable ones follow torch ------------------------------------------------------------------------
def check_frozen_training(name, lib, dev, poison=False):
    """Two steps with weight decay and the average on.  ``poison``: under max_grad_norm and skip_nonfinite=True, each step an
    accumulation cycle of two micro-steps, with NaN written over the frozen ranges of the accumulator (after the first
    micro-step) and of the gradient buffer (before step())."""
    lr, wd = 1e-3, 1e-2
    cfg, model, (x, h, t), (xd, hd, td) = tiny_model(lib, dev)
    frozen = apply_freeze(model, name, TINY_LAYERS)
    assert frozen and len(frozen) < len(list(model.parameters()))
    eng = model.engine
    ref = {k: torch.nn.Parameter(v.detach().cpu().clone()) for k, v in model.state_dict().items()}
    _, _, og = O.train_step(cfg, {k: v.detach() for k, v in ref.items()}, None, x, h, t)
    trainable = [k for k in ref if k not in frozen and og[k] is not None]
    max_norm = None
    if poison:
        max_norm = 0.5 * float(np.sqrt(sum(float((og[k].double() ** 2).sum()) for k in trainable)))
    opt = FusedAdam(model, lr=lr, weight_decay=wd, ema_decay=0.999, max_grad_norm=max_norm, skip_nonfinite=poison)
    ropt = torch.optim.Adam([ref[k] for k in trainable], lr=lr, weight_decay=wd)
    # frozen ranges start from values an update would visibly change: random moments and an average that is not the weights
    fz = frozen_mask(model).to(dev)
    m, v = opt._buffers()
    m[fz] = torch.randn(int(fz.sum()), device=dev)
    v[fz] = torch.rand(int(fz.sum()), device=dev)
    opt.ema[fz] += 0.25
    start = [bits(b) for b in (eng.flat_params, m, v, opt.ema)]
    fzc = fz.cpu()
    ranges = model.trainable().ranges
    for step in range(2):
        _, _, og = O.train_step(cfg, {k: v_.detach() for k, v_ in ref.items()}, None, x, h, t)
        for k in trainable:
            ref[k].grad = og[k].clone()
        tnorm = float(np.sqrt(sum(float((og[k].double() ** 2).sum()) for k in trainable)))
        if poison:
            torch.nn.utils.clip_grad_norm_([ref[k] for k in trainable], max_norm)
        ropt.step()
        if poison:
            model.loss_and_backward(xd, hd, td, grad_scale=0.5, micro_step=(0, 2))
            eng.grad_accum[fz] = float("nan")
            model.loss_and_backward(xd, hd, td, grad_scale=0.5, micro_step=(1, 2))
            eng.grads()[fz] = float("nan")
        else:
            model.loss_and_backward(xd, hd, td)
        for k, p in model.named_parameters():
            assert (p.grad is None) == (k in frozen or og[k] is None), k
        opt.step()
        if poison:
            assert opt.steps_applied() == step + 1 and opt.steps_skipped() == 0
            norm = float(opt.grad_norm)
            n64 = live_norm64(eng.grads(), ranges)
            assert abs(norm - n64) <= CC.NORM_TOL * n64, (norm, n64)
            bound = PC.TOL_GRAD * float(np.sqrt(sum(og[k].numel() * float(og[k].abs().max()) ** 2 for k in trainable)))
            assert abs(norm - tnorm) <= bound + CC.NORM_TOL * tnorm, (norm, tnorm, bound)
        for b, b0, what in zip((eng.flat_params, m, v, opt.ema), start, ("weights", "exp_avg", "exp_avg_sq", "average")):
            assert torch.equal(bits(b)[fzc], b0[fzc]), "%s: frozen %s changed in step %d" % (name, what, step)
    assert opt.steps_applied() == 2
    sd, init = model.state_dict(), O.random_params(cfg, 3)
    for k in trainable:
        e = float((sd[k].cpu() - ref[k].detach()).abs().max())
        assert e <= PC.TOL_ADAM_REL_LR * lr, "%s: %s |dw| err %g (lr %g)" % (name, k, e, lr)
        assert not torch.equal(sd[k].cpu(), init[k]), k
    # the moments of the trainable tensors against torch's (clip_common's tolerance)
    mc, vc = m.cpu(), v.cpu()
    for k, (off, n, shape, dead) in zip(sd.keys(), model._param_slices):
        if k in trainable:
            rst = ropt.state[ref[k]]
            for ours, theirs in ((mc, rst["exp_avg"]), (vc, rst["exp_avg_sq"])):
                assert float((ours[off:off + n].view(shape) - theirs).abs().max()) <= CC.MOMENT_TOL * float(theirs.abs().max()), k


# ---- 2. the range kernels, op level ----------------------------------------------------------------------------------------------
def tables(n):
    """Named live-range lists that exist for a buffer of n elements."""
    out = [("whole", [(0, n)]), ("one_element", [(n // 2, n // 2 + 1)])]
    if n >= 3:
        out.append(("first_and_last", [(0, 1), (n - 1, n)]))
    if n >= 16:   # two long ranges, every bound no multiple of 4: the seam lies inside a block's share of the compacted space
        a = CC._not_multiple_of_4(n // 3, n)
        out.append(("split_unaligned", [(1, a), (a + 2, n - 1)]))
    if n == 1023:
        out.append(("every_other", [(i, i + 1) for i in range(0, n, 2)]))          # 512 ranges: staged in LDS
    if n == 4097:
        out.append(("2000_singles", [(2 * i, 2 * i + 1) for i in range(2000)]))    # beyond the LDS table: read from global memory
        assert len(out[-1][1]) > LDS_RANGES
    for name, lo, hi in CC.skip_ranges(n):
        if name in ("block_boundary", "sweep_boundary"):
            out.append((name, [(lo, hi)]))
            out.append((name + "_around", [(1, lo), (hi, n - 1)]))
    return out


def make_table(lib, dev, ranges, n):
    """(device table, n_ranges, n_live) through wn_live_table."""
    nr = len(ranges)
    flat = (ctypes.c_int64 * (2 * nr))(*[x for r in ranges for x in r])
    host = torch.zeros(3 * nr, dtype=torch.int64)
    n_live = lib.wn_live_table(ctypes.cast(flat, ctypes.c_void_p), nr, n, ctypes.c_void_p(host.data_ptr()))
    assert n_live == sum(hi - lo for lo, hi in ranges), lib.wn_last_error()
    lo = torch.tensor([r[0] for r in ranges])
    hi = torch.tensor([r[1] for r in ranges])
    assert torch.equal(host[:nr], lo) and torch.equal(host[nr:2 * nr], hi)
    assert torch.equal(host[2 * nr:], torch.cumsum(hi - lo, 0) - (hi - lo))
    return host.to(dev), nr, int(n_live)


def live_mask(n, ranges):
    m = torch.zeros(n, dtype=torch.bool)
    for lo, hi in ranges:
        m[lo:hi] = True
    return m


def run_norm_live(lib, dev, g, table, max_norm=0.0, guard=False, state=None, scratch=None, lr=1e-3, betas=(0.9, 0.999)):
    tab, nr, n_live = table
    state = CC.new_state(dev) if state is None else state
    scratch = CC.new_scratch(lib, g.numel(), dev) if scratch is None else scratch
    lib.check(lib.wn_grad_norm_live(_ptr(g), g.numel(), _ptr(tab), nr, n_live, float(max_norm), int(guard), float(lr),
                                    float(betas[0]), float(betas[1]), _ptr(scratch), _ptr(state),
                                    _stream_handle(torch.device(dev))), "wn_grad_norm_live")
    return state


# at the size that needs a second sweep: the tables whose bounds cut it (the small sizes run them all)
BIG_TABLES = ("split_unaligned", "sweep_boundary", "sweep_boundary_around")


def check_norm_live(lib, dev, n, misalign):
    g = CC.buffer(n, misalign, dev)
    for name, ranges in tables(n):
        if n == CC.N_BIG and name not in BIG_TABLES:
            continue
        table = make_table(lib, dev, ranges, n)
        ref = live_norm64(g, ranges)
        st = CC.read_state(run_norm_live(lib, dev, g, table))
        assert abs(st.total_norm - ref) <= CC.NORM_TOL * ref, (n, misalign, name, st.total_norm, ref)
        assert abs(st.sumsq - ref * ref) <= 1e-12 * ref * ref and st.clip_coef == 1.0 and st.apply == 1
        first = CC.state_bits(run_norm_live(lib, dev, g, table, max_norm=0.25))
        assert CC.state_bits(run_norm_live(lib, dev, g, table, max_norm=0.25)) == first, (n, misalign, name, "two calls")
        state, scratch = CC.new_state(dev), CC.new_scratch(lib, n, dev)
        CC.poison(state, scratch)
        assert CC.state_bits(run_norm_live(lib, dev, g, table, max_norm=0.25, state=state, scratch=scratch)) == first, (n, name, "NaN")
        if name == "whole":   # one range = the whole buffer: the value the whole-buffer norm reports
            st0 = CC.read_state(CC.run_norm(lib, dev, g))
            assert abs(st.total_norm - st0.total_norm) <= CC.NORM_TOL * ref


def check_nonfinite_live(lib, dev, misalign):
    """A NaN, inf or -inf outside the ranges never skips the step; one inside always does."""
    n = 4097
    ranges = [(3, 1021), (1022, 1023), (2055, 4090)]   # bounds that are no multiples of 4, a one-element range, one block boundary inside
    table = make_table(lib, dev, ranges, n)
    inside = (3, 1020, 1022, 2055, 4089, 3000)
    outside = (0, 2, 1021, 1023, 2054, 4090, n - 1, 1500)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for idx in inside:
            g = CC.buffer(n, misalign, dev)
            g[idx] = bad
            st = CC.read_state(run_norm_live(lib, dev, g, table, guard=True, max_norm=1.0))
            assert st.apply == 0 and st.steps_skipped == 1 and st.steps_applied == 0, (bad, idx)
        g = CC.buffer(n, misalign, dev)
        ref = live_norm64(g, ranges)
        for idx in outside:
            g[idx] = bad
        st = CC.read_state(run_norm_live(lib, dev, g, table, guard=True))
        assert st.apply == 1 and st.steps_skipped == 0 and abs(st.total_norm - ref) <= CC.NORM_TOL * ref, bad


VARIANTS = ("plain", "guarded", "ema", "guarded_ema")


def _adam_whole(lib, dev, variant, p, g, m, v, e, state, step, sc):
    n, st = p.numel(), _stream_handle(torch.device(dev))
    lr, b1, b2, eps, wd, decay, warm = sc
    if variant == "plain":
        rc = lib.wn_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, step, lr, b1, b2, eps, wd, 0, 0, st)
    elif variant == "guarded":
        rc = lib.wn_adam_step_guarded(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, eps, wd, 0, 0, _ptr(state), st)
    elif variant == "ema":
        rc = lib.wn_adam_step_ema(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), n, step, lr, b1, b2, eps, wd, 0, 0, decay, warm, st)
    else:
        rc = lib.wn_adam_step_guarded_ema(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(e), n, eps, wd, 0, 0, _ptr(state), decay, warm, st)
    lib.check(rc, "whole-buffer " + variant)


def _adam_live(lib, dev, variant, p, g, m, v, e, table, state, step, sc):
    n, st = p.numel(), _stream_handle(torch.device(dev))
    tab, nr, n_live = table
    lr, b1, b2, eps, wd, decay, warm = sc
    ema = _ptr(e) if "ema" in variant else None
    if variant in ("plain", "ema"):
        rc = lib.wn_adam_step_live(_ptr(p), _ptr(g), _ptr(m), _ptr(v), ema, n, _ptr(tab), nr, n_live, step, lr, b1, b2, eps, wd,
                                   decay, warm, st)
    else:
        rc = lib.wn_adam_step_guarded_live(_ptr(p), _ptr(g), _ptr(m), _ptr(v), ema, n, _ptr(tab), nr, n_live, eps, wd, _ptr(state),
                                           decay, warm, st)
    lib.check(rc, "live " + variant)


def check_adam_live(lib, dev, n, misalign, only=None):
    """For each variant: live elements of p, m, v, e bit-identical to the whole-buffer entry point run on copies with the same
    scalars and state block; elements outside the ranges bit-identical to before the call, with NaN in g, m and v there."""
    sc = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.999, 1)
    step = 3
    rs = np.random.RandomState(17 + n)
    mk = lambda a: _misaligned(torch.from_numpy(np.asarray(a, np.float32)), misalign, dev)   # noqa: E731
    for name, ranges in tables(n):
        if (only is not None and name not in only) or (n == CC.N_BIG and name not in BIG_TABLES):
            continue
        table = make_table(lib, dev, ranges, n)
        live = live_mask(n, ranges)
        dead = ~live
        p0, e0 = mk(rs.standard_normal(n)), mk(rs.standard_normal(n))
        g0, m0, v0 = mk(rs.standard_normal(n)), mk(0.1 * rs.standard_normal(n)), mk(0.01 * rs.uniform(size=n))
        for buf in (g0, m0, v0):
            buf[dead.to(dev)] = float("nan")
        # the state block of the guarded variants: from the live norm, clip active
        state = CC.new_state(dev)
        state[3] = step - 1
        run_norm_live(lib, dev, g0, table, max_norm=0.5 * live_norm64(g0, ranges), guard=True, state=state, lr=sc[0], betas=sc[1:3])
        st = CC.read_state(state)
        assert st.apply == 1 and st.steps_applied == step and st.clip_coef < 1.0
        for variant in VARIANTS:
            # (a clone of a misaligned view would be a fresh, aligned tensor: both sides get the misalignment under test)
            a = [_misaligned(x.cpu(), misalign, dev) for x in (p0, g0, m0, v0, e0)]
            b = [_misaligned(x.cpu(), misalign, dev) for x in (p0, g0, m0, v0, e0)]
            assert all(x.data_ptr() % 16 == 4 * misalign for x in a + b)
            _adam_live(lib, dev, variant, *a, table, state, step, sc)
            _adam_whole(lib, dev, variant, *b, state, step, sc)
            for x, y, x0, what in zip(a, b, (p0, g0, m0, v0, e0), "pgmve"):
                assert torch.equal(bits(x)[live], bits(y)[live]), (n, misalign, name, variant, what, "live elements")
                assert torch.equal(bits(x)[dead], bits(x0)[dead]), (n, misalign, name, variant, what, "outside the ranges")
            assert not torch.equal(bits(a[0])[live], bits(p0)[live])
            assert torch.equal(bits(a[4]), bits(e0)) == ("ema" not in variant)


def _misaligned(t_cpu, misalign, dev):
    base = torch.zeros(t_cpu.numel() + 4, dtype=torch.float32, device=dev)
    assert base.data_ptr() % 16 == 0
    out = base[misalign:misalign + t_cpu.numel()]
    out.copy_(t_cpu)
    return out


def check_errors(lib, dev):
    """Every argument error sets wn_last_error."""
    def table_error(ranges, n, null=None):
        nr = len(ranges)
        flat = (ctypes.c_int64 * max(2 * nr, 1))(*[x for r in ranges for x in r])
        host = torch.zeros(max(3 * nr, 1), dtype=torch.int64)
        rc = lib.wn_live_table(None if null == "ranges" else ctypes.cast(flat, ctypes.c_void_p), nr, n,
                               None if null == "table" else ctypes.c_void_p(host.data_ptr()))
        msg = lib.wn_last_error().decode()
        assert rc == -1 and "wn_live_table" in msg, (ranges, rc, msg)
        return msg

    n = 100
    assert "NULL" in table_error([(0, 4)], n, null="ranges") and "NULL" in table_error([(0, 4)], n, null="table")
    assert "empty table" in table_error([], n)
    assert "sorted and disjoint" in table_error([(10, 20), (0, 5)], n)      # not sorted
    assert "sorted and disjoint" in table_error([(0, 10), (9, 20)], n)      # overlapping
    assert "outside" in table_error([(0, 10), (90, 101)], n) and "outside" in table_error([(-1, 10)], n)
    assert "is empty" in table_error([(5, 5)], n) and "is empty" in table_error([(7, 3)], n)
    table = make_table(lib, dev, [(0, 10), (10, 20), (50, 100)], n)   # touching ranges are allowed
    assert table[2] == 70
    tab, nr, n_live = table
    p, g, m, v, e = (torch.zeros(n, device=dev) for _ in range(5))
    state, scratch = CC.new_state(dev), CC.new_scratch(lib, n, dev)
    st = _stream_handle(torch.device(dev))

    def norm(g_=g, tab_=tab, nr_=nr, nl=n_live, scratch_=scratch, state_=state):
        return lib.wn_grad_norm_live(_ptr(g_), n, _ptr(tab_), nr_, nl, 0.0, 1, 1e-3, 0.9, 0.999, _ptr(scratch_), _ptr(state_), st)

    def adam(p_=p, tab_=tab, nr_=nr, nl=n_live, e_=None, step=1, decay=0.9):
        return lib.wn_adam_step_live(_ptr(p_), _ptr(g), _ptr(m), _ptr(v), _ptr(e_), n, _ptr(tab_), nr_, nl, step, 1e-3, 0.9, 0.999,
                                     1e-8, 0.0, decay, 1, st)

    def guarded(p_=p, tab_=tab, nr_=nr, nl=n_live, e_=None, state_=state, decay=0.9):
        return lib.wn_adam_step_guarded_live(_ptr(p_), _ptr(g), _ptr(m), _ptr(v), _ptr(e_), n, _ptr(tab_), nr_, nl, 1e-8, 0.0,
                                             _ptr(state_), decay, 1, st)

    assert norm() == 0 and adam() == 0 and guarded() == 0 and adam(e_=e) == 0 and guarded(e_=e) == 0
    for call, what in ((norm, "wn_grad_norm_live"), (adam, "wn_adam_step_live"), (guarded, "wn_adam_step_guarded_live")):
        for kw in ({"tab_": None}, {"nr_": 0}, {"nl": 0}, {"nl": n + 1}, {"nl": nr - 1}):
            assert call(**kw) != 0 and what in lib.wn_last_error().decode(), (what, kw)
    assert norm(g_=None) != 0 and norm(scratch_=None) != 0 and norm(state_=None) != 0
    assert adam(p_=None) != 0 and adam(step=0) != 0 and guarded(p_=None) != 0 and guarded(state_=None) != 0
    assert adam(e_=p) != 0 and "overlaps" in lib.wn_last_error().decode()
    assert guarded(e_=e, decay=1.0) != 0 and "ema_decay" in lib.wn_last_error().decode()
    # the engine's builder raises with the library's text
    eng = WaveNetEngine(*TINY, device=dev, library=lib)
    for bad in ([], [(5, 3)], [(10, 20), (0, 5)], [(0, eng.n_params + 1)]):
        try:
            eng.live_table(bad)
        except _lib.WnError as err:
            assert "wn_live_table" in str(err)
        else:
            raise AssertionError("live_table(%r) did not raise" % (bad,))


# ---- 4. nothing changed when nothing is frozen ---------------------------------------------------------------------------------
def check_none_is_todays_step(lib, dev, guarded):
    """``none``: the launch logs tests/clip_common.py asserts for the optimizer, and loss, gradient buffer and weights after two
    steps bit-identical to a twin engine driven through the entry points of before."""
    lr, wd = 1e-3, 1e-2
    cfg, model, _, (xd, hd, td) = tiny_model(lib, dev)
    assert apply_freeze(model, "none", TINY_LAYERS) == set()
    ts = model.trainable()
    assert ts.full and not ts.empty and ts.table is None
    eng = model.engine
    opt = FusedAdam(model, lr=lr, weight_decay=wd, skip_nonfinite=guarded)
    twin = WaveNetEngine(*TINY, device=dev, library=lib)
    twin.flat_params.copy_(eng.flat_params)
    tm, tv = torch.zeros_like(twin.flat_params), torch.zeros_like(twin.flat_params)
    tstate, tscratch = twin.new_opt_state(), twin.grad_norm_scratch()
    for step in range(2):
        loss = model.loss_and_backward(xd, hd, td)
        tloss, dl = twin.forward_loss(xd, hd, td, t_start=twin.receptive_field)
        twin.backward(dl, t_first=twin.receptive_field)
        assert torch.equal(bits(loss), bits(tloss))
        assert torch.equal(bits(eng.grads()), bits(twin.grads()))
        log = PC.launch_log(lib, opt.step)
        if guarded:
            assert log == {"grad_sumsq": 1, "grad_norm_finalize": 1, "adam_guarded": 1}, log
            twin.grad_norm(tstate, tscratch, None, True, lr)
            twin.adam_step_guarded(tm, tv, tstate, weight_decay=wd)
        else:
            assert log == {"adam": 1}, log
            twin.adam_step(tm, tv, step + 1, lr, weight_decay=wd)
        assert torch.equal(bits(eng.flat_params), bits(twin.flat_params))
    assert opt.steps_applied() == 2
    assert len(opt.state_dict()["state"]) == sum(not dead for (_, _, _, dead) in model._param_slices)


def check_frozen_launches(lib, dev):
    """A frozen set takes the live kernels, launch for launch; an empty live set issues nothing and counts no step."""
    cfg, model, _, (xd, hd, td) = tiny_model(lib, dev)
    apply_freeze(model, "bottom:1", TINY_LAYERS)
    for kw, want in ((dict(), {"adam_live": 1}), (dict(ema_decay=0.99), {"adam_ema_live": 1}),
                     (dict(skip_nonfinite=True), {"grad_sumsq_live": 1, "grad_norm_finalize": 1, "adam_guarded_live": 1}),
                     (dict(max_grad_norm=1.0, ema_decay=0.99), {"grad_sumsq_live": 1, "grad_norm_finalize": 1, "adam_guarded_ema_live": 1})):
        opt = FusedAdam(model, lr=1e-3, **kw)
        model.loss_and_backward(xd, hd, td)
        log = PC.launch_log(lib, opt.step)
        assert log == want, (kw, log)
    apply_freeze(model, "all", TINY_LAYERS)
    assert model.trainable().empty
    opt = FusedAdam(model, lr=1e-3, skip_nonfinite=True)
    p0 = bits(model.engine.flat_params)
    twin = WaveNetEngine(*TINY, device=dev, library=lib)
    twin.flat_params.copy_(model.engine.flat_params)
    forward_only = PC.launch_log(lib, lambda: twin.forward_loss(xd, hd, td, t_start=twin.receptive_field, want_grad=False))
    log = PC.launch_log(lib, lambda: model.loss_and_backward(xd, hd, td))
    assert log == forward_only, (log, forward_only)   # the log holds no backward launch
    loss = model.loss_and_backward(xd, hd, td)
    now = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref_loss, _, _ = O.train_step(cfg, now, None, *O.synthetic_batch(cfg, 2, 48, 4))
    assert abs(float(loss.cpu()) - float(ref_loss)) <= PC.TOL_LOSS
    assert all(p.grad is None for p in model.parameters())
    assert PC.launch_log(lib, opt.step) == {}
    assert opt.steps_applied() == 0 and opt.steps_skipped() == 0 and opt.state_dict()["state"] == {}
    assert torch.equal(bits(model.engine.flat_params), p0)


def check_freeze_and_train_only(lib, dev):
    cfg, model, _, _ = tiny_model(lib, dev)
    n_tensors = len(list(model.parameters()))
    assert model.freeze(r"^causal\.") == 2 and model.freeze(r"^causal\.") == 0
    assert [k for k, p in model.named_parameters() if not p.requires_grad] == ["causal.conv.weight", "causal.conv.bias"]
    changed = model.train_only(r"conv_post|skip_1x1")
    live = [k for k, p in model.named_parameters() if p.requires_grad]
    assert all(re.search(r"conv_post|skip_1x1", k) for k in live) and len(live) == 4 + 2 * TINY_LAYERS
    assert changed == n_tensors - len(live) - 2
    ts = model.trainable()
    assert len(ts.ranges) == 1 and ts.ranges[0][0] == 0 and not ts.full   # post-net and all skip_1x1 lead the flat buffer: one run
    assert model.trainable() is ts                                         # rebuilt only when the flags change
    assert model.train_only(r".") == n_tensors - len(live) and model.trainable().full
    for fn in (model.freeze, model.train_only):
        try:
            fn(r"no_such_tensor")
        except ValueError:
            pass
        else:
            raise AssertionError("a pattern that matches nothing must raise")
    # bottom(k) collapses into a few ranges
    apply_freeze(model, "bottom:2", TINY_LAYERS)
    assert 1 <= len(model.trainable().ranges) <= 4


# ---- 5. changing the set between steps ---------------------------------------------------------------------------------------------
def check_changing_set(lib, dev, guarded):
    lr = 1e-3
    cfg, model, _, (xd, hd, td) = tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, lr=lr, weight_decay=1e-2, skip_nonfinite=guarded)
    key = "dil_tanh.2.conv.weight"
    idx = [k for k, _ in model.named_parameters()].index(key)
    off, n, shape, dead = model._param_slices[idx]
    sl = slice(off, off + n)
    m, v = opt._buffers()

    def snap():
        return [bits(b[sl]) for b in (eng.flat_params, m, v)]

    def step():
        model.loss_and_backward(xd, hd, td)
        opt.step()

    s0 = snap()
    step(), step()
    s2 = snap()
    assert all(not torch.equal(a, b) for a, b in zip(s0, s2))
    assert model.freeze("^" + re.escape(key) + "$") == 1
    step(), step()
    assert all(torch.equal(a, b) for a, b in zip(s2, snap())), "frozen after two steps: weights and moments must keep their bits"
    assert dict(model.named_parameters())[key].grad is None
    dict(model.named_parameters())[key].requires_grad_(True)
    # unfrozen: it moves again FROM THE KEPT MOMENTS, with the optimizer's one step count (5) in the bias correction
    model.loss_and_backward(xd, hd, td)
    g = eng.grads()[sl].cpu().double() + 1e-2 * eng.flat_params[sl].cpu().double()
    p_before = eng.flat_params[sl].cpu().double()
    m_want = 0.9 * m[sl].cpu().double() + 0.1 * g
    v_want = 0.999 * v[sl].cpu().double() + 0.001 * g * g
    opt.step()
    p_want = p_before - lr / (1 - 0.9 ** 5) * m_want / (v_want.sqrt() / np.sqrt(1 - 0.999 ** 5) + 1e-8)
    assert float((m[sl].cpu().double() - m_want).abs().max()) <= CC.MOMENT_TOL * float(m_want.abs().max())
    assert float((v[sl].cpu().double() - v_want).abs().max()) <= CC.MOMENT_TOL * float(v_want.abs().max())
    assert float((eng.flat_params[sl].cpu().double() - p_want).abs().max()) <= PC.TOL_ADAM_REL_LR * lr
    assert not torch.equal(bits(eng.flat_params[sl]), s2[0])
    assert opt.steps_applied() == 5 and opt.steps_skipped() == 0


def check_skipped_step_trains_nothing(lib, dev):
    """``state_dict()`` carries the tensors that were trainable in an APPLIED step: a tensor whose only step in the live set was
    skipped by the non-finite guard has no entry; after one applied step it has."""
    cfg, model, _, (xd, hd, td) = tiny_model(lib, dev)
    eng = model.engine
    opt = FusedAdam(model, lr=1e-3, skip_nonfinite=True)
    keys = [k for k, _ in model.named_parameters()]
    key = "dil_tanh.2.conv.weight"
    idx = keys.index(key)
    off = model._param_slices[idx][0]
    assert model.freeze("^" + re.escape(key) + "$") == 1
    model.loss_and_backward(xd, hd, td)
    opt.step()
    n_live = sum(not dead for (_, _, _, dead) in model._param_slices)
    assert set(opt.state_dict()["state"].keys()) == {i for i, (_, _, _, dead) in enumerate(model._param_slices) if not dead and i != idx}
    dict(model.named_parameters())[key].requires_grad_(True)
    model.loss_and_backward(xd, hd, td)
    eng.grads()[off] = float("inf")          # inside the tensor that has just joined the live set: the guard skips this step
    opt.step()
    assert (opt.steps_applied(), opt.steps_skipped()) == (1, 1)
    assert idx not in opt.state_dict()["state"] and len(opt.state_dict()["state"]) == n_live - 1
    model.loss_and_backward(xd, hd, td)
    opt.step()
    assert (opt.steps_applied(), opt.steps_skipped()) == (2, 1)
    assert idx in opt.state_dict()["state"] and len(opt.state_dict()["state"]) == n_live


# ---- 6. checkpoints ------------------------------------------------------------------------------------------------------------------
def check_checkpoint(lib, dev):
    lr = 1e-3
    kw = dict(lr=lr, weight_decay=1e-2, max_grad_norm=0.05, skip_nonfinite=True)
    cfg, model, _, (xd, hd, td) = tiny_model(lib, dev)
    frozen = apply_freeze(model, "bottom:1", TINY_LAYERS)
    opt = FusedAdam(model, **kw)
    for _ in range(2):
        model.loss_and_backward(xd, hd, td)
        opt.step()
    sd = opt.state_dict()
    keys = [k for k, _ in model.named_parameters()]
    want = {i for i, (k, (_, _, _, dead)) in enumerate(zip(keys, model._param_slices)) if k not in frozen and not dead}
    assert set(sd["state"].keys()) == want and 0 < len(want) < len(keys)   # entries exactly for the tensors that trained
    assert all(float(s["step"]) == 2.0 for s in sd["state"].values())
    topt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-2)
    topt.load_state_dict(sd)
    assert set(topt.state_dict()["state"].keys()) == want
    resumed = WaveNet(*TINY, _library=lib)
    resumed.load_state_dict(model.state_dict())
    resumed.to(dev)
    apply_freeze(resumed, "bottom:1", TINY_LAYERS)
    ropt = FusedAdam(resumed, **kw)
    ropt.load_state_dict(topt.state_dict())
    assert (ropt.steps_applied(), ropt.steps_skipped()) == (2, 0)
    assert set(ropt.state_dict()["state"].keys()) == want
    for mdl, o in ((model, opt), (resumed, ropt)):
        mdl.loss_and_backward(xd, hd, td)
        o.step()
    assert torch.equal(bits(model.engine.flat_params), bits(resumed.engine.flat_params))
    live = ~frozen_mask(model)
    for a, b in zip(opt._buffers(), ropt._buffers()):
        assert torch.equal(bits(a)[live], bits(b)[live])
    assert opt.steps_applied() == 3 and ropt.steps_applied() == 3


# ---- a frozen set on a second geometry, run to run ---------------------------------------------------------------------------------
def check_run_to_run(lib, dev, cfg_tuple, B, T, name, n_layers, flags, steps=5):
    """Five steps under a freeze set, twice from the same start: bit-identical weights, moments and losses."""
    cfg = O.OracleConfig(*cfg_tuple)
    params = O.random_params(cfg, 5)
    x, h, t = (a.to(dev) for a in O.synthetic_batch(cfg, B, T, 6))
    runs = []
    for _ in range(2):
        model = WaveNet(*cfg_tuple, _library=lib)
        model.load_state_dict(params)
        model.to(dev)
        model.engine.flags |= flags
        frozen = apply_freeze(model, name, n_layers)
        opt = FusedAdam(model, lr=1e-3, weight_decay=1e-2, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.99)
        losses = []
        for _ in range(steps):
            losses.append(bits(model.loss_and_backward(x, h, t)))
            opt.step()
        assert opt.steps_applied() == steps
        runs.append([torch.cat(losses), bits(model.engine.flat_params)] + [bits(b) for b in opt._buffers()] + [bits(opt.ema)])
        sd = model.state_dict()
        for k in frozen:
            assert torch.equal(sd[k].cpu(), params[k]), k
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 3. backward plans: the pass stops at the lowest trainable layer ---------------------------------------------------------------
def bwd_plans():
    return {"default": (0, 0), "flush1": (_lib.flag_dw_flush(1), 0), "lpb1": (0, 1), "no_chain": (_lib.FLAG_NO_CHAIN, 0)}


def bwd_sets(L):
    return ["bottom:1", "bottom:%d" % (L - 1), "bottom:%d" % L, "post_frozen", "aux_only"]


def expected_needs(name, L):
    """(first_layer, needs) a freeze set must come to, written down by hand."""
    if name.startswith("bottom:"):
        return int(name.split(":")[1]), _lib.NEED_POST
    return {"post_frozen": (0, _lib.NEED_FRONT | _lib.NEED_UP), "aux_only": (0, _lib.NEED_UP), "none": (0, _lib.NEED_ALL),
            "all": (L, 0)}[name]


FRONT_TAGS = ("dw_front_scatter", "dw_front_onehot")
UP_TAGS = ("dot",)   # the upsampling bias; its weight is one more reduce_partials
HELPER_TAGS = ("reduce_partials", "dw_redo_if_overflow", "copy4")   # the launches that follow every weight-gradient contraction


def check_backward_plans(shape, flag_set, lib, dev, plans=None):
    """One shape of tests/plan_common.py under one arithmetic: every plan (or those named in ``plans``) x every freeze set against
    the oracle, the full pass on the same inputs and the launch log."""
    from tests import aux_grad_common as AG
    from tests import plan_common as PL
    from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS, flat_to_state, load_state_into_flat
    cfg, B, T = PL.SHAPES[shape]
    base = {"default": DEFAULT_FLAGS, "six_product": SIX_PRODUCT_FLAGS}[flag_set]
    params, x, h, t, loss_ref, logits_ref, grads_ref = PL.reference(tuple(cfg), B, T, PL.SEED)
    ocfg = O.OracleConfig(*cfg)
    shapes = O.param_shapes(ocfg)
    keys = list(shapes.keys())
    L = len(ocfg.dilations)
    chain_shape = shape != "P4"
    # the model derives what the hand-written table says
    model = WaveNet(*cfg, _library=lib)
    for name in bwd_sets(L) + ["none", "all"]:
        apply_freeze(model, name, L)
        ts = model.trainable()
        assert (ts.first_layer, ts.needs) == expected_needs(name, L), (name, ts.first_layer, ts.needs)
    xd, hd, td = x.to(dev), h.to(dev), t.to(dev)
    for plan, (extra, lpb) in bwd_plans().items():
        if plans is not None and plan not in plans:
            continue
        eng = WaveNetEngine(*cfg, device=dev, library=lib)
        eng.flags = base | extra
        load_state_into_flat(eng, params)
        loss, dl = eng.forward_loss(xd, hd, td)
        assert abs(float(loss.cpu()) - float(loss_ref)) <= PC.TOL_LOSS
        tf = eng.receptive_field
        out = {}

        def run(**kw):
            eng.grads().fill_(float("nan"))
            log = PC.launch_log(lib, lambda: out.__setitem__("g", eng.backward(dl, layers_per_bucket=lpb, t_first=tf, **kw)))
            return out["g"].detach().cpu().clone(), log

        full_flat, full_log = run()
        full = flat_to_state(eng, full_flat, shapes)
        chain_on = chain_shape and plan != "no_chain" and full_log.get("fused_bwd_chain", 0) > 0
        if chain_shape and plan != "no_chain":
            assert full_log.get("fused_bwd_chain", 0) == L - 1, (shape, plan, full_log)
        for name in bwd_sets(L):
            what = "%s %s %s %s" % (shape, flag_set, plan, name)
            fl, needs = expected_needs(name, L)
            frozen = frozen_keys(name, keys, L)
            flat, log = run(first_layer=fl, needs=needs)
            got = flat_to_state(eng, flat, shapes)
            for k in keys:
                if k in frozen or grads_ref[k] is None:
                    continue
                assert bool(torch.isfinite(got[k]).all()), "%s: %s not finite (never written?)" % (what, k)
                e = PC.rel_to_max(got[k], grads_ref[k])
                assert e <= PC.TOL_GRAD, "%s: %s grad rel err %g" % (what, k, e)
                if plan == "flush1":   # every flush group is one layer: the full pass's bits
                    assert torch.equal(got[k].view(torch.int32), full[k].view(torch.int32)), "%s: %s differs from the full pass" % (what, k)
            # what the log shows
            if name.startswith("bottom:"):
                if chain_on:
                    assert log.get("fused_bwd_chain", 0) == max(L - 1 - fl, 0), (what, log)
                    assert log.get("fused_bwd_gate", 0) == (1 if fl < L else 0), (what, log)   # the chain head
                assert not any(tag in log for tag in FRONT_TAGS + UP_TAGS), (what, log)
                assert log.get("fused_bwd_dx", 0) == max(full_log.get("fused_bwd_dx", 0) - fl - 1, 0) or chain_on, (what, log)
                assert log.get("bwd_dx_dilated", 0) == max(full_log.get("bwd_dx_dilated", 0) - fl - 1, 0), (what, log)
                assert log.get("dw_post1", 0) == full_log["dw_post1"] and log.get("dw_post2", 0) == full_log["dw_post2"]
                assert log.get("dw_dilated", 0) <= full_log["dw_dilated"] and (fl < L) == ("dw_dilated" in log), (what, log)
                if fl == L:
                    assert not any(tag.startswith(("fused_bwd", "bwd_dz", "bwd_dx", "dw_dil", "dw_skip", "dw_res", "dw_aux", "aux_",
                                                   "gate_bwd")) for tag in log), (what, log)
            elif name == "post_frozen":
                assert "dw_post1" not in log and "dw_post2" not in log, (what, log)
                gone = ("dw_post1", "dw_post2") + HELPER_TAGS   # nothing else falls away
                assert {k: v for k, v in full_log.items() if k not in gone} == {k: v for k, v in log.items() if k not in gone}, (what, log, full_log)
            else:   # aux_only: every layer is computed -- the full pass's chain and per-layer launches; the post-net weight
                    # gradients, the front-conv gradient and the dX_0 launch that feeds it belong to frozen tensors alone
                gone = ("dw_post1", "dw_post2", "fused_bwd_dx", "bwd_dx_dilated") + FRONT_TAGS + HELPER_TAGS
                assert {k: v for k, v in full_log.items() if k not in gone} == {k: v for k, v in log.items() if k not in gone}, (what, log, full_log)
                assert not any(tag in log for tag in FRONT_TAGS + ("dw_post1", "dw_post2")), (what, log)
                for tag in ("fused_bwd_dx", "bwd_dx_dilated"):
                    assert log.get(tag, 0) == max(full_log.get(tag, 0) - 1, 0), (what, tag, log)
        # dh requested: bottom(k) runs the full chain, and dh is the full pass's
        hshape = hd.shape
        dh_full = torch.empty(hshape, dtype=torch.float32, device=dev)
        eng.backward(dl, layers_per_bucket=lpb, t_first=tf, dh=dh_full)
        dh = torch.full(hshape, float("nan"), dtype=torch.float32, device=dev)
        _, log = run(dh=dh, first_layer=0, needs=_lib.NEED_POST)
        if chain_on:
            assert log.get("fused_bwd_chain", 0) == L - 1, (shape, plan, log)
        assert torch.equal(bits(dh), bits(dh_full)), (shape, plan, "dh")
        e = PC.rel_to_max(dh.cpu(), AG.instance(shape)[4])   # the gate of tests/aux_grad_common.py: the oracle's dh in fp64
        assert e <= PC.TOL_GRAD, (shape, plan, "dh", e)
        try:
            eng.backward(dl, t_first=tf, dh=dh, first_layer=1, needs=_lib.NEED_POST)
        except _lib.WnError as err:
            assert "first_layer" in str(err)
        else:
            raise AssertionError("first_layer > 0 with dh must be refused")

