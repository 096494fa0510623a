# -*- coding: utf-8 -*-
"""Training on padded batches of unequal length (``lengths=``): checks shared by tests/test_emu_ragged.py (host emulator) and
tests/test_gpu_ragged.py (MI355X).

The definition under test: the loss positions of sequence b are ``[t_start, lengths[b])``, ``N`` is their count over the batch,
``loss = sum / N`` and ``dlogits`` is exactly zero everywhere else -- ``nn.CrossEntropyLoss()`` (the reference's own loss object)
with the targets behind each end set to its default ``ignore_index`` -100.  The checkers are the reference module itself
(tests/golden/ragged.npz) and the oracle's forward in fp64 with that torch loss computed here.  Gates: the project's own
``PC.TOL_LOSS``, ``PC.TOL_GRAD`` (worst tensor relative to its maximum) and ``PC.TOL_LOGITS``."""
import ctypes
import functools
import os

import numpy as np
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS, WaveNetEngine, _ptr, flat_to_state, load_state_into_flat
from pytorchwavenetvocoder_amd.nets import WaveNet
from tests import mol_common as MC
from tests import parity_common as PC
from tests import plan_common as PL
from tests.golden_util import rel_to_max

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ragged.npz")

# id -> (cfg, B, T, lengths).  F1 / F2: 128..256 classes, the cross-entropy is the epilogue of conv_post_2 (T = 144 / 160: a
# second, partly filled 128-column tile; one sequence ends inside the first tile).  P1 / P3 / P4 / N1: the plan shapes (32
# classes: k_softmax_ce through the logits scratch) -- the K = 3 chain, the any-size path, no upsampling layer.
SHAPES = {
    "F1": ((256, 6, 64, 128, 2, 1, 2, 16), 2, 144, (144, 96)),
    "F2": ((200, 4, 64, 128, 2, 1, 2, 0), 2, 160, (70, 160)),
    "P1": (PL.SHAPES["P1"][0], 1, 256, (200,)),
    "P3": (PL.SHAPES["P3"][0], 1, 256, (131,)),
    "P4": (PL.SHAPES["P4"][0], 2, 128, (128, 72)),
    "N1": ((32, 4, 64, 256, 3, 1, 2, 0), 1, 256, (180,)),
}
FLAG_SETS = {"default": DEFAULT_FLAGS, "six": SIX_PRODUCT_FLAGS}


def masked_targets(t, lengths):
    """``t`` with torch's ``ignore_index`` (-100) from every sequence's end on."""
    tm = t.clone()
    for b, n in enumerate(lengths):
        tm[b, int(n):] = -100
    return tm


def loss_positions(B, T, lengths, t_start):
    """bool (B, T): True on the positions that carry loss."""
    m = torch.zeros(B, T, dtype=torch.bool)
    for b, n in enumerate(lengths):
        m[b, t_start:int(n)] = True
    return m


def frames_behind(cfg_t, B, T, lengths):
    """bool (B, F): True on the aux frames that lie wholly behind their sequence's end (F = T / U, or T without upsampling)."""
    U = cfg_t[7] if cfg_t[7] > 0 else 1
    f0 = torch.arange(T // U) * U
    return torch.stack([f0 >= int(n) for n in lengths])


def oracle_ragged(cfg_t, params, x, h, t, lengths, dtype=torch.float64, t_start=None):
    """The oracle's forward in ``dtype`` + nn.CrossEntropyLoss() with -100 targets behind each length (computed here; the oracle
    is not edited).  Returns (loss, {name: gradient or None}, dh, logits (B, T, Q)) as fp32 tensors / a float."""
    cfg = O.OracleConfig(*cfg_t)
    rf = cfg.receptive_field if t_start is None else t_start
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    hv = h.detach().to(dtype).requires_grad_(True)
    logits = O.forward(cfg, leaves, x, hv)
    tm = masked_targets(t, lengths)
    loss = torch.nn.CrossEntropyLoss()(logits[:, rf:].contiguous().view(-1, cfg.n_quantize), tm[:, rf:].contiguous().view(-1))
    gl = torch.autograd.grad(loss, list(leaves.values()) + [hv], allow_unused=True)
    grads = {k: (None if g is None else g.float()) for k, g in zip(leaves.keys(), gl[:-1])}
    return float(loss.detach()), grads, gl[-1].float(), logits.detach().float()


@functools.lru_cache(maxsize=16)
def instance(shape):
    """Seeded instance of a shape (ReLU kink margin >= PC.KINK_MARGIN over the whole rectangle) and its fp64 reference."""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, margin, sd = PC.pick_instance(O.OracleConfig(*cfg_t), B, T, PL.SEED, 0.1)
    return params, x, h, t, oracle_ragged(cfg_t, params, x, h, t, lengths)


def engine_for(cfg_t, params, lib, device, flags, out_channels=0):
    eng = WaveNetEngine(*cfg_t, device=device, library=lib, out_channels=out_channels)
    eng.flags = flags
    load_state_into_flat(eng, params)
    return eng


def step(eng, x, h, t, lengths, device, **kw):
    """forward_loss(lengths=) + backward with dh on a NaN-poisoned gradient buffer; everything back on the CPU."""
    loss, dl = eng.forward_loss(x.to(device), h.to(device), t.to(device), lengths=lengths, **kw)
    eng.grads().fill_(float("nan"))
    dh = torch.full(h.shape, float("nan"), dtype=torch.float32, device=device)
    g = eng.backward(dl, t_first=kw.get("t_start", eng.receptive_field), dh=dh)
    return loss.cpu().clone(), dl.cpu().clone(), g.cpu().clone(), dh.cpu().clone()


def assert_gates(tag, cfg_t, eng, loss, flat, dh, ref, report=None):
    """loss, every gradient tensor and dh against a reference (loss, grads, dh) within PC.TOL_LOSS / PC.TOL_GRAD."""
    loss_ref, grads_ref, dh_ref = ref[0], ref[1], ref[2]
    e_loss = abs(float(loss) - loss_ref)
    grads = flat_to_state(eng, flat, O.param_shapes(O.OracleConfig(*cfg_t)))
    worst, worst_k = 0.0, None
    for k, r in grads_ref.items():
        if r is None:
            assert float(grads[k].abs().max()) == 0.0, (tag, k)
            continue
        e = rel_to_max(grads[k], r)
        if e > worst:
            worst, worst_k = e, k
    assert bool(torch.isfinite(dh).all()), tag
    e_dh = rel_to_max(dh, dh_ref)
    print("%s: loss err %.3g, worst gradient %.3g (%s), dh %.3g" % (tag, e_loss, worst, worst_k, e_dh))
    if report is not None:
        report[tag] = {"loss": e_loss, "grad": worst, "grad_key": worst_k, "dh": e_dh}
    assert e_loss <= PC.TOL_LOSS, (tag, e_loss)
    assert worst <= PC.TOL_GRAD, (tag, worst_k, worst)
    assert e_dh <= PC.TOL_GRAD, (tag, e_dh)


def assert_exact_zeros(tag, cfg_t, B, T, lengths, t_start, dl, dh):
    live = loss_positions(B, T, lengths, t_start)
    dead = (~live)[:, None, :].expand_as(dl)
    if bool(dead.any()):
        assert float(dl[dead].abs().max()) == 0.0, "%s: dlogits outside the loss positions" % tag
    behind = frames_behind(cfg_t, B, T, lengths)[:, None, :].expand_as(dh)
    if bool(behind.any()):
        assert float(dh[behind].abs().max()) == 0.0, "%s: dh behind a sequence's end" % tag


def check_oracle(shape, arith, lib, device):
    """forward_loss(lengths=) + backward against the fp64 oracle; logits of the same engine within PC.TOL_LOGITS; exact zeros."""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, ref = instance(shape)
    eng = engine_for(cfg_t, params, lib, device, FLAG_SETS[arith])
    logits = eng.forward(x.to(device), h.to(device))
    e_lg = float((logits.transpose(1, 2).cpu() - ref[3]).abs().max())
    assert e_lg <= PC.TOL_LOGITS, (shape, arith, e_lg)
    loss, dl, g, dh = step(eng, x, h, t, lengths, device)
    assert_gates("%s/%s" % (shape, arith), cfg_t, eng, loss, g, dh, ref)
    assert_exact_zeros("%s/%s" % (shape, arith), cfg_t, B, T, lengths, eng.receptive_field, dl, dh)


def golden_cases():
    z = np.load(GOLDEN)
    for i in range(int(z["n_cases"])):
        cfg_t = tuple(int(v) for v in z["c%d/cfg" % i])
        B, T = int(z["c%d/B" % i]), int(z["c%d/T" % i])
        lengths = [int(v) for v in z["c%d/lengths" % i]]
        cfg = O.OracleConfig(*cfg_t)
        sd = int(z["c%d/seed" % i])
        params = O.random_params(cfg, sd, scale=float(z["scale"]))
        x, h, t = O.synthetic_batch(cfg, B, T, sd + 1)
        grads = {}
        for k in O.param_shapes(cfg):
            key = "c%d/g/%s" % (i, k)
            grads[k] = torch.from_numpy(z[key]) if key in z.files else None
        yield cfg_t, B, T, lengths, params, x, h, t, (float(z["c%d/loss" % i]), grads, torch.from_numpy(z["c%d/dh" % i]))


def check_golden(lib, device, arith="default"):
    """WaveNet.loss_and_backward(lengths=, aux_grad=True) against the reference module's own loss, gradients and dL/dh."""
    n = 0
    for cfg_t, B, T, lengths, params, x, h, t, ref in golden_cases():
        model = WaveNet(*cfg_t, _library=lib)
        model.load_state_dict(params)
        model.to(device)
        model.engine.flags = FLAG_SETS[arith]
        if cfg_t[0] >= 128:
            assert model.engine.lib.wn_forward_loss_fused(ctypes.byref(model.engine.cfg), B, T, model.engine.flags) == 1
        logits = model(x.to(device), h.to(device))
        ref_logits = oracle_logits(cfg_t, params, x, h)
        assert float((logits.detach().cpu() - ref_logits).abs().max()) <= PC.TOL_LOGITS
        loss, dh = model.loss_and_backward(x.to(device), h.to(device), t.to(device), lengths=lengths, aux_grad=True)
        for k, p in model.named_parameters():
            assert (p.grad is None) == (ref[1][k] is None), k
        assert_gates("golden%d/%s" % (n, arith), cfg_t, model.engine, loss.cpu(), model.engine.grads().cpu().clone(), dh.cpu(), ref)
        behind = frames_behind(cfg_t, B, T, lengths)[:, None, :].expand_as(dh)
        assert float(dh.cpu()[behind].abs().max()) == 0.0
        assert float(ref[2][behind].abs().max()) == 0.0   # the reference's own dL/dh is zero there too
        n += 1
    assert n >= 2


def oracle_logits(cfg_t, params, x, h):
    with torch.no_grad():
        return O.forward(O.OracleConfig(*cfg_t), params, x, h)


def check_routes_agree(shape, lib, device):
    """The fused epilogue, forward + k_softmax_ce, and autograd with torch's masked loss: the bounds the dense test of the
    epilogue uses (tests/test_emu_parity.py test_cross_entropy_as_the_epilogue_of_conv_post_2)."""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, ref = instance(shape)
    eng = engine_for(cfg_t, params, lib, device, DEFAULT_FLAGS)
    assert eng.lib.wn_forward_loss_fused(ctypes.byref(eng.cfg), B, T, eng.flags) == 1
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    logits = eng.forward(xd, hd)
    loss0, dl0 = eng.loss(logits, td, grad_scale=0.5, lengths=lengths)
    loss1, dl1 = eng.forward_loss(xd, hd, td, grad_scale=0.5, lengths=lengths)
    g1 = eng.backward(dl1, t_first=eng.receptive_field).clone()
    eng.forward(xd, hd)
    g0 = eng.backward(dl0, t_first=eng.receptive_field).clone()
    assert abs(float(loss1.cpu()) - float(loss0.cpu())) <= 2e-6 * max(1.0, abs(float(loss0.cpu())))
    assert float((dl1 - dl0).abs().max()) <= 1e-5 * float(dl0.abs().max())
    assert float((g1 - g0).abs().max()) <= 5e-6 * float(g0.abs().max())
    assert abs(float(loss1.cpu()) - ref[0]) <= PC.TOL_LOSS
    # autograd: model(x, h), torch's loss object with ignored targets, backward
    model = WaveNet(*cfg_t, _library=lib)
    model.load_state_dict(params)
    model.to(device)
    out = model(xd, hd)
    rf, Q = model.receptive_field, cfg_t[0]
    tm = masked_targets(t, lengths).to(device)
    loss2 = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, Q), tm[:, rf:].contiguous().view(-1)) * 0.5
    loss2.backward()
    assert abs(2.0 * float(loss2.detach().cpu()) - float(loss0.cpu())) <= 2e-6 * max(1.0, abs(float(loss0.cpu())))
    g2 = model.engine.grads()
    assert float((g2 - g0).abs().max()) <= 5e-6 * float(g0.abs().max())


def check_fused_form_kept(shape, lib, device):
    """The launch sequence of a ragged loss_and_backward equals the dense one of the same (B, T)."""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, ref = instance(shape)
    model = WaveNet(*cfg_t, _library=lib)
    model.load_state_dict(params)
    model.to(device)
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    model.loss_and_backward(xd, hd, td)   # (allocate the workspace outside the logs)
    dense = PC.launch_sequence(model.engine.lib, lambda: model.loss_and_backward(xd, hd, td))
    ragged = PC.launch_sequence(model.engine.lib, lambda: model.loss_and_backward(xd, hd, td, lengths=lengths))
    assert ragged == dense, (dense, ragged)
    assert "fwd_post2_ce" in ragged and "softmax_ce" not in ragged, ragged


def parent_call(eng, x, h, t, t_start, grad_scale=1.0):
    """The dense C entry point as the parent commit's engine called it (wn_forward_loss, no lengths anywhere)."""
    B, T = x.shape
    cfg = ctypes.byref(eng.cfg)
    fused = bool(eng.lib.wn_forward_loss_fused(cfg, B, T, eng.flags))
    ws = eng.workspace(B, T)
    loss = torch.empty(1, dtype=torch.float32, device=eng.device)
    dl = torch.empty((B, eng.out_channels, T), dtype=torch.float32, device=eng.device)
    scratch = None if fused else torch.empty_like(dl)
    from pytorchwavenetvocoder_amd import _lib
    from pytorchwavenetvocoder_amd.engine import _stream_handle
    rc = eng.lib.wn_forward_loss(cfg, B, T, _ptr(eng.flat_params), _ptr(x), _ptr(h), _ptr(t), int(t_start), float(grad_scale), 1.0,
                                 _ptr(loss), _ptr(dl), _ptr(scratch), _ptr(ws), ws.numel() * 4,
                                 eng.flags | (_lib.FLAG_WS_FINITE if eng.ws_finite else 0), _stream_handle(eng.device))
    eng.lib.check(rc, "wn_forward_loss")
    return loss, dl


def check_nothing_moved(shape, arith, lib, device):
    """lengths=None, lengths=[T] * B and the dense entry point itself: torch.equal loss, dlogits, gradients and dh."""
    cfg_t, B, T, _ = SHAPES[shape]
    params, x, h, t, ref = instance(shape)
    eng = engine_for(cfg_t, params, lib, device, FLAG_SETS[arith])
    base = step(eng, x, h, t, None, device)
    full = step(eng, x, h, t, [T] * B, device)
    full_t = step(eng, x, h, t, torch.tensor([T] * B), device)
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    eng.forward_loss(xd, hd, td)   # (sets the engine's forward state for the backward below)
    loss_p, dl_p = parent_call(eng, xd, hd, td, eng.receptive_field)
    dh = torch.full(h.shape, float("nan"), dtype=torch.float32, device=device)
    g_p = eng.backward(dl_p, t_first=eng.receptive_field, dh=dh)
    parent = (loss_p.cpu(), dl_p.cpu(), g_p.cpu().clone(), dh.cpu())
    for name, other in (("[T] * B", full), ("tensor [T] * B", full_t), ("dense entry point", parent)):
        for what, a, b in zip(("loss", "dlogits", "gradients", "dh"), base, other):
            assert torch.equal(a, b), (shape, arith, name, what)
    # and the dense loss entry point on materialised logits
    logits = eng.forward(xd, hd)
    l0, d0 = eng.loss(logits, td)
    l1, d1 = eng.loss(logits, td, lengths=[T] * B)
    assert torch.equal(l0, l1) and torch.equal(d0, d1)


def padding_fills(cfg_t, B, T, lengths, x, h, t, seed):
    """The batch with the padding (tokens, aux frames wholly behind the end, targets) overwritten by seeded finite values;
    targets get every kind of value the kernels take modulo n_quantize, -100 among them."""
    rs = np.random.RandomState(seed)
    Q = cfg_t[0]
    x2, h2, t2 = x.clone(), h.clone(), t.clone()
    behind = frames_behind(cfg_t, B, T, lengths)
    for b, n in enumerate(lengths):
        n = int(n)
        if n >= T:
            continue
        x2[b, n:] = torch.from_numpy(rs.randint(0, Q, size=T - n))
        t2[b, n:] = torch.from_numpy(rs.choice([-100, -1, 0, Q - 1, Q, 3 * Q + 5, Q // 2], size=T - n))
        nf = int(behind[b].sum())
        if nf:
            h2[b][:, behind[b]] = torch.from_numpy((3.0 * rs.standard_normal((h.shape[1], nf))).astype(np.float32))
    return x2, h2, t2


def check_padding_content(shape, arith, lib, device):
    """Two different finite fills of the padding meet the gates against the SAME reference; bit-equal under the six-product
    arithmetic (the block-scaled fp16 forward may round a valid position differently when its tile also holds padding)."""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, ref = instance(shape)
    eng = engine_for(cfg_t, params, lib, device, FLAG_SETS[arith])
    results = []
    for seed in (101, 202):
        x2, h2, t2 = padding_fills(cfg_t, B, T, lengths, x, h, t, seed)
        assert not torch.equal(x2, x) and not torch.equal(t2, t)
        loss, dl, g, dh = step(eng, x2, h2, t2, lengths, device)
        assert_gates("%s/%s/fill%d" % (shape, arith, seed), cfg_t, eng, loss, g, dh, ref)
        assert_exact_zeros("%s/%s/fill%d" % (shape, arith, seed), cfg_t, B, T, lengths, eng.receptive_field, dl, dh)
        results.append((loss, dl, g, dh))
    if arith == "six":
        for what, a, b in zip(("loss", "dlogits", "gradients", "dh"), results[0], results[1]):
            assert torch.equal(a, b), (shape, what)


def mol_instance():
    cfg = O.OracleConfig(*MC.CFG, out_channels=3 * MC.NM)
    B, T, lengths = 3, 48, (48, 31, 5)
    params, x, h, seed = MC._kink_free_instance(cfg, B, T)
    y = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (B, T)).astype(np.float32))
    return cfg, B, T, lengths, params, x, h, y


def mol_oracle(cfg, params, x, h, y, lengths, dt):
    """The restatement of tests/mol_common.py (O.mol_nll), masked the same way: the sum over [rf, lengths[b]) over N."""
    rf = cfg.receptive_field
    p = {k: v.clone().to(dt).requires_grad_(True) for k, v in params.items()}
    hv = h.to(dt).requires_grad_(True)
    out = O.forward(cfg, p, x, hv)
    total, n = 0.0, 0
    for b, ln in enumerate(lengths):
        if ln > rf:
            total = total + O.mol_nll(out[b:b + 1, :ln], y[b:b + 1, :ln].to(dt), start=rf) * (ln - rf)
            n += ln - rf
    loss = total / n
    gl = torch.autograd.grad(loss, list(p.values()) + [hv], allow_unused=True)
    grads = {k: (None if g is None else g.float()) for k, g in zip(p.keys(), gl[:-1])}
    return float(loss.detach()), grads, gl[-1].float()


def check_mol(lib, device):
    """mol_loss_and_backward(lengths=) against the fp64 restatement, with the allowance check_mol_dh makes for the fp32 error of
    the formula itself; a second fill of the padding (y included) stays inside the same gate."""
    cfg, B, T, lengths, params, x, h, y = mol_instance()
    l64, g64, dh64 = mol_oracle(cfg, params, x, h, y, lengths, torch.float64)
    l32, g32, dh32 = mol_oracle(cfg, params, x, h, y, lengths, torch.float32)
    model = WaveNet(*MC.CFG, n_mixture=MC.NM, _library=lib)
    model.load_state_dict(params)
    model.to(device)
    for fill in (None, 7):
        x2, h2, y2 = x, h, y
        if fill is not None:
            x2, h2, _ = padding_fills(MC.CFG, B, T, lengths, x, h, x, fill)
            y2 = y.clone()
            for b, n in enumerate(lengths):
                y2[b, n:] = torch.from_numpy(np.random.RandomState(fill + b).uniform(-1, 1, T - n).astype(np.float32))
        loss, dh = model.mol_loss_and_backward(x2.to(device), h2.to(device), y2.to(device), lengths=lengths, aux_grad=True)
        assert abs(float(loss.cpu()) - l64) <= 1e-4 * abs(l64)
        ek, eo = rel_to_max(dh.cpu(), dh64), rel_to_max(dh32, dh64)
        assert ek <= PC.TOL_GRAD + eo, (ek, eo)
        for k, p in model.named_parameters():
            if p.grad is None:
                assert g64[k] is None or float(g64[k].abs().max()) == 0.0, k
                continue
            ek, eo = rel_to_max(p.grad.cpu(), g64[k]), rel_to_max(g32[k], g64[k])
            assert ek <= PC.TOL_GRAD + eo, (k, ek, eo)
        behind = frames_behind(MC.CFG, B, T, lengths)[:, None, :].expand_as(dh)
        assert float(dh.cpu()[behind].abs().max()) == 0.0
    # dout itself: exact zeros outside the loss positions
    eng = model.engine
    out = eng.forward(x.to(device), h.to(device))
    _, dout = eng.mol_loss(out, y.to(device), lengths=lengths)
    dead = (~loss_positions(B, T, lengths, eng.receptive_field))[:, None, :].expand_as(dout)
    assert float(dout.cpu()[dead].abs().max()) == 0.0


def check_errors(lib, device):
    """Every misuse raises (Python) or returns non-zero (C ABI) with a message that names the argument."""
    import pytest
    cfg_t, B, T, lengths = SHAPES["F1"]
    params, x, h, t, ref = instance("F1")
    eng = engine_for(cfg_t, params, lib, device, DEFAULT_FLAGS)
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    rf = eng.receptive_field
    logits = eng.forward(xd, hd)
    calls = (lambda ln: eng.forward_loss(xd, hd, td, lengths=ln), lambda ln: eng.loss(logits, td, lengths=ln))
    for call in calls:
        with pytest.raises(ValueError, match="N == 0"):
            call([rf, 1])
        with pytest.raises(ValueError, match=r"lengths\[1\]"):
            call([T, 0])
        with pytest.raises(ValueError, match=r"lengths\[0\]"):
            call([T + 1, T])
        with pytest.raises(ValueError, match="lengths must have one entry per sequence"):
            call([T])
        with pytest.raises(ValueError, match="lengths must have one entry per sequence"):
            call(torch.tensor([[T, T]]))
        with pytest.raises(ValueError, match="lengths must be integers"):
            call([float(T) - 0.5, T])
        with pytest.raises(ValueError, match="lengths must be integers"):
            call(torch.tensor([1.0, 2.0]))
    if device != "cpu":
        with pytest.raises(ValueError, match="lengths must be host integers"):
            eng.forward_loss(xd, hd, td, lengths=torch.tensor(lengths, device=device))
    else:
        with pytest.raises(ValueError, match="lengths must be host integers"):
            eng.forward_loss(xd, hd, td, lengths=torch.tensor(lengths, device="meta"))
    model = WaveNet(*cfg_t, _library=lib)
    model.to(device)
    with pytest.raises(ValueError, match="N == 0"):
        model.loss_and_backward(xd, hd, td, lengths=[1, 2])
    # the C ABI itself
    ws = eng.workspace(B, T)
    loss = torch.empty(1, dtype=torch.float32, device=device)
    t_end = torch.tensor(lengths, dtype=torch.int32).to(device)
    n_ok = sum(max(n - rf, 0) for n in lengths)
    from pytorchwavenetvocoder_amd.engine import _stream_handle
    st = _stream_handle(eng.device)

    def c_forward_loss(te, n):
        rc = eng.lib.wn_forward_loss_ragged(ctypes.byref(eng.cfg), B, T, _ptr(eng.flat_params), _ptr(xd), _ptr(hd), _ptr(td), rf,
                                            _ptr(te), n, 1.0, 1.0, _ptr(loss), None, None, _ptr(ws), ws.numel() * 4, eng.flags, st)
        return rc, eng.lib.wn_last_error().decode()

    def c_ce(te, n):
        rc = eng.lib.wn_softmax_ce_loss_ragged(ctypes.byref(eng.cfg), B, T, _ptr(logits), _ptr(td), rf, _ptr(te), n, 1.0, 1.0,
                                               _ptr(loss), None, _ptr(ws), ws.numel() * 4, st)
        return rc, eng.lib.wn_last_error().decode()

    for c in (c_forward_loss, c_ce):
        rc, err = c(t_end, 0)
        assert rc != 0 and "n_loss" in err, (rc, err)
        rc, err = c(None, n_ok)
        assert rc != 0 and "n_loss" in err and "t_end" in err, (rc, err)
        rc, err = c(t_end, B * (T - rf) + 1)
        assert rc != 0 and "n_loss" in err, (rc, err)
        rc, err = c(t_end, n_ok)
        assert rc == 0, err
        assert abs(float(loss.cpu()) - ref[0]) <= PC.TOL_LOSS
        rc, err = c(None, B * (T - rf))
        assert rc == 0, err
    mcfg, mB, mT, mlengths, mparams, mx, mh, my = mol_instance()
    meng = engine_for(MC.CFG, mparams, lib, device, DEFAULT_FLAGS, out_channels=3 * MC.NM)
    mout = meng.forward(mx.to(device), mh.to(device))
    mws = meng.workspace(mB, mT)
    myd = my.to(device)
    rc = meng.lib.wn_mol_loss_ragged(ctypes.byref(meng.cfg), mB, mT, _ptr(mout), _ptr(myd), meng.receptive_field, None, 5, 1.0, 1.0,
                                     65536, -7.0, _ptr(loss), None, _ptr(mws), mws.numel() * 4, st)
    err = meng.lib.wn_last_error().decode()
    assert rc != 0 and "n_loss" in err and "t_end" in err, (rc, err)
    with pytest.raises(ValueError, match="N == 0"):
        meng.mol_loss(mout, myd, lengths=[1, 1, 1])


def spread_lengths(rf, B, T):
    """B lengths from just above the receptive field to T, evenly spread."""
    return [rf + 1 + (i * (T - rf - 1)) // (B - 1) for i in range(B)]


def check_fullsize(cfg_t, B, T, seed, lib, device, scale=0.05, threads=32):
    """The ragged training step at a size where ReLU kinks are certain, against the oracle on the CPU by the method of
    PC.run_fullsize_vs_oracle: the oracle back-propagates through its two ReLUs with the HIP path's own (output > 0) masks, and
    every loss position where that choice differs from the oracle's own sign must be within 1e-5 of the kink."""
    from pytorchwavenetvocoder_amd import _lib
    cfg = O.OracleConfig(*cfg_t)
    rf = cfg.receptive_field
    lengths = spread_lengths(rf, B, T)
    assert lengths[0] == rf + 1 and lengths[-1] == T
    params = O.random_params(cfg, seed, scale=scale)
    x, h, t = O.synthetic_batch(cfg, B, T, seed + 1)
    x, h, t = padding_fills(cfg_t, B, T, lengths, x, h, t, seed + 2)
    eng = engine_for(cfg_t, params, lib, device, DEFAULT_FLAGS)
    assert eng.lib.wn_forward_loss_fused(ctypes.byref(eng.cfg), B, T, eng.flags) == 1
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    loss, dl = eng.forward_loss(xd, hd, td, lengths=lengths)
    m_skip = (eng.saved(_lib.WS_RELU_SKIP) > 0).float().cpu()
    m_post = (eng.saved(_lib.WS_RELU_POST1) > 0).float().cpu()
    eng.grads().fill_(float("nan"))
    dh = torch.full(h.shape, float("nan"), dtype=torch.float32, device=device)
    g = eng.backward(dl, t_first=rf, dh=dh).cpu().clone()
    live = loss_positions(B, T, lengths, rf)
    assert float(dl.masked_fill(live.to(device)[:, None, :], 0.0).abs().max()) == 0.0, "dlogits outside the loss positions"
    assert float(dl.abs().max()) > 0.0
    del dl
    try:
        navail = len(os.sched_getaffinity(0))
    except AttributeError:
        navail = os.cpu_count() or 1
    old_threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(threads, navail)))   # as PC.run_fullsize_vs_oracle
    try:
        leaves = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
        hv = h.detach().clone().requires_grad_(True)
        logits, inter = O.forward(cfg, leaves, x, hv, return_intermediates=True, relu_masks=(m_skip, m_post))
        tm = masked_targets(t, lengths)
        loss_ref = torch.nn.CrossEntropyLoss()(logits[:, rf:].contiguous().view(-1, cfg.n_quantize), tm[:, rf:].contiguous().view(-1))
        gl = torch.autograd.grad(loss_ref, list(leaves.values()) + [hv], allow_unused=True)
    finally:
        torch.set_num_threads(old_threads)
    flips = 0
    for pre, m in ((inter["skip_sum"].detach(), m_skip), (inter["post1_pre"].detach(), m_post)):
        differ = ((pre > 0).float() != m) & live[:, None, :]
        n = int(differ.sum())
        flips += n
        if n:
            assert float(pre[differ].abs().max()) <= 1e-5, "ReLU mask differs from the oracle's away from the kink"
    grads_ref = {k: gg for k, gg in zip(leaves.keys(), gl[:-1])}
    report = {}
    assert_gates("full size B=%d T=%d lengths=%s" % (B, T, lengths), cfg_t, eng, loss.cpu(), g, dh.cpu(),
                 (float(loss_ref.detach()), grads_ref, gl[-1]), report)
    behind = frames_behind(cfg_t, B, T, lengths)[:, None, :].expand_as(dh)
    assert float(dh.cpu()[behind].abs().max()) == 0.0
    print("full size ragged: %d sub-gradient choices at a kink" % flips)
    return report
