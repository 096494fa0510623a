# -*- coding: utf-8 -*-
"""Scoring held-out data (``WaveNetEngine.forward_nll`` / ``WaveNet.evaluate``, the C entry points ``wn_forward_nll``,
``wn_softmax_nll_rows``, ``wn_mol_nll_rows``, ``wn_op_row_sums``): checks shared by tests/test_emu_eval.py (host emulator) and
tests/test_gpu_eval.py (MI355X).

The definition under test: ``row_nll[b]`` is the SUM of the per-position negative log-likelihoods of sequence b over
``[t_start, min(lengths[b], T))`` (exactly 0.0 where there is none), ``counts[b]`` the number of those positions.  The checker
is the oracle's forward in fp64 with ``F.cross_entropy(reduction="none")`` summed per row, computed here.  A row sum of ~100
positions is a number around 500 whose fp32 spacing alone is 6e-5, so the project's loss gate ``PC.TOL_LOSS`` -- a gate on a
mean per position -- is applied to ``row_nll[b] / counts[b]``, the same kind of quantity."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, _ptr, _stream_handle
from pytorchwavenetvocoder_amd.nets import WaveNet
from tests import mol_common as MC
from tests import parity_common as PC
from tests import plan_common as PL
from tests import ragged_common as RG

# the ragged suite's shapes plus E1: F1's configuration (receptive field 4) with a third sequence that has no loss position
SHAPES = dict(RG.SHAPES)
SHAPES["E1"] = (RG.SHAPES["F1"][0], 3, 144, (144, 96, 3))
FLAG_SETS = RG.FLAG_SETS
SHAPE_ARITH = [(s, a) for s in SHAPES for a in FLAG_SETS]
IDS = ["%s-%s" % sa for sa in SHAPE_ARITH]
OP_NBLK = (1, 2, 63, 64, 65, 255, 256, 257, 1000)


def counts_of(lengths, T, t_start):
    return [max(min(int(n), T) - t_start, 0) for n in lengths]


@functools.lru_cache(maxsize=16)
def instance(shape):
    """(params, x, h, t, row sums in fp64 (B,), counts): the seeded instance the ragged suite uses for the shape and the
    oracle's per-row sums.  E1: F1's parameters with a seeded batch of its own -- no ReLU-kink margin is asked of it, a
    likelihood (unlike a gradient) is continuous across the kink."""
    cfg_t, B, T, lengths = SHAPES[shape]
    cfg = O.OracleConfig(*cfg_t)
    if shape in RG.SHAPES:
        params, x, h, t = RG.instance(shape)[:4]
    else:
        params = RG.instance("F1")[0]
        x, h, t = O.synthetic_batch(cfg, B, T, PL.SEED + 11)
    return params, x, h, t, oracle_rows(cfg, params, x, h, t, lengths), counts_of(lengths, T, cfg.receptive_field)


def oracle_rows(cfg, params, x, h, t, lengths, t_start=None):
    """O.forward in fp64, per-position cross-entropy, summed per row over [t_start, lengths[b])."""
    rf = cfg.receptive_field if t_start is None else t_start
    with torch.no_grad():
        logits = O.forward(cfg, {k: v.double() for k, v in params.items()}, x, h.double())   # (B, T, Q)
        nll = F.cross_entropy(logits.transpose(1, 2), t, reduction="none")                    # (B, T)
    return torch.stack([nll[b, rf:int(n)].sum() for b, n in enumerate(lengths)])


def assert_rows(tag, row, counts, ref_rows, counts_ref):
    """|row_nll[b] / counts[b] - ref_mean[b]| <= PC.TOL_LOSS on every row with a loss position; exactly 0.0 on the others."""
    assert counts == counts_ref, (tag, counts, counts_ref)
    row = row.cpu()
    assert row.dtype == torch.float32 and tuple(row.shape) == (len(counts),)
    for b, n in enumerate(counts):
        if n == 0:
            assert float(row[b]) == 0.0 and not math.copysign(1.0, float(row[b])) < 0, (tag, b, float(row[b]))
            continue
        e = abs(float(row[b]) / n - float(ref_rows[b]) / n)
        print("%s row %d: %d positions, mean err %.3g" % (tag, b, n, e))
        assert e <= PC.TOL_LOSS, (tag, b, e)


def check_oracle(shape, arith, lib, device):
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, ref_rows, counts_ref = instance(shape)
    eng = RG.engine_for(cfg_t, params, lib, device, FLAG_SETS[arith])
    row, counts = eng.forward_nll(x.to(device), h.to(device), target=t.to(device), lengths=lengths)
    assert_rows("%s/%s" % (shape, arith), row, counts, ref_rows, counts_ref)
    if shape == "E1":
        assert counts == [140, 92, 0] and float(row.cpu()[2]) == 0.0
    # lengths=None: every sequence runs to T
    if shape in ("F1", "P4"):
        row_d, counts_d = eng.forward_nll(x.to(device), h.to(device), target=t.to(device))
        ref_d = oracle_rows(O.OracleConfig(*cfg_t), params, x, h, t, [T] * B)
        assert_rows("%s/%s/dense" % (shape, arith), row_d, counts_d, ref_d, [T - eng.receptive_field] * B)


def mol_model(lib, device):
    cfg, B, T, lengths, params, x, h, y = RG.mol_instance()
    model = WaveNet(*MC.CFG, n_mixture=MC.NM, _library=lib)
    model.load_state_dict(params)
    model.to(device)
    return model, cfg, B, T, lengths, params, x, h, y


def check_mol(lib, device):
    """The mixture head against the fp64 mixture NLL of ragged_common.mol_oracle (relative gate 1e-4, its own), per row: the
    oracle returns the mean over the live positions of the lengths it is given, so row b is asked for with every other
    sequence cut in front of the receptive field."""
    model, cfg, B, T, lengths, params, x, h, y = mol_model(lib, device)
    rf = cfg.receptive_field
    row, counts = model.evaluate(x.to(device), h.to(device), y=y.to(device), lengths=lengths)
    assert counts == counts_of(lengths, T, rf) and counts[2] == 0
    row = row.cpu()
    for b, n in enumerate(counts):
        if n == 0:
            assert float(row[b]) == 0.0
            continue
        only_b = [lengths[i] if i == b else 1 for i in range(B)]
        l64 = RG.mol_oracle(cfg, params, x, h, y, only_b, torch.float64)[0]
        e = abs(float(row[b]) / n - l64)
        print("mol row %d: mean %.6f, err %.3g (gate %.3g)" % (b, l64, e, 1e-4 * abs(l64)))
        assert e <= 1e-4 * abs(l64), (b, e)
    l64 = RG.mol_oracle(cfg, params, x, h, y, lengths, torch.float64)[0]
    assert abs(float(row.double().sum()) / sum(counts) - l64) <= 1e-4 * abs(l64)
    # and the mean the training entry point returns for the same batch
    out = model.engine.forward(x.to(device), h.to(device))
    loss, _ = model.engine.mol_loss(out, y.to(device), lengths=lengths, want_grad=False, log_scale_min=model.log_scale_min)
    assert abs(float(row.double().sum()) / sum(counts) - float(loss.cpu())) <= 1e-4 * abs(l64)


def check_training_loss(shape, arith, lib, device):
    """sum(row_nll) / sum(counts) against the loss forward_loss(lengths=) returns for the same inputs."""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, _, counts_ref = instance(shape)
    eng = RG.engine_for(cfg_t, params, lib, device, FLAG_SETS[arith])
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    row, counts = eng.forward_nll(xd, hd, target=td, lengths=lengths)
    loss, _ = eng.forward_loss(xd, hd, td, lengths=lengths, want_grad=False)
    e = abs(float(row.cpu().double().sum()) / sum(counts) - float(loss.cpu()))
    print("%s/%s: pooled mean against the training loss: %.3g" % (shape, arith, e))
    assert counts == counts_ref and e <= PC.TOL_LOSS, (shape, arith, e)


def c_softmax_rows(eng, logits, td, t_start, t_end, row, acc=None, ws=None):
    B, _, T = logits.shape
    ws = eng.eval_workspace(B, T) if ws is None else ws
    rc = eng.lib.wn_softmax_nll_rows(ctypes.byref(eng.cfg), B, T, _ptr(logits), _ptr(td), int(t_start), _ptr(t_end), _ptr(row),
                                     _ptr(acc), _ptr(ws), ws.numel() * 4, _stream_handle(eng.device))
    return rc, eng.lib.wn_last_error().decode()


def check_routes_agree(shape, lib, device):
    """forward_nll fused (the conv_post_2 epilogue), forward + wn_softmax_nll_rows, and the scratch-logits fallback forced by
    FLAG_EXACT_MFMA.  The issue's words are "agree per row within PC.TOL_LOSS"; PC.TOL_LOSS = 1e-5 is the project's gate on a
    MEAN loss per position, and a row SUM here is 400 - 900, where one fp32 ulp is already 3e-5 - 6e-5: the gate is applied to
    the row divided by its count, the quantity the gate was made for and the one the issue's oracle check uses for the same rows."""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, ref_rows, counts_ref = instance(shape)
    eng = RG.engine_for(cfg_t, params, lib, device, DEFAULT_FLAGS)
    assert eng.lib.wn_forward_loss_fused(ctypes.byref(eng.cfg), B, T, eng.flags) == 1
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    seq = PC.launch_sequence(eng.lib, lambda: eng.forward_nll(xd, hd, target=td, lengths=lengths))
    assert "fwd_post2_ce" in seq and "softmax_ce" not in seq and seq.count("row_sums") == 1 and "sum_partials" not in seq, seq
    row0, counts = eng.forward_nll(xd, hd, target=td, lengths=lengths)
    logits = eng.forward(xd, hd)
    row1 = torch.full((B,), float("nan"), dtype=torch.float32, device=device)
    t_end = torch.tensor(lengths, dtype=torch.int32).to(device)
    rc, err = c_softmax_rows(eng, logits, td, eng.receptive_field, t_end, row1)
    assert rc == 0, err
    exact = RG.engine_for(cfg_t, params, lib, device, DEFAULT_FLAGS | _lib.FLAG_EXACT_MFMA)
    assert exact.lib.wn_forward_loss_fused(ctypes.byref(exact.cfg), B, T, exact.flags) == 0
    seq = PC.launch_sequence(exact.lib, lambda: exact.forward_nll(xd, hd, target=td, lengths=lengths))
    assert "softmax_ce" in seq and "fwd_post2_ce" not in seq and seq.count("row_sums") == 1, seq
    row2, counts2 = exact.forward_nll(xd, hd, target=td, lengths=lengths)
    assert counts == counts2 == counts_ref
    rows = [r.cpu().double() for r in (row0, row1, row2)]
    for b, n in enumerate(counts):
        for i in range(3):
            assert abs(float(rows[i][b]) - float(ref_rows[b])) / n <= PC.TOL_LOSS, (shape, b, i)
            for j in range(i):
                assert abs(float(rows[i][b]) - float(rows[j][b])) / n <= PC.TOL_LOSS, (shape, b, i, j)


def other_batch(cfg_t, B, T, seed):
    """A different batch of a different (B, T) for the same model."""
    U = cfg_t[7] if cfg_t[7] > 0 else 16
    B2, T2 = B + 1, T + U
    x, h, t = O.synthetic_batch(O.OracleConfig(*cfg_t), B2, T2, seed)
    return B2, T2, x, h, t, [T2 - 3 * i for i in range(B2)]


ENGINE_STATE = ("_ws", "_ws_key", "_last_shape", "_last_inputs", "_fwd_window", "_fwd_version", "_fwd_flags", "_dlogits_bound",
                "flat_grads", "_lengths_key", "_lengths_dev")


def check_nothing_moved(shape, arith, lib, device):
    """forward_loss -> evaluate (another batch, another (B, T)) -> backward: loss, dlogits, gradients and dh bit-identical to the
    same step without the evaluate; p.grad, flat_grads and the training workspace are the objects (and bits) they were."""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t = instance(shape)[:4]
    model = WaveNet(*cfg_t, _library=lib)
    model.load_state_dict(params)
    model.to(device)
    eng = model.engine
    eng.flags = FLAG_SETS[arith]
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    rf = eng.receptive_field
    B2, T2, x2, h2, t2, len2 = other_batch(cfg_t, B, T, 77)
    x2, h2, t2 = x2.to(device), h2.to(device), t2.to(device)
    model.loss_and_backward(xd, hd, td, lengths=lengths)   # p.grad exists
    for mode in (model.train, model.eval):
        mode()
        results = []
        for with_eval in (False, True):
            loss, dl = eng.forward_loss(xd, hd, td, lengths=lengths)
            if with_eval:
                before = {k: getattr(eng, k) for k in ENGINE_STATE}
                grads_before = [p.grad for p in model.parameters()]
                flat_bits, serial = eng.flat_grads.clone(), model._fwd_serial
                row, counts = model.evaluate(x2, h2, t=t2, lengths=len2)
                assert counts == counts_of(len2, T2, rf) and bool(torch.isfinite(row).all()) and float(row.min()) > 0.0
                for k, v in before.items():
                    assert getattr(eng, k) is v, k
                for p, g in zip(model.parameters(), grads_before):
                    assert p.grad is g
                assert torch.equal(eng.flat_grads, flat_bits) and model._fwd_serial == serial
                assert eng._eval_ws is not None and eng._eval_ws_key == (B2, T2) and eng._eval_ws is not eng._ws
            eng.grads().fill_(float("nan"))
            dh = torch.full(h.shape, float("nan"), dtype=torch.float32, device=device)
            g = eng.backward(dl, t_first=rf, dh=dh)
            results.append((loss.cpu().clone(), dl.cpu().clone(), g.cpu().clone(), dh.cpu().clone()))
        for what, a, b in zip(("loss", "dlogits", "gradients", "dh"), results[0], results[1]):
            assert torch.equal(a, b), (shape, arith, what)
    eng.release_eval_workspace()
    assert eng._eval_ws is None and eng._eval_ws_key is None and eng._ws is not None


WS_CASES = ("F1", "P4", "E1", "MOL")


def check_workspace_independence(shape, arith, lib, device):
    """The same bits on a fresh zero-filled evaluation workspace, on one full of NaN, of 1e30, on the one a stale evaluation of
    another shape left, and on a second call in a row."""
    if shape == "MOL":
        model, cfg, B, T, lengths, params, x, h, y = mol_model(lib, device)
        eng, cfg_t = model.engine, MC.CFG
        kw = {"y": y.to(device), "log_scale_min": model.log_scale_min}
    else:
        cfg_t, B, T, lengths = SHAPES[shape]
        params, x, h, t = instance(shape)[:4]
        eng = RG.engine_for(cfg_t, params, lib, device, FLAG_SETS[arith])
        kw = {"target": t.to(device)}
    eng.flags = FLAG_SETS[arith]
    xd, hd = x.to(device), h.to(device)

    def run():
        with poisoned_outputs():
            row, counts = eng.forward_nll(xd, hd, lengths=lengths, **kw)
        return row.cpu().clone()

    eng.release_eval_workspace()
    base = run()
    assert bool(torch.isfinite(base).all())
    assert torch.equal(run(), base), "second call in a row"
    for fill in (float("nan"), 1e30):
        eng.eval_workspace(B, T).fill_(fill)
        assert torch.equal(run(), base), (shape, arith, fill)
    # a stale evaluation of another shape: its (larger) buffer, as it was left, under this shape's key
    B2, T2, x2, h2, t2, len2 = other_batch(cfg_t, B, T, 78)
    eng.release_eval_workspace()
    if shape == "MOL":
        y2 = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, (B2, T2)).astype(np.float32))
        eng.forward_nll(x2.to(device), h2.to(device), y=y2.to(device), lengths=len2, log_scale_min=kw["log_scale_min"])
    else:
        eng.forward_nll(x2.to(device), h2.to(device), target=t2.to(device), lengths=len2)
    assert eng._eval_ws_key == (B2, T2)
    eng._eval_ws_key = (B, T)
    assert torch.equal(run(), base), (shape, arith, "stale shape")


def poisoned_outputs():
    """torch.empty / empty_like hand out NaN-filled memory (tests/workspace_common.py): an output element the call leaves
    unwritten shows."""
    from tests import workspace_common as WC
    return WC.poisoned_outputs()


def _three_batches(lib, device):
    acc = torch.zeros(1, dtype=torch.float64, device=device)
    rows = []
    for i, shape in enumerate(("F1", "E1", "F2")):
        cfg_t, B, T, lengths = SHAPES[shape]
        params, x, h, t = instance(shape)[:4]
        eng = RG.engine_for(cfg_t, params, lib, device, DEFAULT_FLAGS)
        xd, hd, td = x.to(device), h.to(device), t.to(device)
        row, _ = eng.forward_nll(xd, hd, target=td, lengths=lengths, acc=acc)
        snapshot = acc.clone()
        row_none, _ = eng.forward_nll(xd, hd, target=td, lengths=lengths)   # acc=None: no trace, same rows
        assert torch.equal(acc, snapshot) and torch.equal(row_none, row)
        rows.append(row.cpu())
    return rows, acc


def check_accumulator(lib, device):
    """Three batches with ``acc=``, read once, against the fp64 sum of the three returned ``row_nll`` tensors to 1e-12 relative:
    the scoring entry points add the rows to ``acc`` as they return them (rounded to fp32, added in double), so the total of a
    pass IS the sum of its per-sequence results -- a dozen fp32 values add exactly in double, 1e-12 leaves room for passes of
    any length.  (wn_op_row_sums, the bare reduction, adds the unrounded double sums: check_row_sums_op.)  ``acc=None`` leaves
    no trace (``_three_batches``)."""
    rows, acc = _three_batches(lib, device)
    total = sum(float(r.double().sum()) for r in rows)
    got = float(acc.cpu())
    print("acc %.17g, fp64 sum of the fp32 rows %.17g, relative difference %.3g" % (got, total, abs(got - total) / abs(total)))
    assert abs(got - total) <= 1e-12 * abs(total)


def check_padding_content(shape, arith, lib, device):
    """Padding content is irrelevant: RG.padding_fills applied behind each end changes no bit of ``row_nll``, under the default
    and under the six-product arithmetic alike, and each fill meets the oracle gate.  (The network is causal and the loss
    kernels mask by position, so a valid position never reads padding; the one path by which padding could reach the bits of
    a valid position is the power-of-two tile scale of the block-scaled fp16 forward, WN_FLAG_FUSED_F16PAIR, when a 32-column
    tile holds both -- F2's first sequence ends at 70, inside such a tile; no bit moves there either.)"""
    cfg_t, B, T, lengths = SHAPES[shape]
    params, x, h, t, ref_rows, counts_ref = instance(shape)
    eng = RG.engine_for(cfg_t, params, lib, device, FLAG_SETS[arith])
    base, _ = eng.forward_nll(x.to(device), h.to(device), target=t.to(device), lengths=lengths)
    for seed in (101, 202):
        x2, h2, t2 = RG.padding_fills(cfg_t, B, T, lengths, x, h, t, seed)
        assert not torch.equal(x2, x) and not torch.equal(t2, t)
        row, counts = eng.forward_nll(x2.to(device), h2.to(device), target=t2.to(device), lengths=lengths)
        assert_rows("%s/%s/fill%d" % (shape, arith, seed), row, counts, ref_rows, counts_ref)
        assert torch.equal(row, base), (shape, arith, seed, row.cpu().tolist(), base.cpu().tolist())


def check_errors(lib, device):
    cfg_t, B, T, lengths = SHAPES["F1"]
    params, x, h, t = instance("F1")[:4]
    model = WaveNet(*cfg_t, _library=lib)
    model.load_state_dict(params)
    model.to(device)
    eng = model.engine
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    yd = torch.zeros((B, T), dtype=torch.float32, device=device)
    other = "meta" if device == "cpu" else "cpu"
    with pytest.raises(ValueError, match="softmax head"):
        model.evaluate(xd, hd, y=yd)
    with pytest.raises(ValueError, match="softmax head"):
        eng.forward_nll(xd, hd, y=yd)
    for call in (model.evaluate, eng.forward_nll):
        with pytest.raises(ValueError, match="exactly one"):
            call(xd, hd)
    with pytest.raises(ValueError, match="exactly one"):
        model.evaluate(xd, hd, t=td, y=yd)
    with pytest.raises(ValueError, match="exactly one"):
        eng.forward_nll(xd, hd, target=td, y=yd)
    with pytest.raises(ValueError, match="lengths must be host integers"):
        model.evaluate(xd, hd, t=td, lengths=torch.tensor(lengths, device=("meta" if device == "cpu" else device)))
    with pytest.raises(ValueError, match=r"lengths\[1\]"):
        model.evaluate(xd, hd, t=td, lengths=[T, 0])
    with pytest.raises(ValueError, match=r"lengths\[0\]"):
        model.evaluate(xd, hd, t=td, lengths=[T + 1, T])
    with pytest.raises(ValueError, match="one entry per sequence"):
        model.evaluate(xd, hd, t=td, lengths=[T])
    row, counts = model.evaluate(xd, hd, t=td, lengths=[eng.receptive_field, 1])   # N == 0 is allowed here
    assert counts == [0, 0] and row.cpu().tolist() == [0.0, 0.0]
    with pytest.raises(ValueError, match="acc must be"):
        model.evaluate(xd, hd, t=td, acc=torch.zeros(1, dtype=torch.float32, device=device))
    with pytest.raises(ValueError, match="acc must be"):
        model.evaluate(xd, hd, t=td, acc=torch.zeros(2, dtype=torch.float64, device=device))
    with pytest.raises(_lib.WnError):
        model.evaluate(xd, hd, t=td, acc=torch.zeros(1, dtype=torch.float64, device=other))
    mmodel, mcfg, mB, mT, mlengths, mparams, mx, mh, my = mol_model(lib, device)
    with pytest.raises(ValueError, match="mixture-of-logistics head"):
        mmodel.evaluate(mx.to(device), mh.to(device), t=mx.to(device))
    with pytest.raises(ValueError, match="mixture-of-logistics head"):
        mmodel.engine.forward_nll(mx.to(device), mh.to(device), target=mx.to(device))
    # the C ABI itself: NULL row_nll
    ws = eng.eval_workspace(B, T)
    st = _stream_handle(eng.device)
    rc = eng.lib.wn_forward_nll(ctypes.byref(eng.cfg), B, T, _ptr(eng.flat_params), _ptr(xd), _ptr(hd), _ptr(td), eng.receptive_field,
                                None, None, None, None, _ptr(ws), ws.numel() * 4, eng.flags, st)
    assert rc != 0 and "row_nll" in eng.lib.wn_last_error().decode()
    logits = eng.forward(xd, hd)
    rc, err = c_softmax_rows(eng, logits, td, eng.receptive_field, None, None)
    assert rc != 0 and "row_nll" in err
    mout = mmodel.engine.forward(mx.to(device), mh.to(device))
    mws = mmodel.engine.eval_workspace(mB, mT)
    rc = eng.lib.wn_mol_nll_rows(ctypes.byref(mmodel.engine.cfg), mB, mT, _ptr(mout), _ptr(my.to(device)), mmodel.receptive_field, None,
                                 65536, -7.0, None, None, _ptr(mws), mws.numel() * 4, st)
    assert rc != 0 and "row_nll" in eng.lib.wn_last_error().decode()
    rc = eng.lib.wn_op_row_sums(_ptr(logits), 0, 4, _ptr(logits), None, st)
    assert rc != 0
    # t_start at or behind T: no position anywhere, zeros, no error
    row, counts = eng.forward_nll(xd, hd, target=td, t_start=T)
    assert counts == [0] * B and row.cpu().tolist() == [0.0] * B


def check_row_sums_op(lib, device):
    """wn_op_row_sums with B = 3 rows of seeded floats of mixed sign, magnitudes 1e-6 .. 1e6: every row within ONE fp32 rounding of
    the fp64 sum (2^-23 sum |partial|), acc the fp64 total to 1e-12 relative, repeated calls bit-identical, a pre-filled acc is
    added to."""
    st = None if device == "cpu" else _stream_handle(torch.device(device))
    B = 3
    for nblk in OP_NBLK:
        rs = np.random.RandomState(1000 + nblk)
        p = (rs.choice([-1.0, 1.0], size=(B, nblk)) * 10.0 ** rs.uniform(-6, 6, size=(B, nblk))).astype(np.float32)
        s64 = p.astype(np.float64).sum(axis=1)
        total = math.fsum(p.astype(np.float64).reshape(-1).tolist())
        pd = torch.from_numpy(p).to(device)
        outs = []
        for start in (0.0, 0.0, 12345.678):
            row = torch.full((B,), float("nan"), dtype=torch.float32, device=device)
            acc = torch.full((1,), start, dtype=torch.float64, device=device)
            lib.check(lib.wn_op_row_sums(_ptr(pd), B, nblk, _ptr(row), _ptr(acc), st), "wn_op_row_sums")
            outs.append((row.cpu(), float(acc.cpu())))
            row2 = torch.full((B,), float("nan"), dtype=torch.float32, device=device)
            lib.check(lib.wn_op_row_sums(_ptr(pd), B, nblk, _ptr(row2), None, st), "wn_op_row_sums")
            assert torch.equal(row2.cpu(), outs[-1][0])
        for b in range(B):
            e, gate = abs(float(outs[0][0][b]) - s64[b]), 2.0 ** -23 * float(np.abs(p[b].astype(np.float64)).sum())
            assert e <= gate, (nblk, b, e, gate)
        assert abs(outs[0][1] - total) <= 1e-12 * abs(total), (nblk, outs[0][1], total)
        assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], nblk
        assert torch.equal(outs[0][0], outs[2][0])
        assert abs(outs[2][1] - (12345.678 + total)) <= 1e-12 * abs(12345.678 + total), nblk
    # more rows than the workgroup has waves, and a row count that is no multiple of them
    rs = np.random.RandomState(7)
    p = rs.standard_normal((11, 37)).astype(np.float32)
    row = torch.full((11,), float("nan"), dtype=torch.float32, device=device)
    acc = torch.zeros(1, dtype=torch.float64, device=device)
    lib.check(lib.wn_op_row_sums(_ptr(torch.from_numpy(p).to(device)), 11, 37, _ptr(row), _ptr(acc), st), "wn_op_row_sums")
    s64 = p.astype(np.float64).sum(axis=1)
    assert np.all(np.abs(row.cpu().numpy().astype(np.float64) - s64) <= 2.0 ** -23 * np.abs(p.astype(np.float64)).sum(axis=1))
    assert abs(float(acc.cpu()) - math.fsum(s64.tolist())) <= 1e-12 * abs(math.fsum(s64.tolist()))
