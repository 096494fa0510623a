# -*- coding: utf-8 -*-
"""Backward launch plans under every arithmetic: the plan matrix shared by tests/test_emu_launch_plans.py (host emulator) and
tests/test_gpu_launch_plans.py (MI355X).

wn_backward has two kinds of knobs.  ARITHMETIC knobs decide how each contraction is computed (DW_F16PAIR, MM_F16PAIR,
FUSED_F16PAIR, CHAIN_F16PAIR, DW_3PRODUCT, the source of the fp16 scale); LAUNCH-PLAN knobs decide which launches run and in
which groups (WN_FLAG_DW_FLUSH(n), layers_per_bucket, BWD_OVERLAP[_HEAD], FWD_OVERLAP, NO_CHAIN, AUX_FUSED, the t_first loss
window).  ``pairwise_rows`` covers every PAIR of values of two different axes at least once per shape; ``check_plan`` runs one row
against the oracle with the gradient buffer poisoned (NaN) first, so a gradient element that no launch of the plan writes fails
the gate instead of keeping a value an earlier backward left there."""
import functools

import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS, WaveNetEngine, flat_to_state, load_state_into_flat
from tests import parity_common as PC
from tests.golden_util import rel_to_max

# id -> (cfg, B, T); the path each shape exists for is asserted by PATH_TAGS
SHAPES = {
    "P1": ((32, 4, 64, 256, 3, 1, 2, 16), 1, 256),   # k_dw_skipres8, the chain, aux-fused; L = 3
    "P2": ((32, 4, 64, 512, 2, 2, 2, 16), 1, 256),   # skip + res over two 256-row tiles of the skip channels; L = 4
    "P3": ((32, 4, 64, 256, 3, 1, 3, 16), 1, 256),   # the K = 3 chain class with skip + res
    "P4": ((32, 4, 32, 64, 3, 1, 2, 8), 2, 128),     # R != 64: the any-size layered path
}
SEED = 5

# launches of one backward call under DEFAULT_FLAGS and the default plan: (must appear, must not appear)
PATH_TAGS = {
    "P1": (("dw_skip_res", "fused_bwd_chain", "aux_finish"), ("dw_skip", "aux_bwd")),
    "P2": (("dw_skip_res", "fused_bwd_chain", "aux_finish"), ("dw_skip", "aux_bwd")),
    "P3": (("dw_skip_res", "fused_bwd_chain", "aux_finish"), ("dw_skip", "aux_bwd")),
    "P4": (("dw_skip", "dw_res", "bwd_dx_dilated"), ("dw_skip_res", "fused_bwd_chain")),
}

ARITH = {
    "default": DEFAULT_FLAGS,
    "six": SIX_PRODUCT_FLAGS,
    "default+chain16": DEFAULT_FLAGS | _lib.FLAG_CHAIN_F16PAIR,
    "six+dw16": SIX_PRODUCT_FLAGS | _lib.FLAG_DW_F16PAIR,
    "six+dw3": SIX_PRODUCT_FLAGS | _lib.FLAG_DW_3PRODUCT,
}
OVERLAP = {
    "none": 0,
    "bwd": _lib.FLAG_BWD_OVERLAP,
    "bwd+head": _lib.FLAG_BWD_OVERLAP | _lib.FLAG_BWD_OVERLAP_HEAD,
    "fwd": _lib.FLAG_FWD_OVERLAP,
}
# axis name -> values, in the order the covering walks them
AXES = (
    ("arith", tuple(ARITH)),
    ("flush", ("none", "1", "2", "L-1")),
    ("lpb", (0, 1, 2)),
    ("overlap", tuple(OVERLAP)),
    ("no_chain", (False, True)),
    ("aux_fused", (True, False)),
    ("t_first", ("rf", 0)),
    ("scale", ("ws", "scan", "promise")),
)
# the rows that left skip_1x1 gradients unwritten (WN_FLAG_DW_FLUSH(1), one layer bucket, the fused skip + res launch): the
# default arithmetic, and the fp16 pair weight gradients on their own (the combination first reported)
KNOWN_BAD = (
    {"arith": "default", "flush": "1", "lpb": 0, "overlap": "none", "no_chain": False, "aux_fused": True, "t_first": "rf", "scale": "ws"},
    {"arith": "six+dw16", "flush": "1", "lpb": 0, "overlap": "none", "no_chain": False, "aux_fused": True, "t_first": "rf", "scale": "ws"},
)


def pairwise_rows(axes=AXES, seed_rows=KNOWN_BAD):
    """Deterministic greedy covering array of strength 2: every pair of values of two different axes is in some row.  Starts
    from ``seed_rows``; each new row takes the first pair not yet covered and fills the other axes with the value that covers
    the most pairs not yet covered (first value on ties)."""
    names = [a for a, _ in axes]
    vals = dict(axes)
    uncovered = set()
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for va in vals[a]:
                for vb in vals[b]:
                    uncovered.add((a, va, b, vb))

    def cover(row):
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                uncovered.discard((a, row[a], b, row[b]))

    rows = [dict(r) for r in seed_rows]
    for r in rows:
        cover(r)
    order = [(a, va, b, vb) for i, a in enumerate(names) for b in names[i + 1:] for va in vals[a] for vb in vals[b]]
    while uncovered:
        a, va, b, vb = next(p for p in order if p in uncovered)
        row = {a: va, b: vb}
        for n in names:
            if n in row:
                continue
            best, best_gain = None, -1
            for v in vals[n]:
                gain = sum(1 for m, mv in row.items()
                           if ((m, mv, n, v) if names.index(m) < names.index(n) else (n, v, m, mv)) in uncovered)
                if gain > best_gain:
                    best, best_gain = v, gain
            row[n] = best
        rows.append({n: row[n] for n in names})
        cover(row)
    return rows


def row_id(r):
    return "%s-flush%s-lpb%d-ovl_%s-%s-%s-tf%s-%s" % (r["arith"].replace("+", "_"), r["flush"].replace("-", ""), r["lpb"],
                                                    r["overlap"].replace("+", "_"), "nochain" if r["no_chain"] else "chain",
                                                    "aux" if r["aux_fused"] else "noaux", r["t_first"], r["scale"])


def row_flags(r, n_layers):
    """Engine flags of a matrix row, IN FULL (the arithmetic's own bits included)."""
    f = ARITH[r["arith"]] | OVERLAP[r["overlap"]]
    if r["flush"] != "none":
        f |= _lib.flag_dw_flush(n_layers - 1 if r["flush"] == "L-1" else int(r["flush"]))
    if r["no_chain"]:
        f |= _lib.FLAG_NO_CHAIN
    if not r["aux_fused"]:
        f &= ~_lib.FLAG_AUX_FUSED
    return f


@functools.lru_cache(maxsize=8)
def reference(cfg_tuple, B, T, seed, scale=0.1):
    """Seeded instance (ReLU kink margin >= PC.KINK_MARGIN) and the oracle's fp32 training step on it."""
    cfg = O.OracleConfig(*cfg_tuple)
    params, x, h, t, margin, sd = PC.pick_instance(cfg, B, T, seed, scale)
    loss_ref, logits_ref, grads_ref = O.train_step(cfg, params, None, x, h, t)
    return params, x, h, t, loss_ref, logits_ref, grads_ref


def check_grads(eng, flat, cfg_tuple, grads_ref, what):
    """Gradient gates of a whole flat gradient: every element finite, dead tensors exactly 0, the rest within TOL_GRAD of each
    tensor's maximum.  Returns (worst rel err, its tensor)."""
    assert bool(torch.isfinite(flat).all()), "%s: %d gradient elements not finite (never written?)" % (
        what, int((~torch.isfinite(flat)).sum()))
    grads = flat_to_state(eng, flat.cpu(), O.param_shapes(O.OracleConfig(*cfg_tuple)))
    worst, worst_k = 0.0, None
    for k, ref in grads_ref.items():
        if ref is None:
            assert float(grads[k].abs().max()) == 0.0, "%s: %s is dead but not zero" % (what, k)
        else:
            e = rel_to_max(grads[k], ref)
            if e > worst:
                worst, worst_k = e, k
            assert e <= PC.TOL_GRAD, "%s: %s grad rel err %g" % (what, k, e)
    return worst, worst_k


def check_plan(cfg, B, T, seed, lib, device, flags, lpb, t_first, scale_source, want_log=False):
    """One backward launch plan against the oracle.  ``flags``: the engine flags IN FULL.  ``t_first``: "rf" -- the training
    step: ``forward_loss`` (the loss as the epilogue of the windowed forward) and a backward over the loss window; 0 --
    ``forward`` (logits checked against the oracle's), ``loss`` and a backward over every column.  ``scale_source`` (where the
    fp16 scale of the weight gradients comes from): "ws" -- the unmodified tensor the loss call returned (FLAG_DW_F16_AMAX_WS);
    "scan" -- a copy of it (the library scans it); "promise" -- dlogits_bound = 8 x its true maximum.  The gradient buffer is
    NaN before the backward call.  Returns (flat gradient on the CPU, worst rel err, its tensor, launch log of the backward
    call or None); ``want_log`` turns the launch log on, which runs the side-stream plans serially on the GPU."""
    params, x, h, t, loss_ref, logits_ref, grads_ref = reference(tuple(cfg), B, T, seed)
    eng = WaveNetEngine(*cfg, device=device, library=lib)
    eng.flags = flags
    load_state_into_flat(eng, params)
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    if t_first == "rf":
        loss, dl = eng.forward_loss(xd, hd, td)
        tf = eng.receptive_field
    else:
        logits = eng.forward(xd, hd)
        err = float((logits.transpose(1, 2).cpu() - logits_ref).abs().max())
        assert err <= PC.TOL_LOGITS, "logits max-abs err %g" % err
        loss, dl = eng.loss(logits, td)
        tf = int(t_first)
    assert abs(float(loss.cpu()) - float(loss_ref)) <= PC.TOL_LOSS
    kw = {}
    if scale_source == "scan":
        dl = dl.clone()
    elif scale_source == "promise":
        kw["dlogits_bound"] = float(dl.abs().max()) * 8.0
    else:
        assert scale_source == "ws", scale_source
    eng.grads().fill_(float("nan"))
    out = {}

    def bwd():
        out["g"] = eng.backward(dl, layers_per_bucket=lpb, t_first=tf, **kw)
    log = PC.launch_log(lib, bwd) if want_log else None
    if not want_log:
        bwd()
    flat = out["g"].detach().cpu().clone()
    worst, worst_k = check_grads(eng, flat, cfg, grads_ref, "flags %#x lpb %d t_first %s scale %s" % (flags, lpb, t_first, scale_source))
    return flat, worst, worst_k, log
