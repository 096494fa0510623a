# -*- coding: utf-8 -*-
"""The gradient with respect to the aux features (dL/dh, wn_backward_dh): checks shared by tests/test_emu_aux_grad.py (host
emulator) and tests/test_gpu_aux_grad.py (MI355X).  Every check compares against the oracle's autograd of the same loss (CE on
``[:, receptive_field:]``) with respect to h, within ``PC.TOL_GRAD`` of the maximum of |dh|."""
import ctypes
import functools
import os

import numpy as np
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import WaveNetEngine, _ptr, load_state_into_flat
from pytorchwavenetvocoder_amd.nets import WaveNet
from tests import mol_common as MC
from tests import parity_common as PC
from tests import plan_common as PL
from tests.golden_util import rel_to_max

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "aux_grad.npz")

# the four plan shapes, plus no upsampling layer on the fused R = 64 path and on the any-size path
SHAPES = dict(PL.SHAPES)
SHAPES["N1"] = ((32, 4, 64, 256, 3, 1, 2, 0), 1, 256)
SHAPES["N2"] = ((32, 5, 32, 64, 3, 1, 2, 0), 2, 128)


@functools.lru_cache(maxsize=16)
def instance(shape):
    """Seeded instance of a shape (ReLU kink margin >= PC.KINK_MARGIN, tests/plan_common.py) and the oracle's dh in fp64."""
    cfg, B, T = SHAPES[shape]
    params, x, h, t, margin, sd = PC.pick_instance(O.OracleConfig(*cfg), B, T, PL.SEED, 0.1)
    return params, x, h, t, dh64(cfg, params, x, h, t)


def dh64(cfg_tuple, params, x, h, t, relu_masks=None, dtype=torch.float64):
    cfg = O.OracleConfig(*cfg_tuple)
    p = {k: v.detach().to(dtype) for k, v in params.items()}
    hv = h.detach().to(dtype).requires_grad_(True)
    loss = O.loss_fn(cfg, O.forward(cfg, p, x, hv, relu_masks=relu_masks), t)
    g, = torch.autograd.grad(loss, hv)
    return g.float()


def check_module_dh(shape, lib, device):
    """torch.autograd.grad(loss, h) through WaveNet.forward (the reference's loss on the module output) against the oracle."""
    cfg, B, T = SHAPES[shape]
    params, x, h, t, ref = instance(shape)
    model = WaveNet(*cfg, _library=lib)
    model.load_state_dict(params)
    model.to(device)
    hv = h.detach().clone().to(device).requires_grad_(True)
    out = model(x.to(device), hv)
    rf, Q = model.receptive_field, cfg[0]
    loss = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, Q), t.to(device)[:, rf:].contiguous().view(-1))
    g, = torch.autograd.grad(loss, hv)
    assert g.shape == h.shape and g.dtype == torch.float32
    e = rel_to_max(g.cpu(), ref)
    assert e <= PC.TOL_GRAD, (shape, e)
    return e


def check_golden(lib, device):
    """dL/dh of the reference module itself (tests/golden/aux_grad.npz) through WaveNet.forward."""
    z = np.load(GOLDEN)
    worst = 0.0
    for i in range(int(z["n_cases"])):
        cfg = tuple(int(v) for v in z["c%d/cfg" % i])
        B, T = int(z["c%d/B" % i]), int(z["c%d/T" % i])
        oc = O.OracleConfig(*cfg)
        params = O.random_params(oc, int(z["param_seed"]))
        x, h, t = O.synthetic_batch(oc, B, T, int(z["batch_seed"]))
        model = WaveNet(*cfg, _library=lib)
        model.load_state_dict(params)
        model.to(device)
        hv = h.to(device).requires_grad_(True)
        out = model(x.to(device), hv)
        rf = model.receptive_field
        loss = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, cfg[0]), t.to(device)[:, rf:].contiguous().view(-1))
        loss.backward()
        assert abs(float(loss) - float(z["c%d/loss" % i])) <= PC.TOL_LOSS
        e = rel_to_max(hv.grad.cpu(), torch.from_numpy(z["c%d/dh" % i]))
        assert e <= PC.TOL_GRAD, (cfg, e)
        worst = max(worst, e)
    return worst


def check_mol_dh(lib, device):
    """The mixture-of-logistics head: mol_loss_and_backward(aux_grad=True) against the restatement of tests/mol_common.py, in
    fp64 (the fp32 evaluation of the published formula is itself off by its own error, which the gate allows for)."""
    cfg = O.OracleConfig(*MC.CFG, out_channels=3 * MC.NM)
    B, T = 2, 48
    params, x, h, seed = MC._kink_free_instance(cfg, B, T)
    y = torch.from_numpy(np.random.RandomState(seed).uniform(-1, 1, (B, T)).astype(np.float32))
    model = WaveNet(*MC.CFG, n_mixture=MC.NM, _library=lib)
    model.load_state_dict(params)
    model.to(device)

    def oracle(dt):
        p = {k: v.to(dt) for k, v in params.items()}
        hv = h.to(dt).requires_grad_(True)
        loss = O.mol_nll(O.forward(cfg, p, x, hv), y.to(dt), start=cfg.receptive_field)
        g, = torch.autograd.grad(loss, hv)
        return g.float()
    g32, g64 = oracle(torch.float32), oracle(torch.float64)
    loss, dh = model.mol_loss_and_backward(x.to(device), h.to(device), y.to(device), aux_grad=True)
    ek, eo = rel_to_max(dh.cpu(), g64), rel_to_max(g32, g64)
    assert ek <= PC.TOL_GRAD + eo, (ek, eo)
    return ek


def engine_for(shape, lib, device, flags):
    cfg, B, T = SHAPES[shape]
    params = instance(shape)[0]
    eng = WaveNetEngine(*cfg, device=device, library=lib)
    eng.flags = flags
    load_state_into_flat(eng, params)
    return eng


def check_row(shape, row, lib, device):
    """One row of the plan matrix (tests/plan_common.py) with dh requested: dh and the gradient buffer are NaN before the call;
    every element of dh is finite and within the gate, and so are the weight gradients (check_grads)."""
    cfg, B, T = SHAPES[shape]
    params, x, h, t, ref = instance(shape)
    flags = PL.row_flags(row, cfg[4] * cfg[5])
    eng = engine_for(shape, lib, device, flags)
    xd, hd, td = x.to(device), h.to(device), t.to(device)
    if row["t_first"] == "rf":
        _, dl = eng.forward_loss(xd, hd, td)
        tf = eng.receptive_field
    else:
        _, dl = eng.loss(eng.forward(xd, hd), td)
        tf = 0
    kw = {}
    if row["scale"] == "scan":
        dl = dl.clone()
    elif row["scale"] == "promise":
        kw["dlogits_bound"] = float(dl.abs().max()) * 8.0
    eng.grads().fill_(float("nan"))
    dh = torch.full(h.shape, float("nan"), dtype=torch.float32, device=device)
    g = eng.backward(dl, layers_per_bucket=row["lpb"], t_first=tf, dh=dh, **kw)
    dh = dh.cpu()
    assert bool(torch.isfinite(dh).all()), "%d elements of dh not finite" % int((~torch.isfinite(dh)).sum())
    e = rel_to_max(dh, ref)
    assert e <= PC.TOL_GRAD, (shape, PL.row_id(row), e)
    _, _, _, _, _, _, grads_ref = PL.reference(cfg, B, T, PL.SEED)
    PL.check_grads(eng, g.detach().cpu().clone(), cfg, grads_ref, PL.row_id(row))
    return e


def dh_call(eng, dl, flags_extra=0, lpb=0, grads=True, t_first=None):
    """dh of one backward call of ``eng`` (after its forward), with or without the weight gradients."""
    B, T = eng._last_shape
    h = eng._last_inputs[1]
    dh = torch.full(h.shape, float("nan"), dtype=torch.float32, device=h.device)
    old = eng.flags
    eng.flags = old | flags_extra
    try:
        eng.backward(dl, layers_per_bucket=lpb, t_first=t_first, dh=dh, param_grads=grads)
    finally:
        eng.flags = old
    return dh.cpu()


FORBIDDEN_WITHOUT_GRADS = ("reduce_partials", "copy4", "dot", "gemm6_dw", "dw_redo_if_overflow")


def weight_gradient_tags(seq, keep_scale=False):
    """Tags of a launch sequence that belong to the weight gradients (``keep_scale``: the fp16 scale launches, which
    WN_FLAG_MM_F16PAIR's data contractions use as well, are not counted)."""
    out = []
    for tag in seq:
        if tag == "bucket_event":
            out.append(tag)
        elif tag in ("dw_prepare", "dw_absmax_scan"):
            if not keep_scale:
                out.append(tag)
        elif tag.startswith("dw_") or tag in FORBIDDEN_WITHOUT_GRADS:
            out.append(tag)
    return out


def call_backward_dh(eng, dl, grads, dh, events=None, n_events=0, t_first=0):
    """The C entry point itself (NULL where a tensor is None); returns (rc, error text)."""
    B, T = eng._last_shape
    x, h = eng._last_inputs
    ws = eng.workspace(B, T)
    rc = eng.lib.wn_backward_dh(ctypes.byref(eng.cfg), B, T, _ptr(eng.flat_params), _ptr(x), _ptr(h), _ptr(dl), int(t_first),
                                _ptr(grads), _ptr(dh), _ptr(ws), ws.numel() * 4, events, int(n_events), 0, eng.flags, None)
    return rc, eng.lib.wn_last_error().decode()
