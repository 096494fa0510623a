#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What layer-wise adaptive steps (LAMB) in FusedAdam cost.

HIP events around windows of calls, the variants alternating window by window in one process, median / min / max reported:

  launches   for the benchmark's model (bench.py: 64 / 256 channels, n = 1 594 897 parameters) and the recipe-size model
             (512 / 256, 46 M parameters), on ONE set of flat buffers: the three launches of ``wn_lamb_step`` (unguarded and
             guarded, default adaptation: matrices adapt, biases do not) against the grouped Adam launch ``adam_groups`` /
             ``adam_guarded_groups`` over the same tensors (biases one group, weights the other; its ISA is the parent
             commit's -- ``--parent-lib`` adds the parent's own build to the alternation), and the two launches of
             ``wn_tensor_sumsq``.  LAMB moves 10 words per adapted element against Adam's 7.
  host       ``optimizer.step()`` on the benchmark's model, wall clock per call over windows of calls with the device idle in
             front of each window, with and without layer adaptation, unguarded and guarded.
  norms      ``optimizer.grad_norms()`` (two launches for all tensors) against the loop of ``p.grad.norm()`` over the model's
             tensors, both with one synchronisation at the end of the window.

One JSON line per part.

    python tools/lamb_timing.py [--calls 300] [--windows 7] [--parts benchmark,recipe,host,norms] [--parent-lib PATH/libwavenet_hip.so]
                                [--out profiles/lamb/lamb_timing.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorchwavenetvocoder_amd.engine import _ptr, _stream_handle, group_array  # noqa: E402
from pytorchwavenetvocoder_amd.nets import WaveNet, initialize  # noqa: E402
from pytorchwavenetvocoder_amd.optim import FusedAdam  # noqa: E402
from tools.freeze_timing import MODELS, alternate, spread  # noqa: E402
from tools.groups_timing import group_of, triples  # noqa: E402

VALUES = [(1e-4, 1e-8, 1e-2, False), (1e-4, 1e-8, 0.0, False)]   # (lr, eps, weight_decay, decoupled): weights, biases


def parent_library(path):
    L = ctypes.CDLL(path)
    vp, i, i64, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    L.wn_adam_step_groups.argtypes = [vp, vp, vp, vp, vp, i64, vp, i, i64, i64, vp, i, f, f, d, i, vp]
    return L


def launches(name, calls, windows, dev, parent_lib):
    """Every variant is ONE call into the C ABI with its arguments built beforehand."""
    torch.manual_seed(1)
    cfg = MODELS[name]
    model = WaveNet(*cfg)
    model.apply(initialize)
    model.to(dev)
    eng = model.engine
    n = eng.n_params
    eng.flat_params.add_(1e-2 * torch.randn(n, device=dev))   # (initialize() zeroes the biases; no norm should be zero here)
    opt = FusedAdam(model, lr=1e-4, skip_nonfinite=True)
    m, v = opt._buffers()
    state, scratch = opt._guard_buffers()
    block = eng.new_group_scalars()
    eng.grads().copy_(1e-3 * torch.randn(n, device=dev))   # the optimizer's cost does not depend on the gradient's values
    L, st = eng.lib.lib, _stream_handle(eng.device)
    P, G, M, V, S, B = _ptr(eng.flat_params), _ptr(eng.grads()), _ptr(m), _ptr(v), _ptr(state), _ptr(block)
    arr = group_array(VALUES)
    A = ctypes.cast(arr, ctypes.c_void_p)
    groups = group_of(model, "bias_vs_weight")
    gtab = eng.group_table(triples(model, groups), 2)
    quads = sorted((off, off + k, g, int(len(shape) >= 2)) for g, (off, k, shape, dead) in zip(groups, model._param_slices)
                   if not dead and k > 0)
    ttab = eng.tensor_table(quads, 2)
    stats = torch.zeros(3 * ttab.n_ranges, dtype=torch.float32, device=dev)
    sums = torch.zeros(ttab.n_ranges, dtype=torch.float64, device=dev)
    GT, gnr, gnl = _ptr(gtab.table), gtab.n_ranges, gtab.n_live
    TT, tnr, tnl, SC, ST, SU = _ptr(ttab.table), ttab.n_ranges, ttab.n_live, _ptr(ttab.scratch), _ptr(stats), _ptr(sums)
    fns = {
        "adam_groups": lambda: L.wn_adam_step_groups(P, G, M, V, None, n, GT, gnr, gnl, 1000, A, 2, 0.9, 0.999, 0.0, 0, st),
        "adam_guarded_groups": lambda: L.wn_adam_step_guarded_groups(P, G, M, V, None, n, GT, gnr, gnl, B, S, 0.0, 0, st),
        "lamb": lambda: L.wn_lamb_step(P, G, M, V, None, n, TT, tnr, tnl, 1000, A, 2, 0.9, 0.999, 0.0, None, 0.0, 0, SC, ST, st),
        "lamb_guarded": lambda: L.wn_lamb_step(P, G, M, V, None, n, TT, tnr, tnl, 0, A, 2, 0.9, 0.999, 0.0, S, 0.0, 0, SC, ST, st),
        "tensor_sumsq": lambda: L.wn_tensor_sumsq(G, n, TT, tnr, tnl, SC, SU, st),
    }
    if parent_lib:
        PL = parent_library(parent_lib)
        fns["parent:adam_groups"] = lambda: PL.wn_adam_step_groups(P, G, M, V, None, n, GT, gnr, gnl, 1000, A, 2, 0.9, 0.999, 0.0, 0, st)
    # the guarded launches read the state block and the group block as a norm left them (apply = 1)
    eng.grad_norm_groups(state, scratch, block, gtab, VALUES, None, True, whole=True)
    torch.cuda.synchronize()
    for key, fn in fns.items():
        for _ in range(5):
            assert fn() == 0, key
    torch.cuda.synchronize()
    us = alternate(fns, calls, windows)
    adapted = sum(hi - lo for lo, hi, _, a in quads if a)
    # bytes the launches must move: Adam 7 words per element; LAMB 10 per adapted element and 7 per element that does not adapt
    floor = {"adam_groups": 28.0 * gnl, "lamb": 40.0 * adapted + 28.0 * (tnl - adapted), "tensor_sumsq": 4.0 * tnl}
    out = {"part": "launches", "model": name, "cfg": list(cfg), "n": n, "calls_per_window": calls, "windows": windows,
           "tensors": tnr, "adapted_tensors": sum(a for _, _, _, a in quads), "adapted_elements": adapted, "blocks": ttab.n_blocks,
           "group_table_ranges": gnr, "launch_us": us, "bytes": floor,
           "GBps_at_median": {k: floor[k.replace("_guarded", "").replace("parent:", "")] / (1e3 * val["median"]) for k, val in us.items()},
           "lamb_over_adam": {"median": us["lamb"]["median"] / us["adam_groups"]["median"],
                              "traffic": floor["lamb"] / floor["adam_groups"],
                              "guarded_median": us["lamb_guarded"]["median"] / us["adam_guarded_groups"]["median"]}}
    return out


def _batch(cfg, dev):
    B, T, U = 1, 3840, cfg[7]
    g = torch.Generator().manual_seed(7)
    xx = torch.randint(0, cfg[0], (B, T + 1), generator=g)
    return xx[:, :-1].contiguous().to(dev), torch.randn(B, cfg[1], T // U, generator=g).to(dev), xx[:, 1:].contiguous().to(dev)


def _model(cfg, dev, **kw):
    torch.manual_seed(1)
    model = WaveNet(*cfg)
    model.apply(initialize)
    model.to(dev)
    opt = FusedAdam(model, lr=1e-4, weight_decay=1e-2, **kw)
    model.loss_and_backward(*_batch(cfg, dev))   # (gives every parameter its gradient view)
    return model, opt


def _host_windows(fns, calls, windows, sync_inside=False):
    for fn in fns.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            if sync_inside:
                torch.cuda.synchronize()
            times[k].append(1e6 * (time.perf_counter() - t0) / calls)
    torch.cuda.synchronize()
    return {k: spread(val) for k, val in times.items()}


def host(calls, windows, dev):
    cfg = MODELS["benchmark"]
    fns = {}
    for guarded in (False, True):
        for lamb in (False, True):
            model, opt = _model(cfg, dev, skip_nonfinite=guarded, layer_adaptation=lamb)
            fns["%s%s" % ("guarded:" if guarded else "", "lamb" if lamb else "adam")] = opt.step
    return {"part": "host", "cfg": list(cfg), "tensors": len(list(model.parameters())), "calls_per_window": calls, "windows": windows,
            "step_host_us": _host_windows(fns, calls, windows)}


def norms(calls, windows, dev):
    cfg = MODELS["benchmark"]
    model, opt = _model(cfg, dev)
    params = [p for p in model.parameters() if p.grad is not None]
    fns = {"grad_norms": opt.grad_norms, "loop_of_p.grad.norm": lambda: [p.grad.norm() for p in params]}
    a, b = opt.grad_norms().cpu(), torch.stack([p.grad.double().norm() for p in params]).cpu()
    assert len(opt.tensor_names) == len(params) and float(((a - b).abs() / b.clamp_min(1e-300)).max()) < 1e-12
    return {"part": "norms", "cfg": list(cfg), "tensors": len(params), "calls_per_window": calls, "windows": windows,
            "device_and_host_us": _host_windows(fns, calls, windows, sync_inside=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=300, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--parts", default="benchmark,recipe,host,norms")
    ap.add_argument("--parent-lib", default=None, help="libwavenet_hip.so of the parent commit: its adam_groups joins the alternation")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lamb_timing.py needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    for part in args.parts.split(","):
        if part == "host":
            res = host(args.calls, args.windows, dev)
        elif part == "norms":
            res = norms(args.calls, args.windows, dev)
        else:
            res = launches(part, args.calls, args.windows, dev, args.parent_lib)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
