#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What parameter groups in FusedAdam cost.

HIP events around windows of calls, the variants alternating window by window in one process, median / min / max reported:

  launches   for the benchmark's model (bench.py: 64 / 256 channels, n = 1 594 897 parameters) and the recipe-size model
             (512 / 256, 46 M parameters), on ONE set of flat buffers: the grouped launches ``adam_groups`` and
             ``adam_guarded_groups`` under two layouts -- ``two`` (two groups split at one tensor boundary near the middle of the
             buffer) and ``bias_vs_weight`` (biases one group, weights the other: alternating ranges, about one per tensor) --
             against their yardsticks: with nothing frozen the single-group ``adam`` / ``adam_guarded`` of this build and, with
             ``--parent-lib``, of the parent commit's library loaded beside it; under the freeze set ``bottom20`` ``adam_live`` /
             ``adam_guarded_live`` on the same live ranges.  The grouped kernel moves the same 7 words per element.
  host       ``optimizer.step()`` on the benchmark's model, wall clock per call over windows of calls with the device idle in
             front of each window: no groups, ``two`` and ``bias_vs_weight``, unguarded and guarded.

One JSON line per part.

    python tools/groups_timing.py [--calls 500] [--windows 7] [--parts benchmark,recipe,host] [--parent-lib PATH/libwavenet_hip.so]
                                  [--out profiles/groups/groups_timing.txt]
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
from tools.freeze_timing import MODELS, alternate, apply_freeze, spread  # noqa: E402

VALUES = [(1e-4, 1e-8, 0.0, False), (3e-4, 1e-6, 1e-2, False)]   # (lr, eps, weight_decay, decoupled) of the two groups
LAYOUTS = {"two": None, "bias_vs_weight": r"bias$"}


def group_of(model, layout):
    """Group index per tensor: ``bias_vs_weight`` by name; ``two`` by position in the flat buffer (second half = group 1)."""
    names = [k for k, _ in model.named_parameters()]
    if layout == "bias_vs_weight":
        return [int(k.endswith("bias")) for k in names]
    half = model.engine.n_params // 2
    return [int(off >= half) for (off, n, shape, dead) in model._param_slices]


def triples(model, groups, mask=None):
    out = []
    for lo, hi, g in sorted((off, off + n, g) for i, (g, (off, n, shape, dead)) in enumerate(zip(groups, model._param_slices))
                            if not dead and n > 0 and (mask is None or mask[i])):
        if out and out[-1][1] == lo and out[-1][2] == g:
            out[-1] = (out[-1][0], hi, g)
        else:
            out.append((lo, hi, g))
    return out


def whole_calls(L, prefix, eng, m, v, state):
    """``adam`` / ``adam_guarded`` of a build of the library -- this one's or, through its C ABI, the parent commit's."""
    n, (lo, hi), st = eng.n_params, eng.dead_range, _stream_handle(eng.device)
    P, G, M, V, S = _ptr(eng.flat_params), _ptr(eng.grads()), _ptr(m), _ptr(v), _ptr(state)
    return {prefix + "adam": lambda: L.wn_adam_step(P, G, M, V, n, 1000, 1e-4, 0.9, 0.999, 1e-8, 0.0, lo, hi, st),
            prefix + "adam_guarded": lambda: L.wn_adam_step_guarded(P, G, M, V, n, 1e-8, 0.0, lo, hi, S, st)}


def parent_library(path):
    L = ctypes.CDLL(path)
    vp, i64, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    L.wn_adam_step.argtypes = [vp, vp, vp, vp, i64, i64, f, f, f, f, f, i64, i64, vp]
    L.wn_adam_step_guarded.argtypes = [vp, vp, vp, vp, i64, f, f, i64, i64, vp, vp]
    return L


def launches(name, calls, windows, dev, parent_lib):
    """Every variant is ONE call into the C ABI with its arguments built beforehand: at the benchmark's size a launch takes a
    few microseconds, and a wrapper that builds arguments per call would be what the window measures."""
    torch.manual_seed(1)
    cfg = MODELS[name]
    model = WaveNet(*cfg)
    model.apply(initialize)
    model.to(dev)
    eng = model.engine
    n = eng.n_params
    opt = FusedAdam(model, lr=1e-4, skip_nonfinite=True)
    m, v = opt._buffers()
    state, scratch = opt._guard_buffers()
    block = eng.new_group_scalars()
    eng.grads().copy_(1e-3 * torch.randn(n, device=dev))   # the optimizer's cost does not depend on the gradient's values
    L, st = eng.lib.lib, _stream_handle(eng.device)
    P, G, M, V, S, B = _ptr(eng.flat_params), _ptr(eng.grads()), _ptr(m), _ptr(v), _ptr(state), _ptr(block)
    arr = group_array(VALUES)
    A = ctypes.cast(arr, ctypes.c_void_p)
    fns = whole_calls(L, "", eng, m, v, state)
    if parent_lib:
        fns.update(whole_calls(parent_library(parent_lib), "parent:", eng, m, v, state))
    tables = {}
    for fs in ("none", "bottom20"):
        apply_freeze(model, fs)
        ts = model.trainable()
        if fs != "none":
            live = eng.live_table(ts.ranges)
            tables["live:" + fs] = live
            T, nr, nl = _ptr(live.table), live.n_ranges, live.n_live
            fns["adam_live:" + fs] = lambda T=T, nr=nr, nl=nl: L.wn_adam_step_live(
                P, G, M, V, None, n, T, nr, nl, 1000, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0.0, 0, st)
            fns["adam_guarded_live:" + fs] = lambda T=T, nr=nr, nl=nl: L.wn_adam_step_guarded_live(
                P, G, M, V, None, n, T, nr, nl, 1e-8, 0.0, S, 0.0, 0, st)
        for layout in LAYOUTS:
            tab = eng.group_table(triples(model, group_of(model, layout), ts.mask), 2)
            tables["%s:%s" % (layout, fs)] = tab
            T, nr, nl = _ptr(tab.table), tab.n_ranges, tab.n_live
            fns["adam_groups:%s:%s" % (layout, fs)] = lambda T=T, nr=nr, nl=nl: L.wn_adam_step_groups(
                P, G, M, V, None, n, T, nr, nl, 1000, A, 2, 0.9, 0.999, 0.0, 0, st)
            fns["adam_guarded_groups:%s:%s" % (layout, fs)] = lambda T=T, nr=nr, nl=nl: L.wn_adam_step_guarded_groups(
                P, G, M, V, None, n, T, nr, nl, B, S, 0.0, 0, st)
    apply_freeze(model, "none")
    # the guarded launches read the state block and the group block as a norm left them (apply = 1)
    eng.grad_norm_groups(state, scratch, block, tables["two:none"], VALUES, None, True, whole=True)
    torch.cuda.synchronize()
    for key, fn in fns.items():
        for _ in range(5):
            assert fn() == 0, key
    torch.cuda.synchronize()
    us = alternate(fns, calls, windows)
    out = {"part": "launches", "model": name, "cfg": list(cfg), "n": n, "calls_per_window": calls, "windows": windows,
           "tables": {k: {"ranges": t.n_ranges, "n_live": t.n_live} for k, t in tables.items()}, "launch_us": us, "against": {}}
    for key in us:
        kind, _, rest = key.partition(":")
        if not kind.endswith("_groups"):
            continue
        fs = rest.split(":")[1]
        base = kind[:-len("_groups")]
        for yard in ([base, "parent:" + base] if fs == "none" else ["%s_live:%s" % (base, fs)]):
            if yard in us:
                out["against"]["%s vs %s" % (key, yard)] = {
                    "median_us": us[key]["median"], "yardstick_median_us": us[yard]["median"], "yardstick_min_us": us[yard]["min"],
                    "yardstick_max_us": us[yard]["max"], "inside_spread": us[yard]["min"] <= us[key]["median"] <= us[yard]["max"],
                    "difference_us": us[key]["median"] - us[yard]["median"]}
    return out


def host(calls, windows, dev):
    cfg = MODELS["benchmark"]
    B, T, U = 1, 3840, cfg[7]
    g = torch.Generator().manual_seed(7)
    xx = torch.randint(0, cfg[0], (B, T + 1), generator=g)
    x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
    h = torch.randn(B, cfg[1], T // U, generator=g).to(dev)
    fns = {}
    for guarded in (False, True):
        for layout in (None, "two", "bias_vs_weight"):
            torch.manual_seed(1)
            model = WaveNet(*cfg)
            model.apply(initialize)
            model.to(dev)
            groups = None
            if layout == "bias_vs_weight":
                groups = [(r"bias$", {"lr": 3e-4, "weight_decay": 0.0})]
            elif layout == "two":
                names = [k for (k, _), gi in zip(model.named_parameters(), group_of(model, "two")) if gi]
                groups = [("^(?:%s)$" % "|".join(k.replace(".", r"\.") for k in names), {"lr": 3e-4})]
            opt = FusedAdam(model, lr=1e-4, weight_decay=1e-2, skip_nonfinite=guarded, groups=groups)
            model.loss_and_backward(x, h, t)   # (gives every parameter its gradient view)
            fns["%s%s" % ("guarded:" if guarded else "", layout or "no_groups")] = opt.step
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
            times[k].append(1e6 * (time.perf_counter() - t0) / calls)
    torch.cuda.synchronize()
    return {"part": "host", "cfg": list(cfg), "tensors": len(list(model.parameters())), "calls_per_window": calls, "windows": windows,
            "step_host_us": {k: spread(val) for k, val in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--parts", default="benchmark,recipe,host")
    ap.add_argument("--parent-lib", default=None, help="libwavenet_hip.so of the parent commit: its adam / adam_guarded join the alternation")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/groups_timing.py needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    for part in args.parts.split(","):
        res = host(args.calls, args.windows, dev) if part == "host" else launches(part, args.calls, args.windows, dev, args.parent_lib)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
