#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What training with frozen parameters costs and saves.

HIP events around windows of calls, the variants alternating window by window in one process, median / min / max reported:

  launches   for the benchmark's model (bench.py: 64 / 256 channels, n = 1 594 897 parameters) and the recipe-size model
             (512 / 256, 46 M parameters), on ONE set of flat buffers: the whole-buffer launches ``adam``, ``adam_guarded_ema``
             and the norm (``grad_sumsq`` + ``grad_norm_finalize``) against their live-range forms under three tables --
             ``none`` (every non-dead element: the whole-buffer launch's work through the table), ``bottom20`` (front conv,
             upsampling and the layers below 20 frozen) and ``scatter`` (every third tensor frozen).  The yardstick of a frozen
             set is the whole-buffer launch scaled by ``n_live / n`` (``yardstick_us``); ``excess_us`` is what the live launch
             takes beyond it.
  step       the benchmark's geometry (B = 8, T = 23040): ``loss_and_backward`` + ``FusedAdam.step()`` with nothing frozen
             against ``bottom10``, ``bottom20``, ``bottom30`` (the post-net alone trains) and ``aux_only``, each on a model of
             its own; ms per step, the ratio to the full step, and the library's per-launch table of one step of each
             (which launches fell away, and what the remaining ones take).

One JSON line per part.

    python tools/freeze_timing.py [--calls 500] [--step-calls 10] [--windows 7] [--parts benchmark,recipe,step]
                                  [--out profiles/freeze/freeze_timing.txt]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorchwavenetvocoder_amd.nets import WaveNet, initialize  # noqa: E402
from pytorchwavenetvocoder_amd.optim import FusedAdam  # noqa: E402

MODELS = {"benchmark": (256, 80, 64, 256, 10, 3, 2, 80), "recipe": (256, 80, 512, 256, 10, 3, 2, 80)}
EMA_DECAY = 0.9999
LAYER_KEY = re.compile(r"(?:dil_sigmoid|dil_tanh|aux_1x1_sigmoid|aux_1x1_tanh|skip_1x1|res_1x1)\.(\d+)\.")


def frozen_keys(name, keys):
    """``none``, ``bottomK`` (front conv, upsampling and the layers below K), ``aux_only``, ``scatter`` (every third tensor)."""
    if name == "none":
        return set()
    if name == "scatter":
        return {k for i, k in enumerate(keys) if i % 3 == 0}
    if name == "aux_only":
        return {k for k in keys if not k.startswith(("aux_1x1_", "upsampling."))}
    below = int(name[len("bottom"):])
    out = set()
    for k in keys:
        m = LAYER_KEY.match(k)
        if k.startswith(("causal.", "upsampling.")) or (m is not None and int(m.group(1)) < below):
            out.add(k)
    return out


def apply_freeze(model, name):
    frozen = frozen_keys(name, [k for k, _ in model.named_parameters()])
    for k, p in model.named_parameters():
        p.requires_grad_(k not in frozen)
    return frozen


def window_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def alternate(fns, calls, windows):
    times = {k: [] for k in fns}
    for _ in range(windows):   # alternating: every variant sees the same neighbours on a shared machine
        for k, fn in fns.items():
            times[k].append(window_us(fn, calls))
    return {k: spread(v) for k, v in times.items()}


def launch_table(lib, fn):
    lib.wn_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.wn_prof_enable(0)
    need = lib.wn_prof_report(None, 0)
    buf = ctypes.create_string_buffer(max(need, 16))
    lib.wn_prof_report(buf, len(buf))
    return {k: {"launches": v["count"], "us": 1e3 * v["ms"]} for k, v in json.loads(buf.value.decode() or "{}").items()}


def launches(name, calls, windows, dev):
    torch.manual_seed(1)
    cfg = MODELS[name]
    model = WaveNet(*cfg)
    model.apply(initialize)
    model.to(dev)
    eng = model.engine
    n = eng.n_params
    opt = FusedAdam(model, lr=1e-4, skip_nonfinite=True, ema_decay=EMA_DECAY)
    m, v = opt._buffers()
    ema = opt.ema
    state, scratch = opt._guard_buffers()
    eng.grads().copy_(1e-3 * torch.randn(n, device=dev))   # the optimizer's cost does not depend on the gradient's values
    tables = {}
    for fs in ("none", "bottom20", "scatter"):
        apply_freeze(model, fs)
        ts = model.trainable()
        tables[fs] = eng.live_table(ts.ranges)   # (``none`` is full for the model: its table is built by hand here)
    apply_freeze(model, "none")
    eng.grad_norm(state, scratch, None, True, 1e-4)   # the guarded launches read the state block as a norm left it (apply = 1)
    torch.cuda.synchronize()
    fns = {"adam": lambda: eng.adam_step(m, v, 1000, 1e-4),
           "adam_guarded_ema": lambda: eng.adam_step_guarded_ema(m, v, ema, state, ema_decay=EMA_DECAY),
           "grad_norm": lambda: eng.grad_norm(state, scratch, None, True, 1e-4)}
    for fs, tab in tables.items():
        fns["adam_live:" + fs] = lambda tab=tab: eng.adam_step(m, v, 1000, 1e-4, live=tab)
        fns["adam_guarded_ema_live:" + fs] = lambda tab=tab: eng.adam_step_guarded_ema(m, v, ema, state, ema_decay=EMA_DECAY, live=tab)
        fns["grad_norm_live:" + fs] = lambda tab=tab: eng.grad_norm(state, scratch, None, True, 1e-4, live=tab)
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = alternate(fns, calls, windows)
    out = {"part": "launches", "model": name, "cfg": list(cfg), "n": n, "calls_per_window": calls, "windows": windows,
           "tables": {fs: {"ranges": tab.n_ranges, "n_live": tab.n_live, "live_share": tab.n_live / float(n)} for fs, tab in tables.items()},
           "launch_us": us, "yardstick_us": {}, "excess_us": {}, "whole_spread_us": {}}
    for whole in ("adam", "adam_guarded_ema", "grad_norm"):
        out["whole_spread_us"][whole] = us[whole]["max"] - us[whole]["min"]
        for fs, tab in tables.items():
            key = "%s_live:%s" % (whole, fs)
            out["yardstick_us"][key] = us[whole]["median"] * tab.n_live / float(n)
            out["excess_us"][key] = us[key]["median"] - out["yardstick_us"][key]
    return out


def step(calls, windows, dev):
    cfg = MODELS["benchmark"]
    B, T, U = 8, 23040, cfg[7]
    g = torch.Generator().manual_seed(7)
    xx = torch.randint(0, cfg[0], (B, T + 1), generator=g)
    x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
    h = torch.randn(B, cfg[1], T // U, generator=g).to(dev)
    fns, info, lib = {}, {}, None
    for fs in ("none", "bottom10", "bottom20", "bottom30", "aux_only"):
        torch.manual_seed(1)
        model = WaveNet(*cfg)
        model.apply(initialize)
        model.to(dev)
        frozen = apply_freeze(model, fs)
        opt = FusedAdam(model, lr=1e-4)
        ts = model.trainable()
        info[fs] = {"tensors_frozen": len(frozen), "ranges": len(ts.ranges), "n_live": ts.n_live, "first_layer": ts.first_layer,
                    "needs": ts.needs}
        lib = model.engine.lib

        def one(model=model, opt=opt):
            model.loss_and_backward(x, h, t)
            opt.step()
        fns[fs] = one
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: {s: val / 1e3 for s, val in sp.items()} for k, sp in alternate(fns, calls, windows).items()}
    per_launch = {fs: launch_table(lib, fn) for fs, fn in fns.items()}   # (one step each, serial: the profiler keeps one stream)
    return {"part": "step", "cfg": list(cfg), "B": B, "T": T, "calls_per_window": calls, "windows": windows, "sets": info,
            "ms_per_step": ms, "ratio_to_full": {k: ms[k]["median"] / ms["none"]["median"] for k in ms},
            "per_launch": per_launch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500, help="launches per timed window")
    ap.add_argument("--step-calls", type=int, default=10, help="training steps per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--parts", default="benchmark,recipe,step")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/freeze_timing.py needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    for part in args.parts.split(","):
        res = step(args.step_calls, args.windows, dev) if part == "step" else launches(part, args.calls, args.windows, dev)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
