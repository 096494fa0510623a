#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What the moving average of the weights costs inside the Adam launch.

For the benchmark's model (bench.py: 64 / 256 channels, n = 1 594 897 parameters) and the recipe-size model (512 / 256, 46 M
parameters), HIP events around windows of ``--steps`` calls, the variants alternating window by window:

  launches   ``adam`` against ``adam_ema`` and ``adam_guarded`` against ``adam_guarded_ema`` (the engine's calls, nothing else in
             the window), and beside each fused launch the UNFUSED alternative it replaces: the plain launch followed by torch's
             ``ema.lerp_(p, w)`` -- the yardstick.  The plain kernels move 7 words per element (read p, g, m, v; write p, m, v), the
             fused ones 9 (+ read and write e), the unfused pair 10 in two launches.
  step()     ``optimizer.step()`` of ``FusedAdam`` with ``ema_decay`` off and on, unguarded and guarded.

One JSON line per model.

    python tools/ema_timing.py [--steps 500] [--windows 7] [--out profiles/ema/ema_timing.txt]

The gradient comes from one real training step on a short window (the optimizer's cost does not depend on the minibatch).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorchwavenetvocoder_amd.nets import WaveNet, initialize  # noqa: E402
from pytorchwavenetvocoder_amd.optim import FusedAdam  # noqa: E402

MODELS = {"benchmark": (256, 80, 64, 256, 10, 3, 2, 80), "recipe": (256, 80, 512, 256, 10, 3, 2, 80)}
EMA_DECAY = 0.9999
KINDS = {"plain": dict(), "plain_ema": dict(ema_decay=EMA_DECAY),
         "guarded": dict(skip_nonfinite=True), "guarded_ema": dict(skip_nonfinite=True, ema_decay=EMA_DECAY)}


def window_us(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def alternate(fns, steps, windows):
    times = {k: [] for k in fns}
    for _ in range(windows):   # alternating: every variant sees the same neighbours on a shared machine
        for k, fn in fns.items():
            times[k].append(window_us(fn, steps))
    return {k: spread(v) for k, v in times.items()}


def measure(name, steps, windows, device="cuda:0"):
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_timing.py needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device(device)
    torch.manual_seed(1)
    cfg = MODELS[name]
    U = cfg[7]
    opts = {}
    for kind, kw in KINDS.items():
        model = WaveNet(*cfg)
        model.apply(initialize)
        model.to(dev)
        T = (model.receptive_field // U + 2) * U
        g = torch.Generator().manual_seed(7)
        xx = torch.randint(0, cfg[0], (1, T + 1), generator=g)
        x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
        h = torch.randn(1, cfg[1], T // U, generator=g).to(dev)
        model.loss_and_backward(x, h, t)   # real gradients, and every parameter's .grad a view of the flat buffer
        opts[kind] = (model, FusedAdam(model, lr=1e-4, **kw))
    for _, opt in opts.values():
        for _ in range(20):
            opt.step()
    torch.cuda.synchronize()
    n = opts["plain"][0].engine.n_params
    out = {"model": name, "cfg": list(cfg), "n_params": n, "steps_per_window": steps, "windows": windows, "ema_decay": EMA_DECAY}

    # ---- the launches alone --------------------------------------------------------------------------------------------------
    w = 1.0 - EMA_DECAY
    fns = {}
    eng, opt = opts["plain"][0].engine, opts["plain"][1]
    m, v = opt._buffers()
    shadow = eng.flat_params.clone()
    fns["adam"] = lambda eng=eng, m=m, v=v: eng.adam_step(m, v, 1000, 1e-4)

    def unfused(eng=eng, m=m, v=v, shadow=shadow):
        eng.adam_step(m, v, 1000, 1e-4)
        shadow.lerp_(eng.flat_params, w)
    fns["adam_then_torch_lerp"] = unfused
    eng, opt = opts["plain_ema"][0].engine, opts["plain_ema"][1]
    m, v = opt._buffers()
    fns["adam_ema"] = lambda eng=eng, m=m, v=v, e=opt.ema: eng.adam_step_ema(m, v, e, 1000, 1e-4, ema_decay=EMA_DECAY)
    # the guarded launches read the state block as the last step()'s norm left it (apply = 1)
    eng, opt = opts["guarded"][0].engine, opts["guarded"][1]
    m, v = opt._buffers()
    state = opt._guard_buffers()[0]
    gshadow = eng.flat_params.clone()
    fns["adam_guarded"] = lambda eng=eng, m=m, v=v, s=state: eng.adam_step_guarded(m, v, s)

    def unfused_guarded(eng=eng, m=m, v=v, s=state, shadow=gshadow):
        eng.adam_step_guarded(m, v, s)
        shadow.lerp_(eng.flat_params, w)
    fns["adam_guarded_then_torch_lerp"] = unfused_guarded
    eng, opt = opts["guarded_ema"][0].engine, opts["guarded_ema"][1]
    m, v = opt._buffers()
    state = opt._guard_buffers()[0]
    fns["adam_guarded_ema"] = lambda eng=eng, m=m, v=v, e=opt.ema, s=state: eng.adam_step_guarded_ema(m, v, e, s, ema_decay=EMA_DECAY)
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out["launch_us"] = alternate(fns, steps, windows)
    lu = out["launch_us"]
    bytes_moved = {"adam": 28, "adam_ema": 36, "adam_guarded": 28, "adam_guarded_ema": 36, "adam_then_torch_lerp": 40,
                   "adam_guarded_then_torch_lerp": 40}
    out["launch_gb_per_s"] = {k: bytes_moved[k] * n / (1e3 * lu[k]["median"]) for k in lu}
    out["fused_minus_unfused_us"] = {"plain": lu["adam_ema"]["median"] - lu["adam_then_torch_lerp"]["median"],
                                     "guarded": lu["adam_guarded_ema"]["median"] - lu["adam_guarded_then_torch_lerp"]["median"]}
    out["ema_minus_plain_us"] = {"plain": lu["adam_ema"]["median"] - lu["adam"]["median"],
                                 "guarded": lu["adam_guarded_ema"]["median"] - lu["adam_guarded"]["median"]}

    # ---- optimizer.step() ------------------------------------------------------------------------------------------------------
    out["step_us"] = alternate({k: o.step for k, (_, o) in opts.items()}, steps, windows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--models", default="benchmark,recipe")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for name in args.models.split(","):
        line = json.dumps(measure(name, args.steps, args.windows))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
