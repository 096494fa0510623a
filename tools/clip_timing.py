#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What global-norm clipping and the non-finite-step guard cost per optimizer step.

For the benchmark's model (bench.py: 64 / 256 channels, n = 1 594 897 parameters) and the recipe-size model (512 / 256, 46 M
parameters): ``optimizer.step()`` of the plain ``FusedAdam`` against ``FusedAdam(max_grad_norm=..., skip_nonfinite=True)`` on the
same gradient, alternating, HIP events around windows of ``--steps`` calls; then one step of each under the library's launch log
(per-launch HIP-event times of ``adam`` / ``grad_sumsq`` / ``grad_norm_finalize`` / ``adam_guarded``).  One JSON line per model.

    python tools/clip_timing.py [--steps 2000] [--windows 7] [--out profiles/clip/clip_timing.txt]

The gradient comes from one real training step on a short window (the optimizer's cost does not depend on the minibatch).
"""
import argparse
import ctypes
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


def window_us(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / steps


def measure(name, steps, windows, device="cuda:0"):
    if not torch.cuda.is_available():
        raise SystemExit("tools/clip_timing.py needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device(device)
    torch.manual_seed(1)
    cfg = MODELS[name]
    U = cfg[7]
    opts = {}
    for kind in ("plain", "guarded"):
        model = WaveNet(*cfg)
        model.apply(initialize)
        model.to(dev)
        T = (model.receptive_field // U + 2) * U
        g = torch.Generator().manual_seed(7)
        xx = torch.randint(0, cfg[0], (1, T + 1), generator=g)
        x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
        h = torch.randn(1, cfg[1], T // U, generator=g).to(dev)
        model.loss_and_backward(x, h, t)   # real gradients, and every parameter's .grad a view of the flat buffer
        if kind == "plain":
            opt = FusedAdam(model, lr=1e-4)
        else:
            norm = float(model.engine.grads().double().norm())
            opt = FusedAdam(model, lr=1e-4, max_grad_norm=0.5 * norm, skip_nonfinite=True)   # clip active
        opts[kind] = (model, opt)
    for _, opt in opts.values():
        for _ in range(20):
            opt.step()
    torch.cuda.synchronize()
    times = {"plain": [], "guarded": []}
    for _ in range(windows):   # alternating: both see the same neighbours on a shared machine
        for kind, (_, opt) in opts.items():
            times[kind].append(window_us(opt.step, steps))
    out = {"model": name, "cfg": list(cfg), "n_params": opts["plain"][0].engine.n_params,
           "gradient_bytes": 4 * opts["plain"][0].engine.n_params, "steps_per_window": steps, "windows": windows}
    for kind in times:
        out[kind + "_step_us"] = {"median": statistics.median(times[kind]), "min": min(times[kind]), "max": max(times[kind])}
    out["guarded_minus_plain_us"] = out["guarded_step_us"]["median"] - out["plain_step_us"]["median"]
    for kind, (model, opt) in opts.items():
        out[kind + "_launches"] = launch_table(model.engine.lib, opt.step)
    gopt = opts["guarded"][1]
    out["guarded_steps_applied"], out["guarded_steps_skipped"] = gopt.steps_applied(), gopt.steps_skipped()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000, help="optimizer steps per timed window")
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
