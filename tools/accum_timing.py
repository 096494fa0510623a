#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What gradient accumulation over micro-batches costs.

HIP events around windows of calls, the variants alternating window by window:

  launches   ``grad_accumulate`` in each of its three modes at the benchmark model's n = 1 594 897 and the recipe model's
             n = 46 190 161 floats, beside torch's ``acc.add_(g)`` on the same two buffers -- the yardstick.  SET moves 8 n bytes, ADD,
             FINISH and ``add_`` 12 n (two reads, one write); the TB/s column is that traffic over the median.  ``swap``
             (``wn_op_swap``, the same two-buffer walk in csrc/wn_optim.inl: 16 n bytes) is timed in the same windows.
  cycle      on the benchmark's model: one cycle of A = 4 micro-batches of B = 2 x T = 23040 (``micro_step=(i, 4)``) against four
             plain B = 2 calls (what the cycle costs without its four launches) and against the one B = 8 call (what a device with
             room for it would run instead).  No optimizer step in any of the three.

One JSON line per part.

    python tools/accum_timing.py [--calls 500] [--windows 7] [--out profiles/accum/accum_timing.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorchwavenetvocoder_amd import _lib  # noqa: E402
from pytorchwavenetvocoder_amd.engine import _stream_handle  # noqa: E402
from pytorchwavenetvocoder_amd.nets import WaveNet, initialize  # noqa: E402

SIZES = {"benchmark": 1594897, "recipe": 46190161}
BENCH_CFG = (256, 80, 64, 256, 10, 3, 2, 80)


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


def launches(name, calls, windows, dev):
    n = SIZES[name]
    lib = _lib.load_library()
    st = _stream_handle(dev)
    acc, g, g2 = (1e-3 * torch.randn(n, device=dev) for _ in range(3))   # FINISH writes a gradient buffer of its own (g2)

    def op(mode, grad):
        return lambda: lib.check(lib.wn_op_accumulate(acc.data_ptr(), grad.data_ptr(), n, mode, st), "wn_op_accumulate")
    fns = {"set": op(_lib.ACCUM_SET, g), "add": op(_lib.ACCUM_ADD, g), "finish": op(_lib.ACCUM_FINISH, g2),
           "swap": lambda: lib.check(lib.wn_op_swap(acc.data_ptr(), g.data_ptr(), n, st), "wn_op_swap"),
           "torch_add_": lambda: acc.add_(g)}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = alternate(fns, calls, windows)
    words = {"set": 8, "add": 12, "finish": 12, "swap": 16, "torch_add_": 12}
    return {"part": "launches", "model": name, "n": n, "calls_per_window": calls, "windows": windows, "launch_us": us,
            "tb_per_s": {k: words[k] * n / (1e6 * us[k]["median"]) for k in us},
            "add_minus_torch_us": us["add"]["median"] - us["torch_add_"]["median"],
            "finish_minus_torch_us": us["finish"]["median"] - us["torch_add_"]["median"]}


def cycle(calls, windows, dev):
    torch.manual_seed(1)
    model = WaveNet(*BENCH_CFG)
    model.apply(initialize)
    model.to(dev)
    A, B, T, U = 4, 2, 23040, BENCH_CFG[7]
    g = torch.Generator().manual_seed(7)
    xx = torch.randint(0, BENCH_CFG[0], (A * B, T + 1), generator=g)
    x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
    h = torch.randn(A * B, BENCH_CFG[1], T // U, generator=g).to(dev)
    micro = [(x[i * B:(i + 1) * B].contiguous(), h[i * B:(i + 1) * B].contiguous(), t[i * B:(i + 1) * B].contiguous()) for i in range(A)]

    def accumulated():
        for i, (xb, hb, tb) in enumerate(micro):
            model.loss_and_backward(xb, hb, tb, grad_scale=1.0 / A, micro_step=(i, A))

    def four_plain():
        for xb, hb, tb in micro:
            model.loss_and_backward(xb, hb, tb, grad_scale=1.0 / A)

    def one_big():
        model.loss_and_backward(x, h, t)
    fns = {"cycle_A4_B2": accumulated, "four_plain_B2": four_plain, "one_B8": one_big}   # (one_B8 re-makes the workspace per window)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: {s: v / 1e3 for s, v in sp.items()} for k, sp in alternate(fns, calls, windows).items()}
    return {"part": "cycle", "cfg": list(BENCH_CFG), "A": A, "B": B, "T": T, "calls_per_window": calls, "windows": windows,
            "ms": ms, "cycle_minus_four_plain_ms": ms["cycle_A4_B2"]["median"] - ms["four_plain_B2"]["median"],
            "cycle_minus_one_B8_ms": ms["cycle_A4_B2"]["median"] - ms["one_B8"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500, help="launches per timed window")
    ap.add_argument("--cycle-calls", type=int, default=10, help="cycles per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--parts", default="benchmark,recipe,cycle")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/accum_timing.py needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    for part in args.parts.split(","):
        res = cycle(args.cycle_calls, args.windows, dev) if part == "cycle" else launches(part, args.calls, args.windows, dev)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
