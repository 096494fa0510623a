#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What scoring a batch costs: ``WaveNet.evaluate`` against ``forward_loss(want_grad=False)``.

``evaluate`` is ``forward_loss`` without a gradient plus ONE single-workgroup launch (``row_sums`` instead of ``sum_partials``), in
a workspace of its own.  Two batches of the benchmark's model (bench.py: 64 / 256 channels, U = 80): the benchmark's own size
(B = 8 windows of 20000 + receptive field samples, T = 23040) and one padded utterance batch (B = 8 utterances of 2 - 4 s at
16 kHz padded to T = 64000, ``lengths=``).  HIP events around alternating windows of ``--steps`` calls of each (both see the same
neighbours on a shared machine), then one call of each under the library's launch log (per-launch HIP-event times).
``forward_loss(want_grad=False)`` is the entry point as it was before ``evaluate`` existed: nothing on its path changed.  One
JSON line per batch.

    python tools/eval_timing.py [--steps 20] [--windows 9] [--out profiles/eval/eval_timing.txt]
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

CFG = (256, 80, 64, 256, 10, 3, 2, 80)
BATCHES = {"benchmark": (8, 23040, None), "utterances": (8, 64000, [32000 + 80 * ((i * 32000 // 7) // 80) for i in range(8)])}


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
    return {k: {"launches": v["count"], "us": round(1e3 * v["ms"], 2)} for k, v in json.loads(buf.value.decode() or "{}").items()}


def window_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def measure(name, steps, windows, device="cuda:0"):
    if not torch.cuda.is_available():
        raise SystemExit("tools/eval_timing.py needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device(device)
    B, T, lengths = BATCHES[name]
    torch.manual_seed(1)
    model = WaveNet(*CFG)
    model.apply(initialize)
    model.to(dev)
    eng = model.engine
    g = torch.Generator().manual_seed(7)
    xx = torch.randint(0, CFG[0], (B, T + 1), generator=g)
    x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
    h = torch.randn(B, CFG[1], T // CFG[7], generator=g).to(dev)
    acc = torch.zeros(1, dtype=torch.float64, device=dev)
    kw = {} if lengths is None else {"lengths": lengths}
    calls = {"forward_loss_no_grad": lambda: eng.forward_loss(x, h, t, want_grad=False, **kw),
             "evaluate": lambda: model.evaluate(x, h, t=t, acc=acc, **kw)}
    for fn in calls.values():   # allocate both workspaces, warm up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(windows):
        for k, fn in calls.items():
            times[k].append(window_ms(fn, steps))
    out = {"batch": name, "cfg": list(CFG), "B": B, "T": T, "lengths": lengths, "steps_per_window": steps, "windows": windows}
    for k, v in times.items():
        out[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["evaluate_minus_forward_loss_ms"] = round(out["evaluate_ms"]["median"] - out["forward_loss_no_grad_ms"]["median"], 4)
    for k, fn in calls.items():
        out[k + "_launches"] = launch_table(eng.lib, fn)
    loss, _ = calls["forward_loss_no_grad"]()
    row, counts = model.evaluate(x, h, t=t, **kw)
    out["loss"], out["pooled_mean"] = float(loss), float(row.double().sum()) / sum(counts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--batches", default="benchmark,utterances")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    for name in args.batches.split(","):
        line = json.dumps(measure(name, args.steps, args.windows))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
