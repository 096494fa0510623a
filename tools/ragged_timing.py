#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What a padded batch of unequal lengths costs on the benchmark instance (model 256/80/64/256/10/3/2/80, B = 8, T = 23040):

    python tools/ragged_timing.py [--steps 20] [--rounds 3]

  dense        loss_and_backward(x, h, t) + FusedAdam.step()                      (the benchmark's step)
  full         the same with lengths=[T] * B                                     (the ragged entry point, nothing masked)
  ragged       lengths uniform in [T / 2, T] (seeded)
  autograd     model(x, h) -> nn.CrossEntropyLoss() with -100 targets behind each length -> backward() -> step(): the only
               route to a masked loss before ``lengths=`` existed (logits materialised, gradient scale found by a scan)
  new_lengths  ragged with a DIFFERENT lengths vector every step (one upload of B integers per step)
  workspace    engine.workspace(B, T') for a T' not seen before: the re-allocation + zero-fill a run with varying T pays per step

Variants are interleaved round by round on the same device; a figure is the median over the rounds of the mean step time of a
round (HIP events around --steps steps).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-autograd", action="store_true")
    args = ap.parse_args()
    from pytorchwavenetvocoder_amd.nets import WaveNet, initialize
    from pytorchwavenetvocoder_amd.optim import FusedAdam
    cfg_t, B, T = (256, 80, 64, 256, 10, 3, 2, 80), 8, 23040
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    model = WaveNet(*cfg_t)
    model.apply(initialize)
    model.to(dev)
    opt = FusedAdam(model, lr=1e-4)
    rs = np.random.RandomState(2)
    xx = torch.from_numpy(rs.randint(0, 256, size=(B, T + 1)).astype(np.int64))
    x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
    h = torch.from_numpy(rs.standard_normal((B, 80, T // 80)).astype(np.float32)).to(dev)
    rf, Q = model.receptive_field, 256
    lengths = [int(v) for v in rs.randint(T // 2, T + 1, size=B)]
    many = [[int(v) for v in rs.randint(T // 2, T + 1, size=B)] for _ in range(args.steps)]
    tm = t.clone()
    for b, n in enumerate(lengths):
        tm[b, n:] = -100
    crit = torch.nn.CrossEntropyLoss()

    def dense(i):
        model.loss_and_backward(x, h, t)
        opt.step()

    def full(i):
        model.loss_and_backward(x, h, t, lengths=[T] * B)
        opt.step()

    def ragged(i):
        model.loss_and_backward(x, h, t, lengths=lengths)
        opt.step()

    def new_lengths(i):
        model.loss_and_backward(x, h, t, lengths=many[i])
        opt.step()

    def autograd(i):
        out = model(x, h)
        loss = crit(out[:, rf:].contiguous().view(-1, Q), tm[:, rf:].contiguous().view(-1))
        model.zero_grad()
        loss.backward()
        opt.step()

    variants = [("dense", dense), ("full", full), ("ragged", ragged), ("new_lengths", new_lengths)]
    if not args.no_autograd:
        variants.append(("autograd", autograd))
    times = {k: [] for k, _ in variants}
    for k, fn in variants:           # warm-up: allocations, first launches
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in variants:
            fn(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.steps)
    out = {"B": B, "T": T, "lengths": lengths, "loss_positions": sum(n - rf for n in lengths), "steps": args.steps,
           "ms_per_step_by_round": times, "ms_per_step_median": {k: float(np.median(v)) for k, v in times.items()}}
    # the workspace of a (B, T') not seen before: free + allocate + zero-fill (wall time, device synchronised)
    eng = model.engine
    ws = []
    for Tn in (T - 80, T - 160, T - 240, T - 320):
        torch.cuda.synchronize()
        t0 = time.time()
        eng.workspace(B, Tn)
        torch.cuda.synchronize()
        ws.append((time.time() - t0) * 1e3)
    out["workspace_realloc_ms"] = ws
    print(json.dumps(out))


if __name__ == "__main__":
    main()
