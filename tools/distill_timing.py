#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What the soft-target (knowledge distillation) loss costs on the benchmark instance (model 256/80/64/256/10/3/2/80, B = 8,
T = 23040, a teacher of the same size):

    python tools/distill_timing.py [--iters 20] [--steps 10] [--rounds 3] [--no-step] [--no-autograd]

kernel part -- one loss call on (B, 256, T) logits that already exist, HIP events around --iters calls, variants interleaved
round by round (a figure is the median over the rounds of a round's mean):
  softmax_ce[_nograd]          engine.loss: the stand-alone hard-label launch (reads the logits twice, writes dlogits)
  distill_tau1|2[_nograd]      engine.distill_loss at temperature 1 / 2 (reads student and teacher once, writes dlogits)
  wide_tau1|2[_nograd]         the same calls through k_softmax_distill_wide (WN_DISTILL_WIDE=1): a thread per position, plain
                               loops, each input read three times with dlogits and twice without -- the two-pass shape
  and, with the library's per-launch log, the softmax_distill launch alone (without the reduction behind it).
The floor of the kernel's own bytes is 3 * B * Q * T * 4 (2 * with _nograd) at a streaming plateau of 5.1 TB/s
(profiles/r06/stream_big.txt: `linear 2048wg`, 5.07 TB/s at 5 reads : 2 writes and 5.16 TB/s at 1 : 1 -- the file has no 2 : 1 row).

step part -- a training step (loss_and_backward + FusedAdam.step()), HIP events around --steps steps:
  plain            the benchmark's step (fused cross-entropy epilogue)
  teacher_forward  teacher.teacher_logits(x, h)
  distill          loss_and_backward(teacher_logits=...) with logits computed before (alpha 0.5, temperature 2)
  autograd         model(x, h) -> log_softmax / kl_div / cross_entropy under autograd -> backward() -> step(): the route the
                   feature replaces
Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLATEAU_TBS = 5.1


def interleaved(variants, iters, rounds):
    times = {k: [] for k, _ in variants}
    for k, fn in variants:           # warm-up: allocations, first launches
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in variants:
            fn(0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters)
    return times


def launch_ms(lib, fn, tag, n=10):
    """Mean HIP-event time of the launches tagged ``tag`` over n calls of fn (the library's per-launch log)."""
    lib.wn_prof_enable(1)
    try:
        for _ in range(n):
            fn(0)
    finally:
        lib.wn_prof_enable(0)
    torch.cuda.synchronize()
    need = lib.wn_prof_report(None, 0)
    buf = ctypes.create_string_buffer(max(need, 16))
    lib.wn_prof_report(buf, len(buf))
    rep = json.loads(buf.value.decode() or "{}")
    return rep.get(tag)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-autograd", action="store_true")
    args = ap.parse_args()
    from pytorchwavenetvocoder_amd.nets import WaveNet, initialize
    from pytorchwavenetvocoder_amd.optim import FusedAdam
    cfg_t, B, T, Q = (256, 80, 64, 256, 10, 3, 2, 80), 8, 23040, 256
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    model = WaveNet(*cfg_t)
    model.apply(initialize)
    model.to(dev)
    teacher = WaveNet(*cfg_t)
    teacher.apply(initialize)
    teacher.requires_grad_(False)
    teacher.to(dev)
    rs = np.random.RandomState(2)
    xx = torch.from_numpy(rs.randint(0, 256, size=(B, T + 1)).astype(np.int64))
    x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
    h = torch.from_numpy(rs.standard_normal((B, 80, T // 80)).astype(np.float32)).to(dev)
    eng = model.engine
    rf = model.receptive_field
    s = (3.0 * torch.randn((B, Q, T), device=dev)).contiguous()
    u = (3.0 * torch.randn((B, Q, T), device=dev)).contiguous()
    nbytes = B * Q * T * 4

    kernel_variants = [
        ("softmax_ce", lambda i: eng.loss(s, t, rf)),
        ("softmax_ce_nograd", lambda i: eng.loss(s, t, rf, want_grad=False)),
        ("distill_tau1", lambda i: eng.distill_loss(s, u, t, 0.5, 1.0, rf)),
        ("distill_tau1_nograd", lambda i: eng.distill_loss(s, u, t, 0.5, 1.0, rf, want_grad=False)),
        ("distill_tau2", lambda i: eng.distill_loss(s, u, t, 0.5, 2.0, rf)),
        ("distill_tau2_nograd", lambda i: eng.distill_loss(s, u, t, 0.5, 2.0, rf, want_grad=False)),
    ]
    def wide(fn):
        """The same call through the thread-per-position kernel (the library's WN_DISTILL_WIDE knob): the two-pass shape."""
        def run(i):
            os.environ["WN_DISTILL_WIDE"] = "1"
            try:
                return fn(i)
            finally:
                os.environ.pop("WN_DISTILL_WIDE", None)
        return run

    kernel_variants += [("wide_" + k[len("distill_"):], wide(fn)) for k, fn in kernel_variants if k.startswith("distill_")]
    kt = interleaved(kernel_variants, args.iters, args.rounds)
    out = {"B": B, "T": T, "Q": Q, "iters": args.iters, "rounds": args.rounds, "plateau_TBs": PLATEAU_TBS,
           "call_ms_by_round": kt, "call_ms_median": {k: float(np.median(v)) for k, v in kt.items()}}
    launches = {}
    for name, fn in kernel_variants:
        tag = "softmax_ce" if name.startswith("softmax_ce") else "softmax_distill"
        rep = launch_ms(eng.lib, fn, tag)
        moved = (2 if tag == "softmax_distill" else 1) + (0 if name.endswith("_nograd") else 1)
        if rep:
            ms = rep["ms"] / rep["count"] if "ms" in rep else None
            launches[name] = {"report": rep, "ms_per_launch": ms, "nominal_bytes": moved * nbytes}
            if ms:
                launches[name]["nominal_TBs"] = moved * nbytes / (ms * 1e-3) / 1e12
                launches[name]["fraction_of_floor"] = (moved * nbytes / (PLATEAU_TBS * 1e12)) / (ms * 1e-3)
    out["launch"] = launches
    del s, u
    if not args.no_step:
        opt = FusedAdam(model, lr=1e-4)
        tl = teacher.teacher_logits(x, h)
        alpha, tau = 0.5, 2.0

        def plain(i):
            model.loss_and_backward(x, h, t)
            opt.step()

        def teacher_forward(i):
            teacher.teacher_logits(x, h)

        def distill(i):
            model.loss_and_backward(x, h, t, teacher_logits=tl, distill_alpha=alpha, distill_temperature=tau)
            opt.step()

        def autograd(i):
            logits = model(x, h)[:, rf:].transpose(1, 2)                     # (B, Q, T - rf)
            ce = torch.nn.functional.cross_entropy(logits, t[:, rf:])
            ls = torch.log_softmax(logits / tau, 1)
            lp = torch.log_softmax(tl[:, :, rf:] / tau, 1)
            kl = torch.nn.functional.kl_div(ls, lp, reduction="sum", log_target=True) / (B * (T - rf))
            loss = (1 - alpha) * ce + alpha * tau * tau * kl
            model.zero_grad()
            loss.backward()
            opt.step()

        step_variants = [("plain", plain), ("teacher_forward", teacher_forward), ("distill", distill)]
        if not args.no_autograd:
            step_variants.append(("autograd", autograd))
        st = interleaved(step_variants, args.steps, args.rounds)
        med = {k: float(np.median(v)) for k, v in st.items()}
        out.update({"steps": args.steps, "step_ms_by_round": st, "step_ms_median": med,
                    "distill_minus_plain_ms": med["distill"] - med["plain"]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
