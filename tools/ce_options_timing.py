#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What the weighted cross-entropy head (class weights, label smoothing, position weights) costs on the benchmark instance
(model 256/80/64/256/10/3/2/80, B = 8, T = 23040):

    python tools/ce_options_timing.py [--iters 20] [--steps 10] [--rounds 3] [--no-step] [--no-autograd]

kernel part -- one loss call on (B, 256, T) logits that already exist, HIP events around --iters calls, variants interleaved
round by round (a figure is the median over the rounds of a round's mean):
  softmax_ce[_nograd]        engine.loss: the stand-alone plain launch (reads the logits twice, writes dlogits)
  distill_tau1[_nograd]      engine.distill_loss at temperature 1 (two inputs read once): the upper yardstick
  cew_<opt>[_nograd]         engine.weighted_loss with <opt> in w (class weights), eps (smoothing 0.1), r (position weights),
                             all (the three), each with normalize="weights"; all_pos: the three with normalize="positions"
                             (no divisor launches)
  wide_<opt>[_nograd]        the same calls through k_softmax_cew_wide (WN_CEW_WIDE=1): a thread per position, plain loops
  and, with the library's per-launch log, the softmax_cew / ce_divisor / cew_reduce launches alone.
The floor of the kernel's own bytes is 2 * B * Q * T * 4 = 377 MB (1 * with _nograd) at a streaming plateau of 5.1 TB/s
(profiles/r06/stream_big.txt).

step part -- a training step (loss_and_backward + FusedAdam.step()), HIP events around --steps steps:
  plain      the benchmark's step (fused cross-entropy epilogue)
  distill    loss_and_backward(teacher_logits=...) with logits computed before (alpha 0.5, temperature 1): the other loss head
  cew        loss_and_backward(class_weights=, label_smoothing=0.1, position_weights=)
  autograd   model(x, h) -> F.cross_entropy(weight=, label_smoothing=) under autograd -> backward() -> step(): the route the
             feature replaces (no position weights: torch's criterion has none)
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.distill_timing import PLATEAU_TBS, interleaved, launch_ms  # noqa: E402


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
    rs = np.random.RandomState(2)
    xx = torch.from_numpy(rs.randint(0, 256, size=(B, T + 1)).astype(np.int64))
    x, t = xx[:, :-1].contiguous().to(dev), xx[:, 1:].contiguous().to(dev)
    h = torch.from_numpy(rs.standard_normal((B, 80, T // 80)).astype(np.float32)).to(dev)
    w = torch.from_numpy(rs.uniform(0.25, 4.0, Q).astype(np.float32)).to(dev)
    r = torch.from_numpy(rs.uniform(0.0, 2.0, (B, T)).astype(np.float32)).to(dev)
    eng = model.engine
    rf = model.receptive_field
    s = (3.0 * torch.randn((B, Q, T), device=dev)).contiguous()
    u = (3.0 * torch.randn((B, Q, T), device=dev)).contiguous()
    nbytes = B * Q * T * 4
    options = {"w": (w, 0.0, None, "weights"), "eps": (None, 0.1, None, "weights"), "r": (None, 0.0, r, "weights"),
               "all": (w, 0.1, r, "weights"), "all_pos": (w, 0.1, r, "positions")}

    def cew(opt, grad):
        cw, eps, pw, norm = options[opt]
        return lambda i: eng.weighted_loss(s, t, cw, eps, pw, norm, t_start=rf, want_grad=grad)

    def wide(fn):
        """The same call through the thread-per-position kernel (the library's WN_CEW_WIDE knob)."""
        def run(i):
            os.environ["WN_CEW_WIDE"] = "1"
            try:
                return fn(i)
            finally:
                os.environ.pop("WN_CEW_WIDE", None)
        return run

    kernel_variants = [
        ("softmax_ce", lambda i: eng.loss(s, t, rf)),
        ("softmax_ce_nograd", lambda i: eng.loss(s, t, rf, want_grad=False)),
        ("distill_tau1", lambda i: eng.distill_loss(s, u, t, 0.5, 1.0, rf)),
        ("distill_tau1_nograd", lambda i: eng.distill_loss(s, u, t, 0.5, 1.0, rf, want_grad=False)),
    ]
    for opt in options:
        kernel_variants += [("cew_" + opt, cew(opt, True)), ("cew_%s_nograd" % opt, cew(opt, False))]
    for opt in ("eps", "all"):
        kernel_variants += [("wide_" + opt, wide(cew(opt, True))), ("wide_%s_nograd" % opt, wide(cew(opt, False)))]
    kt = interleaved(kernel_variants, args.iters, args.rounds)
    out = {"B": B, "T": T, "Q": Q, "iters": args.iters, "rounds": args.rounds, "plateau_TBs": PLATEAU_TBS,
           "call_ms_by_round": kt, "call_ms_median": {k: float(np.median(v)) for k, v in kt.items()}}
    launches = {}
    for name, fn in kernel_variants:
        tag = "softmax_ce" if name.startswith("softmax_ce") else "softmax_distill" if name.startswith("distill") else "softmax_cew"
        moved = {"softmax_ce": 1, "softmax_distill": 2, "softmax_cew": 1}[tag] + (0 if name.endswith("_nograd") else 1)
        entry = {}
        for tg in (tag, "ce_divisor", "ce_divisor_tail", "cew_reduce"):
            rep = launch_ms(eng.lib, fn, tg)
            if rep and "ms" in rep:
                entry[tg + "_ms"] = rep["ms"] / rep["count"]
        ms = entry.get(tag + "_ms")
        if ms:
            entry.update(nominal_bytes=moved * nbytes, nominal_TBs=moved * nbytes / (ms * 1e-3) / 1e12,
                         fraction_of_floor=(moved * nbytes / (PLATEAU_TBS * 1e12)) / (ms * 1e-3))
        launches[name] = entry
    out["launch"] = launches
    del s
    if not args.no_step:
        opt = FusedAdam(model, lr=1e-4)
        tl = u

        def plain(i):
            model.loss_and_backward(x, h, t)
            opt.step()

        def distill(i):
            model.loss_and_backward(x, h, t, teacher_logits=tl, distill_alpha=0.5, distill_temperature=1.0)
            opt.step()

        def weighted(i):
            model.loss_and_backward(x, h, t, class_weights=w, label_smoothing=0.1, position_weights=r)
            opt.step()

        def autograd(i):
            logits = model(x, h)[:, rf:].transpose(1, 2)                     # (B, Q, T - rf)
            loss = torch.nn.functional.cross_entropy(logits, t[:, rf:], weight=w, label_smoothing=0.1)
            model.zero_grad()
            loss.backward()
            opt.step()

        step_variants = [("plain", plain), ("distill", distill), ("cew", weighted)]
        if not args.no_autograd:
            step_variants.append(("autograd", autograd))
        st = interleaved(step_variants, args.steps, args.rounds)
        med = {k: float(np.median(v)) for k, v in st.items()}
        out.update({"steps": args.steps, "step_ms_by_round": st, "step_ms_median": med, "cew_minus_plain_ms": med["cew"] - med["plain"]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
