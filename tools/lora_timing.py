#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What the low-rank adapters cost.

HIP events around windows of calls, the variants alternating window by window in one process, median / min / max reported:

  ops    for the benchmark's model (bench.py: 64 / 256 channels, 30 layers) and the recipe-size model (512 / 256, 30 layers) at ranks
         8 and 32, on the default targets: ``wn_lora_merge`` (one launch) and ``wn_lora_project`` (two) against the torch loop over
         the adapted tensors in the same process -- ``torch.addmm`` into the weight views for the merge, two ``torch.mm`` per tensor
         into the views of the adapter gradient for the projection.  Per launch (the library's own per-launch events) the bytes it
         must move against the streaming plateau of this device (profiles/r06/stream_big.txt: 5.3 TB/s one read and one write,
         6.5 TB/s read only).
  step   the whole adapter step -- ``loss_and_backward`` + ``project()`` + ``AdapterAdam.step()`` (which ends with the merge) --
         against the ``FusedAdam`` fine-tuning step of the same model: every weight free, and ``train_only`` on the adapters' targets.

One JSON line per part.

    python tools/lora_timing.py [--calls 100] [--windows 7] [--step-calls 10] [--parts ops,step] [--out profiles/lora/lora_timing.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorchwavenetvocoder_amd.adapters import AdapterAdam, LowRankAdapters  # noqa: E402
from pytorchwavenetvocoder_amd.nets import WaveNet, initialize  # noqa: E402
from pytorchwavenetvocoder_amd.optim import FusedAdam  # noqa: E402
from tools.freeze_timing import MODELS, alternate, launch_table  # noqa: E402

PLATEAU_RW, PLATEAU_R = 5.3e12, 6.5e12   # bytes / s, profiles/r06/stream_big.txt (linear, mean)
RANKS = (8, 32)


def _model(cfg, dev):
    torch.manual_seed(1)
    model = WaveNet(*cfg)
    model.apply(initialize)
    model.to(dev)
    model.engine.flat_params.add_(1e-2 * torch.randn(model.engine.n_params, device=dev))
    return model


def ops(name, rank, calls, windows, dev):
    cfg = MODELS[name]
    model = _model(cfg, dev)
    eng = model.engine
    ad = LowRankAdapters(model, rank=rank)
    for b in ad.B.values():
        b.normal_(0.0, 0.02)
    eng.grads().copy_(1e-3 * torch.randn(eng.n_params, device=dev))
    ad.flat.grad = torch.zeros_like(ad.flat.data)
    params = list(model.parameters())
    pairs = []   # per tensor: weight view, base view, gradient view, A, B, dA, dB as 2-D tensors
    for (key, idx, w_off, rows, cols, a_off, b_off, shape), A, B in zip(ad.entries, ad.A.values(), ad.B.values()):
        sl = slice(w_off, w_off + rows * cols)
        pairs.append((eng.flat_params[sl].view(rows, cols), ad.base[sl].view(rows, cols), eng.grads()[sl].view(rows, cols), A, B,
                      ad.flat.grad[a_off:a_off + rank * cols].view(rank, cols), ad.flat.grad[b_off:b_off + rows * rank].view(rows, rank)))
    scale = ad.scale

    def project():
        for e in ad.entries:   # (project() clears the adapted p.grad: give them back, a host-only assignment)
            params[e[1]].grad = eng.grads()[e[2]:e[2] + e[3] * e[4]].view(e[7])
        ad.project()

    @torch.no_grad()
    def torch_merge():
        for w, b0, g, A, B, dA, dB in pairs:
            torch.addmm(b0, B, A, alpha=scale, out=w)

    @torch.no_grad()
    def torch_project():
        for w, b0, g, A, B, dA, dB in pairs:
            torch.mm(B.t(), g, out=dA)
            torch.mm(g, A.t(), out=dB)
        if scale != 1.0:
            ad.flat.grad.mul_(scale)
    # the two agree (the fused launches against the loop, loosely: both are fp32 sums in different orders)
    ad.merge()
    fused_w = eng.flat_params.clone()
    torch_merge()
    assert float((fused_w - eng.flat_params).abs().max()) <= 1e-5 * float(fused_w.abs().max())
    project()
    fused_g = ad.flat.grad.clone()
    torch_project()
    assert float((fused_g - ad.flat.grad).abs().max()) <= 1e-4 * float(fused_g.abs().max())
    fns = {"merge": ad.merge, "project": project, "torch_merge": torch_merge, "torch_project": torch_project}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = alternate(fns, calls, windows)
    table = launch_table(eng.lib, lambda: (ad.merge(), project()))
    elems = sum(e[3] * e[4] for e in ad.entries)
    scratch = ad._scratch_floats
    need = {"lora_merge": (8.0 * elems + 4.0 * ad.n_adapter, PLATEAU_RW), "lora_partials": (4.0 * elems + 4.0 * ad.n_adapter + 4.0 * scratch, PLATEAU_R),
            "lora_reduce": (4.0 * scratch + 4.0 * ad.n_adapter, PLATEAU_RW)}
    per_launch = {k: {"us": table[k]["us"], "launches": table[k]["launches"], "bytes": need[k][0],
                      "TBps": need[k][0] / (1e6 * table[k]["us"]), "of_plateau": need[k][0] / (1e-6 * table[k]["us"]) / need[k][1]}
                  for k in need}
    return {"part": "ops", "model": name, "cfg": list(cfg), "rank": rank, "tensors": len(ad.entries), "adapted_elements": elems,
            "adapter_elements": ad.n_adapter, "scratch_floats": scratch, "calls_per_window": calls, "windows": windows, "us": us,
            "per_launch_single_run": per_launch,
            "fused_over_torch": {"merge": us["merge"]["median"] / us["torch_merge"]["median"],
                                 "project": us["project"]["median"] / us["torch_project"]["median"]}}


def _batch(cfg, dev):
    B, T, U = 1, 3840, cfg[7]
    g = torch.Generator().manual_seed(7)
    xx = torch.randint(0, cfg[0], (B, T + 1), generator=g)
    return xx[:, :-1].contiguous().to(dev), torch.randn(B, cfg[1], T // U, generator=g).to(dev), xx[:, 1:].contiguous().to(dev)


def step(name, rank, calls, windows, dev):
    cfg = MODELS[name]
    batch = _batch(cfg, dev)
    full = _model(cfg, dev)
    full_opt = FusedAdam(full, lr=1e-4)
    adapted = _model(cfg, dev)
    ad = LowRankAdapters(adapted, rank=rank)
    ad_opt = AdapterAdam(ad, lr=1e-4)
    part = _model(cfg, dev)
    part.train_only(ad._pattern)
    part_opt = FusedAdam(part, lr=1e-4)

    def full_step():
        full.loss_and_backward(*batch)
        full_opt.step()

    def part_step():
        part.loss_and_backward(*batch)
        part_opt.step()

    def adapter_step():
        adapted.loss_and_backward(*batch)
        ad.project()
        ad_opt.step()
    fns = {"adapter_step": adapter_step, "fused_adam_all_weights": full_step, "fused_adam_train_only_targets": part_step}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = alternate(fns, calls, windows)
    return {"part": "step", "model": name, "cfg": list(cfg), "rank": rank, "B": 1, "T": 3840, "calls_per_window": calls, "windows": windows,
            "us": us, "trainable_elements": {"adapter": ad.n_adapter, "targets": sum(e[3] * e[4] for e in ad.entries),
                                             "all": full.engine.n_params},
            "adapter_over_all_weights": us["adapter_step"]["median"] / us["fused_adam_all_weights"]["median"],
            "adapter_over_train_only": us["adapter_step"]["median"] / us["fused_adam_train_only_targets"]["median"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window (ops)")
    ap.add_argument("--step-calls", type=int, default=10, help="steps per timed window (step)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--parts", default="ops,step")
    ap.add_argument("--models", default="benchmark,recipe")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/lora_timing.py needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda:0")
    for part in args.parts.split(","):
        for name in args.models.split(","):
            for rank in RANKS:
                res = ops(name, rank, args.calls, args.windows, dev) if part == "ops" else step(name, rank, args.step_calls, args.windows, dev)
                line = json.dumps(res)
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
