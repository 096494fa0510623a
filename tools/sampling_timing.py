#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What temperature / top-k / top-p sampling (csrc/wn_sample.h) costs per decode step, against plain sampling in the same run:

    python tools/sampling_timing.py [--rounds 5] [--steps 512] [--wide-steps 96] [--plain-only]

  k_decode   the benchmark's model 256/80/64/256/10/3/2/80 (one workgroup per utterance), 1 and 64 utterances
  any-size   the recipes' n_resch 512 model 256/80/512/256/10/3/2/80 (one persistent launch: k_dlp for one utterance, k_dlpf for
             16 and 64), 1, 16 and 64 utterances

A figure is the HIP-event time of the decode launch itself (the library's per-launch log: the `*_steps` / `*_steps_filtered`
tag) divided by its steps, so packing, prefill and allocations of a decode call are not in it.  The variants -- plain argmax,
plain sampling and the five settings of the tests -- alternate round by round; median, min and max over the rounds, and the
added microseconds per step against plain sampling.  --plain-only: argmax and sampling only (the interleaved comparison with a
build of the parent commit runs this tool in both trees).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [("T0.8", dict(temperature=0.8)), ("k8", dict(top_k=8)), ("p0.9", dict(top_p=0.9)),
            ("T0.7_k16_p0.95", dict(temperature=0.7, top_k=16, top_p=0.95)), ("T2_koff_p1", dict(temperature=2.0, top_k=261, top_p=1.0))]


def launch_report(lib, fn):
    lib.wn_prof_enable(1)
    try:
        fn()
    finally:
        lib.wn_prof_enable(0)
    torch.cuda.synchronize()
    need = lib.wn_prof_report(None, 0)
    buf = ctypes.create_string_buffer(max(need, 16))
    lib.wn_prof_report(buf, len(buf))
    return json.loads(buf.value.decode() or "{}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--wide-steps", type=int, default=96)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    from pytorchwavenetvocoder_amd.nets import WaveNet, initialize
    dev = torch.device("cuda:0")
    variants = [("argmax", dict(mode="argmax")), ("sampling", dict(mode="sampling"))]
    if not args.plain_only:
        variants += [(k, dict(mode="sampling", **v)) for k, v in SETTINGS]
    out = {"rounds": args.rounds, "us_per_step": {}}
    for label, cfg_t, batches, n in (("k_decode", (256, 80, 64, 256, 10, 3, 2, 80), (1, 64), args.steps),
                                     ("any_size_r512", (256, 80, 512, 256, 10, 3, 2, 80), (1, 16, 64), args.wide_steps)):
        torch.manual_seed(1)
        model = WaveNet(*cfg_t)
        model.apply(initialize)
        model.to(dev)
        eng = model.engine
        rs = np.random.RandomState(2)
        for B in batches:
            x = torch.from_numpy(rs.randint(0, 256, (B, 1))).long().to(dev)
            h = torch.from_numpy(rs.standard_normal((B, 80, (n + 1) // 80 + 2)).astype(np.float32)).to(dev)
            times = {k: [] for k, _ in variants}
            tags = {}
            for k, kw in variants:   # warm-up
                eng.decode(x, h, [n] * B, **kw)
            for _ in range(args.rounds):
                for k, kw in variants:
                    torch.manual_seed(3)
                    rep = launch_report(eng.lib, lambda: eng.decode(x, h, [n] * B, **kw))
                    hit = [(t, v) for t, v in rep.items() if t.endswith("_steps") or t.endswith("_steps_filtered")]
                    assert len(hit) == 1, rep.keys()
                    tags[k] = hit[0][0]
                    times[k].append(hit[0][1]["ms"] * 1e3 / n)
            base = float(np.median(times["sampling"]))
            out["us_per_step"]["%s_B%d" % (label, B)] = {
                k: {"tag": tags[k], "median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)),
                    "added_vs_sampling": float(np.median(v)) - base} for k, v in times.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
