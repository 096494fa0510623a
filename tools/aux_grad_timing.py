#!/usr/bin/env python
"""Backward-pass time with the gradient with respect to the aux features (wn_backward_dh) at the benchmark's model.

For the headline model (256, 80, 64, 256, 10, 3, 2, U) at B = 8, T = 23040, U = 80 and U = 0, after one forward_loss: the
backward with dh off (the training step's call), with dh on, and with dh only (param_grads=False, a frozen vocoder), as the
median of HIP-event timed repeats; then one call with the per-launch log on for the dh launches themselves.  One JSON line
per U on stdout; ``--out FILE`` also writes them together to FILE.

    python tools/aux_grad_timing.py [--reps N] [--B B] [--T T] [--out FILE]      (on an MI355X)
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pytorchwavenetvocoder_amd.nets import WaveNet, initialize  # noqa: E402


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def prof(lib, fn):
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=23040)
    ap.add_argument("--out", default=None, help="also write the results as one JSON file")
    a = ap.parse_args()
    dev = "cuda:0"
    out = {"B": a.B, "T": a.T, "reps": a.reps, "cases": {}}
    for U in (80, 0):
        torch.manual_seed(1)
        m = WaveNet(256, 80, 64, 256, 10, 3, 2, U)
        m.apply(initialize)
        m.to(dev)
        eng = m.engine
        x = torch.randint(0, 256, (a.B, a.T), device=dev)
        t = torch.randint(0, 256, (a.B, a.T), device=dev)
        h = torch.randn(a.B, 80, a.T // U if U else a.T, device=dev)
        dh = torch.empty_like(h)
        _, dl = eng.forward_loss(x, h, t)
        rf = eng.receptive_field
        modes = {"dh_off": lambda: eng.backward(dl, t_first=rf),
                 "dh_on": lambda: eng.backward(dl, t_first=rf, dh=dh),
                 "dh_only": lambda: eng.backward(dl, t_first=rf, dh=dh, param_grads=False)}
        for f in modes.values():   # warm-up
            f()
        torch.cuda.synchronize()
        r = {k: timed(f, a.reps) for k, f in modes.items()}
        rep = prof(eng.lib, modes["dh_on"])
        r["aux_dh_ms"] = {k: v for k, v in rep.items() if k.startswith("aux_dh")}
        r["fwd_aux_frames"] = prof(eng.lib, lambda: eng.forward(x, h)).get("fwd_aux_frames")
        r["dh_only_over_dh_off"] = r["dh_only"] / r["dh_off"]
        out["cases"]["U%d" % U] = r
        print(json.dumps({"U": U, **r}), flush=True)
        del m, eng, dl, dh
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
