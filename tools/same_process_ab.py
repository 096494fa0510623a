#!/usr/bin/env python
"""The optimizer launches of TWO builds of the library in ONE process (csrc/wn_optim.inl).

Both libraries are loaded side by side and every launch -- the four Adam variants, ``wn_grad_norm``, ``wn_op_swap`` and the three
``wn_op_accumulate`` modes -- runs on the same buffers at the benchmark's and the recipe model's size, HIP events around windows
of calls, the two builds alternating window by window.  This takes out of an A/B what differs from process to process (where
the driver put the buffers), which at these sizes is more than the builds differ.  One JSON line per size.

    python tools/same_process_ab.py OTHER/libwavenet_hip.so [--out profiles/optim_fold/same_process_ab.txt]

"parent" in the output is the library given on the command line, "this" the tree's own build.
"""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorchwavenetvocoder_amd import _lib  # noqa: E402

dev = torch.device("cuda:0")
if len(sys.argv) < 2 or not torch.cuda.is_available():
    raise SystemExit("usage (on the GPU): tools/same_process_ab.py OTHER/libwavenet_hip.so [--out FILE]")
libs = {"parent": _lib.WnLibrary(os.path.abspath(sys.argv[1])), "this": _lib.load_library()}
st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
CALLS, WINDOWS = 200, 9
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None


def window_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / CALLS


for name, n in (("benchmark", 1594897), ("recipe", 46190161)):
    p, g, m, v, e, g2 = (1e-3 * torch.randn(n, device=dev) for _ in range(6))
    v.abs_()
    state = torch.zeros(ctypes.sizeof(_lib.WnOptState) // 8, dtype=torch.int64, device=dev)
    scratch = torch.zeros(int(libs["this"].wn_grad_norm_scratch_floats(n)), device=dev)
    P = lambda t: t.data_ptr()  # noqa: E731

    def make(lib):
        return {
            "grad_norm": lambda: lib.wn_grad_norm(P(g), n, 0, 0, 1e9, 1, 1e-4, 0.9, 0.999, P(scratch), P(state), st),
            "adam": lambda: lib.wn_adam_step(P(p), P(g), P(m), P(v), n, 1000, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0, 0, st),
            "adam_ema": lambda: lib.wn_adam_step_ema(P(p), P(g), P(m), P(v), P(e), n, 1000, 1e-4, 0.9, 0.999, 1e-8, 0.0, 0, 0, 0.9999, 0, st),
            "adam_guarded": lambda: lib.wn_adam_step_guarded(P(p), P(g), P(m), P(v), n, 1e-8, 0.0, 0, 0, P(state), st),
            "adam_guarded_ema": lambda: lib.wn_adam_step_guarded_ema(P(p), P(g), P(m), P(v), P(e), n, 1e-8, 0.0, 0, 0, P(state), 0.9999, 0, st),
            "swap": lambda: lib.wn_op_swap(P(e), P(g2), n, st),
            "accumulate_set": lambda: lib.wn_op_accumulate(P(e), P(g), n, 0, st),
            "accumulate_add": lambda: lib.wn_op_accumulate(P(e), P(g), n, 1, st),
            "accumulate_finish": lambda: lib.wn_op_accumulate(P(e), P(g2), n, 2, st),
        }
    fns = {k: make(lib) for k, lib in libs.items()}
    assert libs["this"].wn_grad_norm(P(g), n, 0, 0, 1e9, 1, 1e-4, 0.9, 0.999, P(scratch), P(state), st) == 0   # apply = 1 in the state block
    for k in fns:
        for fn in fns[k].values():
            for _ in range(3):
                assert fn() == 0
    torch.cuda.synchronize()
    times = {k: {op: [] for op in fns[k]} for k in fns}
    for _ in range(WINDOWS):
        for op in fns["this"]:
            for k in ("parent", "this"):
                times[k][op].append(window_us(fns[k][op]))
    res = {"model": name, "n": n, "calls_per_window": CALLS, "windows": WINDOWS,
           "us": {op: {k: {"median": statistics.median(times[k][op]), "min": min(times[k][op]), "max": max(times[k][op])} for k in times}
                  for op in fns["this"]}}
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")
    del p, g, m, v, e, g2
    torch.cuda.empty_cache()
