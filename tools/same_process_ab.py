#!/usr/bin/env python
"""Launches of TWO builds of the library in ONE process: the optimizer launches (csrc/wn_optim.inl) or, with ``--backward``, the
launches of the backward pass (csrc/wn_fused.hip and the rest of ``wn_backward``).

Both libraries are loaded side by side, windows of calls alternate between the two builds.  This takes out of an A/B what differs
from process to process (where the driver put the buffers), which is often more than the builds differ.

  default      every optimizer launch -- the four Adam variants, ``wn_grad_norm``, ``wn_op_swap`` and the three
               ``wn_op_accumulate`` modes -- on the SAME buffers at the benchmark's and the recipe model's size, HIP events around
               windows of calls.  One JSON line per size.
  --backward   each build gets an engine of the benchmark's model (BASELINE configs[1], B = 8, T = 23040; ``--recipe``: the K = 3
               model of tools/recipe_bench.py) with the same weights and runs the same ``forward_loss``; then windows of
               ``backward`` calls alternate, the library's own launch profiler (HIP events per launch) around each window.  One JSON
               line: ms per step of every ``fused_bwd_*`` tag and of all launches of the call together (``backward_total``), median
               (min, max) over the windows.  ``WN_ENGINE_FLAGS`` selects the arithmetic.  The two engines have their own buffers;
               ``--this-first`` loads, allocates and times this tree's build first, to see whether a difference follows the order.

    python tools/same_process_ab.py OTHER/libwavenet_hip.so [--backward [--recipe] [--this-first]] [--out FILE]

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
    raise SystemExit("usage (on the GPU): tools/same_process_ab.py OTHER/libwavenet_hip.so [--backward [--recipe] [--this-first]] [--out FILE]")
order = ("this", "parent") if "--this-first" in sys.argv else ("parent", "this")
libs = {k: (_lib.WnLibrary(os.path.abspath(sys.argv[1])) if k == "parent" else _lib.load_library()) for k in order}
st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
WINDOWS = 9
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def optimizer_ab():
    CALLS = 200

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
                for k in order:
                    times[k][op].append(window_us(fns[k][op]))
        emit({"model": name, "n": n, "calls_per_window": CALLS, "windows": WINDOWS,
              "us": {op: {k: spread(times[k][op]) for k in times} for op in fns["this"]}})
        del p, g, m, v, e, g2
        torch.cuda.empty_cache()


def backward_ab():
    from pytorchwavenetvocoder_amd.engine import WaveNetEngine
    CALLS = 5
    cfg, B, T = (256, 80, 64, 256, 10, 3, 2, 80), 8, 23040
    if "--recipe" in sys.argv:
        cfg, B, T = (256, 80, 64, 256, 10, 3, 3, 256), 8, 26112
    g = torch.Generator().manual_seed(7)
    x = torch.randint(0, cfg[0], (B, T), generator=g).to(dev)
    t = torch.randint(0, cfg[0], (B, T), generator=g).to(dev)
    h = torch.randn(B, cfg[1], T // cfg[7], generator=g).to(dev)
    runs = {}
    for k in order:
        eng = WaveNetEngine(*cfg, device=dev, library=libs[k])
        eng.flat_params.copy_(0.05 * torch.randn(eng.n_params, generator=torch.Generator().manual_seed(8)))
        _, dl = eng.forward_loss(x, h, t)
        eng.backward(dl)   # warm-up
        runs[k] = (eng, dl, {})
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for k in order:
            eng, dl, acc = runs[k]
            eng.lib.wn_prof_enable(1)
            for _ in range(CALLS):
                eng.backward(dl)
            torch.cuda.synchronize()
            eng.lib.wn_prof_enable(0)
            buf = ctypes.create_string_buffer(max(eng.lib.wn_prof_report(None, 0), 16))
            eng.lib.wn_prof_report(buf, len(buf))
            prof = json.loads(buf.value.decode() or "{}")
            acc.setdefault("backward_total", []).append(sum(v["ms"] for v in prof.values()) / CALLS)
            for tag, v in prof.items():
                if tag.startswith("fused_bwd"):
                    acc.setdefault(tag, []).append(v["ms"] / CALLS)
    emit({"model": "recipe K=3" if "--recipe" in sys.argv else "benchmark", "flags": runs["this"][0].flags, "order": list(order),
          "calls_per_window": CALLS, "windows": WINDOWS,
          "ms": {tag: {k: spread(runs[k][2][tag]) for k in ("parent", "this")} for tag in sorted(runs["this"][2])}})


if "--backward" in sys.argv:
    backward_ab()
else:
    optimizer_ab()
