#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""The bits the optimizer-side entry points produce (csrc/wn_optim.inl), one sha256 per case, for comparing two builds.

Drives the public C entry points through ctypes on seeded inputs (made on the host: the same for every build):

  adam       ``wn_adam_step``, ``wn_adam_step_ema``, ``wn_adam_step_guarded``, ``wn_adam_step_guarded_ema``: three steps each,
             weight decay 0 and 1e-2, skip range [1021, 1290), n = 5003 and n = 600 001 (beyond one trip of the 2048 x 256 grid);
             the guarded ones behind ``wn_grad_norm`` with the clip active (max_norm = half the norm), and once more with a NaN
             in the second step's gradient (the guard skips it).  The digest covers p, m, v, the average and the state block.
  grad_norm  ``wn_grad_norm`` at n = 5003 and n = 2 200 003 (beyond one trip of its 512-block grid), the base pointer 0 and 1
             floats behind a 16-byte boundary.  The digest covers the whole state block and the per-block partial sums in the
             scratch buffer (which block adds which element depends on the alignment: the two offsets give two digests).
  swap, accumulate   ``wn_op_swap`` and the three modes of ``wn_op_accumulate`` at n = 1, 7, 5003, 600 001 with the two pointers
             (0, 0), (1, 1) and (1, 2) floats behind a 16-byte boundary.  The digest covers both backing buffers, margins included.

Run it once per build (``WN_LIB_PATH=other/libwavenet_hip.so`` selects one) and compare the outputs line for line:

    python tools/optim_bits.py --out profiles/optim_fold/optim_bits_this.txt
"""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorchwavenetvocoder_amd import _lib  # noqa: E402
from pytorchwavenetvocoder_amd.engine import _stream_handle  # noqa: E402

SKIP = (1021, 1290)
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.999, 1e-8
EMA_DECAY, MARGIN = 0.999, 8


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def view_at(n, offset, dev, fill=None):
    """n floats `offset` floats behind a 16-byte boundary inside a backing buffer with MARGIN floats on either side"""
    whole = torch.full((n + 2 * MARGIN + 4,), -7.0, device=dev)
    assert whole.data_ptr() % 16 == 0
    v = whole[MARGIN + offset:MARGIN + offset + n]
    if fill is not None:
        v.copy_(fill)
    return whole, v


def adam_cases(lib, dev, st):
    for n in (5003, 600001):
        g = torch.Generator().manual_seed(n)
        p0 = torch.randn(n, generator=g)
        grads = [1e-2 * torch.randn(n, generator=g) for _ in range(3)]
        for kind in ("plain", "ema", "guarded", "guarded_ema", "guarded_nan", "guarded_ema_nan"):
            guarded, ema, nan = "guarded" in kind, "ema" in kind, kind.endswith("nan")
            for wd in (0.0, 1e-2):
                p, m, v = p0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
                e = p.clone() if ema else None
                state = torch.zeros(ctypes.sizeof(_lib.WnOptState) // 8, dtype=torch.int64, device=dev)
                scratch = torch.zeros(int(lib.wn_grad_norm_scratch_floats(n)), device=dev)
                for step, gh in enumerate(grads, 1):
                    gh = gh.clone()
                    if nan and step == 2:
                        gh[n // 2] = float("nan")
                    gd = gh.to(dev)
                    if guarded:
                        live = torch.cat([gh[:SKIP[0]], gh[SKIP[1]:]]).double()
                        max_norm = 0.5 * float(live[torch.isfinite(live)].norm())
                        lib.check(lib.wn_grad_norm(gd.data_ptr(), n, SKIP[0], SKIP[1], max_norm, 1, LR, BETA1, BETA2,
                                                   scratch.data_ptr(), state.data_ptr(), st), "wn_grad_norm")
                    if kind == "plain":
                        rc = lib.wn_adam_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, LR, BETA1, BETA2, EPS,
                                              wd, SKIP[0], SKIP[1], st)
                    elif kind == "ema":
                        rc = lib.wn_adam_step_ema(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, step, LR,
                                                  BETA1, BETA2, EPS, wd, SKIP[0], SKIP[1], EMA_DECAY, 1, st)
                    elif ema:
                        rc = lib.wn_adam_step_guarded_ema(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), n, EPS,
                                                          wd, SKIP[0], SKIP[1], state.data_ptr(), EMA_DECAY, 1, st)
                    else:
                        rc = lib.wn_adam_step_guarded(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, EPS, wd, SKIP[0],
                                                      SKIP[1], state.data_ptr(), st)
                    lib.check(rc, "adam " + kind)
                    torch.cuda.synchronize()
                outs = [p, m, v] + ([e] if ema else []) + ([state] if guarded else [])
                yield "adam %s wd=%g n=%d" % (kind, wd, n), sha(*outs)


def grad_norm_cases(lib, dev, st):
    for n in (5003, 2200003):
        gh = 1e-2 * torch.randn(n, generator=torch.Generator().manual_seed(n))
        for offset in (0, 1):
            _, gd = view_at(n, offset, dev, gh)
            state = torch.zeros(ctypes.sizeof(_lib.WnOptState) // 8, dtype=torch.int64, device=dev)
            scratch = torch.zeros(int(lib.wn_grad_norm_scratch_floats(n)), device=dev)
            lib.check(lib.wn_grad_norm(gd.data_ptr(), n, SKIP[0], SKIP[1], 0.05, 1, LR, BETA1, BETA2, scratch.data_ptr(),
                                       state.data_ptr(), st), "wn_grad_norm")
            torch.cuda.synchronize()
            yield "grad_norm n=%d offset=%d" % (n, offset), sha(state, scratch)


def pair_cases(lib, dev, st):
    ops = [("swap", None), ("accumulate_set", _lib.ACCUM_SET), ("accumulate_add", _lib.ACCUM_ADD),
           ("accumulate_finish", _lib.ACCUM_FINISH)]
    for n in (1, 7, 5003, 600001):
        g = torch.Generator().manual_seed(100 + n)
        ah, bh = torch.randn(n, generator=g), torch.randn(n, generator=g)
        for oa, ob in ((0, 0), (1, 1), (1, 2)):
            for name, mode in ops:
                wa, a = view_at(n, oa, dev, ah)
                wb, b = view_at(n, ob, dev, bh)
                if mode is None:
                    rc = lib.wn_op_swap(a.data_ptr(), b.data_ptr(), n, st)
                else:
                    rc = lib.wn_op_accumulate(a.data_ptr(), b.data_ptr(), n, mode, st)
                lib.check(rc, name)
                torch.cuda.synchronize()
                yield "%s n=%d offsets=(%d,%d)" % (name, n, oa, ob), sha(wa, wb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/optim_bits.py needs the GPU: the digests are those of the gfx950 kernels")
    dev = torch.device("cuda:0")
    lib = _lib.load_library()
    st = _stream_handle(dev)
    lines = []
    for cases in (adam_cases, grad_norm_cases, pair_cases):
        for name, digest in cases(lib, dev, st):
            lines.append("%s  %s" % (digest, name))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
