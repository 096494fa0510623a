#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""The bits one training step's backward pass produces, one sha256 per case, for comparing two builds of the library.

Each case is ``forward_loss`` + ``backward`` (with ``dh``) of a fresh engine on seeded inputs made on the host (the same for
every build).  The workspace is pre-filled with the finite garbage of ``tests/workspace_common.garbage_``, so a write that one
build makes and the other does not shows up; the digest covers the WHOLE workspace, the gradient buffer and ``dh``.

  shapes   configuration (32, 4, 64, 256, 3, 1, K, 16) for K = 1, 2, 3 at (B, T) = (2, 48), (1, 32), (3, 80): 48 and 80 leave a
           tile with lanes past T, T % 16 == 0 keeps the aux form of the gate epilogue legal, B > 1 crosses a sequence boundary
           inside a workgroup's tile walk; shape P2 of tests/plan_common.py (512 skip channels: the 18-chunk gate launch); and
           shape T1 of tests/workspace_common.py (receptive field 255 at T = 288: the only case whose loss window starts behind
           column 0 -- the window start is rounded down to 128 columns, so at the small shapes both t_first values are one plan)
  routes   the backward kernels of csrc/wn_fused.hip each arithmetic / plan flag selects (ROUTES below)
  t_first  the receptive field (the training step's loss window) and 0

A combination the library refuses prints ``refused`` in place of the digest.  Run it once per build (``WN_LIB_PATH`` selects a
library; ``--emu`` runs the host emulator, ``WN_LIB_PATH`` then names an emulator build) and compare the outputs line for line:

    python tools/bwd_bits.py --out profiles/bwd_fold/bwd_bits_gpu_branch.txt
"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pytorchwavenetvocoder_amd import _lib  # noqa: E402
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS, WaveNetEngine  # noqa: E402
from tests.plan_common import SHAPES  # noqa: E402
from tests.workspace_common import SHAPES as WS_SHAPES, garbage_  # noqa: E402

CASES = [("K%d B%d T%d" % (K, B, T), (32, 4, 64, 256, 3, 1, K, 16), B, T) for K in (1, 2, 3) for B, T in ((2, 48), (1, 32), (3, 80))]
CASES.append(("P2",) + SHAPES["P2"])
CASES.append(("T1",) + WS_SHAPES["T1"])
ROUTES = (
    ("default", DEFAULT_FLAGS),
    ("default-auxfused", DEFAULT_FLAGS & ~_lib.FLAG_AUX_FUSED),
    ("chain16", DEFAULT_FLAGS | _lib.FLAG_CHAIN_F16PAIR),
    ("chain16-auxfused", (DEFAULT_FLAGS | _lib.FLAG_CHAIN_F16PAIR) & ~_lib.FLAG_AUX_FUSED),
    ("six", SIX_PRODUCT_FLAGS),
    ("nochain", DEFAULT_FLAGS | _lib.FLAG_NO_CHAIN),
    ("nochain-auxfused", (DEFAULT_FLAGS | _lib.FLAG_NO_CHAIN) & ~_lib.FLAG_AUX_FUSED),
    ("exact", DEFAULT_FLAGS | _lib.FLAG_EXACT_MFMA),
)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def run_case(lib, dev, cfg, B, T, flags, t_first_rf, seed):
    eng = WaveNetEngine(*cfg, device=dev, library=lib)
    eng.flags = flags
    g = torch.Generator().manual_seed(seed)
    eng.flat_params.copy_(0.1 * torch.randn(eng.n_params, generator=g))
    x = torch.randint(0, cfg[0], (B, T), generator=g).to(dev)
    t = torch.randint(0, cfg[0], (B, T), generator=g).to(dev)
    h = torch.randn(B, cfg[1], T // cfg[7], generator=g).to(dev)
    garbage_(eng.workspace(B, T))
    _, dl = eng.forward_loss(x, h, t)
    eng.grads().fill_(float("nan"))
    dh = torch.full(h.shape, float("nan"), dtype=torch.float32, device=dev)
    eng.backward(dl, t_first=eng.receptive_field if t_first_rf else 0, dh=dh)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return sha(eng.workspace(B, T), eng.grads(), dh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--emu", action="store_true", help="the host emulator (tests/emu) instead of the GPU")
    ap.add_argument("--case", default="", help="only the shapes whose name contains this")
    args = ap.parse_args()
    if args.emu:
        from tests.emu import build_emu
        dev = torch.device("cpu")
        lib = _lib.load_library(os.environ.get("WN_LIB_PATH") or build_emu.build(), _test_emulator=True)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("tools/bwd_bits.py needs the GPU (or --emu)")
        dev = torch.device("cuda:0")
        lib = _lib.load_library()
    lines = []
    for ci, (name, cfg, B, T) in enumerate(CASES):
        if args.case not in name:
            continue
        for route, flags in ROUTES:
            for tf in (True, False):
                try:
                    digest = run_case(lib, dev, cfg, B, T, flags, tf, 1000 + ci)
                except _lib.WnError as e:
                    digest = "refused (%s)" % str(e).split("\n")[0][:80]
                lines.append("%s  %s %s t_first=%s" % (digest, name, route, "rf" if tf else "0"))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
