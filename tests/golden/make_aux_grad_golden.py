#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Golden fixture of the reference MODULE's gradient with respect to the aux features, for tests/test_emu_aux_grad.py.

    python oracle/build_ref.py && python tests/golden/make_aux_grad_golden.py
    # writes tests/golden/aux_grad.npz

Drives the reference's own model file (``oracle/_ref/wavenet.py``, the build-time copy made by oracle/build_ref.py) with the
loss of its training loop (nn.CrossEntropyLoss on ``[:, receptive_field:]``, train.py:533-536) on three small models -- the
upsampling layer with kernel_size 2 and 3, and no upsampling layer -- one thread, and stores dL/dh and the loss.  Inputs come
from the numpy RandomState helpers of oracle/wavenet_oracle.py (machine independent: ``random_params(cfg, 5)``,
``synthetic_batch(cfg, B, T, 6)``); every OUTPUT stored here is the reference's.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_step as RS  # noqa: E402
from oracle import wavenet_oracle as O  # noqa: E402  (input generators only)

# (cfg tuple (Q,A,R,S,dd,dr,K,U), B, T)
CASES = [((256, 5, 4, 4, 3, 2, 2, 10), 2, 60), ((64, 8, 64, 32, 3, 1, 3, 8), 2, 64), ((32, 6, 8, 8, 4, 1, 2, 0), 1, 40)]
PARAM_SEED, BATCH_SEED = 5, 6
OUT = os.path.join(HERE, "aux_grad.npz")


def main():
    ref = RS.load_reference()
    if ref is None:
        raise SystemExit("oracle/_ref/wavenet.py is missing: run oracle/build_ref.py first")
    torch.set_num_threads(1)
    z = {"n_cases": np.int64(len(CASES)), "param_seed": np.int64(PARAM_SEED), "batch_seed": np.int64(BATCH_SEED)}
    for i, (cfg_t, B, T) in enumerate(CASES):
        cfg = O.OracleConfig(*cfg_t)
        p = O.random_params(cfg, PARAM_SEED)
        x, h, t = O.synthetic_batch(cfg, B, T, BATCH_SEED)
        model = ref.WaveNet(*cfg_t)
        model.load_state_dict(p)
        model.train()
        hv = h.clone().requires_grad_(True)
        out = model(x, hv)
        rf, Q = model.receptive_field, cfg_t[0]
        loss = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, Q), t[:, rf:].contiguous().view(-1))
        loss.backward()
        z["c%d/cfg" % i] = np.array(cfg_t, dtype=np.int64)
        z["c%d/B" % i] = np.int64(B)
        z["c%d/T" % i] = np.int64(T)
        z["c%d/loss" % i] = np.float64(loss.item())
        z["c%d/dh" % i] = hv.grad.detach().numpy().astype(np.float32)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
