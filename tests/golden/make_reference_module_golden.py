#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Golden fixture of the reference MODULE's training loop, for tests/test_oracle_golden.py.

    python oracle/build_ref.py && python tests/golden/make_reference_module_golden.py
    # writes tests/golden/reference_module_steps.npz

Drives the reference's own model file (``oracle/_ref/wavenet.py``, the build-time copy made by oracle/build_ref.py) under
the reference's training loop (``oracle/ref_step.ReferenceTrainer``: nn.CrossEntropyLoss + torch.optim.Adam, lr 1e-3,
weight decay 0.01) for two steps on three small models, one thread, and stores the loss and logits of each step and the
weights after the second step.  Inputs come from the numpy RandomState helpers of oracle/wavenet_oracle.py (machine
independent: ``random_params(cfg, 5)``, ``synthetic_batch(cfg, B, T, 6)``); every OUTPUT stored here is the reference's.
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

# (cfg tuple (Q,A,R,S,dd,dr,K,U), B, T): the models of test_restatement_equals_the_reference_module_copy
CASES = [((256, 5, 4, 4, 3, 2, 2, 10), 2, 60), ((64, 8, 64, 32, 3, 1, 3, 8), 2, 64), ((32, 6, 8, 8, 4, 1, 2, 0), 1, 40)]
PARAM_SEED, BATCH_SEED, LR, WD, STEPS = 5, 6, 1e-3, 0.01, 2
OUT = os.path.join(HERE, "reference_module_steps.npz")


def main():
    if not RS.available():
        raise SystemExit("oracle/_ref/wavenet.py is missing: run oracle/build_ref.py first")
    torch.set_num_threads(1)
    z = {"n_cases": np.int64(len(CASES)), "param_seed": np.int64(PARAM_SEED), "batch_seed": np.int64(BATCH_SEED),
         "lr": np.float64(LR), "wd": np.float64(WD), "steps": np.int64(STEPS)}
    for i, (cfg_t, B, T) in enumerate(CASES):
        cfg = O.OracleConfig(*cfg_t)
        p = O.random_params(cfg, PARAM_SEED)
        x, h, t = O.synthetic_batch(cfg, B, T, BATCH_SEED)
        tr = RS.ReferenceTrainer(cfg_t, state=p, lr=LR, weight_decay=WD)
        z["c%d/cfg" % i] = np.array(cfg_t, dtype=np.int64)
        z["c%d/B" % i] = np.int64(B)
        z["c%d/T" % i] = np.int64(T)
        for s in range(STEPS):
            loss, out = tr.step(x, h, t)
            z["c%d/loss%d" % (i, s)] = np.float64(loss)
            z["c%d/logits%d" % (i, s)] = out.detach().numpy().astype(np.float32)
        for k, v in tr.model.state_dict().items():
            z["c%d/after/%s" % (i, k)] = v.detach().numpy().astype(np.float32)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
