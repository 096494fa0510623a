#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""Golden fixture of the reference MODULE trained on a padded batch of unequal lengths, for tests/ragged_common.py.

    python oracle/build_ref.py && python tests/golden/make_ragged_golden.py
    # writes tests/golden/ragged.npz

Drives the reference's own model file (``oracle/_ref/wavenet.py``, the build-time copy made by oracle/build_ref.py) with the
loss object of its training loop (``nn.CrossEntropyLoss()`` on ``[:, receptive_field:]``, train.py:461,533-536) and the
targets behind every sequence's end set to that object's default ``ignore_index`` (-100): one case with the upsampling layer
on the fused 64-channel path, one without on the any-size path; 128 classes, so that the cross-entropy runs as the epilogue
of conv_post_2.  Each batch has one full-length sequence, one that ends inside a 128-column tile and one that ends inside the
receptive field (it carries no loss).  Inputs come from the numpy RandomState helpers of oracle/wavenet_oracle.py, on the
first seed whose ReLU-kink margin ON THE LOSS POSITIONS is above 1e-5 (the seed walk and the margin of tests/parity_common.py
pick_instance, restated here so that the generator needs no built library); every OUTPUT stored here is the reference's:
the loss, every parameter gradient, dL/dh.
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

# (cfg tuple (Q,A,R,S,dd,dr,K,U), B, T, lengths)
CASES = [((128, 4, 64, 128, 2, 1, 2, 16), 3, 160, (160, 100, 4)),
         ((128, 4, 32, 64, 2, 1, 2, 0), 3, 160, (160, 140, 3))]
SEED, SCALE, KINK_MARGIN = 5, 0.1, 1e-5
OUT = os.path.join(HERE, "ragged.npz")


def margin(cfg, params, x, h, lengths):
    """min |pre-ReLU value| over the positions that carry loss: [receptive_field, lengths[b]) of every sequence (the padding
    carries no gradient, so a kink there does not matter)."""
    with torch.no_grad():
        _, inter = O.forward(cfg, params, x, h, return_intermediates=True)
    m = float("inf")
    for b, n in enumerate(lengths):
        if n > cfg.receptive_field:
            for k in ("skip_sum", "post1_pre"):
                m = min(m, float(inter[k][b, :, cfg.receptive_field:n].abs().min()))
    return m


def pick(cfg, B, T, lengths):
    for i in range(200):
        sd = SEED + 1009 * i
        params = O.random_params(cfg, sd, scale=SCALE)
        x, h, t = O.synthetic_batch(cfg, B, T, sd + 1)
        if margin(cfg, params, x, h, lengths) >= KINK_MARGIN:
            return sd, params, x, h, t
    raise SystemExit("no instance away from the ReLU kinks")


def main():
    ref = RS.load_reference()
    if ref is None:
        raise SystemExit("oracle/_ref/wavenet.py is missing: run oracle/build_ref.py first")
    torch.set_num_threads(1)
    z = {"n_cases": np.int64(len(CASES)), "scale": np.float64(SCALE)}
    for i, (cfg_t, B, T, lengths) in enumerate(CASES):
        cfg = O.OracleConfig(*cfg_t)
        sd, p, x, h, t = pick(cfg, B, T, lengths)
        model = ref.WaveNet(*cfg_t)
        model.load_state_dict(p)
        model.train()
        hv = h.clone().requires_grad_(True)
        out = model(x, hv)
        rf, Q = model.receptive_field, cfg_t[0]
        assert min(lengths) <= rf and max(lengths) == T
        tm = t.clone()
        for b, n in enumerate(lengths):
            tm[b, n:] = -100
        loss = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, Q), tm[:, rf:].contiguous().view(-1))
        loss.backward()
        z["c%d/cfg" % i] = np.array(cfg_t, dtype=np.int64)
        z["c%d/B" % i] = np.int64(B)
        z["c%d/T" % i] = np.int64(T)
        z["c%d/lengths" % i] = np.array(lengths, dtype=np.int64)
        z["c%d/seed" % i] = np.int64(sd)
        z["c%d/loss" % i] = np.float64(loss.item())
        z["c%d/dh" % i] = hv.grad.detach().numpy().astype(np.float32)
        for k, v in model.named_parameters():
            if v.grad is not None:
                z["c%d/g/%s" % (i, k)] = v.grad.detach().numpy().astype(np.float32)
    np.savez_compressed(OUT, **z)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
