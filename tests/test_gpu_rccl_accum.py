# -*- coding: utf-8 -*-
"""Gradient accumulation through the exchange path on one GPU: a process group of ONE ``nccl`` (= RCCL) rank, the reducer told
to exchange even when alone (the shape, model and tensors of tests/test_gpu_rccl_single_rank.py).  An A = 3 cycle then runs the
N > 1 code: non-final micro-steps accumulate on the caller's stream; the final one records the bucket events, and on the side
stream every bucket waits for its event, has the accumulator added into its range and is all-reduced; the caller's stream joins.
A one-rank all-reduce is the identity, so with the default buckets the summed gradient is BIT-identical to the same cycle through
a plain reducer -- which it is only if event, finish, all-reduce and join are ordered."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CODE = r"""
import os, sys
import torch
import torch.distributed as dist
sys.path.insert(0, %(root)r)
os.environ["MASTER_ADDR"] = "127.0.0.1"
os.environ["MASTER_PORT"] = "%(port)d"
from pytorchwavenetvocoder_amd.distributed import GradientReducer, rccl_footprint_defaults
from pytorchwavenetvocoder_amd.nets import WaveNet, initialize
from oracle import wavenet_oracle as O
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
rccl_footprint_defaults()
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
cfg_t = (256, 80, 64, 256, 10, 3, 2, 80)
cfg = O.OracleConfig(*cfg_t)
torch.manual_seed(3)
model = WaveNet(*cfg_t)
model.apply(initialize)
model.to(dev)
x, h, t = O.synthetic_batch(cfg, 2, 3200 + 80 * 3, 9)
x, h, t = x.to(dev), h.to(dev), t.to(dev)
A = 3
batches = [(x[:1].contiguous(), h[:1].contiguous(), t[:1].contiguous()), (x[1:].contiguous(), h[1:].contiguous(), t[1:].contiguous()),
           (x, h, t)]
shares = [0.25, 0.25, 0.5]

def cycle(red):
    losses = []
    for i, (xb, hb, tb) in enumerate(batches):
        losses.append(red.loss_and_backward(xb, hb, tb, grad_scale=shares[i], micro_step=(i, A)))
    torch.cuda.synchronize()
    assert model.engine.accumulation is None
    return torch.cat(losses), model.engine.grads().clone()

plain = GradientReducer(model)
assert not plain.exchange_alone
l0, g0 = cycle(plain)
assert float(g0.abs().max()) > 0.0 and bool(torch.isfinite(g0).all())
for lpb in (None, 10):
    red = GradientReducer(model, layers_per_bucket=lpb, exchange_when_alone=True)
    assert red.exchange_alone and red.cuda and red._gaps == []
    model.engine.grads().zero_()
    l1, g1 = cycle(red)
    assert torch.equal(l0, l1), (l0.tolist(), l1.tolist())
    if lpb is None:
        assert torch.equal(g0, g1), float((g0 - g1).abs().max())
    else:   # other launch groups: other split-K plans, round-off only
        assert float((g0 - g1).abs().max()) <= 2e-5 * float(g0.abs().max())
dist.destroy_process_group()
print("RCCL single-rank accumulation ok")
"""


def test_rccl_single_rank_accumulation_cycle():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", CODE % {"root": root, "port": port}], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0 and "RCCL single-rank accumulation ok" in out, out[-3000:]
