# -*- coding: utf-8 -*-
"""Two gloo ranks on the CPU (kernel emulator), the weighted cross-entropy on an UNEVEN ragged minibatch: rank 0 holds two
utterances, rank 1 one, each padded to its own longest, each rank with the position weights of its own shard.  With
``normalize="positions"`` and the shares N_local / N_global the exchanged gradient is the one-process gradient of the whole
padded minibatch (tolerances: those of tests/test_distributed_gloo_ragged.py for the same comparison)."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import wavenet_oracle as O
from tests import parity_common as PC
from tests.test_distributed_gloo import CFG, SEED, _free_port

pytestmark = pytest.mark.emu

B, T, LENGTHS = 3, 48, (48, 40, 36)
EPS = 0.1


def _weights():
    rs = np.random.RandomState(SEED + 11)
    w = torch.from_numpy(rs.uniform(0.25, 4.0, CFG[0]).astype(np.float32))
    r = torch.from_numpy(rs.uniform(0.0, 2.0, (B, T)).astype(np.float32))
    r[:, 3::5] = 0.0
    return w, r


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytorchwavenetvocoder_amd.bin.train import _shard_range
        from pytorchwavenetvocoder_amd.distributed import GradientReducer
        from pytorchwavenetvocoder_amd.nets import WaveNet
        from tests.emu_util import emu_library
        cfg = O.OracleConfig(*CFG)
        params = O.random_params(cfg, SEED)
        x, h, t = O.synthetic_batch(cfg, B, T, SEED + 1)
        w, r = _weights()
        lo, hi = _shard_range(B, (rank, world))
        lengths = list(LENGTHS[lo:hi])
        Tr = max(lengths)
        assert Tr % CFG[7] == 0
        xs, hs, ts = x[lo:hi, :Tr].contiguous(), h[lo:hi, :, :Tr // CFG[7]].contiguous(), t[lo:hi, :Tr].contiguous()
        rf = cfg.receptive_field
        n_local = sum(max(n - rf, 0) for n in lengths)
        n_global = sum(max(n - rf, 0) for n in LENGTHS)
        model = WaveNet(*CFG, _library=emu_library())
        model.load_state_dict(params)
        red = GradientReducer(model, layers_per_bucket=2)
        loss = red.loss_and_backward(xs, hs, ts, grad_scale=n_local / float(n_global), lengths=lengths, class_weights=w,
                                     label_smoothing=EPS, position_weights=r[lo:hi, :Tr].contiguous(), normalize="positions")
        torch.save({"grads": model.engine.grads().clone(), "loss": float(loss), "parts": model.criterion_parts.clone(),
                    "share": n_local / float(n_global), "n": n_local}, os.path.join(out_dir, "rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_uneven_ragged_weighted_shards_equal_the_single_process(tmp_path):
    from pytorchwavenetvocoder_amd.nets import WaveNet
    from tests.emu_util import emu_library
    emu_library()  # build once in the parent
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2)]
    cfg = O.OracleConfig(*CFG)
    x, h, t = O.synthetic_batch(cfg, B, T, SEED + 1)
    w, r = _weights()
    model = WaveNet(*CFG, _library=emu_library())
    model.load_state_dict(O.random_params(cfg, SEED))
    assert min(got[0]["share"], got[1]["share"]) > 0.0 and got[0]["share"] != got[1]["share"]
    loss = model.loss_and_backward(x, h, t, lengths=list(LENGTHS), class_weights=w, label_smoothing=EPS, position_weights=r,
                                   normalize="positions")
    ref = model.engine.grads()
    assert torch.equal(got[0]["grads"], got[1]["grads"])
    for off, n, shape, dead in model._param_slices:
        if dead:
            continue
        e = PC.rel_to_max(got[0]["grads"][off:off + n], ref[off:off + n])
        assert e <= PC.TOL_GRAD, (off, e)
    assert abs(got[0]["share"] + got[1]["share"] - 1.0) <= 1e-12
    # criterion and plain cross-entropy pool with the shares; the divisors are the ranks' own position counts
    parts = got[0]["share"] * got[0]["parts"] + got[1]["share"] * got[1]["parts"]
    assert abs(got[0]["share"] * got[0]["loss"] + got[1]["share"] * got[1]["loss"] - float(loss)) <= PC.TOL_LOSS
    assert float((parts[0:2] - model.criterion_parts[0:2]).abs().max()) <= PC.TOL_LOSS
    assert float(got[0]["parts"][2]) == got[0]["n"] and float(got[1]["parts"][2]) == got[1]["n"]
    assert float(model.criterion_parts[2]) == got[0]["n"] + got[1]["n"]
