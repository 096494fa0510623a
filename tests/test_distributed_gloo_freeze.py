# -*- coding: utf-8 -*-
"""Frozen parameters under data parallelism, on the CPU: two gloo ranks through the kernel emulator under
``bottom(1)`` (front conv, upsampling and layer 0 frozen), bucketed all-reduce (GradientReducer) and FusedAdam with the clip, the
non-finite guard, weight decay and the average on.  The reducer exchanges WHOLE buckets, so the ranges of frozen tensors travel
with whatever they hold: here NaN, written over the whole gradient buffer before every backward call (a range no launch writes
keeps it through the all-reduce) and over the frozen ranges again before every ``step()``.  No step may be skipped, both ranks
must end with bit-identical weights, moments and norms, every frozen tensor must keep its bits, and the trainable ones must be
those of ONE process on the whole minibatch.  Modelled on tests/test_distributed_gloo_clip.py (same model, sizes and uneven
minibatch of three)."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import wavenet_oracle as O
from tests.test_distributed_gloo import CFG, SEED, T, _free_port

LR = 1e-3
WD = 1e-2
MAX_NORM = 0.02   # far below this model's gradient norm (asserted): the clip is active on every step
BTOT = 3
N_LAYERS = CFG[4] * CFG[5]
FREEZE = "bottom:1"
NAN = float("nan")


def _optimizer(model):
    from pytorchwavenetvocoder_amd.optim import FusedAdam
    return FusedAdam(model, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM, skip_nonfinite=True, ema_decay=0.999)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytorchwavenetvocoder_amd.bin.train import _shard_range
        from pytorchwavenetvocoder_amd.distributed import GradientReducer
        from pytorchwavenetvocoder_amd.nets import WaveNet
        from tests import freeze_common as F
        from tests.emu_util import emu_library
        cfg = O.OracleConfig(*CFG)
        x, h, t = O.synthetic_batch(cfg, BTOT, T, SEED + 1)
        lo, hi = _shard_range(BTOT, (rank, world))
        sl = slice(lo, hi)
        model = WaveNet(*CFG, _library=emu_library())
        model.load_state_dict(O.random_params(cfg, SEED))
        F.apply_freeze(model, FREEZE, N_LAYERS)
        opt = _optimizer(model)
        red = GradientReducer(model, layers_per_bucket=2)
        eng = model.engine
        fz = F.frozen_mask(model)
        norms, travelled = [], []
        for _ in range(2):
            eng.grads().fill_(NAN)
            red.loss_and_backward(x[sl].contiguous(), h[sl].contiguous(), t[sl].contiguous(), grad_scale=(hi - lo) / float(BTOT))
            g = eng.grads()
            assert bool(torch.isfinite(g[~fz]).all())            # every live element was written and reduced
            travelled.append(int(torch.isnan(g[fz]).sum()))      # frozen ranges no launch wrote: NaN went through the all-reduce
            g[fz] = NAN
            opt.step()
            norms.append(opt.grad_norm.clone())
        m, v = opt._buffers()
        torch.save({"params": eng.flat_params.clone(), "m": m.clone(), "v": v.clone(), "ema": opt.ema.clone(),
                    "norms": torch.stack(norms), "travelled": travelled, "applied": opt.steps_applied(),
                    "skipped": opt.steps_skipped(), "grad_none": [p.grad is None for p in model.parameters()]},
                   os.path.join(out_dir, "rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_frozen_parameters_ignore_nan_in_frozen_ranges_and_stay_bit_identical(tmp_path):
    from pytorchwavenetvocoder_amd.nets import WaveNet
    from tests import freeze_common as F
    from tests.emu_util import emu_library
    emu_library()  # build once in the parent
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2)]
    for what in ("params", "m", "v", "ema", "norms"):
        assert torch.equal(got[0][what].view(torch.int32), got[1][what].view(torch.int32)), what
    for r in range(2):
        assert (got[r]["applied"], got[r]["skipped"]) == (2, 0), r
        assert all(n > 0 for n in got[r]["travelled"]), got[r]["travelled"]
        assert bool(torch.isfinite(got[r]["norms"]).all())

    cfg = O.OracleConfig(*CFG)
    init = O.random_params(cfg, SEED)
    x, h, t = O.synthetic_batch(cfg, BTOT, T, SEED + 1)
    model = WaveNet(*CFG, _library=emu_library())
    model.load_state_dict(init)
    frozen = F.apply_freeze(model, FREEZE, N_LAYERS)
    assert frozen and len(frozen) < len(init)
    start = F.bits(model.engine.flat_params)
    fz = F.frozen_mask(model)
    keys = [k for k, _ in model.named_parameters()]
    assert got[0]["grad_none"] == [k in frozen or dead for k, (_, _, _, dead) in zip(keys, model._param_slices)]
    # frozen tensors untouched on the ranks: weights keep their bits, the moments stay zero, the average stays the weights
    assert torch.equal(got[0]["params"].view(torch.int32)[fz], start[fz])
    assert torch.equal(got[0]["ema"].view(torch.int32)[fz], start[fz])
    assert not bool(got[0]["m"][fz].any()) and not bool(got[0]["v"][fz].any())
    assert not torch.equal(got[0]["params"].view(torch.int32)[~fz], start[~fz])

    opt = _optimizer(model)
    for step in range(2):
        model.loss_and_backward(x, h, t)
        opt.step()
        norm = float(opt.grad_norm)
        assert norm > MAX_NORM   # clip active
        # the two ranks' norm is the norm of the SUM of their weighted gradients over the live ranges: the whole minibatch's,
        # up to the rounding of the fp32 gradients themselves (1e-4 of a tensor's maximum is the project's gradient gate)
        assert abs(float(got[0]["norms"][step]) - norm) <= 1e-4 * norm
    assert float((got[0]["params"] - model.engine.flat_params).abs().max()) <= 1e-2 * LR   # 1e-2 * lr, as tests/test_distributed_gloo.py
