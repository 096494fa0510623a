# -*- coding: utf-8 -*-
"""Global-norm clipping under data parallelism, on the CPU: two gloo ranks through the kernel emulator, bucketed all-reduce
(GradientReducer) and FusedAdam(max_grad_norm=...) with the clip active, against ONE process on the whole minibatch.  The norm is
the global gradient's on every rank, so both ranks must hold bit-identical weights and bit-identical ``grad_norm`` values.
Modelled on tests/test_distributed_gloo.py (same model, sizes and uneven minibatch of three)."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import wavenet_oracle as O
from tests.test_distributed_gloo import CFG, SEED, T, _free_port

LR = 1e-3
MAX_NORM = 0.02   # far below this model's gradient norm (asserted): the clip is active on every step
BTOT = 3


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytorchwavenetvocoder_amd.bin.train import _shard_range
        from pytorchwavenetvocoder_amd.distributed import GradientReducer
        from pytorchwavenetvocoder_amd.nets import WaveNet
        from pytorchwavenetvocoder_amd.optim import FusedAdam
        from tests.emu_util import emu_library
        cfg = O.OracleConfig(*CFG)
        x, h, t = O.synthetic_batch(cfg, BTOT, T, SEED + 1)
        lo, hi = _shard_range(BTOT, (rank, world))
        sl = slice(lo, hi)
        model = WaveNet(*CFG, _library=emu_library())
        model.load_state_dict(O.random_params(cfg, SEED))
        opt = FusedAdam(model, lr=LR, max_grad_norm=MAX_NORM)
        red = GradientReducer(model, layers_per_bucket=2)
        norms = []
        for _ in range(2):
            red.loss_and_backward(x[sl].contiguous(), h[sl].contiguous(), t[sl].contiguous(), grad_scale=(hi - lo) / float(BTOT))
            opt.step()
            norms.append(opt.grad_norm.clone())
        torch.save({"params": model.engine.flat_params.clone(), "norms": torch.stack(norms)}, os.path.join(out_dir, "rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_clip_by_the_global_norm_and_stay_bit_identical(tmp_path):
    from pytorchwavenetvocoder_amd.nets import WaveNet
    from pytorchwavenetvocoder_amd.optim import FusedAdam
    from tests.emu_util import emu_library
    emu_library()  # build once in the parent
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2)]
    assert torch.equal(got[0]["params"].view(torch.int32), got[1]["params"].view(torch.int32))
    assert torch.equal(got[0]["norms"].view(torch.int32), got[1]["norms"].view(torch.int32))

    cfg = O.OracleConfig(*CFG)
    x, h, t = O.synthetic_batch(cfg, BTOT, T, SEED + 1)
    model = WaveNet(*CFG, _library=emu_library())
    model.load_state_dict(O.random_params(cfg, SEED))
    opt = FusedAdam(model, lr=LR, max_grad_norm=MAX_NORM)
    for step in range(2):
        model.loss_and_backward(x, h, t)
        opt.step()
        norm = float(opt.grad_norm)
        assert norm > MAX_NORM   # clip active
        # the two ranks' norm is the norm of the SUM of their weighted gradients: the whole minibatch's, up to the rounding of
        # the fp32 gradients themselves (1e-4 of a tensor's maximum is the project's gradient gate)
        assert abs(float(got[0]["norms"][step]) - norm) <= 1e-4 * norm
    assert float((got[0]["params"] - model.engine.flat_params).abs().max()) <= 1e-2 * LR   # 1e-2 * lr, as tests/test_distributed_gloo.py
