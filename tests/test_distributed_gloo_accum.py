# -*- coding: utf-8 -*-
"""Gradient accumulation under data parallelism on the CPU: two gloo ranks on the kernel emulator, GradientReducer with
layers_per_bucket=2, A = 2 micro-steps per optimizer step, two optimizer steps (the constants of tests/test_distributed_gloo.py).

Four rows: rank r runs row 2 i + r as micro-batch i.  Every rank needs a row in every micro-step, so four rows cannot be uneven in
their NUMBER per rank; the shards are uneven in what ``grad_scale`` is about, their loss positions: the rows have different
lengths (``lengths=``), and each call's share is N_row / N_all.  The sum over the micro-batches is exchanged ONCE per optimizer
step (one all-reduce per bucket), the ranks end with bit-identical weights, and the reduced gradient of the first cycle is the
fp64 oracle's gradient of the four padded rows as one batch."""
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import wavenet_oracle as O
from tests import parity_common as PC
from tests import ragged_common as RC
from tests.test_distributed_gloo import B, CFG, SEED, T, _free_port

A = 2
LENGTHS = [48, 40, 44, 33]


def _instance():
    cfg = O.OracleConfig(*CFG)
    params, x, h, t, margin, sd = PC.pick_instance(cfg, B, T, SEED, 0.1)
    return cfg, params, x, h, t


def _worker(rank, world, port, out_dir):
    import os
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pytorchwavenetvocoder_amd.distributed import GradientReducer
        from pytorchwavenetvocoder_amd.nets import WaveNet
        from pytorchwavenetvocoder_amd.optim import FusedAdam
        from tests.emu_util import emu_library
        cfg, params, x, h, t = _instance()
        rf = cfg.receptive_field
        counts = [n - rf for n in LENGTHS]
        model = WaveNet(*CFG, _library=emu_library())
        model.load_state_dict(params)
        opt = FusedAdam(model, lr=1e-3)
        red = GradientReducer(model, layers_per_bucket=2)
        assert red.world == world and len(red.ranges) == 1 + 3 + 1
        assert red.ranges[0][0] == 0 and red.ranges[-1][1] == model.engine.n_params and red._gaps == []   # the buckets tile the buffer
        for (a0, a1), (b0, b1) in zip(red.ranges[:-1], red.ranges[1:]):
            assert a0 < a1 == b0
        calls = []
        real = dist.all_reduce

        def counting(*args, **kw):
            calls.append(1)
            return real(*args, **kw)
        dist.all_reduce = counting
        try:
            first = None
            for step in range(2):
                before = len(calls)
                for i in range(A):
                    row = 2 * i + rank
                    sl = slice(row, row + 1)
                    red.loss_and_backward(x[sl].contiguous(), h[sl].contiguous(), t[sl].contiguous(), lengths=[LENGTHS[row]],
                                          grad_scale=counts[row] / float(sum(counts)), micro_step=(i, A))
                    assert len(calls) - before == (0 if i < A - 1 else len(red.ranges))   # exchanged once, behind the last micro-step
                if first is None:
                    first = model.engine.grads().clone()
                opt.step()
        finally:
            dist.all_reduce = real
        assert len(calls) == 2 * len(red.ranges)
        torch.save({"params": model.engine.flat_params.clone(), "grad": first}, "%s/rank%d.pt" % (out_dir, rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_exchange_the_accumulated_gradient_once(tmp_path):
    from pytorchwavenetvocoder_amd.engine import flat_to_state
    from pytorchwavenetvocoder_amd.nets import WaveNet
    from tests.emu_util import emu_library
    emu_library()  # build once in the parent
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2)]
    assert torch.equal(got[0]["params"].view(torch.int32), got[1]["params"].view(torch.int32))
    assert torch.equal(got[0]["grad"].view(torch.int32), got[1]["grad"].view(torch.int32))
    cfg, params, x, h, t = _instance()
    ref = RC.oracle_ragged(CFG, params, x, h, t, LENGTHS)[1]
    eng = WaveNet(*CFG, _library=emu_library()).engine
    grads = flat_to_state(eng, got[0]["grad"], O.param_shapes(cfg))
    worst = 0.0
    for k, r in ref.items():
        if r is None:
            assert float(grads[k].abs().max()) == 0.0, k
            continue
        worst = max(worst, PC.rel_to_max(grads[k], r))
    print("reduced gradient of the first cycle against the fp64 oracle: worst tensor %.3g of its maximum" % worst)
    assert worst <= PC.TOL_GRAD
