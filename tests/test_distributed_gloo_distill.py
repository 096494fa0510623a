# -*- coding: utf-8 -*-
"""Two gloo ranks on the CPU (kernel emulator), knowledge distillation on an UNEVEN ragged minibatch: rank 0 holds two
utterances, rank 1 one, each padded to its own longest, each rank with the teacher's logits of its own shard.  With the shares
N_local / N_global the exchanged gradient is the one-process gradient of the whole padded minibatch against the same teacher
(tolerances: those of tests/test_distributed_gloo_ragged.py for the same comparison)."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import wavenet_oracle as O
from tests import parity_common as PC
from tests.test_distributed_gloo import CFG, SEED, _free_port

pytestmark = pytest.mark.emu

B, T, LENGTHS = 3, 48, (48, 40, 36)   # every shard keeps loss positions behind the teacher's receptive field (31)
ALPHA, TAU = 0.6, 2.0
TEACHER_CFG = CFG[:4] + (CFG[4] + 1,) + CFG[5:]   # one dilation more: a longer receptive field than the student's


def _teacher(lib):
    from pytorchwavenetvocoder_amd.nets import WaveNet
    teacher = WaveNet(*TEACHER_CFG, _library=lib)
    teacher.load_state_dict(O.random_params(O.OracleConfig(*TEACHER_CFG), SEED + 7))
    teacher.requires_grad_(False)
    return teacher


def _t_start():
    return max(O.OracleConfig(*CFG).receptive_field, O.OracleConfig(*TEACHER_CFG).receptive_field)


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
        lo, hi = _shard_range(B, (rank, world))
        lengths = list(LENGTHS[lo:hi])
        Tr = max(lengths)
        assert Tr % CFG[7] == 0
        xs, hs, ts = x[lo:hi, :Tr].contiguous(), h[lo:hi, :, :Tr // CFG[7]].contiguous(), t[lo:hi, :Tr].contiguous()
        rf = _t_start()
        n_local = sum(max(n - rf, 0) for n in lengths)
        n_global = sum(max(n - rf, 0) for n in LENGTHS)
        model = WaveNet(*CFG, _library=emu_library())
        model.load_state_dict(params)
        tl = _teacher(emu_library()).teacher_logits(xs, hs)
        red = GradientReducer(model, layers_per_bucket=2)
        loss = red.loss_and_backward(xs, hs, ts, t_start=rf, grad_scale=n_local / float(n_global), lengths=lengths,
                                     teacher_logits=tl, distill_alpha=ALPHA, distill_temperature=TAU)
        torch.save({"grads": model.engine.grads().clone(), "loss": float(loss), "parts": model.distill_parts.clone(),
                    "share": n_local / float(n_global)}, os.path.join(out_dir, "rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_uneven_ragged_distillation_shards_equal_the_single_process(tmp_path):
    from pytorchwavenetvocoder_amd.nets import WaveNet
    from tests.emu_util import emu_library
    emu_library()  # build once in the parent
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2)]
    cfg = O.OracleConfig(*CFG)
    x, h, t = O.synthetic_batch(cfg, B, T, SEED + 1)
    model = WaveNet(*CFG, _library=emu_library())
    model.load_state_dict(O.random_params(cfg, SEED))
    rf = _t_start()
    assert rf > cfg.receptive_field and min(got[0]["share"], got[1]["share"]) > 0.0
    tl = _teacher(emu_library()).teacher_logits(x, h)
    loss = model.loss_and_backward(x, h, t, t_start=rf, lengths=list(LENGTHS), teacher_logits=tl, distill_alpha=ALPHA,
                                   distill_temperature=TAU)
    ref = model.engine.grads()
    assert torch.equal(got[0]["grads"], got[1]["grads"])
    for off, n, shape, dead in model._param_slices:
        if dead:
            continue
        e = PC.rel_to_max(got[0]["grads"][off:off + n], ref[off:off + n])
        assert e <= PC.TOL_GRAD, (off, e)
    assert abs(got[0]["share"] + got[1]["share"] - 1.0) <= 1e-12
    assert abs(got[0]["share"] * got[0]["loss"] + got[1]["share"] * got[1]["loss"] - float(loss)) <= PC.TOL_LOSS
    parts = got[0]["share"] * got[0]["parts"] + got[1]["share"] * got[1]["parts"]
    assert float((parts - model.distill_parts).abs().max()) <= PC.TOL_LOSS
