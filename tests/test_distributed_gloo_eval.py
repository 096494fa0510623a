# -*- coding: utf-8 -*-
"""Two gloo ranks on the CPU (kernel emulator): each scores its shard of a held-out list, one all-reduce of the float64 pair
[nll, positions] -- the dev loss both ranks then hold is the one-rank value to 1e-12 relative.  In the style of
tests/test_distributed_gloo_ragged.py."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_distributed_gloo import _free_port
from tests.test_train_cli import DIM, U, make_corpus

pytestmark = pytest.mark.emu
Q = 64


def _dev(root):
    from pytorchwavenetvocoder_amd.bin import train as T
    from pytorchwavenetvocoder_amd.nets import WaveNet, encode_mu_law, initialize
    from tests.emu_util import emu_library
    wavs = [os.path.join(root, "wav", "utt%d.wav" % i) for i in range(5)]
    feats = [os.path.join(root, "h5", "utt%d.h5" % i) for i in range(5)]
    torch.manual_seed(3)
    model = WaveNet(Q, DIM, 8, 12, 3, 2, 2, U, _library=emu_library())
    model.apply(initialize)
    kw = dict(feature_type="melspc", wav_transform=lambda x: encode_mu_law(x, Q), feat_transform=lambda h: h,
              upsampling_factor=U, use_upsampling_layer=True, transforms_elementwise=True, length_cache={})
    return T, model, (wavs, feats, 2, kw)


def _worker(rank, world, port, root):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        T, model, dev = _dev(root)
        loss, n_utt, n_pos = T.dev_loss(model, dev, rank, world, torch.device("cpu"))
        torch.save({"loss": loss, "n_utt": n_utt, "n_pos": n_pos}, os.path.join(root, "rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_one_rank_dev_loss(tmp_path):
    from tests.emu_util import emu_library
    emu_library()  # build once in the parent
    make_corpus(str(tmp_path), n=5)
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(str(tmp_path / ("rank%d.pt" % r))) for r in range(2)]
    T, model, dev = _dev(str(tmp_path))
    loss, n_utt, n_pos = T.dev_loss(model, dev, 0, 1, torch.device("cpu"))
    assert got[0] == got[1]
    assert (got[0]["n_utt"], got[0]["n_pos"]) == (n_utt, n_pos) == (5, n_pos) and n_pos > 0
    assert abs(got[0]["loss"] - loss) <= 1e-12 * abs(loss), (got[0]["loss"], loss)
