# -*- coding: utf-8 -*-
"""The training CLI with gradient accumulation on the GPU (``--accum_steps``): windowed mode on the tiny corpus of
tests/test_train_cli.py.  The slicer deals the windows of the first walk of the list in order, so ``--batch_size 1 --accum_steps 2``
and ``--batch_size 2`` see the same two windows before any update: their iteration-1 losses agree.  An iteration is one optimizer
step (checkpoint "iterations", Adam's "step").  Without the flag: today's files, keys and log lines."""
import logging
import os
import re

import pytest
import torch

from pytorchwavenetvocoder_amd.bin import train as T
from tests import parity_common as PC
from tests.test_train_cli import DIM, U, make_corpus
from tests.test_train_cli_eval import _scp

pytestmark = pytest.mark.gpu
LOSS_LINE = r"\(iter:(\d+)\) average loss = ([0-9.]+) \([0-9.]+ sec / batch\)$"
PRINT_RESOLUTION = 1e-6   # two numbers printed with six decimals: half a unit of the last place each


def _argv(tmp_path, wavs, feats, stats, exp, batch_size, iters, ckpt):
    # batch_length 800: the first utterance alone (60 frames of 80 samples) holds the first two windows (stride 800 samples)
    return ["--waveforms", _scp(tmp_path, "wav.scp", wavs), "--feats", _scp(tmp_path, "feats.scp", feats), "--stats", stats,
            "--feature_type", "melspc", "--n_aux", str(DIM), "--n_resch", "64", "--n_skipch", "32", "--dilation_depth", "4",
            "--dilation_repeat", "2", "--upsampling_factor", str(U), "--batch_length", "800", "--batch_size", str(batch_size),
            "--intervals", "1", "--checkpoint_interval", str(ckpt), "--lr", "1e-3", "--verbose", "1", "--expdir", exp,
            "--iters", str(iters), "--resume", ""]


def _losses(caplog):
    got = [m for m in (re.match(LOSS_LINE, r.getMessage()) for r in caplog.records) if m]
    return {int(m.group(1)): float(m.group(2)) for m in got}


def test_accum_steps_two_of_batch_one_is_the_step_of_batch_two(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=4)
    exp_a, exp_b = str(tmp_path / "accum"), str(tmp_path / "plain")
    with caplog.at_level(logging.INFO):
        T.main(_argv(tmp_path, wavs, feats, stats, exp_a, 1, 3, 3) + ["--accum_steps", "2"])
    accum = _losses(caplog)
    assert "accum_steps = 2" in [r.getMessage() for r in caplog.records]
    caplog.clear()
    with caplog.at_level(logging.INFO):
        T.main(_argv(tmp_path, wavs, feats, stats, exp_b, 2, 1, 1))
    plain = _losses(caplog)
    msgs = [r.getMessage() for r in caplog.records]
    assert sorted(accum) == [1, 2, 3] and sorted(plain) == [1]
    print("iteration 1: --batch_size 1 --accum_steps 2 %.6f, --batch_size 2 %.6f" % (accum[1], plain[1]))
    assert abs(accum[1] - plain[1]) <= PC.TOL_LOSS * plain[1] + PRINT_RESOLUTION
    # an iteration is one optimizer step
    ck = torch.load(exp_a + "/checkpoint-3.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations"} and ck["iterations"] == 3
    steps = {float(s["step"]) for s in ck["optimizer"]["state"].values()}
    assert steps == {3.0}
    assert sorted(os.listdir(exp_a)) == ["checkpoint-3.pkl", "checkpoint-final.pkl", "model.conf"]
    # without the flag: the files, keys and log lines of a run before the flag existed (the start-up echo of the arguments
    # lists the flag's default, as it lists every argument)
    assert sorted(os.listdir(exp_b)) == ["checkpoint-1.pkl", "checkpoint-final.pkl", "model.conf"]
    ck = torch.load(exp_b + "/checkpoint-1.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations"} and ck["iterations"] == 1
    assert {float(s["step"]) for s in ck["optimizer"]["state"].values()} == {1.0}
    assert set(torch.load(exp_b + "/checkpoint-final.pkl", weights_only=False).keys()) == {"model"}
    assert [m for m in msgs if m.startswith("accum") or "micro_step" in m] == ["accum_steps = 1"]   # (paths may hold the test's name)
    assert len([m for m in msgs if re.match(LOSS_LINE, m)]) == 1 and "1-iter checkpoint created." in msgs
