# -*- coding: utf-8 -*-
"""The training CLI with a held-out set on the GPU: four iterations at lr 0 with a pass over two held-out utterances every two --
two equal ``dev loss`` lines (the weights do not move: determinism end to end), ``dev_loss.txt``, ``checkpoint-best.pkl``, the
``"dev"`` key of the regular checkpoint, and the logged value against the autograd route on the same padded batch.  Without the
dev flags: none of it.  In the style of tests/test_train_cli_clip.py."""
import logging
import os
import re

import pytest
import torch

from pytorchwavenetvocoder_amd.bin import decode as D
from pytorchwavenetvocoder_amd.bin import train as T
from pytorchwavenetvocoder_amd.nets import encode_mu_law
from pytorchwavenetvocoder_amd.utils import make_feat_transform, read_hdf5
from tests import parity_common as PC
from tests.test_train_cli import DIM, U, make_corpus

pytestmark = pytest.mark.gpu


def _scp(tmp_path, name, lines):
    path = str(tmp_path / name)
    open(path, "w").write("\n".join(lines) + "\n")
    return path


def _argv(tmp_path, wavs, feats, stats, exp):
    return ["--waveforms", _scp(tmp_path, "wav.scp", wavs[:4]), "--feats", _scp(tmp_path, "feats.scp", feats[:4]), "--stats", stats,
            "--feature_type", "melspc", "--n_aux", str(DIM), "--n_resch", "64", "--n_skipch", "32", "--dilation_depth", "4",
            "--dilation_repeat", "2", "--upsampling_factor", str(U), "--batch_length", "800", "--batch_size", "2",
            "--intervals", "2", "--checkpoint_interval", "4", "--lr", "0", "--verbose", "1", "--expdir", exp, "--iters", "4",
            "--resume", ""]


def test_train_cli_scores_the_held_out_set(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=6)
    exp = str(tmp_path / "exp")
    argv = _argv(tmp_path, wavs, feats, stats, exp) + [
        "--dev_waveforms", _scp(tmp_path, "dev_wav.scp", wavs[4:]), "--dev_feats", _scp(tmp_path, "dev_feats.scp", feats[4:]),
        "--eval_interval", "2"]
    with caplog.at_level(logging.INFO):
        T.main(argv)
    lines = [r.getMessage() for r in caplog.records if "dev loss" in r.getMessage() and "best checkpoint" not in r.getMessage()]
    assert len(lines) == 2, caplog.text
    got = [re.match(r"\(iter:(\d+)\) dev loss = ([0-9.]+) \((\d+) utterances, (\d+) samples, [0-9.]+ sec\)$", ln) for ln in lines]
    assert all(got), lines
    assert [int(m.group(1)) for m in got] == [2, 4] and got[0].group(2) == got[1].group(2)
    assert all(int(m.group(3)) == 2 for m in got)
    logged = float(got[0].group(2))
    rows = [ln.split() for ln in open(exp + "/dev_loss.txt").read().splitlines()]
    assert [r[0] for r in rows] == ["2", "4"] and all(r[1] == got[0].group(2) and r[2] == "2" for r in rows)
    ck = torch.load(exp + "/checkpoint-4.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations", "dev"}
    assert ck["dev"]["best_iterations"] == 2 and abs(ck["dev"]["best_loss"] - logged) <= 1e-6
    best = torch.load(exp + "/checkpoint-best.pkl", weights_only=False)
    assert set(best.keys()) == {"model", "iterations", "dev_loss"} and best["iterations"] == 2
    # the autograd route on the same padded batch: model(x, h) + nn.CrossEntropyLoss() with -100 behind every end
    conf = torch.load(exp + "/model.conf", weights_only=False)
    model = D.build_model(conf)
    model.load_state_dict(best["model"])
    model.cuda()
    mean, scale = read_hdf5(stats, "/melspc/mean"), read_hdf5(stats, "/melspc/scale")
    gen = T.train_generator(wavs[4:], feats[4:], receptive_field=model.receptive_field, batch_length=None, batch_size=2,
                            pad_utterances=True, shuffle=False, feature_type="melspc", upsampling_factor=U,
                            wav_transform=lambda x: encode_mu_law(x, conf.n_quantize), feat_transform=make_feat_transform(mean, scale),
                            device=torch.device("cuda"), n_quantize=conf.n_quantize, transforms_elementwise=True)
    try:
        (x, h), t, lengths, _ = gen.next()
    finally:
        gen.close()
    rf = model.receptive_field
    tm = t.clone()
    for b, n in enumerate(lengths.tolist()):
        tm[b, n:] = -100
    with torch.no_grad():
        out = model(x, h)
        ref = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, conf.n_quantize), tm[:, rf:].contiguous().view(-1))
    n_pos = int((lengths - rf).clamp(min=0).sum())
    assert int(got[0].group(4)) == n_pos
    print("dev loss logged %.6f, autograd route %.8f" % (logged, float(ref)))
    assert abs(logged - float(ref)) <= PC.TOL_LOSS


def test_train_cli_without_the_dev_flags_is_unchanged(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=6)
    exp = str(tmp_path / "exp")
    with caplog.at_level(logging.INFO):
        T.main(_argv(tmp_path, wavs, feats, stats, exp))
    assert not [r for r in caplog.records if "dev loss" in r.getMessage()]
    assert not os.path.exists(exp + "/dev_loss.txt") and not os.path.exists(exp + "/checkpoint-best.pkl")
    ck = torch.load(exp + "/checkpoint-4.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations"}


def test_resume_from_a_checkpoint_written_before_the_first_dev_pass(tmp_path, caplog):
    """--checkpoint_interval 2 with --eval_interval 4: checkpoint-2.pkl is written in front of the first pass ("dev" holds Nones);
    --resume from it runs on, scores at iteration 4 and carries that value in checkpoint-4.pkl, which restores in turn."""
    wavs, feats, stats = make_corpus(str(tmp_path), n=6)
    exp = str(tmp_path / "exp")
    dev = ["--dev_waveforms", _scp(tmp_path, "dev_wav.scp", wavs[4:]), "--dev_feats", _scp(tmp_path, "dev_feats.scp", feats[4:]),
           "--eval_interval", "4"]
    argv = _argv(tmp_path, wavs, feats, stats, exp) + dev
    argv[argv.index("--checkpoint_interval") + 1] = "2"
    first = list(argv)
    first[first.index("--iters") + 1] = "2"
    T.main(first)
    ck2 = torch.load(exp + "/checkpoint-2.pkl", weights_only=False)
    assert ck2["dev"] == {"best_loss": None, "best_iterations": None} and not os.path.exists(exp + "/dev_loss.txt")
    second = list(argv)
    second[second.index("--resume") + 1] = exp + "/checkpoint-2.pkl"
    with caplog.at_level(logging.INFO):
        T.main(second)
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("(iter:4) dev loss")]
    assert len(lines) == 1, caplog.text
    ck4 = torch.load(exp + "/checkpoint-4.pkl", weights_only=False)
    assert ck4["dev"]["best_iterations"] == 4 and T.dev_best_from_checkpoint(ck4)[1] == 4
    assert abs(ck4["dev"]["best_loss"] - float(lines[0].split("=")[1].split()[0])) <= 1e-6
