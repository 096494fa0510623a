# -*- coding: utf-8 -*-
"""The training CLI with a moving average of the weights on the GPU: four iterations with --ema_decay 0.5 and a pass over two
held-out utterances every two -- the "ema" key of the checkpoints, the averaged weights in ``checkpoint-best.pkl``, the logged dev
loss against a model loaded with them, --resume, and ``decode.py --weights``.  Without the flag: today's files, keys and log
lines.  In the style of tests/test_train_cli_eval.py (same tiny corpus)."""
import logging
import re

import pytest
import torch

from pytorchwavenetvocoder_amd.bin import decode as D
from pytorchwavenetvocoder_amd.bin import train as T
from pytorchwavenetvocoder_amd.nets import encode_mu_law
from pytorchwavenetvocoder_amd.utils import make_feat_transform, read_hdf5
from tests.test_train_cli import U, make_corpus
from tests.test_train_cli_eval import _argv, _scp

pytestmark = pytest.mark.gpu
DEV_LINE = r"\(iter:(\d+)\) dev loss = ([0-9.]+) \((\d+) utterances, (\d+) samples, [0-9.]+ sec\)$"


def _same(a, b):
    return list(a.keys()) == list(b.keys()) and all(torch.equal(a[k].cpu().view(torch.int32), b[k].cpu().view(torch.int32)) for k in a)


def _train_argv(tmp_path, wavs, feats, stats, exp):
    argv = _argv(tmp_path, wavs, feats, stats, exp) + [
        "--dev_waveforms", _scp(tmp_path, "dev_wav.scp", wavs[4:]), "--dev_feats", _scp(tmp_path, "dev_feats.scp", feats[4:]),
        "--eval_interval", "2"]
    argv[argv.index("--lr") + 1] = "1e-3"                 # the weights move: the average differs from them
    argv[argv.index("--checkpoint_interval") + 1] = "2"
    return argv


def _dev_loss_of(weights, conf, wavs, feats, stats):
    """The held-out loss of a fresh model loaded with ``weights``, by the trainer's own pass (one batch of the two utterances)."""
    model = D.build_model(conf)
    model.load_state_dict(weights)
    model.cuda()
    mean, scale = read_hdf5(stats, "/melspc/mean"), read_hdf5(stats, "/melspc/scale")
    dev = (wavs[4:], feats[4:], 8,
           dict(feature_type="melspc", wav_transform=lambda x: encode_mu_law(x, conf.n_quantize),
                feat_transform=make_feat_transform(mean, scale), upsampling_factor=U, use_upsampling_layer=True,
                use_speaker_code=False, transforms_elementwise=True, n_quantize=conf.n_quantize, length_cache={}))
    return T.dev_loss(model, dev, 0, 1, torch.device("cuda"))[0]


def test_train_cli_keeps_scores_and_saves_the_averaged_weights(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=6)
    exp = str(tmp_path / "exp")
    argv = _train_argv(tmp_path, wavs, feats, stats, exp) + ["--ema_decay", "0.5"]
    with caplog.at_level(logging.INFO):
        T.main(argv)
    msgs = [r.getMessage() for r in caplog.records]
    got = [m for m in (re.match(DEV_LINE, ln) for ln in msgs) if m]
    assert [int(m.group(1)) for m in got] == [2, 4], caplog.text          # the dev loss line keeps its format
    assert len([ln for ln in msgs if "averaged weights" in ln]) == 2        # ... and one more line says what was scored
    cks = {it: torch.load(exp + "/checkpoint-%d.pkl" % it, weights_only=False) for it in (2, 4)}
    for ck in cks.values():
        assert set(ck.keys()) == {"model", "optimizer", "iterations", "dev", "ema"}
        assert set(ck["optimizer"].keys()) == {"state", "param_groups"}
        assert list(ck["ema"].keys()) == list(ck["model"].keys()) and not _same(ck["ema"], ck["model"])
    best = torch.load(exp + "/checkpoint-best.pkl", weights_only=False)
    assert set(best.keys()) == {"model", "iterations", "dev_loss", "ema_decay"} and best["ema_decay"] == 0.5
    assert best["iterations"] in cks and _same(best["model"], cks[best["iterations"]]["ema"])
    # the logged loss is that of the averaged weights, not of the last iterate
    conf = torch.load(exp + "/model.conf", weights_only=False)
    logged = {int(m.group(1)): float(m.group(2)) for m in got}
    for it, ck in cks.items():
        want = _dev_loss_of(ck["ema"], conf, wavs, feats, stats)
        other = _dev_loss_of(ck["model"], conf, wavs, feats, stats)
        print("iter %d: logged %.6f, averaged weights %.8f, last iterate %.8f" % (it, logged[it], want, other))
        assert abs(logged[it] - want) <= 1e-6          # (the line prints six decimals of the same deterministic pass)
        assert abs(other - want) > 1e-5                 # (the two weight sets score differently: the check means something)
    assert abs(best["dev_loss"] - logged[best["iterations"]]) <= 1e-6
    final = torch.load(exp + "/checkpoint-final.pkl", weights_only=False)
    assert set(final.keys()) == {"model", "ema"} and _same(final["ema"], cks[4]["ema"])
    assert _same(D.checkpoint_weights(exp + "/checkpoint-4.pkl", "ema"), cks[4]["ema"])
    assert _same(D.checkpoint_weights(exp + "/checkpoint-4.pkl"), cks[4]["model"])

    # --resume restores the average bit for bit (no iteration is left to run: the final checkpoint shows what was restored)
    exp2 = str(tmp_path / "exp2")
    second = list(argv)
    second[second.index("--expdir") + 1] = exp2
    second[second.index("--resume") + 1] = exp + "/checkpoint-4.pkl"
    T.main(second)
    final2 = torch.load(exp2 + "/checkpoint-final.pkl", weights_only=False)
    assert _same(final2["ema"], cks[4]["ema"]) and _same(final2["model"], cks[4]["model"])


def test_without_the_flag_everything_is_as_before_and_decode_names_the_missing_key(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=6)
    exp = str(tmp_path / "exp")
    argv = _train_argv(tmp_path, wavs, feats, stats, exp)
    with caplog.at_level(logging.INFO):
        T.main(argv)
    msgs = [r.getMessage() for r in caplog.records]
    assert len([ln for ln in msgs if re.match(DEV_LINE, ln)]) == 2 and not [ln for ln in msgs if "averaged" in ln]
    ck = torch.load(exp + "/checkpoint-4.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations", "dev"}
    assert set(torch.load(exp + "/checkpoint-best.pkl", weights_only=False).keys()) == {"model", "iterations", "dev_loss"}
    assert set(torch.load(exp + "/checkpoint-final.pkl", weights_only=False).keys()) == {"model"}

    # --resume with --ema_decay from a checkpoint without "ema": a warning, and the average starts from the model weights
    exp2 = str(tmp_path / "exp2")
    second = list(argv) + ["--ema_decay", "0.5"]
    second[second.index("--expdir") + 1] = exp2
    second[second.index("--resume") + 1] = exp + "/checkpoint-4.pkl"
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        T.main(second)
    assert [r for r in caplog.records if r.levelno == logging.WARNING and "moving average" in r.getMessage()]
    final2 = torch.load(exp2 + "/checkpoint-final.pkl", weights_only=False)
    assert _same(final2["ema"], ck["model"])

    caplog.clear()
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as err:
        D.main(["--feats", _scp(tmp_path, "dec_feats.scp", feats[4:5]), "--checkpoint", exp + "/checkpoint-4.pkl", "--outdir",
                str(tmp_path / "wav_out"), "--stats", stats, "--config", exp + "/model.conf", "--weights", "ema"])
    assert err.value.code == 1
    assert [r for r in caplog.records if "--weights ema" in r.getMessage() and "no \"ema\" entry" in r.getMessage()]
