# -*- coding: utf-8 -*-
"""The training CLI with the weighted criterion (``--label_smoothing E``, ``--class_weights FILE``, ``--loss_normalize``).
Without a device: every refusal exits with an error while main() looks at the arguments, before anything is built.  On the GPU,
like the other CLI tests (the training loop needs the device), on the tiny corpus of tests/test_train_cli.py: the plain ``ce``
log line, ``--label_smoothing 0`` without ``--class_weights`` as the plain run with its files and keys, and the composition with
--accum_steps and padded utterance batches."""
import logging
import os
import re

import numpy as np
import pytest
import torch

from pytorchwavenetvocoder_amd.bin import train as T
from pytorchwavenetvocoder_amd.distributed import GradientReducer
from tests.test_train_cli import make_corpus
from tests.test_train_cli_distill import _argv, _conf, _refused, _run
from tests.test_train_cli_freeze import _flags

CE_LINE = r"\(iter:(\d+)\) average ce = ([0-9.]+) \(label smoothing ([0-9.e+-]+), normalized by (weights|positions)\)$"
LOSS_LINE = r"\(iter:(\d+)\) average loss = ([0-9.]+) \([0-9.]+ sec / batch\)$"
Q = 256


def _weights(tmp_path, name="weights.npy", values=None):
    values = np.linspace(0.25, 4.0, Q).astype(np.float32) if values is None else np.asarray(values)
    path = str(tmp_path / name)
    if name.endswith(".npy"):
        np.save(path, values)
    else:
        np.savetxt(path, values)
    return path


def _parsed(*extra):
    return T.get_parser().parse_args(_flags("w", "f", "s", "e", 1, 1, 1) + list(extra))


def test_check_criterion_args_reads_both_formats(tmp_path):
    for name in ("weights.npy", "weights.txt"):
        w = T.check_criterion_args(_parsed("--class_weights", _weights(tmp_path, name), "--label_smoothing", "0.1"))
        assert w.dtype == torch.float32 and tuple(w.shape) == (Q,)
        assert float((w - torch.linspace(0.25, 4.0, Q)).abs().max()) <= 1e-6
    assert T.check_criterion_args(_parsed()) is None
    assert T.check_criterion_args(_parsed("--label_smoothing", "0.2", "--loss_normalize", "positions")) is None


@pytest.mark.parametrize("value", ["1", "1.5", "-0.1", "nan"])
def test_label_smoothing_out_of_range(tmp_path, caplog, value):
    _refused(tmp_path, caplog, ["--label_smoothing", value], "--label_smoothing")


@pytest.mark.parametrize("values,word", [(np.ones(Q - 1), "n_quantize"), (-np.ones(Q), "finite and >= 0"),
                                         (np.full(Q, np.inf), "finite and >= 0"), (np.full(Q, np.nan), "finite and >= 0")])
def test_class_weights_refused(tmp_path, caplog, values, word):
    _refused(tmp_path, caplog, ["--class_weights", _weights(tmp_path, values=values)], "--class_weights", word)


def test_class_weights_missing_or_unreadable(tmp_path, caplog):
    _refused(tmp_path, caplog, ["--class_weights", str(tmp_path / "nothing.npy")], "--class_weights", "does not exist")
    caplog.clear()
    path = str(tmp_path / "words.txt")
    with open(path, "w") as fh:
        fh.write("one two three\n")
    _refused(tmp_path, caplog, ["--class_weights", path], "--class_weights", "cannot be read")


def test_loss_normalize_unknown(tmp_path, caplog):
    _refused(tmp_path, caplog, ["--loss_normalize", "sum"], "--loss_normalize")


@pytest.mark.parametrize("which", ["smoothing", "weights"])
def test_criterion_with_the_mixture_head_or_a_teacher(tmp_path, caplog, which):
    flags = ["--label_smoothing", "0.1"] if which == "smoothing" else ["--class_weights", _weights(tmp_path)]
    _refused(tmp_path, caplog, flags + ["--n_mixture", "2"], flags[0], "--n_mixture")
    caplog.clear()
    ckpt, conf = _conf(tmp_path, "teacher")
    _refused(tmp_path, caplog, flags + ["--teacher", ckpt, "--teacher_config", conf], flags[0], "--teacher")


# ---- on the device ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp("cew_cli")
    return make_corpus(str(root), n=4)


@pytest.mark.gpu
def test_label_smoothing_zero_is_the_plain_run(tmp_path, caplog, corpus, monkeypatch):
    wavs, feats, stats = corpus
    seen = []
    plain = GradientReducer.loss_and_backward

    def spy(self, x, h, t, **kw):
        seen.append(sorted(k for k in kw if k in ("class_weights", "label_smoothing", "position_weights", "normalize")))
        return plain(self, x, h, t, **kw)

    monkeypatch.setattr(GradientReducer, "loss_and_backward", spy)
    exp_a, exp_b = str(tmp_path / "plain"), str(tmp_path / "eps0")
    _run(caplog, _argv(tmp_path, wavs, feats, stats, exp_a, 2, 2, 2))
    msgs = _run(caplog, _argv(tmp_path, wavs, feats, stats, exp_b, 2, 2, 2) + ["--label_smoothing", "0", "--loss_normalize", "positions"])
    assert not any(re.match(CE_LINE, m) for m in msgs) and seen == [[]] * 4
    assert sorted(os.listdir(exp_b)) == sorted(os.listdir(exp_a)) == ["checkpoint-2.pkl", "checkpoint-final.pkl", "model.conf"]
    a = torch.load(exp_a + "/checkpoint-2.pkl", weights_only=False)
    b = torch.load(exp_b + "/checkpoint-2.pkl", weights_only=False)
    assert set(a.keys()) == set(b.keys()) == {"model", "optimizer", "iterations"} and list(a["model"]) == list(b["model"])
    for k in a["model"]:
        assert torch.equal(a["model"][k].cpu().view(torch.int32), b["model"][k].cpu().view(torch.int32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--accum_steps", "2"], ["--utterance_batch", "true", "--batch_size", "2"]],
                         ids=["accum_steps", "utterance_batch"])
def test_three_iterations_with_both_flags(tmp_path, caplog, corpus, extra):
    wavs, feats, stats = corpus
    exp = str(tmp_path / "run")
    msgs = _run(caplog, _argv(tmp_path, wavs, feats, stats, exp, 1, 3, 3) +
                ["--label_smoothing", "0.1", "--class_weights", _weights(tmp_path), "--loss_normalize", "positions"] + extra)
    parts = [re.match(CE_LINE, m) for m in msgs if re.match(CE_LINE, m)]
    losses = [re.match(LOSS_LINE, m) for m in msgs if re.match(LOSS_LINE, m)]
    assert [int(m.group(1)) for m in parts] == [1, 2, 3] and len(losses) == 3
    for p in parts:
        assert float(p.group(2)) > 0.0 and float(p.group(3)) == 0.1 and p.group(4) == "positions"
    assert sorted(os.listdir(exp)) == ["checkpoint-3.pkl", "checkpoint-final.pkl", "model.conf"]
    ck = torch.load(exp + "/checkpoint-3.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations"} and ck["iterations"] == 3
    assert {float(s["step"]) for s in ck["optimizer"]["state"].values()} == {3.0}
    assert all(bool(torch.isfinite(v).all()) for v in ck["model"].values())
