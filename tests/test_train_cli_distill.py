# -*- coding: utf-8 -*-
"""The training CLI with a teacher (``--teacher CKPT --teacher_config CONF [--distill_alpha] [--distill_temperature]``).  Without
a device: every refusal exits with an error while main() looks at the arguments, before anything is built.  On the GPU, like the
other CLI tests (the training loop needs the device), on the tiny corpus of tests/test_train_cli.py: the ce / kl log line, a
checkpoint without a trace of the teacher, alpha 0 as the run without a teacher, the loss window of the deeper model, and the
composition with --accum_steps and padded utterance batches."""
import logging
import os
import re

import pytest
import torch

from pytorchwavenetvocoder_amd.bin import train as T
from pytorchwavenetvocoder_amd.distributed import GradientReducer
from pytorchwavenetvocoder_amd.nets import WaveNet
from tests.test_train_cli import DIM, U, make_corpus
from tests.test_train_cli_eval import _scp
from tests.test_train_cli_freeze import _flags

PARTS_LINE = r"\(iter:(\d+)\) average ce = ([0-9.]+), average kl = ([0-9.]+) \(alpha ([0-9.e+-]+), temperature ([0-9.e+-]+)\)$"
LOSS_LINE = r"\(iter:(\d+)\) average loss = ([0-9.]+) \([0-9.]+ sec / batch\)$"
BATCH_LENGTH = 800


def _conf(tmp_path, name, **changes):
    """A model.conf as a run with _flags would save it (the parsed arguments), with ``changes``; and an (empty) checkpoint file."""
    args = T.get_parser().parse_args(_flags("w", "f", "s", "e", 1, 1, 1))
    for k, v in changes.items():
        setattr(args, k, v)
    conf, ckpt = str(tmp_path / (name + ".conf")), str(tmp_path / (name + ".pkl"))
    torch.save(args, conf)
    torch.save({"model": {}}, ckpt)
    return ckpt, conf


def _refused(tmp_path, caplog, extra, *words):
    exp = str(tmp_path / "exp")
    argv = _flags(str(tmp_path / "wav.scp"), str(tmp_path / "feats.scp"), str(tmp_path / "stats.h5"), exp, 1, 1, 1)
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as err:
        T.main(argv + extra)
    assert err.value.code == 1
    msgs = [r.getMessage() for r in caplog.records if r.levelno >= logging.ERROR]
    assert any(all(w in m for w in words) for m in msgs), msgs
    assert not os.path.exists(exp)


def test_teacher_without_its_config_and_the_reverse(tmp_path, caplog):
    ckpt, conf = _conf(tmp_path, "teacher")
    _refused(tmp_path, caplog, ["--teacher", ckpt], "--teacher", "--teacher_config")
    caplog.clear()
    _refused(tmp_path, caplog, ["--teacher_config", conf], "--teacher", "--teacher_config")


def test_teacher_with_the_mixture_head(tmp_path, caplog):
    ckpt, conf = _conf(tmp_path, "teacher")
    _refused(tmp_path, caplog, ["--teacher", ckpt, "--teacher_config", conf, "--n_mixture", "2"], "--teacher", "--n_mixture")


@pytest.mark.parametrize("flag,value", [("--distill_alpha", "1.5"), ("--distill_alpha", "-0.1"), ("--distill_temperature", "0"),
                                        ("--distill_temperature", "-2"), ("--distill_temperature", "inf")])
def test_alpha_and_temperature_out_of_range(tmp_path, caplog, flag, value):
    ckpt, conf = _conf(tmp_path, "teacher")
    _refused(tmp_path, caplog, ["--teacher", ckpt, "--teacher_config", conf, flag, value], flag)


@pytest.mark.parametrize("key,value", [("n_quantize", 128), ("n_aux", DIM + 1), ("upsampling_factor", U // 2), ("use_upsampling_layer", False)])
def test_teacher_of_another_interface(tmp_path, caplog, key, value):
    ckpt, conf = _conf(tmp_path, "teacher", **{key: value})
    _refused(tmp_path, caplog, ["--teacher", ckpt, "--teacher_config", conf], "teacher", key)


# ---- on the device ----------------------------------------------------------------------------------------------------------------
def _argv(tmp_path, wavs, feats, stats, exp, batch_size, iters, ckpt):
    return _flags(_scp(tmp_path, "wav.scp", wavs), _scp(tmp_path, "feats.scp", feats), stats, exp, batch_size, iters, ckpt) + ["--resume", ""]


def _run(caplog, argv):
    caplog.clear()
    with caplog.at_level(logging.INFO):
        T.main(argv)
    return [r.getMessage() for r in caplog.records]


def _student_rf():
    return WaveNet(256, DIM, 64, 32, 4, 2, 2, U).receptive_field


@pytest.fixture(scope="module")
def corpus_and_teachers(tmp_path_factory):
    """The tiny corpus, a teacher of the student's own configuration and a deeper one (one iteration of training each), made
    once for the tests of this file."""
    root = tmp_path_factory.mktemp("distill_cli")
    wavs, feats, stats = make_corpus(str(root), n=4)
    same, deep = str(root / "teacher_same"), str(root / "teacher_deep")
    T.main(_argv(root, wavs, feats, stats, same, 2, 1, 1) + ["--seed", "5"])
    T.main(_argv(root, wavs, feats, stats, deep, 2, 1, 1) + ["--seed", "6", "--dilation_depth", "5"])
    return wavs, feats, stats, same, deep


def _teacher_flags(expdir):
    return ["--teacher", expdir + "/checkpoint-1.pkl", "--teacher_config", expdir + "/model.conf"]


@pytest.mark.gpu
def test_three_iterations_with_a_teacher(tmp_path, caplog, corpus_and_teachers, monkeypatch):
    wavs, feats, stats, same, deep = corpus_and_teachers
    calls = []
    plain = GradientReducer.loss_and_backward

    def spy(self, x, h, t, **kw):
        calls.append((tuple(x.shape), kw.get("t_start"), kw.get("teacher_logits") is not None, kw.get("lengths")))
        return plain(self, x, h, t, **kw)

    monkeypatch.setattr(GradientReducer, "loss_and_backward", spy)
    exp = str(tmp_path / "student")
    msgs = _run(caplog, _argv(tmp_path, wavs, feats, stats, exp, 2, 3, 3) + _teacher_flags(deep) + ["--distill_temperature", "2"])
    parts = [re.match(PARTS_LINE, m) for m in msgs if re.match(PARTS_LINE, m)]
    losses = [re.match(LOSS_LINE, m) for m in msgs if re.match(LOSS_LINE, m)]
    assert [int(m.group(1)) for m in parts] == [1, 2, 3] and len(losses) == 3
    for p, l in zip(parts, losses):
        ce, kl, alpha, tau = (float(p.group(i)) for i in (2, 3, 4, 5))
        assert (alpha, tau) == (0.5, 2.0) and ce > 0.0 and kl >= 0.0
        assert abs(float(l.group(2)) - ((1 - alpha) * ce + alpha * tau * tau * kl)) <= 1e-4 * float(l.group(2)) + 3e-6
    # the deeper teacher sets the window: every call carries batch * (T - max rf) = batch * batch_length loss positions
    rf_student = _student_rf()
    rf_teacher = WaveNet(256, DIM, 64, 32, 5, 2, 2, U).receptive_field
    assert rf_teacher > rf_student and len(calls) == 3
    for shape, t_start, has_teacher, lengths in calls:
        assert t_start == rf_teacher and has_teacher and lengths is None
        assert shape[0] * (shape[1] - t_start) == 2 * (BATCH_LENGTH - (rf_teacher + BATCH_LENGTH) % U)
    # the checkpoint holds nothing of the teacher and loads into a plain model
    assert sorted(os.listdir(exp)) == ["checkpoint-3.pkl", "checkpoint-final.pkl", "model.conf"]
    ck = torch.load(exp + "/checkpoint-3.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations"} and not any("teacher" in k for k in ck["model"])
    model = WaveNet(256, DIM, 64, 32, 4, 2, 2, U)
    model.load_state_dict(ck["model"])
    assert len(ck["optimizer"]["state"]) == len(ck["model"]) - 2


@pytest.mark.gpu
def test_alpha_zero_is_the_run_without_a_teacher(tmp_path, caplog, corpus_and_teachers):
    wavs, feats, stats, same, deep = corpus_and_teachers
    exp_a, exp_b = str(tmp_path / "plain"), str(tmp_path / "alpha0")
    _run(caplog, _argv(tmp_path, wavs, feats, stats, exp_a, 2, 2, 2))
    msgs = _run(caplog, _argv(tmp_path, wavs, feats, stats, exp_b, 2, 2, 2) + _teacher_flags(same) + ["--distill_alpha", "0"])
    assert not any(re.match(PARTS_LINE, m) for m in msgs)
    a = torch.load(exp_a + "/checkpoint-final.pkl", weights_only=False)["model"]
    b = torch.load(exp_b + "/checkpoint-final.pkl", weights_only=False)["model"]
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k].cpu().view(torch.int32), b[k].cpu().view(torch.int32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--accum_steps", "2"], ["--utterance_batch", "true", "--batch_size", "2"]],
                         ids=["accum_steps", "utterance_batch"])
def test_teacher_composes(tmp_path, caplog, corpus_and_teachers, extra):
    wavs, feats, stats, same, deep = corpus_and_teachers
    exp = str(tmp_path / "student")
    msgs = _run(caplog, _argv(tmp_path, wavs, feats, stats, exp, 1, 2, 2) + _teacher_flags(deep) + extra)
    parts = [re.match(PARTS_LINE, m) for m in msgs if re.match(PARTS_LINE, m)]
    losses = [re.match(LOSS_LINE, m) for m in msgs if re.match(LOSS_LINE, m)]
    assert [int(m.group(1)) for m in parts] == [1, 2] and len(losses) == 2
    for p, l in zip(parts, losses):
        ce, kl = float(p.group(2)), float(p.group(3))
        assert abs(float(l.group(2)) - (0.5 * ce + 0.5 * kl)) <= 1e-4 * float(l.group(2)) + 3e-6
    ck = torch.load(exp + "/checkpoint-2.pkl", weights_only=False)
    assert ck["iterations"] == 2 and {float(s["step"]) for s in ck["optimizer"]["state"].values()} == {2.0}
    assert all(bool(torch.isfinite(v).all()) for v in ck["model"].values())
