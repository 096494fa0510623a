# -*- coding: utf-8 -*-
"""The training CLI with layer-wise adaptive steps (``--layer_adaptation``, ``--max_trust_ratio``, ``--param_group REGEX:adapt=``).
On the GPU, like the other CLI tests (the training loop itself needs the device), on the tiny corpus of tests/test_train_cli.py:
the run logs the trust-ratio line at every ``--intervals`` line, writes a checkpoint in torch.optim.Adam's format and resumes; a
run without the flag logs and saves what it did before.  Without a device: the flags' syntax and conflicts, checked before
anything is read or built."""
import logging
import os
import re

import pytest
import torch

from pytorchwavenetvocoder_amd.bin import train as T
from tests.test_train_cli import make_corpus
from tests.test_train_cli_freeze import _argv, _flags

LAMB = ["--layer_adaptation", "true", "--param_group", "bias$:adapt=true", "--max_trust_ratio", "10"]
RATIO_LINE = r"\(iter:(\d+)\) trust ratio min = (\S+), median = (\S+), max = (\S+) \((\d+) adapted tensors\)$"


def test_the_flags_parse():
    assert T.parse_param_group("bias$:adapt=true") == (r"bias$", {"layer_adaptation": True})
    assert T.parse_param_group("weight$:lr=1e-4,adapt=false") == (r"weight$", {"lr": 1e-4, "layer_adaptation": False})
    args = T.get_parser().parse_args(_flags("w", "f", "s", "e", 1, 1, 1) + LAMB)
    assert bool(args.layer_adaptation) is True and args.max_trust_ratio == 10.0 and args.param_group == ["bias$:adapt=true"]
    args = T.get_parser().parse_args(_flags("w", "f", "s", "e", 1, 1, 1))
    assert bool(args.layer_adaptation) is False and args.max_trust_ratio == 0.0


@pytest.mark.parametrize("extra, text", [(["--max_trust_ratio", "10"], "--max_trust_ratio"),
                                         (["--layer_adaptation", "true", "--max_trust_ratio", "-1"], "--max_trust_ratio"),
                                         (["--param_group", "bias$:adapt=true"], "adapt="),
                                         (["--layer_adaptation", "true", "--param_group", "bias$:adapt=maybe"], "--param_group")])
def test_conflicting_flags_exit_with_an_error(tmp_path, caplog, extra, text):
    """No corpus and no device: main() refuses the flags while it looks at the arguments."""
    exp = str(tmp_path / "exp")
    argv = _flags(str(tmp_path / "wav.scp"), str(tmp_path / "feats.scp"), str(tmp_path / "stats.h5"), exp, 1, 1, 1)
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as err:
        T.main(argv + extra)
    assert err.value.code not in (0, None)
    assert any(text in r.getMessage() for r in caplog.records)
    assert not os.path.exists(exp)


@pytest.mark.gpu
def test_lamb_run_logs_the_ratios_and_resumes(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=4)
    exp_a, exp_b = str(tmp_path / "plain"), str(tmp_path / "lamb")
    with caplog.at_level(logging.INFO):
        T.main(_argv(tmp_path, wavs, feats, stats, exp_a, 2, 1, 1))
    # without the flag: the files, keys and log lines of before
    assert sorted(os.listdir(exp_a)) == ["checkpoint-1.pkl", "checkpoint-final.pkl", "model.conf"]
    ck = torch.load(exp_a + "/checkpoint-1.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations"}
    assert len(ck["optimizer"]["param_groups"]) == 1 and "layer_adaptation" not in ck["optimizer"]["param_groups"][0]
    assert not any("trust ratio" in r.getMessage() or "layer-wise" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.INFO):
        T.main(_argv(tmp_path, wavs, feats, stats, exp_b, 2, 2, 1) + LAMB)
    msgs = [r.getMessage() for r in caplog.records]
    lines = [re.match(RATIO_LINE, m) for m in msgs if re.match(RATIO_LINE, m)]
    assert [int(m.group(1)) for m in lines] == [1, 2]   # one line per --intervals line
    keys = list(ck["model"].keys())
    for m in lines:
        lo, med, hi = (float(m.group(k)) for k in (2, 3, 4))
        assert 0.0 < lo <= med <= hi <= 10.0
        assert int(m.group(5)) == len(keys) - 2   # every tensor but the dead last res_1x1: the biases adapt too here
    assert sum("layer-wise adaptive steps" in m and "max trust ratio 10" in m and "adapt=True" in m for m in msgs) == 1
    out = torch.load(exp_b + "/checkpoint-1.pkl", weights_only=False)
    assert set(out.keys()) == {"model", "optimizer", "iterations"}
    assert all(sorted(st.keys()) == ["exp_avg", "exp_avg_sq", "step"] for st in out["optimizer"]["state"].values())
    assert any(not torch.equal(out["model"][k].cpu(), ck["model"][k].cpu()) for k in keys)   # not Adam's step
    # --resume with the same flags continues from the checkpoint's moments and count
    exp_c = str(tmp_path / "resumed")
    argv = _argv(tmp_path, wavs, feats, stats, exp_c, 2, 2, 1)
    T.main(argv[:-2] + ["--resume", exp_b + "/checkpoint-1.pkl"] + LAMB)
    assert sorted(os.listdir(exp_c)) == ["checkpoint-2.pkl", "checkpoint-final.pkl", "model.conf"]
    b = torch.load(exp_c + "/checkpoint-2.pkl", weights_only=False)
    assert b["iterations"] == 2 and {float(s["step"]) for s in b["optimizer"]["state"].values()} == {2.0}
    assert any(not torch.equal(b["model"][k].cpu(), out["model"][k].cpu()) for k in keys)
