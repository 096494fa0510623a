# -*- coding: utf-8 -*-
"""The training CLI with parameter groups (``--param_group``).  On the GPU, like the other CLI tests (the training loop itself
needs the device), on the tiny corpus of tests/test_train_cli.py: the groups are logged once with their tensor and element
counts, the checkpoint carries them in torch's format and resumes, a pattern that matches nothing is refused, and a run without
the flag writes the files and keys of before.  Without a device: the flag's syntax, checked before anything is read or built."""
import logging
import os
import re

import pytest
import torch

from pytorchwavenetvocoder_amd.bin import train as T
from tests.test_train_cli import make_corpus
from tests.test_train_cli_freeze import _argv, _flags

GROUPS = ["--param_group", r"bias$:lr=3e-3,weight_decay=0", "--param_group", r"conv_post|skip_1x1:lr=1e-4,weight_decay=0.1,decoupled=true,eps=1e-6"]
LOG_LINE = r"parameter group (\d) \((.*)\): lr=(\S+) weight_decay=(\S+) eps=(\S+) decoupled=(True|False), (\d+) tensors, (\d+) elements$"


def test_the_flag_parses():
    assert T.parse_param_group(GROUPS[1]) == (r"bias$", {"lr": 3e-3, "weight_decay": 0.0})
    assert T.parse_param_group(GROUPS[3]) == (r"conv_post|skip_1x1", {"lr": 1e-4, "weight_decay": 0.1, "decoupled_weight_decay": True,
                                                                       "eps": 1e-6})
    assert T.parse_param_group(r"^(?:a|b):c:lr=1") == (r"^(?:a|b):c", {"lr": 1.0})   # the values stand behind the last colon
    args = T.get_parser().parse_args(_flags("w", "f", "s", "e", 1, 1, 1) + GROUPS)
    assert args.param_group == [GROUPS[1], GROUPS[3]]
    assert T.get_parser().parse_args(_flags("w", "f", "s", "e", 1, 1, 1)).param_group is None


@pytest.mark.parametrize("spec", ["bias", "bias:", "bias:lr", "bias:momentum=0.9", "bias:betas=0.5", "bias:lr=fast", "(:lr=1e-3",
                                  "bias:decoupled=maybe"])
def test_a_malformed_group_exits_with_an_error(tmp_path, spec, caplog):
    """No corpus and no device: main() refuses the flag while it looks at the arguments."""
    exp = str(tmp_path / "exp")
    argv = _flags(str(tmp_path / "wav.scp"), str(tmp_path / "feats.scp"), str(tmp_path / "stats.h5"), exp, 1, 1, 1)
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as err:
        T.main(argv + ["--param_group", spec])
    assert err.value.code not in (0, None)
    assert any("--param_group" in r.getMessage() and repr(spec) in r.getMessage() for r in caplog.records)
    assert not os.path.exists(exp)


@pytest.mark.gpu
def test_groups_are_logged_saved_and_resumed(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=4)
    exp_a, exp_b = str(tmp_path / "plain"), str(tmp_path / "groups")
    with caplog.at_level(logging.INFO):
        T.main(_argv(tmp_path, wavs, feats, stats, exp_a, 2, 1, 1))
    # without the flag: the files, keys and log lines of before
    assert sorted(os.listdir(exp_a)) == ["checkpoint-1.pkl", "checkpoint-final.pkl", "model.conf"]
    ck = torch.load(exp_a + "/checkpoint-1.pkl", weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations"}
    assert len(ck["optimizer"]["param_groups"]) == 1 and "decoupled_weight_decay" not in ck["optimizer"]["param_groups"][0]
    assert ck["optimizer"]["param_groups"][0]["params"] == list(range(len(ck["model"])))
    assert not any(re.match(LOG_LINE, r.getMessage()) for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.INFO):
        T.main(_argv(tmp_path, wavs, feats, stats, exp_b, 2, 2, 1) + GROUPS)
    lines = [re.match(LOG_LINE, r.getMessage()) for r in caplog.records if re.match(LOG_LINE, r.getMessage())]
    assert len(lines) == 3   # logged once
    keys = list(ck["model"].keys())
    of = [1 if re.search(r"bias$", k) else 2 if re.search(r"conv_post|skip_1x1", k) else 0 for k in keys]
    for i, m in enumerate(lines):
        mine = [k for k, g in zip(keys, of) if g == i]
        assert int(m.group(1)) == i and (int(m.group(7)), int(m.group(8))) == (len(mine), sum(ck["model"][k].numel() for k in mine))
    assert [float(m.group(3)) for m in lines] == [1e-3, 3e-3, 1e-4] and [m.group(6) for m in lines] == ["False", "False", "True"]
    out = torch.load(exp_b + "/checkpoint-1.pkl", weights_only=False)
    pg = out["optimizer"]["param_groups"]
    assert [g["lr"] for g in pg] == [1e-3, 3e-3, 1e-4] and [g["decoupled_weight_decay"] for g in pg] == [False, False, True]
    assert sorted(i for g in pg for i in g["params"]) == list(range(len(keys))) and [len(g["params"]) for g in pg] == [of.count(i) for i in range(3)]
    # --resume with the same groups continues from the checkpoint's moments, count and group values
    exp_c = str(tmp_path / "resumed")
    argv = _argv(tmp_path, wavs, feats, stats, exp_c, 2, 2, 1)
    T.main(argv[:-2] + ["--resume", exp_b + "/checkpoint-1.pkl"] + GROUPS)
    assert sorted(os.listdir(exp_c)) == ["checkpoint-2.pkl", "checkpoint-final.pkl", "model.conf"]
    b = torch.load(exp_c + "/checkpoint-2.pkl", weights_only=False)
    assert b["iterations"] == 2 and [g["lr"] for g in b["optimizer"]["param_groups"]] == [1e-3, 3e-3, 1e-4]
    assert {float(s["step"]) for s in b["optimizer"]["state"].values()} == {2.0}
    assert any(not torch.equal(b["model"][k].cpu(), out["model"][k].cpu()) for k in keys)
    # ... and without them the structure does not match
    with pytest.raises(ValueError, match="parameter groups"):
        T.main(argv[:-2] + ["--resume", exp_b + "/checkpoint-1.pkl", "--expdir", str(tmp_path / "mismatch")])


@pytest.mark.gpu
def test_a_pattern_that_matches_nothing_is_refused(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=4)
    with caplog.at_level(logging.ERROR), pytest.raises(SystemExit) as err:
        T.main(_argv(tmp_path, wavs, feats, stats, str(tmp_path / "exp"), 2, 1, 1) + ["--param_group", "no_such_tensor:lr=1e-3"])
    assert err.value.code not in (0, None)
    assert any("matches no parameter" in r.getMessage() for r in caplog.records)
