# -*- coding: utf-8 -*-
"""The training CLI's two clipping options: the parser (CPU) and a few iterations on the GPU whose interval line reports the
gradient norm and the skipped steps.  In the style of tests/test_train_cli.py."""
import logging
import re

import pytest

from pytorchwavenetvocoder_amd.bin import train as T
from tests.test_train_cli import DIM, U, make_corpus

REQUIRED = ["--waveforms", "w", "--feats", "f", "--stats", "s", "--expdir", "e"]


def test_parser_takes_the_clipping_options_and_they_default_to_off():
    a = T.get_parser().parse_args(REQUIRED)
    assert a.max_grad_norm == 0.0 and not a.skip_nonfinite_steps
    a = T.get_parser().parse_args(REQUIRED + ["--max_grad_norm", "0.5", "--skip_nonfinite_steps", "true"])
    assert a.max_grad_norm == 0.5 and a.skip_nonfinite_steps == 1


@pytest.mark.gpu
def test_train_cli_logs_the_gradient_norm_and_the_skipped_steps(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path), n=4)
    scp_w, scp_f = str(tmp_path / "wav.scp"), str(tmp_path / "feats.scp")
    open(scp_w, "w").write("\n".join(wavs) + "\n")
    open(scp_f, "w").write("\n".join(feats) + "\n")
    max_norm = 1e-3   # far below the gradient norm of a freshly initialised model: the clip is active
    argv = ["--waveforms", scp_w, "--feats", scp_f, "--stats", stats, "--feature_type", "melspc",
            "--n_aux", str(DIM), "--n_resch", "64", "--n_skipch", "32", "--dilation_depth", "4",
            "--dilation_repeat", "2", "--upsampling_factor", str(U), "--batch_length", "800", "--batch_size", "2",
            "--intervals", "2", "--checkpoint_interval", "4", "--lr", "1e-3", "--verbose", "1",
            "--expdir", str(tmp_path / "exp"), "--iters", "4", "--resume", "",
            "--max_grad_norm", str(max_norm), "--skip_nonfinite_steps", "true"]
    with caplog.at_level(logging.INFO):
        T.main(argv)
    lines = [r.getMessage() for r in caplog.records if "gradient norm" in r.getMessage()]
    assert len(lines) == 2, caplog.text   # one per interval
    for line in lines:
        m = re.search(r"average gradient norm before clipping = ([0-9.eE+-]+), skipped steps = (\d+)", line)
        assert m, line
        assert float(m.group(1)) > max_norm and int(m.group(2)) == 0
