# -*- coding: utf-8 -*-
"""Padded utterance batches of the training CLI (``train_generator(pad_utterances=True)``, ``--utterance_batch``): the
valid parts are the batch-size-1 utterance batches element for element, the padding is as documented, ``lengths`` is right,
two ranks' batches are the rows of the one-rank batch.  CPU only; the HIP step of the CLI is the gpu-marked test below."""
import os
import subprocess
import sys

import pytest
import torch

from pytorchwavenetvocoder_amd.bin import train as T
from pytorchwavenetvocoder_amd.nets import encode_mu_law
from tests.test_train_cli import DIM, U, make_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 64


def _gen(wavs, feats, upsample, **kw):
    return T.train_generator(wavs, feats, receptive_field=300, batch_length=None, feature_type="melspc",
                             wav_transform=lambda x: encode_mu_law(x, Q), feat_transform=lambda h: h, shuffle=False,
                             upsampling_factor=U, use_upsampling_layer=upsample, device=None, n_quantize=Q, **kw)


@pytest.mark.parametrize("with_wave", [False, True])
@pytest.mark.parametrize("upsample", [True, False])
def test_padded_batches_hold_the_single_utterance_batches(tmp_path, upsample, with_wave):
    wavs, feats, stats = make_corpus(str(tmp_path), n=6)
    single = _gen(wavs, feats, upsample, batch_size=1, with_wave=with_wave)
    padded = _gen(wavs, feats, upsample, batch_size=3, pad_utterances=True, with_wave=with_wave)
    for _ in range(4):   # two walks of the six utterances
        item = padded.next()
        (x, h), t = item[0], item[1]
        lengths, all_lengths = item[-2], item[-1]
        assert x.shape[0] == 3 and torch.equal(lengths, all_lengths) and lengths.dtype == torch.int64
        assert x.shape[1] == int(lengths.max()) and x.shape == t.shape
        if upsample:
            assert x.shape[1] % U == 0 and h.shape[2] * U == x.shape[1]
        else:
            assert h.shape[2] == x.shape[1]
        for b in range(3):
            one = single.next()
            (x1, h1), t1 = one[0], one[1]
            n = int(lengths[b])
            assert x1.shape == (1, n)
            assert torch.equal(x[b, :n], x1[0]) and torch.equal(t[b, :n], t1[0])
            assert bool((x[b, n:] == Q // 2).all()) and bool((t[b, n:] == Q // 2).all())
            f = h1.shape[2]
            assert torch.equal(h[b, :, :f], h1[0])
            assert torch.equal(h[b, :, f:], h1[0, :, -1:].expand(-1, h.shape[2] - f))   # the last frame, repeated
            if with_wave:
                assert torch.equal(item[2][b, :n], one[2][0]) and bool((item[2][b, n:] == 0).all())
    single.close()
    padded.close()


@pytest.mark.parametrize("upsample", [True, False])
def test_two_ranks_hold_the_rows_of_the_one_rank_batch(tmp_path, upsample):
    wavs, feats, stats = make_corpus(str(tmp_path), n=6)
    whole = _gen(wavs, feats, upsample, batch_size=3, pad_utterances=True)
    ranks = [_gen(wavs, feats, upsample, batch_size=3, pad_utterances=True, shard=(r, 2)) for r in range(2)]
    for _ in range(3):
        (x, h), t, lengths, all_lengths = whole.next()
        lo = 0
        for r in range(2):
            (xr, hr), tr, lr, ar = ranks[r].next()
            assert torch.equal(ar, all_lengths)
            rows = T._shard_range(3, (r, 2))
            assert rows[0] == lo and xr.shape[0] == rows[1] - rows[0]
            assert torch.equal(lr, lengths[rows[0]:rows[1]])
            Tr = int(lr.max())                       # padded to the rank's OWN longest utterance
            assert xr.shape[1] == Tr and Tr <= x.shape[1]
            assert torch.equal(xr, x[rows[0]:rows[1], :Tr]) and torch.equal(tr, t[rows[0]:rows[1], :Tr])
            assert torch.equal(hr, h[rows[0]:rows[1], :, :hr.shape[2]])
            lo = rows[1]
        assert lo == 3
    for g in [whole] + ranks:
        g.close()


def test_default_stays_batch_size_one(tmp_path, caplog):
    wavs, feats, stats = make_corpus(str(tmp_path))
    gen = _gen(wavs, feats, True, batch_size=3)
    item = gen.next()
    assert len(item) == 2 and item[0][0].shape[0] == 1
    gen.close()


def test_cli_flag():
    p = T.get_parser()
    base = ["--waveforms", "w", "--feats", "f", "--stats", "s", "--expdir", "e"]
    assert p.parse_args(base).utterance_batch is False
    assert p.parse_args(base + ["--utterance_batch", "true", "--batch_size", "3"]).utterance_batch


def _train(tmp_path, extra, env_extra=None):
    root = str(tmp_path)
    wavs, feats, stats = make_corpus(os.path.join(root, "corpus"), n=6)
    scp_w, scp_f = os.path.join(root, "wav.scp"), os.path.join(root, "feats.scp")
    open(scp_w, "w").write("\n".join(wavs) + "\n")
    open(scp_f, "w").write("\n".join(feats) + "\n")
    exp = os.path.join(root, "exp")
    cmd = [sys.executable, "-m", "pytorchwavenetvocoder_amd.bin.train", "--waveforms", scp_w, "--feats", scp_f, "--stats", stats,
           "--expdir", exp, "--feature_type", "melspc", "--n_quantize", "128", "--n_aux", str(DIM), "--n_resch", "64",
           "--n_skipch", "128", "--dilation_depth", "3", "--dilation_repeat", "1", "--upsampling_factor", str(U),
           "--utterance_batch", "true", "--batch_size", "3", "--iters", "4", "--checkpoint_interval", "2", "--intervals", "2"] + extra
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")   # (as tests/test_gpu_two_ranks_one_gpu.py)
    env.update(env_extra or {})
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "(iter:4) average loss" in r.stderr and "final checkpoint created." in r.stderr
    return exp, feats, stats


def _check_checkpoint(exp, feats, stats, tmp_path):
    ck = torch.load(os.path.join(exp, "checkpoint-final.pkl"), map_location="cpu", weights_only=False)
    for k, v in ck["model"].items():
        assert bool(torch.isfinite(v).all()), k
    assert os.path.exists(os.path.join(exp, "checkpoint-4.pkl"))
    # decode.py rebuilds the model from model.conf, loads the checkpoint and writes the wavs
    from pytorchwavenetvocoder_amd.bin import decode as D
    out = os.path.join(str(tmp_path), "wav_out")
    D.main(["--feats", os.path.dirname(feats[0]), "--checkpoint", os.path.join(exp, "checkpoint-final.pkl"), "--stats", stats,
            "--outdir", out, "--batch_size", "2", "--intervals", "1000", "--verbose", "0"])
    assert len([f for f in os.listdir(out) if f.endswith(".wav")]) == len(feats)


@pytest.mark.gpu
def test_train_cli_utterance_batches(tmp_path):
    exp, feats, stats = _train(tmp_path, [])
    _check_checkpoint(exp, feats, stats, tmp_path)


@pytest.mark.gpu
def test_train_cli_utterance_batches_two_ranks_one_gpu(tmp_path):
    exp, feats, stats = _train(tmp_path, ["--n_gpus", "2"], {"WN_TRAIN_BACKEND": "gloo"})
    _check_checkpoint(exp, feats, stats, tmp_path)
