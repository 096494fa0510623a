# -*- coding: utf-8 -*-
"""Host side of the held-out loss of the training CLI: ``evaluate_corpus`` on the kernel emulator (every utterance once, the odd
last group, shards, utterances shorter than the receptive field), the four flags, and ``train_generator`` still bit-equal to
the reference generator's golden minibatches now that its reading / transform code is shared.  CPU only; the CLI itself runs
in tests/test_train_cli_eval.py."""
import logging
import math
import os

import numpy as np
import pytest
import torch

from pytorchwavenetvocoder_amd.bin import train as T
from pytorchwavenetvocoder_amd.nets import WaveNet, encode_mu_law, initialize
from pytorchwavenetvocoder_amd.utils import write_hdf5
from tests import parity_common as PC
from tests.emu_util import emu_library
from tests.test_train_cli import DIM, FS, U, _slicer_kwargs, _write_slicer_corpus, make_corpus

pytestmark = pytest.mark.emu
Q = 64
REQUIRED = ["--waveforms", "w", "--feats", "f", "--stats", "s", "--expdir", "e"]


def _model(upsampling_factor):
    torch.manual_seed(3)
    model = WaveNet(Q, DIM, 8, 12, 3, 2, 2, upsampling_factor, _library=emu_library())
    model.apply(initialize)
    return model


def _kw(upsample=True, u=U):
    return dict(feature_type="melspc", wav_transform=lambda x: encode_mu_law(x, Q), feat_transform=lambda h: h,
                upsampling_factor=u, use_upsampling_layer=upsample, transforms_elementwise=True)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dev"))
    wavs, feats, _ = make_corpus(root, n=5)
    model = _model(U)
    full = T.evaluate_corpus(model, wavs, feats, 2, **_kw())
    return wavs, feats, model, full


def test_every_utterance_is_scored_exactly_once(corpus):
    wavs, feats, model, (nll, npos, per_utt, n_short) = corpus
    assert [i for i, _, _ in per_utt] == [0, 1, 2, 3, 4] and n_short == 0   # 5 utterances in groups of 2: the odd last group too
    rf = model.receptive_field
    for i, v, n in per_utt:
        frames = 60 + 7 * i          # make_corpus: the utterance modes keep frames - 1 whole frames
        assert n == (frames - 1) * U - rf and v > 0.0
    assert npos == sum(n for _, _, n in per_utt)
    # the device-side double accumulator is the fp64 sum of the fp32 per-utterance sums
    assert abs(nll - math.fsum(v for _, v, _ in per_utt)) <= 1e-12 * nll
    assert model.engine._eval_ws is None   # released at the end of the pass


def test_per_utterance_values_equal_the_utterance_alone(corpus):
    wavs, feats, model, (nll, npos, per_utt, _) = corpus
    for i, v, n in per_utt:
        _, n1, alone, _ = T.evaluate_corpus(model, [wavs[i]], [feats[i]], 1, **_kw())
        assert alone[0][2] == n == n1
        assert abs(alone[0][1] / n - v / n) <= PC.TOL_LOSS, (i, alone[0][1] / n, v / n)


def test_two_shards_are_the_unsharded_pass(corpus):
    wavs, feats, model, (nll, npos, per_utt, _) = corpus
    cache = {}
    parts = [T.evaluate_corpus(model, wavs, feats, 2, shard=(r, 2), length_cache=cache, **_kw()) for r in range(2)]
    assert len(cache) == 5
    assert [len(p[2]) for p in parts] == [3, 2]   # groups 0 and 2 (2 + 1 utterances) / group 1
    union = sorted(parts[0][2] + parts[1][2])
    assert union == per_utt                       # identical per-utterance bits
    assert parts[0][1] + parts[1][1] == npos
    assert abs(parts[0][0] + parts[1][0] - nll) <= 1e-12 * nll


def test_utterances_not_longer_than_the_receptive_field(tmp_path, caplog):
    """Sample-rate features (no upsampling layer), three utterances of 11, 41 and 31 samples, receptive field 15: the first
    has no position to score, counts 0, is warned about once and is still listed."""
    from scipy.io import wavfile
    rs = np.random.RandomState(1)
    wavs, feats = [], []
    for i, n in enumerate((11, 41, 31)):
        w, f = str(tmp_path / ("s%d.wav" % i)), str(tmp_path / ("s%d.h5" % i))
        wavfile.write(w, FS, (rs.uniform(-0.5, 0.5, size=n) * 32767).astype(np.int16))
        write_hdf5(f, "/melspc", rs.standard_normal((n, DIM)).astype(np.float32))
        wavs.append(w)
        feats.append(f)
    model = _model(0)
    assert model.receptive_field == 15
    with caplog.at_level(logging.WARNING):
        nll, npos, per_utt, n_short = T.evaluate_corpus(model, wavs, feats, 2, **_kw(upsample=False, u=1))
    assert n_short == 1 and len([r for r in caplog.records if "receptive field" in r.getMessage()]) == 1
    assert [(i, n) for i, _, n in per_utt] == [(0, 0), (1, 25), (2, 15)] and per_utt[0][1] == 0.0
    assert npos == 40 and nll > 0.0


def test_parser_takes_the_dev_flags_and_they_default_to_off():
    a = T.get_parser().parse_args(REQUIRED)
    assert a.dev_waveforms is None and a.dev_feats is None and a.eval_interval == 0 and a.eval_batch_size == 8
    a = T.get_parser().parse_args(REQUIRED + ["--dev_waveforms", "dw", "--dev_feats", "df", "--eval_interval", "50",
                                              "--eval_batch_size", "4"])
    assert (a.dev_waveforms, a.dev_feats, a.eval_interval, a.eval_batch_size) == ("dw", "df", 50, 4)


@pytest.mark.parametrize("name,workers,pre", [("utt_up", 0, True), ("utt_noup", 3, False), ("win_up_spk", 3, True),
                                              ("win_noup", 0, False)])
def test_train_generator_is_still_the_reference_generator(tmp_path, name, workers, pre):
    """The reading / transform code evaluate_corpus shares with train_generator was lifted out of its closure: the minibatches
    are still bit-equal to the reference generator's (tests/golden/slicer.npz, the helpers of tests/test_train_cli.py)."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "slicer.npz"))
    wavs, feats, mean, scale = _write_slicer_corpus(str(tmp_path))
    kw, nb = _slicer_kwargs(name, mean, scale)
    gen = T.train_generator(wavs, feats, workers=workers, transforms_elementwise=pre, **kw)
    try:
        for i in range(nb):
            (x, h), t = gen.next()
            np.testing.assert_array_equal(x.numpy(), z["%s/%d/x" % (name, i)].astype(np.int64))
            np.testing.assert_array_equal(t.numpy(), z["%s/%d/t" % (name, i)].astype(np.int64))
            gh = z["%s/%d/h" % (name, i)]
            assert h.numpy().shape == gh.shape and (h.numpy().view(np.uint32) == gh.view(np.uint32)).all()
    finally:
        gen.close()


def test_padding_is_the_padded_generators(tmp_path):
    """A group of evaluate_corpus is padded exactly as train_generator(pad_utterances=True) pads the same utterances."""
    wavs, feats, _ = make_corpus(str(tmp_path), n=2)
    gen = T.train_generator(wavs, feats, receptive_field=15, batch_length=None, batch_size=2, pad_utterances=True, shuffle=False,
                            device=None, n_quantize=Q, **_kw())
    try:
        (gx, gh), gt, glen, _ = gen.next()
    finally:
        gen.close()
    seen = []

    class Spy(object):
        n_quantize, n_mixture, receptive_field = Q, 0, 15

        class engine(object):
            device = torch.device("cpu")

            @staticmethod
            def release_eval_workspace():
                pass

        def evaluate(self, x, h, t=None, lengths=None, acc=None):
            seen.append((x, h, t, lengths))
            return torch.zeros(x.size(0)), [0] * x.size(0)

    T.evaluate_corpus(Spy(), wavs, feats, 2, **_kw())
    (x, h, t, lengths), = seen
    assert torch.equal(x, gx) and torch.equal(h, gh) and torch.equal(t, gt) and torch.equal(lengths, glen)


@pytest.mark.parametrize("dev_best", [None, (5.25, 20)], ids=["before_the_first_pass", "after_a_pass"])
def test_dev_state_round_trips_through_a_checkpoint(tmp_path, dev_best):
    """The "dev" entry of a regular checkpoint and what --resume restores from it: a checkpoint written in front of the first
    pass over the held-out set (--eval_interval larger than --checkpoint_interval, or only NaN losses so far) holds Nones and
    restores to "no best yet"; a run without a held-out set writes no entry."""
    net = torch.nn.Linear(2, 2)
    opt = torch.optim.Adam(net.parameters())
    T.save_checkpoint(str(tmp_path), net, opt, 7, dev=T.dev_best_state(dev_best))
    ck = torch.load(str(tmp_path / "checkpoint-7.pkl"), weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations", "dev"} and set(ck["dev"]) == {"best_loss", "best_iterations"}
    assert T.dev_best_from_checkpoint(ck) == dev_best
    T.save_checkpoint(str(tmp_path), net, opt, 8)
    ck = torch.load(str(tmp_path / "checkpoint-8.pkl"), weights_only=False)
    assert set(ck.keys()) == {"model", "optimizer", "iterations"} and T.dev_best_from_checkpoint(ck) is None
    assert T.dev_best_from_checkpoint({"dev": {"best_loss": None, "best_iterations": 3}}) is None
