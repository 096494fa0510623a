# -*- coding: utf-8 -*-
"""decode.py --temperature / --top_k / --top_p (extension flags): defaults are the identity, --top_k 1 writes the waveform of an
argmax decode, and without the flags the tool writes what a plain sampling decode under the same seed writes."""
import os

import numpy as np
import pytest
import torch

from pytorchwavenetvocoder_amd.bin import decode as D
from pytorchwavenetvocoder_amd.nets import decode_mu_law, encode_mu_law
from tests.test_train_cli import DIM, U, make_corpus


def test_sampling_flags_default_to_the_identity_and_stay_out_of_the_reference_table():
    a = D.get_parser().parse_args(["--feats", "f", "--checkpoint", "c", "--outdir", "o"])
    assert (a.temperature, a.top_k, a.top_p) == (1.0, 0, 1.0)
    a = D.get_parser().parse_args(["--feats", "f", "--checkpoint", "c", "--outdir", "o", "--temperature", "0.8", "--top_k", "16",
                                   "--top_p", "0.95"])
    assert (a.temperature, a.top_k, a.top_p) == (0.8, 16, 0.95)
    assert not {"temperature", "top_k", "top_p"} & {f[0] for f in D._FLAGS}   # the reference's own flags are as they were


def _module_wavs(tmp_path, ckpt, stats, outdir, seed, **kw):
    """What decode.py does for --batch_size 1, through the module API: seed, model, one fast_generate per file."""
    from pytorchwavenetvocoder_amd.utils import find_files, make_feat_transform, read_hdf5
    config = torch.load(os.path.join(os.path.dirname(ckpt), "model.conf"), weights_only=False)
    np.random.seed(seed)
    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    model = D.build_model(config)
    model.load_state_dict(D.checkpoint_weights(ckpt))
    model.eval()
    model.to(dev)
    mean = read_hdf5(stats, "/" + config.feature_type + "/mean")
    scale = read_hdf5(stats, "/" + config.feature_type + "/scale")
    gen = D.decode_generator(sorted(find_files(os.path.join(str(tmp_path), "h5"), "*.h5")), batch_size=1,
                             feature_type=config.feature_type, wav_transform=lambda x: encode_mu_law(x, config.n_quantize),
                             feat_transform=make_feat_transform(mean, scale), upsampling_factor=config.upsampling_factor,
                             use_upsampling_layer=config.use_upsampling_layer, use_speaker_code=config.use_speaker_code, device=dev)
    os.makedirs(outdir, exist_ok=True)
    with torch.no_grad():
        for feat_id, (x, h, n) in gen:
            D.write_wav(os.path.join(outdir, feat_id + ".wav"), decode_mu_law(model.fast_generate(x, h, n, 1000, **kw), config.n_quantize), 16000)


@pytest.mark.gpu
def test_top_k_1_is_the_argmax_waveform_and_no_flags_is_the_plain_decode(tmp_path):
    from pytorchwavenetvocoder_amd.bin import train as T
    wavs, feats, stats = make_corpus(str(tmp_path), n=2)
    exp = str(tmp_path / "exp")
    T.main(["--waveforms", os.path.join(str(tmp_path), "wav"), "--feats", os.path.join(str(tmp_path), "h5"),
            "--stats", stats, "--expdir", exp, "--feature_type", "melspc", "--n_aux", str(DIM), "--n_resch", "16",
            "--n_skipch", "16", "--dilation_depth", "3", "--dilation_repeat", "2", "--upsampling_factor", str(U),
            "--batch_length", "2000", "--batch_size", "2", "--iters", "2", "--checkpoint_interval", "2",
            "--intervals", "1", "--verbose", "0"])
    ckpt = os.path.join(exp, "checkpoint-final.pkl")
    common = ["--feats", os.path.join(str(tmp_path), "h5"), "--checkpoint", ckpt, "--stats", stats, "--batch_size", "1",
              "--intervals", "1000", "--verbose", "0", "--seed", "4"]
    D.main(common + ["--outdir", str(tmp_path / "k1"), "--top_k", "1"])
    _module_wavs(tmp_path, ckpt, stats, str(tmp_path / "argmax"), 4, mode="argmax")
    D.main(common + ["--outdir", str(tmp_path / "plain")])
    _module_wavs(tmp_path, ckpt, stats, str(tmp_path / "module"), 4)
    for i in range(2):
        name = "utt%d.wav" % i
        k1, am = (open(os.path.join(str(tmp_path / d), name), "rb").read() for d in ("k1", "argmax"))
        assert k1 == am and len(k1) > 44
        pl, mo = (open(os.path.join(str(tmp_path / d), name), "rb").read() for d in ("plain", "module"))
        assert pl == mo and pl != am
