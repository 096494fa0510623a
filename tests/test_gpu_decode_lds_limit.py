# -*- coding: utf-8 -*-
"""The dynamic-LDS limit of a kernel follows the launch, not the first model of the process (csrc/wn_device.h, wn_dyn_lds).

The one-workgroup decode kernel keeps every layer's queue taps and bias tables in LDS, so its dynamic LDS grows with the number
of layers while its compiled class (kernel_size <= 2, n_resch <= 64: ``k_decode<8,2,8,32,32>``) stays the same.  Two toy models
of that class, both beyond the 64 KB a kernel gets by default (wn_decode_make_plan: 40 layers = 75 328 bytes, 52 layers =
96 832 bytes), decode one after the other in one process: the second launch needs a limit above the one the first launch set.
"""
import numpy as np
import pytest
import torch

from oracle import wavenet_oracle as O
from tests import parity_common as PC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG_A = (256, 16, 64, 64, 4, 10, 2, 16)   # 40 layers
CFG_B = (256, 16, 64, 64, 4, 13, 2, 16)   # 52 layers
N = 12                                     # generated samples (as smoke())


def _decode(cfg_t, seed):
    from pytorchwavenetvocoder_amd.nets import WaveNet
    cfg = O.OracleConfig(*cfg_t)
    params = O.random_params(cfg, seed)
    model = WaveNet(*cfg_t)
    model.load_state_dict(params)
    model.to(DEV)
    assert model.engine.decode_supported()
    gx = torch.tensor([[3, 200, 17]]).long()
    gh = torch.from_numpy(np.random.RandomState(seed + 1).standard_normal((1, 16, 2)).astype("float32"))
    out = {}
    log = PC.launch_log(model.engine.lib, lambda: out.update(p=model.engine.decode(gx.to(DEV), gh.to(DEV), [N], return_logits=True)))
    assert log.get("decode_steps", 0) >= 1 and "dl_dilated" not in log and "dlp_steps" not in log, log
    return cfg, params, gx, gh, out["p"][0][0].cpu().numpy(), out["p"][1][0].cpu()


def test_a_later_model_of_the_same_decode_class_gets_the_larger_lds_it_needs():
    _decode(CFG_A, 21)
    cfg, params, gx, gh, tok, lg = _decode(CFG_B, 23)
    ref_tok, ref_lg = O.fast_generate(cfg, params, gx, gh, N, return_logits=True)
    e = float((lg - ref_lg).abs().max())
    print("52 layers after 40 in one process: decode logits vs oracle err %.3g (max |logit| %.3g)" % (e, float(ref_lg.abs().max())))
    assert e <= 1e-4, e
    top2 = ref_lg.topk(2, dim=1).values
    safe = ((top2[:, 0] - top2[:, 1]) > 1e-3).numpy()
    assert (tok[safe] == np.asarray(ref_tok)[safe]).all()
