# -*- coding: utf-8 -*-
"""Temperature / top-k / top-p sampling on the MI355X: every decode route of the real library against the per-position float64
oracle of tests/sampling_common.py (pools of at least 1000 positions per route and setting), the external pin on the reference's
golden tokens, and the exact invariants.  The same checks run on the host emulator in tests/test_emu_sampling.py."""
import numpy as np
import pytest
import torch

from tests import sampling_common as SC

pytestmark = pytest.mark.gpu

GPU_POOL = 1000


@pytest.fixture(scope="module")
def lib():
    from pytorchwavenetvocoder_amd import _lib
    return _lib.load_library()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda")


@pytest.fixture(scope="module")
def r64(lib, dev):
    """The 256-class model of the golden case decode_r64_k2_up (the one-workgroup kernel's class) with 6 utterances."""
    from pytorchwavenetvocoder_amd.nets import WaveNet
    from tests.decode_common import DecodeCase
    g = DecodeCase("decode_r64_k2_up")
    model = WaveNet(*g.cfg.as_tuple(), _library=lib)
    model.load_state_dict(g.params)
    model.to(dev)
    rs = np.random.RandomState(77)
    B, n = 6, 200
    x = torch.from_numpy(rs.randint(0, g.cfg.n_quantize, (B, 3))).long().to(dev)
    h = torch.from_numpy(rs.standard_normal((B, g.cfg.n_aux, (3 + n) // g.cfg.upsampling_factor + 2)).astype(np.float32)).to(dev)
    return model, x, h, [n - 7 * b for b in range(B)]


@pytest.mark.parametrize("setting", SC.SETTINGS, ids=SC.setting_id)
def test_one_workgroup_kernel_against_the_float64_oracle(lib, r64, setting):
    model, x, h, ns = r64
    torch.manual_seed(11)
    toks, lgs, log = SC.decode_logged(lib, model.engine, x, h, ns, **SC.resolve(setting, 256))
    assert SC.only_tag(log, "decode_steps_filtered"), log
    npos, nexc = SC.check_decode(model.engine, toks, lgs, 3, ns, setting, "k_decode")
    assert npos >= GPU_POOL
    SC.check_pool(npos, nexc, "k_decode %s" % SC.setting_id(setting))


@pytest.mark.parametrize("setting", SC.SETTINGS, ids=SC.setting_id)
@pytest.mark.parametrize("route", sorted(SC.ROUTES))
def test_any_size_routes_against_the_float64_oracle(lib, dev, route, setting):
    """The smallest models that reach each kernel (32 channels; k_dlp with one and with three utterances, the others with 12), and
    with the combined setting the variants: 40 classes (not a multiple of 64) on every route, 100 (two classes per lane, the last
    lanes empty) and 256 classes on the layer-wise launches, 256 classes on a 128-channel model on the persistent kernels (the plan
    of the 32-channel model does not cover 256 classes)."""
    npos = nexc = 0
    for K, B in SC.ROUTES[route]["shapes"]:
        a, b = SC.run_any_size(lib, dev, route, setting, K, B, 32, 1100 // B + 3, 21)
        npos, nexc = npos + a, nexc + b
    assert npos >= GPU_POOL
    if setting is SC.SETTINGS[3]:
        B = 3 if route == "k_dlp" else 12
        for Q in (40,) + ((100, 256) if route == "k_dl_select" else ()):
            a, b = SC.run_any_size(lib, dev, route, setting, 2, B, Q, 40, 22)
            npos, nexc = npos + a, nexc + b
        if route != "k_dl_select":
            from oracle import wavenet_oracle as O
            from pytorchwavenetvocoder_amd.nets import WaveNet
            cfg_t = (256, 4, 128, 32, 3, 2, 2, 4)
            model = WaveNet(*cfg_t, _library=lib)
            model.load_state_dict(O.random_params(O.OracleConfig(*cfg_t), 31, scale=0.2))
            model.to(dev)
            a, b = SC.run_any_size(lib, dev, route, setting, 2, B, 256, 40, 23, model=model)
            npos, nexc = npos + a, nexc + b
    SC.check_pool(npos, nexc, "%s %s" % (route, SC.setting_id(setting)))


@pytest.mark.parametrize("name", ["decode_tiny_k2_up", "decode_tiny_k3_noup", "decode_r64_k2_up", "decode_r64_longctx"])
def test_top_k_1_and_a_tiny_nucleus_reproduce_the_reference_tokens(lib, dev, name):
    SC.check_golden_pin(name, lib, dev)


def test_exact_invariants(lib, dev):
    SC.check_invariants(lib, dev)


def test_two_groups_and_the_time_out_fall_back_carry_the_setting(lib, dev):
    SC.check_groups_and_fall_back(lib, dev)
