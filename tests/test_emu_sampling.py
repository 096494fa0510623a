# -*- coding: utf-8 -*-
"""CPU-only: temperature / top-k / top-p sampling of the decode kernels (csrc/wn_sample.h) on the host emulator -- the five
token-choice sites (k_decode, k_dlp, k_dlpm, k_dlpf, k_dl_select_filtered) against the per-position float64 oracle of
tests/sampling_common.py, the external pin on the reference's golden tokens, and the exact invariants.  The seeds were picked so
that the float64 reference alone excuses less than the cap; the GPU suite repeats this on the real library."""
import pytest
import torch

from tests import sampling_common as SC
from tests.decode_common import DECODE_CASES, DecodeCase
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("setting", SC.SETTINGS, ids=SC.setting_id)
def test_one_workgroup_kernel_against_the_float64_oracle(setting):
    """k_decode on the golden cases (32, 32, 256 and 64 classes; 188 positions)."""
    from pytorchwavenetvocoder_amd.nets import WaveNet
    lib = emu_library()
    npos = nexc = 0
    for name in DECODE_CASES:
        g = DecodeCase(name)
        model = WaveNet(*g.cfg.as_tuple(), _library=lib)
        model.load_state_dict(g.params)
        torch.manual_seed(3)
        toks, lgs, log = SC.decode_logged(lib, model.engine, g.x, g.h, g.n_list, **SC.resolve(setting, g.cfg.n_quantize))
        assert SC.only_tag(log, "decode_steps_filtered"), log
        a, b = SC.check_decode(model.engine, toks, lgs, g.T0, g.n_list, setting, name)
        npos, nexc = npos + a, nexc + b
    SC.check_pool(npos, nexc, "k_decode %s" % SC.setting_id(setting))


# (kernel_size, utterances, samples): one utterance and three through k_dlp, 12 through the others -- the smallest shapes that
# reach each kernel (tests/test_emu_parity.py), as many samples as the pool of 150 positions needs
EMU_SHAPES = {"k_dlp": [(2, 1, 6), (3, 3, 50)], "k_dlpf": [(2, 12, 14)], "k_dlpm": [(2, 12, 14)], "k_dl_select": [(2, 12, 14)]}


@pytest.mark.parametrize("setting", SC.SETTINGS, ids=SC.setting_id)
@pytest.mark.parametrize("route", sorted(SC.ROUTES))
def test_any_size_routes_against_the_float64_oracle(route, setting):
    lib = emu_library()
    npos = nexc = 0
    for K, B, n in EMU_SHAPES[route]:
        a, b = SC.run_any_size(lib, "cpu", route, setting, K, B, 32, n, 5)
        npos, nexc = npos + a, nexc + b
    SC.check_pool(npos, nexc, "%s %s" % (route, SC.setting_id(setting)))


@pytest.mark.parametrize("route,Q", [("k_dlp", 40), ("k_dlpf", 40), ("k_dlpm", 40), ("k_dl_select", 40), ("k_dl_select", 100),
                                     ("k_dl_select", 256)])
def test_class_counts_that_are_no_multiple_of_64_and_256_classes(route, Q):
    """40 classes (one per lane, 24 lanes empty) on every any-size route; 100 (two per lane, the last lanes empty) and 256 on the
    layer-wise launches -- no persistent plan covers 256 classes on the 32-channel model (asserted), the GPU suite runs them on
    a 128-channel one.  The combined setting; every position is held to the oracle (token in B_hi; equal to the float64 token
    unless the float64 reference itself excuses the position).  These few positions are no pool of their own: the cap on the
    excused share is the routes' test above."""
    import ctypes
    lib = emu_library()
    B = 3 if route == "k_dlp" else 12
    if Q == 256:
        model = SC.any_size_model(lib, 2, 256)
        assert lib.wn_decode_layered_error_offset(ctypes.byref(model.engine.cfg), B, 0) < 0
    npos, nexc = SC.run_any_size(lib, "cpu", route, SC.SETTINGS[3], 2, B, Q, 5, 6)
    print("%s Q=%d: %d positions, %d excused" % (route, Q, npos, nexc))
    assert npos >= 12


@pytest.mark.parametrize("name", DECODE_CASES)
def test_top_k_1_and_a_tiny_nucleus_reproduce_the_reference_tokens(name):
    SC.check_golden_pin(name, emu_library(), "cpu")


def test_exact_invariants():
    SC.check_invariants(emu_library(), "cpu")


def test_two_groups_and_the_time_out_fall_back_carry_the_setting():
    SC.check_groups_and_fall_back(emu_library(), "cpu")
