# -*- coding: utf-8 -*-
"""Global-norm gradient clipping and the non-finite-step guard on the MI355X, through the real library: the cases of
tests/test_emu_clip.py (tests/clip_common.py), the second golden case, and the norm of one buffer on two streams and in two
engines."""
import pytest
import torch

from tests import clip_common as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("n", CC.SIZES)
def test_norm_op_level(n, misalign):
    CC.check_norm(_lib(), DEV, n, misalign)


def test_norm_range():
    CC.check_range(_lib(), DEV)


@pytest.mark.parametrize("misalign", [0, 1])
def test_nonfinite_detection(misalign):
    CC.check_nonfinite(_lib(), DEV, misalign)


@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["clip_active", "clip_inactive"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_clipped_step_against_torch_op_level(weight_decay, factor):
    CC.check_clipped_step(_lib(), DEV, weight_decay, factor)


@pytest.mark.parametrize("name", ["tiny_k2_up", "r64_k2_up"])
def test_module_level_clipped_training(name):
    CC.check_module_clipped_training(name, _lib(), DEV)


def test_nonfinite_step_is_skipped_and_the_next_one_is_adams_first():
    CC.check_skip(_lib(), DEV)


def test_guard_off_nan_reaches_the_weights_as_in_torch():
    CC.check_guard_off_nan_reaches_the_weights(_lib(), DEV)


def test_defaults_are_the_plain_path_bit_for_bit():
    CC.check_defaults(_lib(), DEV)


def test_guarded_path_launches_and_agreement_with_the_plain_path():
    CC.check_guarded_launches_and_plain_agreement(_lib(), DEV)


def test_checkpoint_round_trip():
    CC.check_checkpoint(_lib(), DEV)


def test_autograd_route_and_live_parameters_without_a_gradient():
    CC.check_autograd_route_and_missing_gradients(_lib(), DEV)


def test_norm_is_bit_identical_on_two_streams_and_in_two_engines():
    """One buffer: the norm on the default stream, on two other streams, and through two engines' wrappers (each with its own
    scratch and state) -- the same bits every time."""
    from pytorchwavenetvocoder_amd.engine import WaveNetEngine
    lib = _lib()
    engines = [WaveNetEngine(*CC.TINY, device=DEV, library=lib) for _ in range(2)]
    n = engines[0].n_params
    g = CC.buffer(n, 0, DEV, seed=9)
    lo, hi = engines[0].dead_range
    want = CC.state_bits(CC.run_norm(lib, DEV, g, lo, hi, max_norm=0.5))
    torch.cuda.synchronize()
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            got = CC.run_norm(lib, DEV, g, lo, hi, max_norm=0.5)
        s.synchronize()
        assert CC.state_bits(got) == want
    for eng in engines:
        eng.grads().copy_(g)
        state, scratch = eng.new_opt_state(), eng.grad_norm_scratch()
        eng.grad_norm(state, scratch, max_norm=0.5)
        assert CC.state_bits(state) == want
        assert float(eng.opt_state_views(state)["total_norm"]) == CC.read_state(state).total_norm
