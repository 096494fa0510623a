# -*- coding: utf-8 -*-
"""The C-ABI library builds for gfx950, loads without a GPU and exports every symbol that
include/wavenet_hip.h declares; the pure-host entry points answer like the oracle."""
import ctypes
import os
import re

import numpy as np

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import WaveNetEngine, key_to_kind, state_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_exported():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    declared = set(re.findall(r"\b(wn_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = _lib.load_library()
    for name in declared:
        assert getattr(lib.lib, name) is not None
    assert lib.wn_abi_version() == _lib.ABI_VERSION


def test_layout_matches_reference_inventory():
    lib = _lib.load_library()
    for cfg_t in [(256, 80, 64, 256, 10, 3, 2, 80), (256, 28, 512, 256, 10, 3, 2, 0), (64, 5, 8, 12, 3, 2, 3, 10)]:
        cfg = O.OracleConfig(*cfg_t)
        eng = WaveNetEngine(*cfg_t, library=lib)
        shapes = O.param_shapes(cfg)
        assert eng.receptive_field == cfg.receptive_field
        assert eng.n_params == sum(int(np.prod(s)) for s in shapes.values())
        assert state_keys(eng.cfg) == list(shapes.keys())
        spans = []
        for k, shp in shapes.items():
            off, n = eng.param_slice(*key_to_kind(k))
            assert n == int(np.prod(shp)), k
            spans.append((off, off + n))
        spans.sort()
        assert spans[0][0] == 0 and spans[-1][1] == eng.n_params
        for (a0, a1), (b0, b1) in zip(spans[:-1], spans[1:]):
            assert a1 == b0  # exact tiling, no overlap
        # buckets tile the buffer front to back
        for lpb in (1, 4, 10, 0):
            r = eng.bucket_ranges(lpb)
            assert r[0][0] == 0 and r[-1][1] == eng.n_params
            for (a0, a1), (b0, b1) in zip(r[:-1], r[1:]):
                assert a1 == b0
        L = len(cfg.dilations)
        lo, hi = eng.dead_range
        off_w, n_w = eng.param_slice(_lib.P_RES_W, L - 1)
        off_b, n_b = eng.param_slice(_lib.P_RES_B, L - 1)
        assert (lo, hi) == (off_w, off_b + n_b) and off_w + n_w == off_b


def test_cfg2_workspace_is_sane():
    lib = _lib.load_library()
    cfg = _lib.WnConfig(256, 80, 64, 256, 10, 3, 2, 80)
    nbytes = lib.wn_workspace_bytes(ctypes.byref(cfg), 8, 23040)
    assert 4e9 < nbytes < 40e9  # a few GB of the 288 GB HBM3E
    assert lib.wn_workspace_bytes(ctypes.byref(cfg), 8, 23041) == 0  # T must be a multiple of U


def test_emulator_seam_stays_in_its_three_blocks():
    """The host-emulator build switch is named by one #ifdef / #ifndef line in wn_device.h (the two halves), wn_api.hip (the
    side-stream runtime) and wn_prof.hip (two implementations of one interface) and nowhere else in the product sources, and
    the dynamic-LDS limit is raised in one place (wn_dyn_lds of wn_device.h)."""
    csrc = os.path.join(ROOT, "pytorchwavenetvocoder_amd", "csrc")
    seam, attr = {}, set()
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hip", ".h", ".inl")):
            continue
        lines = open(os.path.join(csrc, name)).read().splitlines()
        hits = [ln for ln in lines if re.search(r"WN_EMU(?![A-Za-z0-9_])", ln)]   # (WN_EMU_EXTRA_FLAGS etc. are other names)
        if hits:
            seam[name] = hits
        if any("hipFuncSetAttribute" in ln for ln in lines):
            attr.add(name)
    assert sorted(seam) == ["wn_api.hip", "wn_device.h", "wn_prof.hip"], sorted(seam)
    for name, hits in seam.items():
        assert len(hits) == 1 and re.match(r"\s*#\s*ifn?def\s+WN_EMU\s*$", hits[0]), (name, hits)
    assert attr == {"wn_device.h"}, attr
