# -*- coding: utf-8 -*-
"""CPU-only: csrc/build.py keeps the ONE list of what the library is made of (the emulator build and the instrumented builds
under tools/ import it).  A source or header that is in the directory but not in the list would silently stay out of the
library, or out of the digest that decides whether it is rebuilt."""
import os

from pytorchwavenetvocoder_amd.csrc import build as hip_build
from tests.emu import build_emu


def _in_csrc(*suffixes):
    return sorted(f for f in os.listdir(hip_build.HERE) if f.endswith(suffixes))


def test_every_hip_source_is_listed():
    assert sorted(hip_build.SOURCES) == _in_csrc(".hip")
    assert len(set(hip_build.SOURCES)) == len(hip_build.SOURCES)


def test_every_header_is_listed():
    listed = [h for h in hip_build.HEADERS if not h.startswith("../")]
    assert sorted(listed) == _in_csrc(".h", ".inl")
    assert len(set(hip_build.HEADERS)) == len(hip_build.HEADERS)
    for h in hip_build.HEADERS:   # the public headers outside the directory exist too
        assert os.path.isfile(os.path.join(hip_build.HERE, h)), h


def test_the_emulator_builds_the_same_translation_units():
    assert build_emu.SOURCES is hip_build.SOURCES
    assert set(build_emu.SOURCE_FLAGS) <= set(hip_build.SOURCES)
