"""The host-only entry points of libzly.so (zly_frame_bytes, zly_view_bytes, zly_view_tight, zly_view_crop, zly_letterbox_geometry, zly_tile_grid)
against tests/golden/frame_rules_parent.json: what the library answered before their rules moved into csrc/frame_rules.h.  Every case is replayed
and compared field by field -- return code, zly_last_error text, outputs, and that a refused call left its outputs alone.  No device is touched.
The cases and the file's layout: tests/frame_rules_cases.py."""
import json

import pytest

import frame_rules_cases as frc
import zly


@pytest.fixture(scope="module")
def golden():
    return frc.load()


def test_the_file_holds_the_cases_of_the_generator(golden):
    """the inputs are the generator's, in its order: a case added there without a recording, or dropped from the file, shows here"""
    for fam in frc.FAMILIES:
        assert [i for i, _ in golden[fam]] == frc.INPUTS[fam](), fam


@pytest.mark.parametrize("fam", frc.FAMILIES)
def test_replay(golden, fam):
    lib = zly.load_library()
    names = ("rc", "message") + {"frame": ("frame_bytes", "tight view", "view_bytes of it"), "surface": ("view_bytes",),
                                 "crop": ("w, h, offsets", "view_bytes of the crop", "rest as the surface"),
                                 "crop2": ("w, h, offsets", "view_bytes of the crop", "rest as the surface"),
                                 "letterbox": ("nw", "nh", "pad_x", "pad_y"), "tiles": ("n_out", "tiles", "nothing behind them")}[fam]
    assert len(golden[fam]) > 0
    bad = []
    for inputs, want in golden[fam]:
        got = json.loads(json.dumps(frc.RUN[fam](lib, inputs)))
        assert len(got) == len(want) == len(names)
        bad += [f"{fam}{inputs}: {n} = {g!r}, recorded {w!r}" for n, g, w in zip(names, got, want) if g != w]
    assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:20])
