"""What the device entries and the read-backs of libzly.so answer when they refuse a call, against tests/golden/call_refusals_parent.json: what the
library answered before the entries' shared scaffolding in csrc/engine.cpp was joined.  Every case is replayed on an engine of its set-up and
compared field by field -- return code, zly_last_error text, the deltas of the engine's counters; then the engine makes one good call, whose results
must be, byte for byte, those of a twin engine that saw no refusal: a refused call enqueued nothing and left nothing half-set.  One more test pins
how far a successful call of each device entry moves the counters.  The cases and the file's layout: tests/call_refusal_cases.py."""
import pytest
import torch            # before the first engine: the process then uses torch's HIP runtime throughout, as tests/test_gpu_parity.py does

import call_refusal_cases as crc


@pytest.fixture(scope="module")
def golden():
    return crc.load()


def test_the_file_holds_the_cases_of_the_generator(golden):
    """the cases are the generator's, in its order: a case added there without a recording, or dropped from the file, shows here"""
    assert list(golden["refusals"]) == list(crc.SETUPS)
    for setup in crc.SETUPS:
        assert [(r[0], r[1]) for r in golden["refusals"][setup]] == crc.cases(setup), setup
        assert all(r[2] != 0 and r[3] for r in golden["refusals"][setup]), "every recorded case is a refusal with a text"
    assert [r[0] for r in golden["success"]] == list(crc.SUCCESS)
    # every entry meets an engine without its feature, and the store's readers one without the store only, one without the feature only, one without both
    for entry, needs in crc.NEEDS.items():
        lacking = [s for s in crc.SETUPS if (entry, "good") in crc.cases(s)]
        assert lacking or not needs, entry
        if "store" in needs and len(needs) > 1:
            assert {"bare", "store", "features"} <= set(lacking), entry


@pytest.mark.gpu
@pytest.mark.parametrize("setup", list(crc.SETUPS))
def test_replay(weights_path, golden, setup):
    ctx, twin = crc.Ctx(weights_path, setup), crc.Ctx(weights_path, setup)
    try:
        got, want = crc.run_refusals(ctx), golden["refusals"][setup]
        assert len(got) == len(want) > 0
        names = ("entry", "variant", "rc", "message", "deltas of " + ", ".join(crc.STAT_FIELDS))
        bad = [f"{g[0]} / {g[1]}: {n} = {a!r}, recorded {b!r}" for g, w in zip(got, want) for n, a, b in zip(names, g, w) if a != b]
        assert not bad, f"{len(bad)} fields differ:\n" + "\n".join(bad[:20])
        assert crc.good_call(ctx) == crc.good_call(twin), "the call after the refusals differs from a twin engine's first call"
    finally:
        ctx.close()
        twin.close()


@pytest.mark.gpu
def test_counters_of_a_successful_call(weights_path, golden):
    ctx = crc.Ctx(weights_path, "full")
    try:
        got = crc.run_success(ctx)
    finally:
        ctx.close()
    assert got == golden["success"], (crc.STAT_FIELDS, got, golden["success"])
    # a plain, view, surfaces, tiled or delta call counts its n frames; a zoom call its n x (1 + K) views
    assert {r[0]: r[1][0] for r in got} == {"plain": crc.N, "view": crc.N, "surfaces": crc.N, "zoom": 2 * crc.N, "tiled": 2, "delta": crc.N}
    assert all(r[1][1] == 0 for r in got)
