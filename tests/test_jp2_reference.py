"""CPU: the plain-Python restatement of the JPEG 2000 decoder (tests/jp2_reference.py) against Pillow, byte for byte, on every intact
case of tests/jp2_cases.py, and its refusals.  The restatement is what the host parser and the device decoder are then held to."""
import numpy as np
import pytest

import jp2_cases as jc
import jp2_reference as jr

INTACT = jc.intact()
REFUSED = jc.refused()


@pytest.mark.parametrize("case", INTACT, ids=[c[0] for c in INTACT])
def test_restatement_equals_pillow(case):
    name, data = case
    status, reason, info, rgb = jc.reference(data)
    assert status == 0, (name, status, reason)
    exp = jc.expected(data)
    assert rgb.shape == exp.shape and info[0] == exp.shape[1] and info[1] == exp.shape[0]
    assert np.array_equal(rgb, exp), (name, int(np.abs(rgb.astype(int) - exp).max()))


def test_cases_cover_the_list():
    """the cases hold what they are named for: layered files carry several layers, the progression orders differ, six levels are reached"""
    info = {name: jc.reference(data)[2] for name, data in INTACT}
    assert {info[f"prog_{p}"][5] for p in ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL")} == {0, 1, 2, 3, 4}
    assert info["layers_rate_RGB"][4] == 3 and info["layers_db_L"][4] == 2 and info["prog_LRCP"][4] == 2
    assert info["res7_RGB"][3] == 6 and info["res1_RGB"][3] == 0
    assert info["cb8x64_RGB"][6:8] == [8, 64] and info["cb64x8_L"][6:8] == [64, 8] and info["cb4x4_L"][6:8] == [4, 4]
    raw = dict(INTACT)["no_jp2_RGB"]
    assert raw[:4] == b"\xff\x4f\xff\x51" and b"\xff\x58" in dict(INTACT)["plt_RGB"]


def test_layered_files_are_lossy():
    """the layered cases stop blocks early (so the truncated-block rule is exercised): their pixels differ from the source's"""
    for name in ("layers_rate_RGB", "layers_db_L", "layers_rate_noise_L"):
        st, _, _, rgb = jc.reference(dict(INTACT)[name])
        assert st == 0
    src = jc.content("page", 100, 130, "RGB", 60)
    assert not np.array_equal(jc.reference(dict(INTACT)["layers_rate_RGB"])[3], src)


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_with_reason(case):
    name, data, word = case
    jc.expected(data)   # Pillow reads it: the file is valid
    status, reason, info = jr.probe(data)
    assert status == -2 and word in reason, (name, status, reason)


def test_reasons_are_distinct():
    reasons = [jr.probe(data)[1] for _, data, _ in REFUSED]
    assert len(set(reasons)) == len(reasons), reasons


def test_box_length_forms():
    """a jp2c box of length 0 (to the end of the file) and one with the 64-bit length form decode as the plain file does"""
    data = dict(INTACT)["s63x65_L"]
    p = data.index(b"jp2c") - 4
    assert int.from_bytes(data[p:p + 4], "big") == len(data) - p
    exp = jc.expected(data)
    zero = data[:p] + b"\x00\x00\x00\x00" + data[p + 4:]
    wide = data[:p] + b"\x00\x00\x00\x01jp2c" + (len(data) - p + 8).to_bytes(8, "big") + data[p + 8:]
    for variant in (zero, wide):
        st, reason, _, rgb = jr.decode(variant)
        assert st == 0, reason
        assert np.array_equal(rgb, exp) and np.array_equal(jc.expected(variant), exp)


def test_strictness():
    data = dict(INTACT)["no_jp2_L"]
    assert jr.probe(data[:-2])[0] == -1            # no EOC
    assert jr.probe(data + b"\x00")[0] == -1       # bytes after EOC
    assert jr.probe(b"")[0] == -1 and jr.probe(b"\xff\x4f\xff\x51")[0] == -1
