"""CPU: the JBIG2 restatement (tests/jbig2_reference.py) against what pins it.  The arithmetic coder against the standard's own test
sequence (T.88 H.2); the templates structurally (sizes, raster order, no position twice, the SLTP contexts as pictures); the writer
(tests/jbig2_writer.py) -> restatement round trip on every case of tests/jbig2_cases.py, which must give the source bitmap; every
refusal with its status and reason; and the host probe of the library (lumina_ocr_jbig2_probe, no GPU) with the restatement's answers."""
import numpy as np
import pytest

import jbig2_cases as jc
import jbig2_reference as jr
import jbig2_writer as jw

H2_SOURCE = bytes.fromhex("00020051000000C00352872AAAAAAAAA82C02000FCD79EF6BF7FED904F46A3BF")
H2_CODED = bytes.fromhex("84C73BFCE1A143040220000041 0DBB86F4317FFF88FF37471ADB6ADF".replace(" ", ""))


def _bits_msb_first(data):
    return [(b >> (7 - k)) & 1 for b in data for k in range(8)]


def test_h2_known_answer_decoder():
    """the 256 decisions of T.88 H.2 come back from its 28 coded bytes (followed by the marker FF AC), one context at state 0 / MPS 0"""
    mq = jr.MQ88(H2_CODED + b"\xff\xac", 1)
    assert [mq.decode(0) for _ in range(256)] == _bits_msb_first(H2_SOURCE)


def test_h2_known_answer_encoder():
    enc = jw.MQEncoder88(1)
    for b in _bits_msb_first(H2_SOURCE):
        enc.encode(0, b)
    assert enc.finish() == H2_CODED


# ---- structural pins of the templates

def test_template_sizes():
    assert [len(jr.positions(t)) for t in range(4)] == [16, 13, 10, 10]
    assert [len(jr.NOMINAL_AT[t]) for t in range(4)] == [4, 1, 1, 1]


@pytest.mark.parametrize("tmpl", range(4))
def test_template_positions_precede_the_pixel_and_are_distinct(tmpl):
    pos = jr.positions(tmpl)
    assert all(dy < 0 or (dy == 0 and dx < 0) for dx, dy in pos)
    assert len(set(pos)) == len(pos)


# columns x - 4 .. x + 3 of rows y - 2, y - 1, y; X: the pixel being decoded, '.': not in the template
SLTP_PICTURES = {
    0: ("..10011.",
        ".0110010",
        "0101X..."),
    1: ("...0011.",
        "..110010",
        ".101X..."),
    2: ("...001..",
        "..11001.",
        "..01X..."),
    3: ("........",
        ".011001.",
        "0101X..."),
}


@pytest.mark.parametrize("tmpl", range(4))
def test_sltp_context_is_the_picture(tmpl):
    pic = SLTP_PICTURES[tmpl]
    assert pic[2][4] == "X"
    cells = {(c - 4, r - 2): ch for r, line in enumerate(pic) for c, ch in enumerate(line) if ch in "01"}
    pos = jr.positions(tmpl)
    assert set(cells) == set(pos)   # the picture shows the template with its nominal AT pixels, nothing else
    cx = sum(int(cells[p]) << b for b, p in enumerate(pos))
    assert cx == jr.SLTP[tmpl] == (0x9B25, 0x0795, 0x00E5, 0x0195)[tmpl]


def test_template_rows_are_the_table():
    """row y - 2 | row y - 1 | row y of the fixed pixels, as the table in csrc/jbig2_dec.h gives them"""
    want = {0: (range(-1, 2), range(-2, 3), range(-4, 0)), 1: (range(-1, 3), range(-2, 3), range(-3, 0)),
            2: (range(-1, 2), range(-2, 2), range(-2, 0)), 3: (range(0), range(-3, 2), range(-4, 0))}
    for t, rows in want.items():
        fixed = [p for p in jr.TEMPLATES[t] if p[0] != "A"]
        for dy, xs in zip((-2, -1, 0), rows):
            assert sorted(dx for dx, yy in fixed if yy == dy) == list(xs), (t, dy)
    assert jr.NOMINAL_AT == {0: [(3, -1), (-3, -1), (2, -2), (-2, -2)], 1: [(3, -1)], 2: [(2, -1)], 3: [(2, -1)]}


# ---- writer -> restatement

@pytest.mark.parametrize("case", jc.intact(), ids=lambda c: c.name)
def test_round_trip(case):
    st, info, reason = jr.probe(case.stream, case.globals_data)
    assert (st, reason) == (0, "")
    assert (info[1], info[0]) == case.bits.shape
    st, bits = jr.page_bits(case.stream, case.globals_data)
    assert st == 0 and np.array_equal(bits, case.bits)


def test_info_fields():
    by = {c.name: c for c in jc.intact()}
    assert jr.probe(by["operators_default1"].stream)[1] == [70, 37, 8, 7, 1, 3, 1, 0]
    assert jr.probe(by["striped_unknown_height"].stream)[1] == [65, 40, 3, 2, 1, 1, 1, 1]
    assert jr.probe(by["mmr_33x5"].stream)[1] == [33, 5, 1, 0, 1, 0, 0, 0]


def test_to_rgb_and_other_size():
    c = {c.name: c for c in jc.intact()}["size_33x5_t1"]
    st, rgb = jr.decode(c.stream, None, 5, 33)
    assert st == 0 and np.array_equal(rgb[..., 0], np.where(c.bits, 0, 255)) and np.array_equal(rgb[..., 0], rgb[..., 2])
    assert np.array_equal(jr.decode(c.stream, None, 5, 33, invert=True)[1], 255 - rgb)
    assert jr.decode(c.stream, None, 5, 32) == (-4, None)


@pytest.mark.parametrize("case", jc.refused(), ids=lambda c: c.name)
def test_refusals(case):
    st, _, reason = jr.probe(case.stream, case.globals_data)
    assert (st, reason) == (case.status, case.reason)


def test_refusal_list_is_whole():
    """each -2 and -1 cause the parser knows is built at least once"""
    reasons = {c.reason for c in jc.refused()}
    assert set(jr.OUTSIDE.values()) <= reasons
    assert len([c for c in jc.refused() if c.status == -2]) >= 20 and len([c for c in jc.refused() if c.status == -1]) >= 20


def test_a_damaged_mmr_region_refuses_the_page():
    base, _ = jc.sweep_bases()["mmr"]
    states = [st for (name, _, _), (st, _, _) in zip(jc.damage_sweep(), jc.sweep_restatement()) if name == "mmr"]
    assert -1 in states and 0 in states


# ---- the library's host probe (no GPU): lumina_ocr_jbig2_probe gives the restatement's status, info and reason

def _probe(stream, g):
    from lumina_ocr.engine import Engine
    rc, d = Engine.jbig2_probe(stream, g)
    return rc, [d["width"], d["height"], d["regions"], d["arithmetic_regions"], d["mmr_regions"], d["highest_template"], d["tpgdon"], d["striped"]], d["reason"]


def test_library_probe_intact_and_refused():
    for c in jc.intact():
        assert _probe(c.stream, c.globals_data) == jr.probe(c.stream, c.globals_data), c.name
    for c in jc.refused():
        rc, info, reason = _probe(c.stream, c.globals_data)
        assert (rc, reason) == (c.status, c.reason) and info == jr.probe(c.stream, c.globals_data)[1], c.name


def test_library_probe_damage_sweep():
    bad = []
    for (name, label, d), (st, info, bits) in zip(jc.damage_sweep(), jc.sweep_restatement()):
        if not d:
            continue   # (an empty stream has no pointer to give)
        pst, pinfo, _ = jr.probe(d)
        if _probe(d, None)[:2] != (pst, pinfo):
            bad.append((name, label))
    assert not bad, bad[:10]


def test_library_reason_strings():
    from lumina_ocr.engine import load_library
    lib = load_library()
    assert lib.lumina_ocr_jbig2_reason(-4) == b"another size than the batch"
    assert lib.lumina_ocr_jbig2_reason(0) == b"read"
    for code, text in jr.GENERAL_REASON.items():
        if code not in (-1, -2):
            assert lib.lumina_ocr_jbig2_reason(code).decode() == text
