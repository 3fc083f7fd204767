"""The barcode symbol tables (lumina_ocr/utils/barcodes.py): Code 128 is typed and pinned structurally and by anchors, Code 39 is built
from its rule and pinned by known characters; the device's copy (csrc/barcode_tables.h) is the same tables."""
import itertools
from pathlib import Path

from lumina_ocr import synth
from lumina_ocr.utils import barcodes as bc


def test_code128_is_exactly_the_set_of_even_bar_sum_patterns():
    universe = {"".join(map(str, p)) for p in itertools.product(range(1, 5), repeat=6) if sum(p) == 11}
    assert len(universe) == 216
    even = {p for p in universe if (int(p[0]) + int(p[2]) + int(p[4])) % 2 == 0}
    assert len(even) == 108
    table = list(bc.CODE128_PATTERNS) + [bc.CODE128_STOP[:6], bc.CODE128_STOP[::-1][:6]]
    assert len(bc.CODE128_PATTERNS) == 106 and bc.CODE128_STOP[::-1][:6] == "211133"
    assert len(set(table)) == len(table) == 108 and set(table) == even


def test_code128_anchors():
    anchors = {0: "212222", 1: "222122", 2: "222221", 103: "211412", 104: "211214", 105: "211232"}
    assert all(bc.CODE128_PATTERNS[v] == p for v, p in anchors.items())
    assert bc.CODE128_STOP == "2331112" and bc.CODE128_MATCH[106] == "233111" and len(bc.CODE128_MATCH) == 107
    assert (bc.C128_START_A, bc.C128_START_B, bc.C128_START_C, bc.C128_STOP) == (103, 104, 105, 106)


def test_code39_construction():
    t = bc.CODE39_PATTERNS
    assert len(t) == 44 == len(bc.CODE39_CHARS) and len(set(t)) == 44
    assert all(len(p) == 9 and p.count("3") == 3 and p.count("1") == 6 for p in t)        # three wide of nine
    known = {"1": "311311113", "A": "311113113", "K": "311111133", "U": "331111113", "0": "111331311", "*": "131131311",
             "$": "131313111", "/": "131311131", "+": "131113131", "%": "111313131", " ": "133111311", "-": "131111313"}
    assert all(t[bc.CODE39_CHARS.index(c)] == p for c, p in known.items())
    for c in "$/+%":                                                                      # narrow bars only, three wide gaps
        p = t[bc.CODE39_CHARS.index(c)]
        assert p[0::2] == "11111" and p[1::2].count("3") == 3
    regular = [p for c, p in zip(bc.CODE39_CHARS, t) if c not in "$/+%"]
    assert all(p[0::2].count("3") == 2 and p[1::2].count("3") == 1 for p in regular)       # two of five bars, one gap
    assert bc.CODE39_CHARS.index("*") == bc.C39_STAR == 43


def test_the_device_header_is_the_tables():
    header = Path(__file__).resolve().parent.parent / "ocr-system_amd" / "csrc" / "barcode_tables.h"
    assert header.read_text() == bc.device_header()


def test_encoder_round_trips_through_the_decoder():
    for text in ("Hello World", "12345678", "AB\x01cd", "ab\x01cd1234ef", "A1234B", "00", "a\x01\x02b", "~}|{", "1", "123", "X12345"):
        syms = synth.code128_symbols(text)
        assert bc.code128_text(syms) == text, (text, syms)
        assert (syms[0] + sum(k * v for k, v in enumerate(syms[1:-2], 1))) % 103 == syms[-2] and syms[-1] == 106
    assert synth.code128_symbols("12345678")[0] == bc.C128_START_C and 98 in synth.code128_symbols("ab\x01cd")
    assert bc.code39_text(synth.code39_symbols("AB-12 $/+%.")) == "AB-12 $/+%."
    assert sum(synth.barcode_modules(synth.code128_symbols("ab"), "Code128")) == 11 * 4 + 13
    assert sum(synth.barcode_modules(synth.code39_symbols("AB"), "Code39")) == 15 * 4 + 3
