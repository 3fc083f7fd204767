"""Barcodes, host half (pure Python): the symbol tables of Code 128 and Code 39, the symbol values of a device row
(lumina_ocr_barcodes: x0, y0, x1, y1, kind, nsym, rows, flags + the symbol values) -> text, and the entries the provider reports.

The tables are our reading of the public standards (ISO/IEC 15417 and 16388).  Code 39 is built from its rule; Code 128 is typed
and pinned structurally (tests/test_barcode_tables.py).  csrc/barcode_tables.h holds the same tables for the device (device_header()
writes it; the test compares)."""
from __future__ import annotations

from typing import List, Optional, Sequence

MAX_SYMS = 64
KINDS = ("Code128", "Code39")
FLAG_REVERSED, FLAG_VERTICAL = 1, 2

# ---- Code 128: values 0..105 are six elements (bar, space, bar, space, bar, space) of 1..4 modules, 11 modules in all; the stop
# (106) is seven elements, 13 modules: its first six are matched like any symbol and a two-module bar ends it ----
CODE128_PATTERNS = (
    "212222 222122 222221 121223 121322 131222 122213 122312 132212 221213 "
    "221312 231212 112232 122132 122231 113222 123122 123221 223211 221132 "
    "221231 213212 223112 312131 311222 321122 321221 312212 322112 322211 "
    "212123 212321 232121 111323 131123 131321 112313 132113 132311 211313 "
    "231113 231311 112133 112331 132131 113123 113321 133121 313121 211331 "
    "231131 213113 213311 213131 311123 311321 331121 312113 312311 332111 "
    "314111 221411 431111 111224 111422 121124 121421 141122 141221 112214 "
    "112412 122114 122411 142112 142211 241211 221114 413111 241112 134111 "
    "111242 121142 121241 114212 124112 124211 411212 421112 421211 212141 "
    "214121 412121 111143 111341 131141 114113 114311 411113 411311 113141 "
    "114131 311141 411131 211412 211214 211232").split()
CODE128_STOP = "2331112"
C128_START_A, C128_START_B, C128_START_C, C128_STOP = 103, 104, 105, 106
C128_MODULES = 11
# what the device matches: 107 six-element patterns, the last one the stop's first six
CODE128_MATCH = tuple(CODE128_PATTERNS) + (CODE128_STOP[:6],)
_SHIFT, _CODE_C, _CODE_B, _CODE_A = 98, 99, 100, 101     # (CODE_B is 100 in sets A and C, CODE_A is 101 in sets B and C)

# ---- Code 39: nine elements (five bars, four gaps), three of them wide; wide = 3 modules here, so 15 modules a character ----
CODE39_CHARS = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ-. $/+%*"
C39_STAR = 43
C39_MODULES = 15
C39_WIDE = 3


def _code39_table() -> List[str]:
    """-> for every value 0..43 its nine elements as a string of '1' (narrow) and '3' (wide), built from the rule: the bars are
    two-of-five with weights 1, 2, 4, 7, 0 (the digit 0 is 4 + 7), the position of the one wide gap selects the decade; the four
    characters with narrow bars only have three wide gaps."""
    weights = (1, 2, 4, 7, 0)
    bars = {}
    for a in range(5):
        for b in range(a + 1, 5):
            bars[weights[a] + weights[b]] = [i in (a, b) for i in range(5)]
    decades = (("1234567890", 1), ("ABCDEFGHIJ", 2), ("KLMNOPQRST", 3), ("UVWXYZ-. *", 0))
    table = [None] * len(CODE39_CHARS)
    for chars, wide_gap in decades:
        for col, ch in enumerate(chars):
            b = bars[col + 1 if col < 9 else 11]
            el = []
            for i in range(5):
                el.append(C39_WIDE if b[i] else 1)
                if i < 4:
                    el.append(C39_WIDE if i == wide_gap else 1)
            table[CODE39_CHARS.index(ch)] = "".join(map(str, el))
    for ch, narrow_gap in (("$", 3), ("/", 2), ("+", 1), ("%", 0)):
        el = []
        for i in range(5):
            el.append(1)
            if i < 4:
                el.append(1 if i == narrow_gap else C39_WIDE)
        table[CODE39_CHARS.index(ch)] = "".join(map(str, el))
    return table


CODE39_PATTERNS = tuple(_code39_table())


def device_header() -> str:
    """The text of csrc/barcode_tables.h: Code 128 as six nibbles a pattern (element i in bits 4 i), Code 39 as nine bits (bit i set:
    element i is wide)."""
    c128 = [sum(int(c) << (4 * i) for i, c in enumerate(p)) for p in CODE128_MATCH]
    c39 = [sum((c == "3") << i for i, c in enumerate(p)) for p in CODE39_PATTERNS]
    rows = lambda v, f: ",\n".join("    " + ", ".join(f % x for x in v[i:i + 8]) for i in range(0, len(v), 8))
    return ("#pragma once\n// Written by lumina_ocr.utils.barcodes.device_header(); tests/test_barcode_tables.py compares.  Code 128: values 0..105 and the\n"
            "// first six elements of the stop (106), element i in bits 4 i .. 4 i + 3.  Code 39: values 0..43, bit i set when element i is wide.\n"
            "constexpr int BC_N128 = %d, BC_N39 = %d;\n__constant__ const unsigned BC_C128[BC_N128] = {\n%s};\n__constant__ const unsigned BC_C39[BC_N39] = {\n%s};\n"
            % (len(c128), len(c39), rows(c128, "0x%06x"), rows(c39, "0x%03x")))


# ---- symbols -> text ----
def code128_text(syms: Sequence[int]) -> Optional[str]:
    """start, data ..., check, stop -> the text (FNC1-4 dropped), or None when the sequence is not a Code 128 message."""
    syms = [int(s) for s in syms]
    if len(syms) < 3 or syms[0] not in (C128_START_A, C128_START_B, C128_START_C) or syms[-1] != C128_STOP:
        return None
    cur = "ABC"[syms[0] - C128_START_A]
    out, shift = [], False
    for v in syms[1:-2]:
        if v > 102:
            return None
        use = cur
        if shift:
            use, shift = ("B" if cur == "A" else "A"), False
        if use == "C":
            if v < 100:
                out.append("%02d" % v)
            elif v == 100:
                cur = "B"
            elif v == 101:
                cur = "A"
            continue
        if v < 96:
            out.append(chr(v + 32) if use == "B" or v < 64 else chr(v - 64))
        elif v == _SHIFT:
            shift = True
        elif v == _CODE_C:
            cur = "C"
        elif v == _CODE_B and use == "A":
            cur = "B"
        elif v == _CODE_A and use == "B":
            cur = "A"
        # what is left is FNC1-4: no text
    return "".join(out)


def code39_text(syms: Sequence[int]) -> Optional[str]:
    syms = [int(s) for s in syms]
    if len(syms) < 2 or syms[0] != C39_STAR or syms[-1] != C39_STAR or any(not 0 <= s < C39_STAR for s in syms[1:-1]):
        return None
    return "".join(CODE39_CHARS[s] for s in syms[1:-1])


def symbols_text(kind: int, syms: Sequence[int]) -> Optional[str]:
    return code128_text(syms) if kind == 0 else code39_text(syms)


def read_barcodes(codes, syms) -> List[dict]:
    """Device rows int32 [m,8] + symbol values [m,64] -> one dict a barcode, in the rows' order: kind, content, confidence (the share
    of the box's rows across the bars that read), polygon (TL, TR, BR, BL as 8 floats), box, reversed, vertical.  A row whose symbols
    are no message of its kind is left out."""
    out = []
    for c, s in zip(codes, syms):
        x0, y0, x1, y1, kind, nsym, rows, flags = (int(v) for v in c)
        text = symbols_text(kind, list(s[:nsym]))
        if text is None:
            continue
        vertical = bool(flags & FLAG_VERTICAL)
        extent = (x1 - x0 + 1) if vertical else (y1 - y0 + 1)
        out.append({"kind": KINDS[kind], "content": text, "confidence": min(1.0, rows / float(max(extent, 1))),
                    "polygon": [float(v) for v in (x0, y0, x1 + 1, y0, x1 + 1, y1 + 1, x0, y1 + 1)], "box": (x0, y0, x1, y1),
                    "reversed": bool(flags & FLAG_REVERSED), "vertical": vertical})
    return out


def inside_any(quad, found: Sequence[dict]) -> bool:
    """Does the centre of a quad (8 numbers or 4 points) lie inside the box of one of the barcodes?"""
    flat = [float(v) for p in quad for v in (p if hasattr(p, "__len__") else (p,))]
    cx, cy = sum(flat[0::2]) / 4.0, sum(flat[1::2]) / 4.0
    return any(b["box"][0] <= cx <= b["box"][2] + 1 and b["box"][1] <= cy <= b["box"][3] + 1 for b in found)
