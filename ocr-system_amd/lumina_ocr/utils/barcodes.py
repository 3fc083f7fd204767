"""Barcodes, host half (pure Python): the symbol tables of Code 128, Code 39, EAN / UPC and ITF, the symbol values of a device row
(lumina_ocr_barcodes / lumina_ocr_barcodes_kinds: x0, y0, x1, y1, kind, nsym, rows, flags + the symbol values) -> text, and the
entries the provider reports.

The tables are our reading of the public standards (ISO/IEC 15417, 16388, 15420 and 16390).  Code 39 and ITF are built from their
rule; Code 128 and EAN's set L and parity rows are typed and pinned structurally (tests/test_barcode_tables.py,
tests/test_linear_tables.py).  csrc/barcode_tables.h holds Code 128 and Code 39 for the device (device_header() writes it),
csrc/linear_tables.h the EAN / UPC / ITF tables (linear_device_header()); the tests compare."""
from __future__ import annotations

from typing import List, Optional, Sequence

MAX_SYMS = 64
KINDS = ("Code128", "Code39", "EAN13", "EAN8", "UPCE", "ITF")      # by device kind; an EAN13 with first digit 0 is reported as "UPCA"
KIND_CODE128, KIND_CODE39, KIND_EAN13, KIND_EAN8, KIND_UPCE, KIND_ITF = range(6)
FLAG_REVERSED, FLAG_VERTICAL, FLAG_ITF14 = 1, 2, 4

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


# ---- EAN / UPC: a digit is four elements of 1..4 modules, 7 modules in all.  Set L (left half, odd parity) is typed, space first;
# set R (right half) has the same widths bar first; set G (left half, even parity) is L's widths reversed, space first ----
EAN_L = "3211 2221 2122 1411 1132 1231 1114 1312 1213 3112".split()
EAN_R = tuple(EAN_L)
EAN_G = tuple(p[::-1] for p in EAN_L)
EAN_MATCH = tuple(EAN_L) + EAN_G        # what the device matches a left-half digit against: L 0-9 are values 0..9, G 0-9 values 10..19
EAN_MODULES = 7
EAN13_PARITY = "LLLLLL LLGLGG LLGGLG LLGGGL LGLLGG LGGLLG LGGGLL LGLGLG LGLGGL LGGLGL".split()     # by the first digit
UPCE_PARITY_0 = "EEEOOO EEOEOO EEOOEO EEOOOE EOEEOO EOOEEO EOOOEE EOEOEO EOEOOE EOOEOE".split()    # number system 0, by the check digit
UPCE_PARITY = tuple(UPCE_PARITY_0) + tuple(p.translate({69: 79, 79: 69}) for p in UPCE_PARITY_0)   # then number system 1: the complement
# layout by device kind: digits read, digits of the left half, first element of the centre guard (or None), of the end guard, the end
# guard's elements, bars
EAN_LAYOUT = {KIND_EAN13: (12, 6, 27, 56, 3, 30), KIND_EAN8: (8, 4, 19, 40, 3, 22), KIND_UPCE: (6, 6, None, 27, 6, 17)}

# ---- ITF: a quintuple (the five bars of a pair, or its five spaces) is two-of-five with weights 1, 2, 4, 7, 0; the digit 0 is 4 + 7 ----
ITF_WEIGHTS = (1, 2, 4, 7, 0)
ITF_RATIOS = (14, 16, 18)               # half-modules of a quintuple at wide : narrow = 2, 2.5 and 3 (narrow 2, wide 4, 5, 6)
ITF_MIN_DIGITS, ITF_MAX_DIGITS = 6, 64


def _itf_table() -> List[str]:
    """-> for every digit its five elements as 'n' (narrow) and 'w' (wide)"""
    table = [None] * 10
    for a in range(5):
        for b in range(a + 1, 5):
            v = ITF_WEIGHTS[a] + ITF_WEIGHTS[b]
            table[0 if v == 11 else v] = "".join("w" if i in (a, b) else "n" for i in range(5))
    return table


ITF_PATTERNS = tuple(_itf_table())


def itf_widths(digit: int, modules: int) -> List[int]:
    """The five elements of a digit in half-modules at a quintuple of `modules` half-modules (ITF_RATIOS)."""
    return [(modules - 6) // 2 if c == "w" else 2 for c in ITF_PATTERNS[digit]]


def mod10_ok(digits: Sequence[int]) -> bool:
    """The GS1 check of a digit string that ends in its check digit: from the right the weights are 1 (the check), 3, 1, 3 ..."""
    return sum(int(v) * (3 if i % 2 else 1) for i, v in enumerate(reversed(list(digits)))) % 10 == 0


def upce_to_upca(syms: Sequence[int]) -> Optional[List[int]]:
    """The 8 digits of a UPC-E (number system, six digits a b c d e f, check) -> the 12 digits of the UPC-A it abbreviates, by its last
    digit f: 0-2 -> manufacturer a b f 0 0, product 0 0 c d e; 3 -> a b c 0 0, 0 0 0 d e; 4 -> a b c d 0, 0 0 0 0 e; 5-9 -> a b c d e,
    0 0 0 0 f.  The check digit is the UPC-A's."""
    syms = [int(s) for s in syms]
    if len(syms) != 8 or syms[0] not in (0, 1) or any(not 0 <= s <= 9 for s in syms):
        return None
    a, b, c, d, e, f = syms[1:7]
    if f <= 2:
        body = [a, b, f, 0, 0, 0, 0, c, d, e]
    elif f == 3:
        body = [a, b, c, 0, 0, 0, 0, 0, d, e]
    elif f == 4:
        body = [a, b, c, d, 0, 0, 0, 0, 0, e]
    else:
        body = [a, b, c, d, e, 0, 0, 0, 0, f]
    return [syms[0]] + body + [syms[7]]


def linear_device_header() -> str:
    """The text of csrc/linear_tables.h: the 20 left-half digit patterns as four nibbles (element i in bits 4 i), the parity rows as
    six bits (bit k set: digit k is of set G / E), ITF's digits as five bits (bit i set: element i is wide)."""
    ean = [sum(int(c) << (4 * i) for i, c in enumerate(p)) for p in EAN_MATCH]
    p13 = [sum((c == "G") << i for i, c in enumerate(p)) for p in EAN13_PARITY]
    pe = [sum((c == "E") << i for i, c in enumerate(p)) for p in UPCE_PARITY]
    itf = [sum((c == "w") << i for i, c in enumerate(p)) for p in ITF_PATTERNS]
    rows = lambda v, f: ",\n".join("    " + ", ".join(f % x for x in v[i:i + 10]) for i in range(0, len(v), 10))
    return ("#pragma once\n// Written by lumina_ocr.utils.barcodes.linear_device_header(); tests/test_linear_tables.py compares.  EAN / UPC: sets L (values\n"
            "// 0..9) and G (10..19), element i in bits 4 i .. 4 i + 3; set R has L's widths.  Parity rows: bit k set when left digit k is of set G\n"
            "// (EAN-13, by the first digit) or E (UPC-E, number system 0 by the check digit, then number system 1).  ITF: bit i set when element i\n"
            "// of the digit's quintuple is wide.\n"
            "constexpr int BC_NEAN = %d, BC_NUPCE = %d;\n__constant__ const unsigned BC_EAN[BC_NEAN] = {\n%s};\n"
            "__constant__ const unsigned BC_EAN13_PARITY[10] = {\n%s};\n__constant__ const unsigned BC_UPCE_PARITY[BC_NUPCE] = {\n%s};\n"
            "__constant__ const unsigned BC_ITF[10] = {\n%s};\n"
            % (len(ean), len(pe), rows(ean, "0x%04x"), rows(p13, "0x%02x"), rows(pe, "0x%02x"), rows(itf, "0x%02x")))


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


def digits_text(kind: int, syms: Sequence[int]) -> Optional[str]:
    """The digits of an EAN-13 (13), EAN-8 (8), UPC-E (its 8: number system, six digits, check) or ITF (even, 6..64) -> the string, or
    None when they are no message of the kind: a wrong count, no digits, a failing mod-10 check (ITF has none)."""
    syms = [int(s) for s in syms]
    if any(not 0 <= s <= 9 for s in syms):
        return None
    if kind == KIND_ITF:
        ok = ITF_MIN_DIGITS <= len(syms) <= ITF_MAX_DIGITS and len(syms) % 2 == 0
    elif kind == KIND_UPCE:
        full = upce_to_upca(syms)
        ok = full is not None and mod10_ok(full)
    else:
        ok = len(syms) == (13 if kind == KIND_EAN13 else 8) and mod10_ok(syms)
    return "".join(map(str, syms)) if ok else None


def symbols_text(kind: int, syms: Sequence[int]) -> Optional[str]:
    if kind == KIND_CODE128:
        return code128_text(syms)
    if kind == KIND_CODE39:
        return code39_text(syms)
    return digits_text(kind, syms) if kind in (KIND_EAN13, KIND_EAN8, KIND_UPCE, KIND_ITF) else None


def read_barcodes(codes, syms) -> List[dict]:
    """Device rows int32 [m,8] + symbol values [m,64] -> one dict a barcode, in the rows' order: kind, content, confidence (the share
    of the box's rows across the bars that read), polygon (TL, TR, BR, BL as 8 floats), box, reversed, vertical.  A row whose symbols
    are no message of its kind is left out.  An EAN-13 whose first digit is 0 is a UPC-A: kind "UPCA", its 12 digits the content.  An ITF
    of 14 digits whose mod-10 check holds (flags bit 2) has "itf14": True."""
    out = []
    for c, s in zip(codes, syms):
        x0, y0, x1, y1, kind, nsym, rows, flags = (int(v) for v in c)
        text = symbols_text(kind, list(s[:nsym]))
        if text is None:
            continue
        vertical = bool(flags & FLAG_VERTICAL)
        extent = (x1 - x0 + 1) if vertical else (y1 - y0 + 1)
        name = KINDS[kind]
        if kind == KIND_EAN13 and text[0] == "0":
            name, text = "UPCA", text[1:]
        out.append({"kind": name, "content": text, "confidence": min(1.0, rows / float(max(extent, 1))),
                    "polygon": [float(v) for v in (x0, y0, x1 + 1, y0, x1 + 1, y1 + 1, x0, y1 + 1)], "box": (x0, y0, x1, y1),
                    "reversed": bool(flags & FLAG_REVERSED), "vertical": vertical})
        if kind == KIND_ITF and flags & FLAG_ITF14:
            out[-1]["itf14"] = True
    return out


def inside_any(quad, found: Sequence[dict]) -> bool:
    """Does the centre of a quad (8 numbers or 4 points) lie inside the box of one of the barcodes?"""
    flat = [float(v) for p in quad for v in (p if hasattr(p, "__len__") else (p,))]
    cx, cy = sum(flat[0::2]) / 4.0, sum(flat[1::2]) / 4.0
    return any(b["box"][0] <= cx <= b["box"][2] + 1 and b["box"][1] <= cy <= b["box"][3] + 1 for b in found)
