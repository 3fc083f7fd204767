"""Pages for the EAN / UPC / ITF tests (test infrastructure): every regime the issue names on three 420 x 640 pages, the pages of
tests/test_barcode_reference.py with such strips added, and the restatement's answer for a page set and a kind set, computed once."""
import functools

import numpy as np

from lumina_ocr import arch, synth
from lumina_ocr.utils import barcodes as bc

import barcode_reference as br
import linear_reference as lr

H, W = 420, 640
ALL = lr.ALL_KINDS
BIT = {"Code128": 1, "Code39": 2, "EAN13": 4, "UPCA": 4, "EAN8": 8, "UPCE": 16, "ITF": 32}
EAN13_A, EAN13_B, UPCA, EAN8, UPCE, ITF14, ITF6 = "4006381333931", "5901234123457", "0036000291452", "96385074", "01234565", "00012345678905", "123456"


def blank(h: int, w: int) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def name_of(kind: str, digits: str):
    """-> (reported kind, reported content)"""
    return ("UPCA", digits[1:]) if kind == "EAN13" and digits[0] == "0" else (kind, digits)


def put(page, want, x, y, kind, digits, m=2, height=24, ratio=2.0, reversed=False, vertical=False, read=True):
    """Draw a strip and, when it is to be read, note it in want: {box: (kind, content, flags)}."""
    box = synth.render_linear(page, x, y, kind, digits, m, height, ratio, reversed=reversed, vertical=vertical)
    if read:
        flags = int(reversed) | 2 * int(vertical) | (4 if kind == "ITF" and len(digits) == 14 and bc.mod10_ok([int(c) for c in digits]) else 0)
        want[box] = name_of(kind, digits) + (flags,)
    return box


def put128(page, want, x, y, text, kind="Code128", m=2, height=24, **kw):
    syms = synth.code128_symbols(text) if kind == "Code128" else synth.code39_symbols(text)
    box = synth.render_barcode(page, x, y, syms, kind, m, height, **kw)
    want[box] = (kind, text, int(kw.get("reversed", False)) | 2 * int(kw.get("vertical", False)))
    return box


@functools.lru_cache(maxsize=None)
def regime_pages():
    """-> (uint8 [3,420,640,3], [want of page 0, 1, 2]) with every kind on"""
    pages = np.stack([blank(H, W) for _ in range(3)])
    wants = [{}, {}, {}]
    p, w = pages[0], wants[0]             # module widths 2, 3, 4; ITF ratios 2, 2.5, 3; upside down; vertical
    put(p, w, 30, 8, "EAN13", EAN13_A, m=2)
    put(p, w, 260, 8, "EAN8", EAN8, m=2)
    put(p, w, 430, 8, "UPCE", UPCE, m=3)
    put(p, w, 30, 44, "EAN13", EAN13_B, m=3)
    put(p, w, 350, 44, "EAN8", EAN8, m=4, reversed=True)
    put(p, w, 30, 80, "EAN13", UPCA, m=4)
    put(p, w, 440, 80, "UPCE", UPCE, m=2, reversed=True)
    put(p, w, 30, 116, "ITF", ITF6, m=2, ratio=2.0)
    put(p, w, 160, 116, "ITF", ITF6, m=2, ratio=2.5)
    put(p, w, 300, 116, "ITF", ITF6, m=2, ratio=3.0)
    put(p, w, 30, 152, "ITF", ITF14, m=3, ratio=2.5)
    put(p, w, 30, 188, "ITF", ITF14, m=4, ratio=3.0)
    put(p, w, 30, 224, "ITF", ITF14, m=3, ratio=2.0, reversed=True)
    put(p, w, 400, 224, "EAN13", EAN13_A, m=2, reversed=True)
    put(p, w, 30, 266, "EAN8", EAN8, m=2, vertical=True)
    put(p, w, 80, 266, "UPCE", UPCE, m=3, vertical=True, reversed=True)
    put(p, w, 130, 266, "ITF", ITF6, m=2, ratio=2.5, vertical=True)
    put(p, w, 300, 300, "EAN13", EAN13_B, m=2, height=8)                    # min_rows rows exactly
    put(p, w, 300, 330, "EAN13", EAN13_B, m=2, height=7, read=False)        # one fewer
    p, w = pages[1], wants[1]             # neighbours, the page edge, quiet zones, a failing check, candidates from the second chunk
    put(p, w, 0, 8, "EAN13", EAN13_A, m=2)                                  # from x = 0: the edge is quiet
    put128(p, w, 230, 8, "L-128")                                           # a Code 128 in the same rows
    put(p, w, W - 3 * 51, 8, "UPCE", UPCE, m=3)                             # up to the right edge
    put(p, w, 20, 44, "EAN8", EAN8, m=2)                                    # two strips side by side, 10 modules apart
    put(p, w, 20 + 2 * 67 + 20, 44, "EAN8", "55123457", m=2)
    put128(p, w, 380, 44, "C39", "Code39")
    box = put(p, w, 20, 80, "EAN13", EAN13_A, m=2, read=False)              # the trailing quiet zone filled by a bar
    p[80:104, box[2] + 5:box[2] + 12] = 0
    box = put(p, w, 300, 80, "ITF", ITF6, m=2, read=False)                  # the same behind an ITF's stop
    p[80:104, box[2] + 5:box[2] + 12] = 0
    box = put(p, w, 40, 224, "ITF", ITF14, m=2, read=False)                 # and the leading one
    p[224:248, box[0] - 12:box[0] - 4] = 0
    put(p, w, 20, 116, "EAN13", "4006381333932", m=2, read=False)           # one digit altered: the check fails
    put(p, w, 260, 116, "EAN8", "96385075", m=2, read=False)
    put(p, w, 430, 116, "UPCE", "01234575", m=2, read=False)                # (the parity row of another check digit)
    put(p, w, 20, 152, "ITF", "1234", m=2, read=False)                      # four digits: too short
    put(p, w, 120, 152, "ITF", "00012345678906", m=2)                       # 14 digits whose check fails: read, not ITF-14
    for k in range(70):                                                     # 70 uneven bars, then a strip: its start is run 70 of the row
        p[188:212, 4 + 6 * k:4 + 6 * k + 1 + k % 3] = 0
    put(p, w, 4 + 6 * 70 + 20, 188, "EAN8", EAN8, m=2)
    put(p, w, 600, 150, "ITF", ITF14, m=2, ratio=3.0, vertical=True, reversed=True)
    put(p, w, 200, H - 2 * 67, "EAN8", EAN8, m=2, vertical=True)            # down to the bottom edge
    p, w = pages[2], wants[2]             # text above, strips below
    p[:200] = synth.synth_page(200, W, 21, n_lines=6, noise=0.0)[0]
    put(p, w, 40, 240, "EAN13", EAN13_B, m=2, height=40)
    put(p, w, 300, 250, "ITF", ITF14, m=2, ratio=2.5, height=30)
    put128(p, w, 40, 320, "INV-0042", height=30)
    return pages, wants


@functools.lru_cache(maxsize=None)
def reference_pages():
    """The pages tests/test_barcode_reference.py builds, with EAN and ITF strips added to them -> [uint8 [h,w,3]]"""
    put_old = lambda page, x, y, text, kind="Code128", m=2, height=12, **kw: put128(page, {}, x, y, text, kind, m, height, **kw)
    out = []
    page = blank(330, 330)
    put_old(page, 20, 10, "REV-1", reversed=True)
    put_old(page, 10, 40, "VERT", vertical=True)
    put_old(page, 60, 40, "BOTH", "Code39", vertical=True, reversed=True)
    put(page, {}, 110, 60, "EAN13", EAN13_A, height=12)
    put(page, {}, 110, 90, "ITF", ITF14, height=12, reversed=True)
    put(page, {}, 300, 120, "EAN8", EAN8, height=12, vertical=True)
    out.append(page)
    page = blank(24, 640)
    put_old(page, 0, 3, "edge")
    put_old(page, 200, 5, "C39", "Code39")
    put(page, {}, 420, 4, "UPCE", UPCE, height=12)
    put(page, {}, 540, 4, "ITF", ITF6, height=12)
    out.append(page)
    page = synth.synth_barcode_page(1, h=360, w=900, text_lines=3)[0].copy()
    put(page, {}, 20, 300, "EAN13", EAN13_B, height=30)
    put(page, {}, 300, 300, "ITF", ITF14, height=30, ratio=3.0)
    out.append(page)
    page = synth.synth_barcode_decoys()[0].copy()
    put(page, {}, 20, 340, "EAN13", UPCA, height=30)
    put(page, {}, 300, 340, "ITF", ITF6, height=30)
    out.append(page)
    return out


def found(rc, rs):
    """rows + symbol values -> {box: (kind, content, flags)} as the host half reports them"""
    return {b["box"]: (b["kind"], b["content"], int(b["reversed"]) | 2 * int(b["vertical"]) | 4 * int(b.get("itf14", False)))
            for b in bc.read_barcodes(rc, rs)}


def only(want: dict, kinds: int) -> dict:
    return {box: v for box, v in want.items() if BIT[v[0]] & kinds}


_CACHE = {}


def reference(key, page: np.ndarray, kinds: int):
    """The restatement's (mask, codes, syms) of a page, computed once for (key, kinds); the caller leaves them unchanged."""
    if (key, kinds) not in _CACHE:
        _CACHE[key, kinds] = lr.barcodes(page, kinds)
    return _CACHE[key, kinds]


def old_reference(key, page: np.ndarray):
    if (key, "old") not in _CACHE:
        _CACHE[key, "old"] = br.barcodes(page)
    return _CACHE[key, "old"]
