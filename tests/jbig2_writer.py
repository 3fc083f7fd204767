"""Test-side JBIG2 encoder for the generic-region subset (embedded organisation, as PDF's /JBIG2Decode holds it): arithmetic-coded
generic regions of any template, with any legal AT pixels and with or without typical prediction, coded with jp2_writer.MQEncoder over
65 536 contexts; MMR regions through ccitt_cases.g4_encode (libtiff); segment headers in all their field widths; pages striped or not,
with part of their segments split off as globals.  The templates and contexts are read from jbig2_reference, which states them once."""
import struct

import numpy as np

import jbig2_reference as jr
from jp2_writer import MQEncoder

OR, AND, XOR, XNOR, REPLACE = range(5)


class MQEncoder88(MQEncoder):
    """jp2_writer.MQEncoder over `contexts` adaptive contexts, all starting at state 0 / MPS 0"""
    def __init__(self, contexts=1 << 16):
        super().__init__()
        self.I = [0] * contexts
        self.mps = [0] * contexts


def contexts(bm, tmpl, at=None):
    """int32 [h][w]: the context of every pixel of the bitmap, all at once (a pixel outside the bitmap reads 0)"""
    h, w = bm.shape
    cx = np.zeros((h, w), np.int32)
    for b, (dx, dy) in enumerate(jr.positions(tmpl, at)):
        # pixel (y + dy, x + dx) under (y, x), for the (y, x) where it lies inside
        y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        if y0 < y1 and x0 < x1:
            cx[y0:y1, x0:x1] |= bm[y0 + dy:y1 + dy, x0 + dx:x1 + dx].astype(np.int32) << b
    return cx


def encode_generic(bitmap, tmpl=0, at=None, tpgd=False):
    """bool / 0-1 [h][w] -> the arithmetic-coded data of a generic region"""
    bm = np.asarray(bitmap).astype(np.uint8)
    h, w = bm.shape
    enc = MQEncoder88(1 << (16, 13, 10, 10)[tmpl])
    cx = contexts(bm, tmpl, at)
    ltp = 0
    zero = np.zeros(w, np.uint8)
    for y in range(h):
        if tpgd:
            typical = int(np.array_equal(bm[y], bm[y - 1] if y else zero))
            enc.encode(jr.SLTP[tmpl], typical ^ ltp)
            ltp = typical
            if typical:
                continue
        encode = enc.encode
        for c, b in zip(cx[y].tolist(), bm[y].tolist()):
            encode(c, b)
    return enc.finish()


def segment(number, typ, data, page=1, refs=(), long_count=False, page4=False, length=None):
    """one segment: header in the field widths its number and the options ask for, then the data.  length: the value of the length
    field where it shall differ from len(data)"""
    flags = typ | (0x40 if page4 else 0)
    out = struct.pack(">IB", number, flags)
    if long_count or len(refs) > 4:
        out += struct.pack(">I", 0xE0000000 | len(refs)) + bytes((len(refs) + 8) // 8)
    else:
        out += bytes([len(refs) << 5])
    size = 1 if number <= 256 else 2 if number <= 65536 else 4
    for r in refs:
        out += r.to_bytes(size, "big")
    out += page.to_bytes(4 if page4 else 1, "big")
    out += struct.pack(">I", len(data) if length is None else length)
    return out + data


def page_info(width, height, default_pixel=0, default_op=OR, override=True, striped=False, max_stripe=0, flags_extra=0):
    """height None: unknown (0xFFFFFFFF; the page must be striped)"""
    flags = 1 | default_pixel << 2 | default_op << 3 | int(override) << 6 | flags_extra
    return struct.pack(">IIIIBH", width, 0xFFFFFFFF if height is None else height, 0, 0, flags, (0x8000 if striped else 0) | max_stripe)


def region_data(bitmap, x=0, y=0, op=OR, tmpl=0, at=None, tpgd=False, mmr=False, region_flags_extra=0, generic_flags_extra=0, width=None, height=None):
    """the data of an immediate generic region segment: region segment information, generic region flags, AT bytes, coded data"""
    bm = np.asarray(bitmap).astype(np.uint8)
    h, w = bm.shape
    out = struct.pack(">IIIIB", w if width is None else width, h if height is None else height, x, y, op | region_flags_extra)
    out += bytes([int(mmr) | tmpl << 1 | int(tpgd) << 3 | generic_flags_extra])
    if mmr:
        from ccitt_cases import g4_encode
        return out + g4_encode(bm.astype(bool))
    at = jr.NOMINAL_AT[tmpl] if at is None else at
    for ax, ay in at:
        out += struct.pack(">bb", ax, ay)
    return out + encode_generic(bm, tmpl, at, tpgd)


def page(width, height, regions, default_pixel=0, default_op=OR, override=True, first_number=0, lossless=True, end_of_page=True,
         stripes=None, unknown_height=False, **header):
    """regions: [dict(bitmap=..., x=, y=, op=, tmpl=, at=, tpgd=, mmr=)] -> the page's stream.  stripes: row indices (the y of each
    stripe's last row) after which an end-of-stripe segment is written, each behind the regions that end at or above it; with
    unknown_height the page information says 0xFFFFFFFF.  header: options of segment() for every segment."""
    num = first_number
    out = segment(num, 48, page_info(width, None if unknown_height else height, default_pixel, default_op, override, striped=stripes is not None), **header)
    num += 1
    pending = sorted(stripes) if stripes else []
    for r in regions:
        while pending and pending[0] < r.get("y", 0):
            out += segment(num, 50, struct.pack(">I", pending.pop(0)), **header)
            num += 1
        out += segment(num, 39 if lossless else 38, region_data(**r), **header)
        num += 1
    for s in pending:
        out += segment(num, 50, struct.pack(">I", s), **header)
        num += 1
    if end_of_page:
        out += segment(num, 49, b"", **header)
    return out


def split_globals(stream, count):
    """the first `count` segments of a stream made by page() with default headers and small numbers, as (globals, rest)"""
    p = 0
    for _ in range(count):
        number, flags = struct.unpack(">IB", stream[p:p + 5])
        assert number <= 256 and not flags & 0x40 and stream[p + 5] >> 5 == 0
        ln = struct.unpack(">I", stream[p + 7:p + 11])[0]
        p += 11 + ln
    return stream[:p], stream[p:]
