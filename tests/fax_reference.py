"""Integer restatement of the fax decoder behind lumina_ocr_fax_decode for K >= 0 (ITU-T T.4: Group 3 one- and two-dimensional coding,
and the EOL-less byte-aligned coding TIFF calls CCITT RLE), as the fx_decode kernel of csrc/ccitt.hip implements it: the tables and the
two-dimensional mode walk of ccitt_reference, the same order of checks, the same statuses.

    decode(stream, columns, rows, k=0, align=False, black_is_1=False) -> (status, bits)

bits: uint8 [rows][columns] in PDF's convention, as ccitt_reference.decode gives them.  Every line begins with the zero bits in front of
it: 11 or more of them followed by a 1 are an EOL, and a stream carries an EOL in front of every line or of none (the first line
decides).  With k > 0 the bit after an EOL says how the line is coded: 1 one-dimensional, 0 two-dimensional against the line above (the
first line of a stream has a white line above it).  align: without EOLs every line begins on a byte boundary (TIFF Compression 2; PDF's
/K 0 with /EncodedByteAlign true).  A one-dimensional line is white and black runs in turn, white first, that add up to `columns`
exactly; only the first white run of a line may be 0 long.

status 0 ok; -1 corrupt: an unused code, a line whose runs pass `columns`, a run of length 0 other than a line's first, what
ccitt_reference refuses in a two-dimensional line, an EOL in front of some lines and not of others, bits other than 0 between a line's end
and the next EOL, bits read past the stream's end, fewer than `rows` lines, and with align a line after the first that begins in the
stream's last byte (libtiff 4.7.1 pads its bit window with zeros when a code lookup reaches the strip's end, counts the padding when it
then skips to the byte boundary, and so reads that last line from the wrong bit; the host path is libtiff, so the device refuses what
libtiff may misread.  Only lines narrower than 64 pixels fit in one byte); -2 unsupported: k > 0 in a stream without EOLs, align in a
stream with EOLs (nothing can serve as the oracle of either).  Decoding stops after `rows` lines; an RTC, fill or anything else after
them is ignored.
"""
import numpy as np

import ccitt_reference as cr

MAX_COLUMNS = cr.MAX_COLUMNS


def _line_1d(b, W: int):
    """-> the line's changing elements, or None (corrupt)"""
    cur, a0, white, first = [], 0, True, True
    while True:
        r = cr._run(b, white, W - a0)
        if r < 0 or (r == 0 and not first):
            return None
        first = False
        a0 += r
        if a0 >= W:
            return cur
        cur.append(a0)
        white = not white


def _line_2d(b, ref, W: int):
    """ccitt_reference.decode_ex's mode walk over one line. -> the line's changing elements, or None (corrupt)"""
    cur = []
    a0, white, ri = -1, True, 0
    while a0 < W:
        while ref[ri] <= a0:
            ri += 2
        b1, b2 = ref[ri], ref[ri + 1]
        e = int(cr.MODE_TABLE[b.peek(cr.MODE_BITS)])
        if e == 0:
            return None
        b.pos += e >> 12
        if b.pos > b.limit:
            return None
        mode = e & 4095
        if mode == cr.M_PASS:
            if b2 >= W:
                return None
            a0 = b2
            continue
        if mode == cr.M_HORIZ:
            start = max(a0, 0)
            r1 = cr._run(b, white, W - start)
            if r1 < 0:
                return None
            r2 = cr._run(b, not white, W - start - r1)
            if r2 < 0 or start + r1 + r2 <= a0:
                return None
            new = [t for t in (start + r1, start + r1 + r2) if t < W]
            if len(cur) + len(new) > W + 1:
                return None
            cur += new
            a0 = start + r1 + r2
            continue
        a1 = b1 + cr.V_DELTA[mode]
        if a1 <= a0 or a1 > W:
            return None
        if a1 < W:
            if len(cur) + 1 > W + 1:
                return None
            cur.append(a1)
        a0 = a1
        white = not white
        ri = ri - 1 if ri > 0 else ri + 1
    return cur


def _zeros_then_one(b) -> bool:
    """at a line's start: True and the position behind the 1 when 11 or more zero bits and a 1 follow (an EOL), False and the position
    unchanged when fewer zeros do; None when the zeros run to the stream's end"""
    if b.peek(11) != 0:
        return False
    while b.peek(1) == 0:
        b.pos += 1
        if b.pos > b.limit:
            return None
    b.pos += 1
    return None if b.pos > b.limit else True


def decode(stream, columns: int, rows: int, k: int = 0, align: bool = False, black_is_1: bool = False):
    status, out, _ = decode_ex(stream, columns, rows, k, align, black_is_1)
    return status, out


def decode_ex(stream, columns: int, rows: int, k: int = 0, align: bool = False, black_is_1: bool = False):
    """decode, and the number of bits read when the last line ended"""
    assert 0 < columns <= MAX_COLUMNS and rows > 0 and k >= 0
    W = columns
    out = np.zeros((rows, W), np.uint8)
    b = cr._Bits(stream)
    ref = [W, W, W]
    eol_mode = False
    for y in range(rows):
        if align:
            b.pos = (b.pos + 7) & ~7
            if y > 0 and b.limit - b.pos <= 8:   # libtiff misreads a line in the strip's last byte: see the module's text
                return -1, out, b.pos
        eol = _zeros_then_one(b)
        if eol is None:
            return -1, out, b.pos
        if y == 0:
            eol_mode = eol
            if (k > 0 and not eol) or (align and eol):
                return -2, out, b.pos
        elif eol != eol_mode:
            return -1, out, b.pos
        one_d = True
        if eol and k > 0:
            one_d = b.peek(1) == 1
            b.pos += 1
            if b.pos > b.limit:
                return -1, out, b.pos
        cur = _line_1d(b, W) if one_d else _line_2d(b, ref, W)
        if cur is None:
            return -1, out, b.pos
        line = np.zeros(W + 1, np.int64)
        for t in cur:
            line[t] += 1
        out[y] = ((np.cumsum(line[:W]) & 1) == 0) ^ bool(black_is_1)
        ref = cur + [W, W, W]
    return 0, out, b.pos


to_rgb = cr.to_rgb
