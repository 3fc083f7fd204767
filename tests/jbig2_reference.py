"""Plain-Python restatement of the JBIG2 generic-region subset: the host parser (csrc/jbig2_parse.h, every check in the same order, with
the statuses and the reason strings) and the decoder (csrc/jbig2_dec.h, csrc/jbig2.hip): arithmetic-coded generic regions with the four
templates, adaptive pixels and typical prediction; MMR regions through the fax restatement (ccitt_reference); the combination of the
regions onto the page.  Written from the same recollection of T.88 as the code under test: what pins the two to the standard is the
arithmetic coder's known answer (T.88 H.2, tests/test_jbig2_reference.py), libtiff behind the MMR path, and the structural pins of the
templates there; the segment syntax rests on recollection alone."""
import numpy as np

import ccitt_reference as cr
from jp2_reference import MQ

MAX_COLS = 8192
MAX_REGIONS = 256

KNOWN_TYPES = (0, 4, 6, 7, 16, 20, 22, 23, 36, 38, 39, 40, 42, 43, 48, 49, 50, 51, 52, 53, 62)
OUTSIDE = {0: "symbol dictionary", 4: "text region", 6: "text region", 7: "text region", 16: "pattern dictionary",
           20: "halftone region", 22: "halftone region", 23: "halftone region", 36: "intermediate generic region",
           40: "generic refinement region", 42: "generic refinement region", 43: "generic refinement region", 53: "code tables"}
GENERAL_REASON = {0: "read", -1: "corrupt or irregular JBIG2 stream", -2: "valid JBIG2 outside the device subset", -4: "another size than the batch"}

# the templates as the issue's table gives them: per template the fixed pixels (dx, dy) in context bit order, with the AT slots as
# ("A", k).  Bit order: current row from x - 1 leftwards; A1; row y - 1 right to left; T0: A2, A3; row y - 2 right to left; T0: A4.
def _row(dy, right, left):
    return [(dx, dy) for dx in range(right, left - 1, -1)]


TEMPLATES = {
    0: _row(0, -1, -4) + [("A", 0)] + _row(-1, 2, -2) + [("A", 1), ("A", 2)] + _row(-2, 1, -1) + [("A", 3)],
    1: _row(0, -1, -3) + [("A", 0)] + _row(-1, 2, -2) + _row(-2, 2, -1),
    2: _row(0, -1, -2) + [("A", 0)] + _row(-1, 1, -2) + _row(-2, 1, -1),
    3: _row(0, -1, -4) + [("A", 0)] + _row(-1, 1, -3),
}
NOMINAL_AT = {0: [(3, -1), (-3, -1), (2, -2), (-2, -2)], 1: [(3, -1)], 2: [(2, -1)], 3: [(2, -1)]}
SLTP = {0: 0x9B25, 1: 0x0795, 2: 0x00E5, 3: 0x0195}


def positions(tmpl, at=None):
    """the template's pixels (dx, dy) in context bit order, AT pixels at `at` (default: nominal)"""
    at = NOMINAL_AT[tmpl] if at is None else at
    return [at[p[1]] if p[0] == "A" else p for p in TEMPLATES[tmpl]]


class MQ88(MQ):
    """jp2_reference.MQ (T.800 Annex C = T.88 Annex E) over `contexts` adaptive contexts, all starting at state 0 / MPS 0"""
    def __init__(self, data, contexts=1 << 16):
        super().__init__(data)
        self.I = [0] * contexts
        self.mps = [0] * contexts


class Refused(Exception):
    def __init__(self, status, reason):
        super().__init__(reason)
        self.status, self.reason = status, reason


def _be(d, p, n):
    return int.from_bytes(d[p:p + n], "big")


class Page:
    def __init__(self):
        self.info = [0] * 8
        self.width = self.height = self.default_pixel = self.default_op = self.override_ok = self.striped = 0
        self.regions = []
        self.reason = ""


def _segments(d, from_globals, pg, s):
    n, p = len(d), 0
    bad, out = (lambda m: Refused(-1, m)), (lambda m: Refused(-2, m))
    while p < n and not s["stop"]:
        if n - p < 6:
            raise bad("segment header past the stream")
        number, flags = _be(d, p, 4), d[p + 4]
        typ = flags & 63
        q = p + 5
        count = d[q] >> 5
        if count in (5, 6):
            raise bad("reserved referred-to segment count")
        if count == 7:
            if n - q < 4:
                raise bad("segment header past the stream")
            count = _be(d, q, 4) & 0x1FFFFFFF
            q += 4
            retain = (count + 8) // 8
            if n - q < retain:
                raise bad("segment header past the stream")
            q += retain
        else:
            q += 1
        ref_bytes = count * (1 if number <= 256 else 2 if number <= 65536 else 4)
        if n - q < ref_bytes:
            raise bad("segment header past the stream")
        q += ref_bytes
        pa = 4 if flags & 0x40 else 1
        if n - q < pa + 4:
            raise bad("segment header past the stream")
        assoc = _be(d, q, pa)
        q += pa
        ln = _be(d, q, 4)
        q += 4
        if typ not in KNOWN_TYPES:
            raise bad("a segment type that T.88 does not define")
        if assoc > 1:
            raise out("a segment of another page than page 1")
        if typ in OUTSIDE:
            raise out(OUTSIDE[typ])
        if ln == 0xFFFFFFFF:
            raise out("a segment of unknown length")
        if n - q < ln:
            raise bad("segment data past the stream")
        body, nxt = q, q + ln
        if typ == 48:
            if s["have_page"]:
                raise out("a second page information segment")
            if ln != 19:
                raise bad("page information of the wrong length")
            w, h = _be(d, body, 4), _be(d, body + 4, 4)
            pf, striping = d[body + 16], _be(d, body + 17, 2)
            if pf & 0x80:
                raise bad("reserved page flag bits")
            if w == 0 or h == 0:
                raise bad("an empty page")
            if w > MAX_COLS:
                raise out("page wider than 8192")
            if h != 0xFFFFFFFF and h > 0x7FFFFFFF:
                raise out("page higher than 2^31 - 1")
            s["have_page"] = True
            s["height_known"] = h != 0xFFFFFFFF
            pg.width, pg.height = w, (h if s["height_known"] else 0)
            pg.default_pixel, pg.default_op, pg.override_ok = (pf >> 2) & 1, (pf >> 3) & 3, (pf >> 6) & 1
            pg.striped = (striping >> 15) & 1
            pg.info[0], pg.info[1], pg.info[7] = pg.width, pg.height, pg.striped
        elif typ in (38, 39):
            if not s["have_page"]:
                raise bad("a region before the page information")
            if ln < 18:
                raise bad("generic region shorter than its header")
            r = dict(w=_be(d, body, 4), h=_be(d, body + 4, 4), x=_be(d, body + 8, 4), y=_be(d, body + 12, 4))
            rf, gf = d[body + 16], d[body + 17]
            if (rf & 0xF8) or (rf & 7) > 4:
                raise bad("reserved region flag bits")
            if gf & 0xE0:
                raise bad("reserved generic region flag bits")
            if gf & 0x10:
                raise out("extended template (EXTTEMPLATE)")
            r["op"] = rf & 7
            if not pg.override_ok and r["op"] != pg.default_op:
                raise bad("a region operator other than the page's, which forbids overriding")
            r["mmr"], r["tmpl"], r["tpgd"] = gf & 1, (gf >> 1) & 3, (gf >> 3) & 1
            at_bytes = 0
            r["at"] = list(NOMINAL_AT[r["tmpl"]])
            if not r["mmr"]:
                at_bytes = 8 if r["tmpl"] == 0 else 2
                if ln < 18 + at_bytes:
                    raise bad("generic region shorter than its header")
                at = []
                for i in range(0, at_bytes, 2):
                    ax, ay = d[body + 18 + i], d[body + 19 + i]
                    ax, ay = ax - 256 * (ax > 127), ay - 256 * (ay > 127)
                    if ay > 0 or (ay == 0 and ax >= 0):
                        raise bad("an adaptive template pixel that is not before the current pixel")
                    at.append((ax, ay))
                r["at"] = at
            if r["w"] == 0 or r["h"] == 0:
                raise bad("an empty region")
            if r["w"] > MAX_COLS:
                raise out("region wider than 8192")
            if len(pg.regions) >= MAX_REGIONS:
                raise out("more than 256 regions on the page")
            r["data"] = bytes(d[body + 18 + at_bytes:nxt])
            pg.regions.append(r)
            pg.info[2] += 1
            pg.info[3] += 1 - r["mmr"]
            pg.info[4] += r["mmr"]
            if not r["mmr"]:
                pg.info[5] = max(pg.info[5], r["tmpl"])
                if r["tpgd"]:
                    pg.info[6] = 1
        elif typ == 50:
            if ln != 4:
                raise bad("end of stripe of the wrong length")
            s["have_stripe"] = True
            s["last_stripe"] = _be(d, body, 4)
        elif typ in (49, 51):
            s["stop"] = True
        p = nxt


def parse(stream, globals_data=None):
    """-> (status, reason, Page): the page as far as it was read"""
    pg = Page()
    stream = bytes(stream)
    g = bytes(globals_data) if globals_data else b""
    try:
        if len(stream) >= 1 << 28 or len(g) >= 1 << 28:
            raise Refused(-2, "a stream of 2^28 bytes or more")
        s = dict(have_page=False, height_known=False, have_stripe=False, stop=False, last_stripe=0)
        if g:
            _segments(g, 1, pg, s)
        if not s["stop"]:
            _segments(stream, 0, pg, s)
        if not s["have_page"]:
            raise Refused(-1, "no page information")
        if not s["height_known"]:
            if not s["have_stripe"]:
                raise Refused(-1, "unknown page height without an end of stripe")
            if s["last_stripe"] + 1 > 0x7FFFFFFF:
                raise Refused(-2, "page higher than 2^31 - 1")
            pg.height = s["last_stripe"] + 1
            pg.info[1] = pg.height
        for r in pg.regions:
            if r["x"] >= pg.width or r["y"] >= pg.height:
                raise Refused(-1, "a region that does not meet the page")
    except Refused as e:
        pg.reason = e.reason
        return e.status, e.reason, pg
    return 0, "", pg


def probe(stream, globals_data=None):
    """what Engine.jbig2_probe answers: (status, info list, reason)"""
    st, reason, pg = parse(stream, globals_data)
    return st, list(pg.info), reason


def decode_generic(data, w, rows, tmpl, at, tpgd, decisions=None):
    """an arithmetic-coded generic region -> uint8 [rows][w]; never fails (past its data the decoder reads 0xFF)"""
    mq = MQ88(data, 1 << (16, 13, 10, 10)[tmpl])
    pos = positions(tmpl, at)
    out = np.zeros((rows, w), np.uint8)
    ltp = 0
    for y in range(rows):
        if tpgd:
            ltp ^= mq.decode(SLTP[tmpl])
            if ltp:
                if y:
                    out[y] = out[y - 1]
                continue
        row = out[y]
        for x in range(w):
            cx = 0
            for b, (dx, dy) in enumerate(pos):
                xx, yy = x + dx, y + dy
                if 0 <= xx < w and yy >= 0 and out[yy, xx]:
                    cx |= 1 << b
            row[x] = mq.decode(cx)
    return out


def decode_region(r, page_height):
    """(status, bits uint8 [rows][w]) of one parsed region, its rows clipped to the page's bottom"""
    rows = min(r["h"], page_height - r["y"])
    if r["mmr"]:
        return cr.decode(r["data"], r["w"], rows, black_is_1=True)
    return 0, decode_generic(r["data"], r["w"], rows, r["tmpl"], r["at"], r["tpgd"])


def combine(page, bits, r, plane):
    """the region's plane onto the page's bits with its operator, clipped to the page"""
    H, W = bits.shape
    h, w = min(plane.shape[0], H - r["y"]), min(plane.shape[1], W - r["x"])
    dst = bits[r["y"]:r["y"] + h, r["x"]:r["x"] + w]
    src = plane[:h, :w]
    op = r["op"]
    dst[...] = (dst | src, dst & src, dst ^ src, 1 - (dst ^ src), src)[op]


def page_bits(stream, globals_data=None):
    """-> (status, bits uint8 [H][W] with 1 = black, or None)"""
    st, _, pg = parse(stream, globals_data)
    if st:
        return st, None
    bits = np.full((pg.height, pg.width), pg.default_pixel, np.uint8)
    status = 0
    for r in pg.regions:
        rs, plane = decode_region(r, pg.height)
        if rs:
            status = -1
            continue
        combine(pg, bits, r, plane)
    return (status, None) if status else (0, bits)


def to_rgb(bits, invert=False):
    """/JBIG2Decode's samples as DeviceGray shows them: bit 1 -> 0 (black), bit 0 -> 255; invert (/Decode [1 0]) swaps them"""
    g = np.where(bits.astype(bool) ^ bool(invert), 0, 255).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


def decode(stream, globals_data=None, height=None, width=None, invert=False):
    """what lumina_ocr_jbig2_decode answers for one page of a height x width batch: (status, RGB uint8 [H][W][3] or None)"""
    st, _, pg = parse(stream, globals_data)
    if st:
        return st, None
    if height is not None and (pg.height, pg.width) != (height, width):
        return -4, None
    st, bits = page_bits(stream, globals_data)
    return (st, None) if st else (0, to_rgb(bits, invert))
