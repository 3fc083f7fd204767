"""The JPEG 2000 subset of csrc/jp2dec.hip restated in plain Python / numpy: boxes, main and tile-part headers, tier 2 (packet headers),
tier 1 (MQ decoder + EBCOT context modelling), the inverse 5/3 DWT and the reversible colour transform.

decode(data) -> (status, reason, info, rgb): status 0 => rgb is uint8 [H, W, 3], the bytes of Image.open(...).convert('RGB');
-2 => a valid file outside the subset; -1 => corrupt / irregular (the decoder is strict).  info = [width, height, components, levels,
layers, progression order, code-block width, code-block height] as lumina_ocr_jp2_probe fills it.  probe(data) is decode without tier 1.
Slow; the suite's cases are small enough for it."""
import numpy as np

MAX_SIDE = 16384
MAX_PIXELS = 1 << 26
MAX_LAYERS = 32
MAX_LEVELS = 6
MAX_MB = 15          # magnitude bit-planes a block may have (8-bit samples through six 5/3 levels need 11 with two guard bits;
#                      tests/test_jp2_unusual.py::test_deep_cases_are_deep holds the files that reach 15, Pillow writes none)
MAX_BLOCKS = 1 << 20


class Refuse(Exception):
    def __init__(self, status, reason):
        Exception.__init__(self, reason)
        self.status, self.reason = status, reason


def _bad(reason):
    raise Refuse(-1, reason)


def _out(reason):
    raise Refuse(-2, reason)


def _be(d, p, n):
    return int.from_bytes(d[p:p + n], "big")


# ---------------------------------------------------------------------------------------------------------------- container
def find_codestream(d):
    """-> (start, end, box_info) of the codestream in d; box_info = None for a raw codestream, else (height, width, nc, enumcs)."""
    n = len(d)
    if n >= 4 and d[:4] == b"\xff\x4f\xff\x51":
        return 0, n, None
    if n < 12 or d[:12] != b"\x00\x00\x00\x0cjP  \r\n\x87\n":
        _bad("not a JPEG 2000 file")
    p = 12
    seen_ftyp = False
    hdr = None
    while True:
        if p + 8 > n:
            _bad("no codestream box")
        ln, typ, hl = _be(d, p, 4), d[p + 4:p + 8], 8
        if ln == 1:
            if p + 16 > n:
                _bad("box header past the end of the file")
            ln, hl = _be(d, p + 8, 8), 16
        elif ln == 0:
            ln = n - p
        if ln < hl or ln > n - p:
            _bad("box length outside the file")
        body, end = p + hl, p + ln
        if typ == b"ftyp":
            if seen_ftyp or p != 12 or end - body < 8 or (end - body) % 4:
                _bad("irregular ftyp box")
            seen_ftyp = True
            brand = d[body:body + 4]
            compat = [d[q:q + 4] for q in range(body + 8, end, 4)]
            if not (brand == b"jp2 " or (brand == b"jpx " and (b"jp2 " in compat or b"jpxb" in compat))):
                _out("ftyp brand is neither jp2 nor baseline jpx")
        elif typ == b"jp2h":
            if not seen_ftyp or hdr is not None:
                _bad("jp2h out of order")
            hdr = _jp2h(d, body, end)
        elif typ == b"jp2c":
            if hdr is None:
                _bad("jp2c before jp2h")
            return body, end, hdr
        elif typ in (b"rreq", b"xml ", b"uuid", b"uinf", b"jp2i"):
            if not seen_ftyp:
                _bad("box before ftyp")
        else:
            if not seen_ftyp:
                _bad("box before ftyp")
            _out("box %r outside the subset" % typ)
        p = end


def _jp2h(d, p, end):
    ihdr = None
    colr = None
    first = True
    while p < end:
        if p + 8 > end:
            _bad("box header past the end of jp2h")
        ln, typ = _be(d, p, 4), d[p + 4:p + 8]
        if ln < 8 or ln > end - p:
            _bad("box length outside jp2h")
        b, e = p + 8, p + ln
        if first != (typ == b"ihdr"):
            _bad("ihdr is not the first box of jp2h")
        first = False
        if typ == b"ihdr":
            if e - b != 14:
                _bad("ihdr of the wrong length")
            hh, ww, nc, bpc, ctype = _be(d, b, 4), _be(d, b + 4, 4), _be(d, b + 8, 2), d[b + 10], d[b + 11]
            if ctype != 7:
                _bad("ihdr compression type is not 7")
            ihdr = (hh, ww, nc, bpc)
        elif typ == b"colr":
            if colr is not None:
                _out("more than one colr box")
            if e - b < 3:
                _bad("colr of the wrong length")
            meth = d[b]
            if meth == 2:
                _out("colr with an ICC profile")
            if meth != 1:
                _bad("colr method")
            if e - b != 7:
                _bad("colr of the wrong length")
            colr = _be(d, b + 3, 4)
            if colr == 18:
                _out("sYCC colour space")
            if colr not in (16, 17):
                _out("enumerated colour space outside sRGB / grey")
        elif typ == b"res ":
            pass
        else:
            _out("box %r outside the subset" % typ)
        p = e
    if ihdr is None or colr is None:
        _bad("jp2h without ihdr or colr")
    hh, ww, nc, bpc = ihdr
    if bpc != 7:
        _out("bit depth other than 8 unsigned")
    if nc not in (1, 3):
        _out("component count other than 1 or 3")
    if (nc == 3) != (colr == 16):
        _out("colour space does not match the component count")
    return hh, ww, nc, colr


# ---------------------------------------------------------------------------------------------------------------- headers
class Params:
    pass


SKIP_MAIN = (0xFF64, 0xFF55)            # COM, TLM
SKIP_TILE = (0xFF64, 0xFF58)            # COM, PLT
OUTSIDE = {0xFF5F: "POC", 0xFF5E: "RGN", 0xFF60: "PPM", 0xFF61: "PPT", 0xFF57: "PLM", 0xFF63: "CRG", 0xFF58: "PLT", 0xFF55: "TLM",
           0xFF52: "COD", 0xFF5C: "QCD", 0xFF53: "COC", 0xFF5D: "QCC"}


def parse_headers(d, s, e, box, info):
    """Main header and tile-part headers of the codestream d[s:e] -> Params with .parts = [(data start, data end)]."""
    P = Params()
    if e - s < 4 or d[s:s + 4] != b"\xff\x4f\xff\x51":
        _bad("no SOC + SIZ")
    p = s + 4
    if p + 2 > e:
        _bad("SIZ cut short")
    L = _be(d, p, 2)
    if L < 41 or p + L > e:
        _bad("SIZ of the wrong length")
    rsiz, X, Y, XO, YO, XT, YT, XTO, YTO, C = (_be(d, p + 2, 2), _be(d, p + 4, 4), _be(d, p + 8, 4), _be(d, p + 12, 4), _be(d, p + 16, 4),
                                               _be(d, p + 20, 4), _be(d, p + 24, 4), _be(d, p + 28, 4), _be(d, p + 32, 4), _be(d, p + 36, 2))
    info[0:3] = [min(X, 0x7FFFFFFF), min(Y, 0x7FFFFFFF), C]
    if C == 0 or L != 38 + 3 * C:
        _bad("SIZ of the wrong length")
    if X == 0 or Y == 0 or XT == 0 or YT == 0:
        _bad("SIZ with an empty image or tile")
    if rsiz != 0:
        _out("capabilities (Rsiz) other than 0")
    if XO or YO or XTO or YTO:
        _out("non-zero image or tile origin")
    if XT < X or YT < Y:
        _out("more than one tile")
    if C not in (1, 3):
        _out("component count other than 1 or 3")
    for c in range(C):
        ssiz, xr, yr = d[p + 38 + 3 * c], d[p + 39 + 3 * c], d[p + 40 + 3 * c]
        if xr == 0 or yr == 0:
            _bad("SIZ with zero sub-sampling")
        if ssiz != 7:
            _out("bit depth other than 8 unsigned")
        if xr != 1 or yr != 1:
            _out("sub-sampled components")
    if X > MAX_SIDE or Y > MAX_SIDE or X * Y > MAX_PIXELS:
        _out("image larger than the decoder takes")
    if box is not None and (box[0] != Y or box[1] != X or box[2] != C):
        _bad("ihdr disagrees with SIZ")
    P.W, P.H, P.C = X, Y, C
    p += L
    cod = qcd = None
    cocs, qccs = [], []
    while True:
        if p + 4 > e:
            _bad("main header cut short")
        m, L = _be(d, p, 2), _be(d, p + 2, 2)
        if m == 0xFF90:
            break
        if m < 0xFF00:
            _bad("not a marker in the main header")
        if L < 2 or p + 2 + L > e:
            _bad("marker segment of the wrong length")
        b, be_ = p + 4, p + 2 + L
        if m == 0xFF52:
            if cod is not None:
                _bad("second COD")
            if L < 12:
                _bad("COD of the wrong length")
            cod = bytes(d[b:be_])
        elif m == 0xFF5C:
            if qcd is not None:
                _bad("second QCD")
            if L < 4:
                _bad("QCD of the wrong length")
            qcd = bytes(d[b:be_])
        elif m == 0xFF53:
            cocs.append(bytes(d[b:be_]))
        elif m == 0xFF5D:
            qccs.append(bytes(d[b:be_]))
        elif m in SKIP_MAIN:
            pass
        elif m in OUTSIDE:
            _out("%s marker" % OUTSIDE[m])
        else:
            _bad("marker %04X in the main header" % m)
        p = be_
    if cod is None or qcd is None:
        _bad("main header without COD or QCD")
    scod, P.order, P.layers, mct = cod[0], cod[1], _be(cod, 2, 2), cod[4]
    P.levels, xcb, ycb, style, xform = cod[5], cod[6], cod[7], cod[8], cod[9]
    if scod & ~7 or P.order > 4 or mct > 1 or P.layers == 0 or xcb > 15 or ycb > 15 or xform > 1 or P.levels > 32 or style & ~63:
        _bad("COD field out of range")
    if len(cod) != (10 + P.levels + 1 if scod & 1 else 10):
        _bad("COD of the wrong length")
    if xcb > 8 or ycb > 8 or xcb + ycb > 8:
        _bad("code-block size out of range")
    P.cbw, P.cbh, P.mct = 4 << xcb, 4 << ycb, mct
    info[3:8] = [P.levels, P.layers, P.order, P.cbw, P.cbh]
    if scod & 1:
        _out("user precinct sizes")
    if scod & 6:
        _out("SOP or EPH markers")
    if xform == 0:
        _out("the 9/7 irreversible transform")
    if style:
        _out("code-block style bits")
    if P.cbw > 64 or P.cbh > 64:
        _out("code-block side over 64")
    if P.layers > MAX_LAYERS:
        _out("more than 32 layers")
    if P.levels > MAX_LEVELS:
        _out("more than 6 decomposition levels")
    if mct and C != 3:
        _bad("component transform on a one-component image")
    nb = 3 * P.levels + 1
    sq = qcd[0]
    if sq & 31 > 2:
        _bad("QCD style out of range")
    if sq & 31:
        _out("quantised (scalar) step sizes with the reversible transform")
    if len(qcd) != 1 + nb:
        _bad("QCD of the wrong length")
    guard = sq >> 5
    P.mb = []
    for i in range(nb):
        if qcd[1 + i] & 7:
            _bad("QCD exponent byte with mantissa bits")
        mb = guard + (qcd[1 + i] >> 3) - 1
        if mb < 0:
            _bad("sub-band without magnitude bits")
        if mb > MAX_MB:
            _out("more magnitude bit-planes than the decoder takes")
        P.mb.append(mb)
    for coc in cocs:
        if len(coc) < 2 or coc[0] >= C:
            _bad("COC of the wrong length or component")
        if (coc[1] & 1) != (scod & 1) or coc[1] & ~1 or coc[2:] != cod[5:]:
            _out("COC that differs from COD")
    for qcc in qccs:
        if len(qcc) < 2 or qcc[0] >= C:
            _bad("QCC of the wrong length or component")
        if qcc[1:] != qcd:
            _out("QCC that differs from QCD")
    # tile-parts
    P.parts = []
    tp = 0
    while True:
        if p + 12 > e:
            _bad("SOT cut short")
        if _be(d, p, 2) != 0xFF90 or _be(d, p + 2, 2) != 10:
            _bad("SOT expected")
        isot, psot, tpsot, tnsot = _be(d, p + 4, 2), _be(d, p + 6, 4), d[p + 10], d[p + 11]
        if isot != 0:
            _bad("tile index past the only tile")
        if tpsot != tp or (tnsot and tpsot >= tnsot):
            _bad("tile-parts out of order")
        if psot == 0:
            pend = e - 2
        else:
            pend = p + psot
        if psot and psot < 14 or pend > e - 2:
            _bad("tile-part length outside the file")
        q = p + 12
        while True:
            if q + 2 > pend:
                _bad("tile-part header cut short")
            m = _be(d, q, 2)
            if m == 0xFF93:
                q += 2
                break
            if q + 4 > pend:
                _bad("tile-part header cut short")
            L = _be(d, q + 2, 2)
            if m < 0xFF00:
                _bad("not a marker in the tile-part header")
            if L < 2 or q + 2 + L > pend:
                _bad("marker segment of the wrong length")
            if m in SKIP_TILE:
                pass
            elif m in OUTSIDE:
                _out("%s marker in a tile-part header" % OUTSIDE[m])
            else:
                _bad("marker %04X in a tile-part header" % m)
            q += 2 + L
        P.parts.append((q, pend))
        p = pend
        tp += 1
        if tp > 255:
            _bad("too many tile-parts")
        if p + 2 <= e and _be(d, p, 2) == 0xFFD9:
            break
    if p + 2 != e:
        _bad("data after EOC")
    return P


# ---------------------------------------------------------------------------------------------------------------- geometry
def _cdiv(a, b):
    return -(-a // b)


class Band:
    pass


class Block:
    pass


def geometry(P):
    """bands[c][r] = list of Band (orient, x0/y0 in the component's Mallat plane, w, h, mb, blocks grid)."""
    comps = []
    nblocks = 0
    for c in range(P.C):
        res = []
        for r in range(P.levels + 1):
            rw, rh = _cdiv(P.W, 1 << (P.levels - r)), _cdiv(P.H, 1 << (P.levels - r))
            bands = []
            if r == 0:
                shapes = [(0, 0, 0, rw, rh, 0)]
            else:
                lw, lh = _cdiv(rw, 2), _cdiv(rh, 2)
                shapes = [(1, lw, 0, rw - lw, lh, 3 * r - 2), (2, 0, lh, lw, rh - lh, 3 * r - 1), (3, lw, lh, rw - lw, rh - lh, 3 * r)]
            for orient, x0, y0, w, h, qi in shapes:
                B = Band()
                B.orient, B.x0, B.y0, B.w, B.h, B.mb = orient, x0, y0, w, h, P.mb[qi]
                B.nx, B.ny = (_cdiv(w, P.cbw), _cdiv(h, P.cbh)) if w and h else (0, 0)
                B.blocks = []
                for by in range(B.ny):
                    for bx in range(B.nx):
                        K = Block()
                        K.c, K.r, K.orient, K.bx, K.by = c, r, orient, bx, by
                        K.x, K.y = x0 + bx * P.cbw, y0 + by * P.cbh
                        K.w, K.h = min(P.cbw, w - bx * P.cbw), min(P.cbh, h - by * P.cbh)
                        K.mb, K.zbp, K.passes, K.segs, K.included, K.lblock = B.mb, 0, 0, [], False, 3
                        B.blocks.append(K)
                nblocks += len(B.blocks)
                if nblocks > MAX_BLOCKS:
                    _out("more code-blocks than the decoder takes")
                B.incl, B.zbpt = TagTree(B.nx, B.ny), TagTree(B.nx, B.ny)
                bands.append(B)
            res.append(bands)
        comps.append(res)
    return comps


# ---------------------------------------------------------------------------------------------------------------- tier 2
class Bits:
    """The packet-header bit reader: after a 0xFF byte the next byte carries 7 bits."""

    def __init__(self, d, p, end):
        self.d, self.p, self.end, self.buf, self.ct = d, p, end, 0, 0

    def _bytein(self):
        if self.p >= self.end:
            _bad("packet header runs past its tile-part")
        self.ct = 7 if self.buf == 0xFF else 8
        self.buf = self.d[self.p]
        self.p += 1

    def bit(self):
        if self.ct == 0:
            self._bytein()
        self.ct -= 1
        return (self.buf >> self.ct) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def align(self):
        self.ct = 0
        if self.buf == 0xFF:
            self._bytein()
            self.ct = 0
        return self.p


class TagTree:
    def __init__(self, nx, ny):
        self.levels = []
        off = 0
        while True:
            self.levels.append((off, nx, ny))
            off += nx * ny
            if nx * ny <= 1:
                break
            nx, ny = (nx + 1) // 2, (ny + 1) // 2
        self.value = [1 << 30] * off
        self.low = [0] * off

    def decode(self, bio, x, y, threshold):
        path = []
        for off, nx, ny in self.levels:
            path.append(off + y * nx + x)
            x, y = x >> 1, y >> 1
        low = 0
        for node in reversed(path):
            if low > self.low[node]:
                self.low[node] = low
            else:
                low = self.low[node]
            while low < threshold and low < self.value[node]:
                if bio.bit():
                    self.value[node] = low
                else:
                    low += 1
            self.low[node] = low
        return self.value[path[0]] < threshold


def _npasses(bio):
    if not bio.bit():
        return 1
    if not bio.bit():
        return 2
    v = bio.bits(2)
    if v != 3:
        return 3 + v
    v = bio.bits(5)
    if v != 31:
        return 6 + v
    return 37 + bio.bits(7)


def packet_order(P):
    L, R, C = range(P.layers), range(P.levels + 1), range(P.C)
    if P.order == 0:
        return [(l, r, c) for l in L for r in R for c in C]
    if P.order == 1:
        return [(l, r, c) for r in R for l in L for c in C]
    if P.order == 2:
        return [(l, r, c) for r in R for c in C for l in L]
    return [(l, r, c) for c in C for r in R for l in L]   # PCRL and CPRL: one precinct per resolution, all at position (0, 0)


def tier2(d, P, comps):
    part = 0
    pos, pend = P.parts[0]
    for layer, r, c in packet_order(P):
        while pos == pend and part + 1 < len(P.parts):
            part += 1
            pos, pend = P.parts[part]
        bio = Bits(d, pos, pend)
        got = []
        if bio.bit():
            for B in comps[c][r]:
                for K in B.blocks:
                    if not K.included:
                        inc = B.incl.decode(bio, K.bx, K.by, layer + 1)
                    else:
                        inc = bio.bit()
                    if not inc:
                        continue
                    if not K.included:
                        i = 1
                        while not B.zbpt.decode(bio, K.bx, K.by, i):
                            i += 1
                            if i > K.mb + 1:
                                _bad("zero bit-plane count above Mb")
                        K.zbp = i - 1
                        K.included = True
                    n = _npasses(bio)
                    while bio.bit():
                        K.lblock += 1
                        if K.lblock > 32:
                            _bad("Lblock out of range")
                    K.passes += n
                    if K.passes > 3 * (K.mb - K.zbp) - 2:
                        _bad("more coding passes than the bit-planes hold")
                    ln = bio.bits(K.lblock + n.bit_length() - 1)
                    got.append((K, ln))
        pos = bio.align()
        for K, ln in got:
            if ln > pend - pos:
                _bad("segment length outside the tile-part")
            if len(K.segs) >= MAX_LAYERS:
                _bad("too many segments")
            K.segs.append((pos, ln))
            pos += ln
    while pos == pend and part + 1 < len(P.parts):
        part += 1
        pos, pend = P.parts[part]
    if pos != pend or part + 1 != len(P.parts):
        _bad("data left over after the last packet")


# ---------------------------------------------------------------------------------------------------------------- tier 1
_QE = [0x5601, 0x3401, 0x1801, 0x0AC1, 0x0521, 0x0221, 0x5601, 0x5401, 0x4801, 0x3801, 0x3001, 0x2401, 0x1C01, 0x1601, 0x5601, 0x5401,
       0x5101, 0x4801, 0x3801, 0x3401, 0x3001, 0x2801, 0x2401, 0x2201, 0x1C01, 0x1801, 0x1601, 0x1401, 0x1201, 0x1101, 0x0AC1, 0x09C1,
       0x08A1, 0x0521, 0x0441, 0x02A1, 0x0221, 0x0141, 0x0111, 0x0085, 0x0049, 0x0025, 0x0015, 0x0009, 0x0005, 0x0001, 0x5601]
_NMPS = [1, 2, 3, 4, 5, 38, 7, 8, 9, 10, 11, 12, 13, 29, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35,
         36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 45, 46]
_NLPS = [1, 6, 9, 12, 29, 33, 6, 14, 14, 14, 17, 18, 20, 21, 14, 14, 15, 16, 17, 18, 19, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,
         32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 46]
_SWITCH = [1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1] + [0] * 32
CTX_RUN, CTX_UNI = 17, 18


class MQ:
    def __init__(self, data):
        self.d = bytes(data) + b"\xff\xff"
        self.p = 0
        self.I = [0] * 19
        self.mps = [0] * 19
        self.I[0], self.I[CTX_RUN], self.I[CTX_UNI] = 4, 3, 46
        self.c = self.d[0] << 16
        self.ct = 0
        self._bytein()
        self.c <<= 7
        self.ct -= 7
        self.a = 0x8000

    def _bytein(self):
        nxt = self.d[self.p + 1]
        if self.d[self.p] == 0xFF:
            if nxt > 0x8F:
                self.c += 0xFF00
                self.ct = 8
            else:
                self.p += 1
                self.c += nxt << 9
                self.ct = 7
        else:
            self.p += 1
            self.c += nxt << 8
            self.ct = 8

    def decode(self, cx):
        i = self.I[cx]
        qe = _QE[i]
        self.a -= qe
        if (self.c >> 16) < qe:
            if self.a < qe:
                bit = self.mps[cx]
                self.I[cx] = _NMPS[i]
            else:
                bit = 1 - self.mps[cx]
                if _SWITCH[i]:
                    self.mps[cx] = bit
                self.I[cx] = _NLPS[i]
            self.a = qe
        else:
            self.c -= qe << 16
            if self.a & 0x8000:
                return self.mps[cx]
            if self.a < qe:
                bit = 1 - self.mps[cx]
                if _SWITCH[i]:
                    self.mps[cx] = bit
                self.I[cx] = _NLPS[i]
            else:
                bit = self.mps[cx]
                self.I[cx] = _NMPS[i]
        while True:
            if self.ct == 0:
                self._bytein()
            self.a <<= 1
            self.c = (self.c << 1) & 0xFFFFFFFF
            self.ct -= 1
            if self.a & 0x8000:
                break
        return bit


def zc_context(orient, h, v, d):
    if orient == 1:
        h, v = v, h
    if orient == 3:
        hv = h + v
        if d >= 3:
            return 8
        if d == 2:
            return 7 if hv >= 1 else 6
        if d == 1:
            return 5 if hv >= 2 else 4 if hv == 1 else 3
        return 2 if hv >= 2 else hv
    if h == 2:
        return 8
    if h == 1:
        return 7 if v >= 1 else 6 if d >= 1 else 5
    if v == 2:
        return 4
    if v == 1:
        return 3
    return 2 if d >= 2 else d


_SC = {(1, 1): (13, 0), (1, 0): (12, 0), (1, -1): (11, 0), (0, 1): (10, 0), (0, 0): (9, 0), (0, -1): (10, 1), (-1, 1): (11, 1),
       (-1, 0): (12, 1), (-1, -1): (13, 1)}


_T1_CACHE = {}


def tier1_block(data, w, h, orient, nbps, npasses):
    """tier1_block_walk behind a memo: the damage sweeps decode thousands of files that differ from their base in one block."""
    key = (bytes(data), w, h, orient, nbps, npasses)
    got = _T1_CACHE.get(key)
    if got is None:
        if len(_T1_CACHE) > 20000:
            _T1_CACHE.clear()
        got = _T1_CACHE[key] = tier1_block_walk(*key)
    return got


def tier1_block_walk(data, w, h, orient, nbps, npasses):
    """-> int32 [h, w] coefficients of one code-block.  A block that stops early keeps one fractional bit: a coefficient that becomes
    significant in plane p is 1.5 * 2^p, each refinement in plane q moves it by 2^(q-1), and the value is halved toward zero at the end."""
    S = w + 2
    sig = [0] * ((h + 2) * S)    # 0 / +1 / -1 (significant, by sign)
    vis = [0] * ((h + 2) * S)
    ref = [0] * ((h + 2) * S)
    mag = [0] * ((h + 2) * S)    # magnitude in half units
    mq = MQ(data)
    dec = mq.decode

    def nbr(i):
        hh = (sig[i - 1] != 0) + (sig[i + 1] != 0)
        vv = (sig[i - S] != 0) + (sig[i + S] != 0)
        dd = (sig[i - S - 1] != 0) + (sig[i - S + 1] != 0) + (sig[i + S - 1] != 0) + (sig[i + S + 1] != 0)
        return hh, vv, dd

    def sign(i):
        hc = max(-1, min(1, sig[i - 1] + sig[i + 1]))
        vc = max(-1, min(1, sig[i - S] + sig[i + S]))
        cx, x = _SC[(hc, vc)]
        return dec(cx) ^ x

    bp = nbps - 1
    kind = 2
    for _ in range(npasses):
        for y0 in range(0, h, 4):
            rows = min(4, h - y0)
            for x in range(w):
                base = (y0 + 1) * S + x + 1
                if kind == 0:
                    for k in range(rows):
                        i = base + k * S
                        if sig[i] == 0:
                            hh, vv, dd = nbr(i)
                            if hh or vv or dd:
                                if dec(zc_context(orient, hh, vv, dd)):
                                    sig[i] = -1 if sign(i) else 1
                                    mag[i] = 3 << bp
                                vis[i] = 1
                elif kind == 1:
                    for k in range(rows):
                        i = base + k * S
                        if sig[i] != 0 and not vis[i]:
                            if ref[i]:
                                cx = 16
                            else:
                                hh, vv, dd = nbr(i)
                                cx = 15 if hh or vv or dd else 14
                            mag[i] += (1 << bp) if dec(cx) else -(1 << bp)
                            ref[i] = 1
                else:
                    k = 0
                    if rows == 4 and all(sig[base + j * S] == 0 and not vis[base + j * S] and nbr(base + j * S) == (0, 0, 0) for j in range(4)):
                        if not dec(CTX_RUN):
                            continue
                        k = (dec(CTX_UNI) << 1) | dec(CTX_UNI)
                        i = base + k * S
                        sig[i] = -1 if sign(i) else 1
                        mag[i] = 3 << bp
                        k += 1
                    for k in range(k, rows):
                        i = base + k * S
                        if sig[i] == 0 and not vis[i]:
                            if dec(zc_context(orient, *nbr(i))):
                                sig[i] = -1 if sign(i) else 1
                                mag[i] = 3 << bp
        if kind == 2:
            vis = [0] * len(vis)
            bp -= 1
        kind = (kind + 1) % 3
    out = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            i = (y + 1) * S + x + 1
            out[y, x] = (mag[i] >> 1) * (-1 if sig[i] < 0 else 1)
    return out


# ---------------------------------------------------------------------------------------------------------------- DWT, colour
def _idwt_1d(a):
    """Inverse 5/3 along axis 1 of a [m, n] array whose first ceil(n/2) columns are low-pass (origin 0)."""
    n = a.shape[1]
    if n == 1:
        return a.copy()   # a single low-pass sample is copied (a single high-pass sample, which needs an odd origin, would be halved)
    sn = (n + 1) // 2
    s, d = a[:, :sn].astype(np.int64), a[:, sn:].astype(np.int64)
    dn = n - sn
    dl = np.concatenate([d[:, :1], d], axis=1)[:, :sn]                     # d[k-1], d[-1] = d[0]
    dr = np.concatenate([d, d[:, -1:]], axis=1)[:, :sn]                    # d[k], d[dn] = d[dn-1]
    ev = s - ((dl + dr + 2) >> 2)
    en = np.concatenate([ev[:, 1:], ev[:, -1:]], axis=1)[:, :dn]           # x[2k+2], mirrored at the end
    od = d + ((ev[:, :dn] + en) >> 1)
    out = np.empty_like(a)
    out[:, 0::2] = ev
    out[:, 1::2] = od
    return out


def inverse_dwt(plane, W, H, levels):
    for r in range(1, levels + 1):
        rw, rh = _cdiv(W, 1 << (levels - r)), _cdiv(H, 1 << (levels - r))
        t = _idwt_1d(plane[:rh, :rw])
        plane[:rh, :rw] = _idwt_1d(np.ascontiguousarray(t.T)).T
    return plane


def decode(data, tier1=True):
    d = bytes(data)
    info = [0] * 8
    try:
        s, e, box = find_codestream(d)
        P = parse_headers(d, s, e, box, info)
        comps = geometry(P)
        tier2(d, P, comps)
        if not tier1:
            return 0, "", info, None
        planes = np.zeros((P.C, P.H, P.W), np.int32)
        for c in range(P.C):
            for bands in comps[c]:
                for B in bands:
                    for K in B.blocks:
                        if K.passes:
                            blob = b"".join(d[o:o + n] for o, n in K.segs)
                            planes[c, K.y:K.y + K.h, K.x:K.x + K.w] = tier1_block(blob, K.w, K.h, K.orient, K.mb - K.zbp, K.passes)
            inverse_dwt(planes[c], P.W, P.H, P.levels)
        if P.mct:
            y, u, v = planes[0], planes[1], planes[2]
            g = y - ((u + v) >> 2)
            planes = np.stack([v + g, g, u + g])
        rgb = np.clip(planes + 128, 0, 255).astype(np.uint8)
        if P.C == 1:
            rgb = np.repeat(rgb, 3, axis=0)
        return 0, "", info, np.ascontiguousarray(rgb.transpose(1, 2, 0))
    except Refuse as r:
        return r.status, r.reason, info, None


def probe(data):
    st, reason, info, _ = decode(data, tier1=False)
    return st, reason, info
