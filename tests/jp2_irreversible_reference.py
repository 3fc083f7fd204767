"""The 9/7 irreversible side of the JPEG 2000 decoder (csrc/jp2_parse.h with the irreversible option, csrc/jp2_t1.h, csrc/jp2dec.hip)
restated in numpy float32 on top of tests/jp2_reference.py: the header checks with 9/7 and its expounded step sizes let in, tier 1 read
in half units, the float dequantisation, the 9/7 inverse lifting, the irreversible colour transform and the rounding.

decode(data) / probe(data): as jp2_reference's, for files of either transform; a 5/3 file takes jp2_reference's integer path.  Every
float operation is single precision, in the order OpenJPEG evaluates it, with no fused multiply-add; subnormals are kept."""
import numpy as np

import jp2_reference as jr
from jp2_reference import MAX_LAYERS, MAX_LEVELS, MAX_MB, MAX_SIDE, MAX_PIXELS, OUTSIDE, SKIP_MAIN, SKIP_TILE, Params, _bad, _be, _cdiv, _out

F = np.float32
K_LOW, K_HIGH = F(1.230174105), F(1.625732422)                             # the scaling of the low-pass and high-pass samples
LIFT = (F(0.443506852), F(0.882911075), F(-0.052980118), F(-1.586134342))   # even, odd, even, odd: x -= (left + right) * c


def parse_headers(d, s, e, box, info):
    """jp2_reference.parse_headers with the irreversible option: the same checks in the same order, and transform 0 is taken with an
    expounded QCD.  Params gains .irreversible and .step (float32 per sub-band, QCD order; empty for 5/3)."""
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
    P.irreversible = xform == 0
    info[3:8] = [P.levels, P.layers, P.order, P.cbw, P.cbh]
    if scod & 1:
        _out("user precinct sizes")
    if scod & 6:
        _out("SOP or EPH markers")
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
    if P.irreversible:
        for r in range(1, P.levels + 1):
            if _cdiv(X, 1 << (P.levels - r)) == 1 or _cdiv(Y, 1 << (P.levels - r)) == 1:
                _out("the 9/7 transform over a line of one sample")
    nb = 3 * P.levels + 1
    sq = qcd[0]
    if sq & 31 > 2:
        _bad("QCD style out of range")
    guard = sq >> 5
    P.mb, P.step = [], []
    if not P.irreversible:
        if sq & 31:
            _out("quantised (scalar) step sizes with the reversible transform")
        if len(qcd) != 1 + nb:
            _bad("QCD of the wrong length")
        for i in range(nb):
            if qcd[1 + i] & 7:
                _bad("QCD exponent byte with mantissa bits")
            mb = guard + (qcd[1 + i] >> 3) - 1
            if mb < 0:
                _bad("sub-band without magnitude bits")
            if mb > MAX_MB:
                _out("more magnitude bit-planes than the decoder takes")
            P.mb.append(mb)
    else:
        if sq & 31 != 2:
            _out("the 9/7 transform with derived or no quantisation")
        if len(qcd) != 1 + 2 * nb:
            _bad("QCD of the wrong length")
        for i in range(nb):
            v = _be(qcd, 1 + 2 * i, 2)
            expn, mant = v >> 11, v & 0x7FF
            mb = guard + expn - 1
            if mb < 0:
                _bad("sub-band without magnitude bits")
            if mb > MAX_MB:
                _out("more magnitude bit-planes than the decoder takes")
            P.mb.append(mb)
            P.step.append(F((1.0 + mant / 2048.0) * 2.0 ** (8 - expn)))   # in double, then rounded once
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


# ---------------------------------------------------------------------------------------------------------------- tier 1 in half units
_T1_CACHE = {}


def tier1_half_units(data, w, h, orient, nbps, npasses):
    """-> int32 [h, w]: the signed magnitudes of one code-block with their fractional bit kept (jp2_reference halves them): the walk
    one bit-plane higher gives every value doubled, and its halving then gives the half units back exactly."""
    key = (bytes(data), w, h, orient, nbps, npasses)
    got = _T1_CACHE.get(key)
    if got is None:
        if len(_T1_CACHE) > 20000:
            _T1_CACHE.clear()
        got = _T1_CACHE[key] = jr.tier1_block_walk(key[0], w, h, orient, nbps + 1, npasses)
    return got


# ---------------------------------------------------------------------------------------------------------------- 9/7 lifting, colour
def _idwt97_1d(a):
    """Inverse 9/7 along axis 1 of a float32 [m, n] array (n >= 2) whose first ceil(n/2) columns are low-pass (origin 0)."""
    n = a.shape[1]
    sn = (n + 1) // 2
    x = np.empty_like(a)
    x[:, 0::2] = a[:, :sn] * K_LOW
    x[:, 1::2] = a[:, sn:] * K_HIGH
    for step, c in enumerate(LIFT):
        idx = np.arange(step & 1, n, 2)
        left = np.where(idx > 0, idx - 1, idx + 1)        # a neighbour outside the line is replaced by the other one
        right = np.where(idx + 1 < n, idx + 1, idx - 1)
        x[:, idx] = x[:, idx] - (x[:, left] + x[:, right]) * c
    return x


def inverse_dwt97(plane, W, H, levels):
    for r in range(1, levels + 1):
        rw, rh = _cdiv(W, 1 << (levels - r)), _cdiv(H, 1 << (levels - r))
        t = _idwt97_1d(plane[:rh, :rw])
        plane[:rh, :rw] = _idwt97_1d(np.ascontiguousarray(t.T)).T
    return plane


def finish(planes, mct):
    """float32 [C, H, W] -> uint8 [C, H, W]: the irreversible colour transform, round to nearest even, level shift, clamp"""
    if mct:
        y, u, v = planes[0], planes[1], planes[2]
        r = y + v * F(1.402)
        g = y - u * F(0.34413) - v * F(0.71414)
        b = y + u * F(1.772)
        planes = np.stack([r, g, b])
    assert planes.dtype == np.float32
    return np.clip(np.rint(planes).astype(np.int64) + 128, 0, 255).astype(np.uint8)


def decode(data, tier1=True):
    d = bytes(data)
    info = [0] * 8
    try:
        s, e, box = jr.find_codestream(d)
        P = parse_headers(d, s, e, box, info)
        if not P.irreversible:
            return jr.decode(d, tier1)
        comps = jr.geometry(P)
        jr.tier2(d, P, comps)
        if not tier1:
            return 0, "", info, None
        planes = np.zeros((P.C, P.H, P.W), np.float32)
        for c in range(P.C):
            for r, bands in enumerate(comps[c]):
                for B in bands:
                    hs = F(0.5) * P.step[3 * r - 3 + B.orient if r else 0]
                    for K in B.blocks:
                        if K.passes:
                            blob = b"".join(d[o:o + n] for o, n in K.segs)
                            half = tier1_half_units(blob, K.w, K.h, K.orient, K.mb - K.zbp, K.passes)
                            planes[c, K.y:K.y + K.h, K.x:K.x + K.w] = half.astype(np.float32) * hs
            inverse_dwt97(planes[c], P.W, P.H, P.levels)
        rgb = finish(planes, P.mct)
        if P.C == 1:
            rgb = np.repeat(rgb, 3, axis=0)
        return 0, "", info, np.ascontiguousarray(rgb.transpose(1, 2, 0))
    except jr.Refuse as r:
        return r.status, r.reason, info, None


def probe(data):
    st, reason, info, _ = decode(data, tier1=False)
    return st, reason, info


_REF = {}


def reference(data):
    """decode(data), computed once per distinct file of a test session -> (status, reason, info, rgb)"""
    got = _REF.get(data)
    if got is None:
        got = _REF[data] = decode(data)
    return got
