"""The tiled side of the JPEG 2000 decoder (csrc/jp2_parse.h with JP2_TAKE_TILES, the parity-aware lifting of csrc/jp2_t1.h,
csrc/jp2dec.hip) restated in plain Python / numpy on top of tests/jp2_reference.py and tests/jp2_irreversible_reference.py: image and
tile origins, the tile grid, tile-parts of any tile in any order, user precinct sizes, the geometry in canvas coordinates, the five
progression orders over several precincts, and both inverse transforms over lines that may start on an odd coordinate.

decode(data, flags=TILES | IRREVERSIBLE) / probe(data, flags): as jp2_reference's.  info[0:2] are the image area's width and height
once SIZ's origins have passed their checks.  The checks come in the parser's order."""
import numpy as np

import jp2_irreversible_reference as ir
import jp2_reference as jr
from jp2_reference import MAX_BLOCKS, MAX_LAYERS, MAX_LEVELS, MAX_MB, MAX_PIXELS, MAX_SIDE, OUTSIDE, SKIP_MAIN, SKIP_TILE, Params, _bad, _be, _cdiv, _out

IRREVERSIBLE, TILES = 1, 2
MAX_TILES = 4096
MAX_CANVAS = 1 << 30
F = np.float32


def parse_headers(d, s, e, box, info, irreversible=True):
    """The main header and the tile-part headers with JP2_TAKE_TILES.  Params gains .X0/.Y0 (image origin), .tiles (canvas corners
    tx0, ty0, tx1, ty1 per tile), .pp ((PPx, PPy) per resolution) and .parts as (tile, start, end)."""
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
    if XO >= X or YO >= Y:
        _bad("image origin outside the reference grid")
    if XTO > XO or YTO > YO or XTO + XT <= XO or YTO + YT <= YO:
        _bad("origins that leave the first tile empty")
    if X > MAX_CANVAS or Y > MAX_CANVAS:
        _out("reference grid larger than the decoder takes")
    ntx, nty = _cdiv(X - XTO, XT), _cdiv(Y - YTO, YT)
    if ntx * nty > MAX_TILES:
        _out("more than 4096 tiles")
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
    W, H = X - XO, Y - YO
    info[0:2] = [W, H]
    if W > MAX_SIDE or H > MAX_SIDE or W * H > MAX_PIXELS:
        _out("image larger than the decoder takes")
    if box is not None and (box[0] != H or box[1] != W or box[2] != C):
        _bad("ihdr disagrees with SIZ")
    P.W, P.H, P.C, P.X0, P.Y0 = W, H, C, XO, YO
    P.tiles = []
    for ty in range(nty):
        for tx in range(ntx):
            P.tiles.append((max(XTO + tx * XT, XO), max(YTO + ty * YT, YO), min(XTO + (tx + 1) * XT, X), min(YTO + (ty + 1) * YT, Y)))
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
    P.pp = [(cod[10 + r] & 15, cod[10 + r] >> 4) if scod & 1 else (15, 15) for r in range(P.levels + 1)]
    for r in range(1, P.levels + 1):
        if P.pp[r][0] == 0 or P.pp[r][1] == 0:
            _bad("precinct of one sample above resolution 0")
    if scod & 6:
        _out("SOP or EPH markers")
    if P.irreversible and not irreversible:
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
    if P.irreversible:
        for tx0, ty0, tx1, ty1 in P.tiles:
            for r in range(1, P.levels + 1):
                sh = P.levels - r
                if _cdiv(tx1, 1 << sh) - _cdiv(tx0, 1 << sh) == 1 or _cdiv(ty1, 1 << sh) - _cdiv(ty0, 1 << sh) == 1:
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
    else:
        if sq & 31 != 2:
            _out("the 9/7 transform with derived or no quantisation")
        if len(qcd) != 1 + 2 * nb:
            _bad("QCD of the wrong length")
    for i in range(nb):
        if not P.irreversible:
            if qcd[1 + i] & 7:
                _bad("QCD exponent byte with mantissa bits")
            expn = qcd[1 + i] >> 3
        else:
            v = _be(qcd, 1 + 2 * i, 2)
            expn = v >> 11
            P.step.append(F((1.0 + (v & 0x7FF) / 2048.0) * 2.0 ** (8 - expn)))   # in double, then rounded once
        mb = guard + expn - 1
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
    # tile-parts: of any tile, in any order; TPsot counts up within its tile
    P.parts = []
    nt = len(P.tiles)
    next_tp, total = [0] * nt, [0] * nt
    while True:
        if p + 12 > e:
            _bad("SOT cut short")
        if _be(d, p, 2) != 0xFF90 or _be(d, p + 2, 2) != 10:
            _bad("SOT expected")
        isot, psot, tpsot, tnsot = _be(d, p + 4, 2), _be(d, p + 6, 4), d[p + 10], d[p + 11]
        if isot >= nt:
            _bad("tile index outside the grid")
        if tpsot != next_tp[isot] or (tnsot and tpsot >= tnsot):
            _bad("tile-parts out of order")
        if tnsot:
            if total[isot] and total[isot] != tnsot:
                _bad("tile-part count changes within a tile")
            total[isot] = tnsot
        pend = p + psot if psot else e - 2
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
        P.parts.append((isot, q, pend))
        p = pend
        next_tp[isot] += 1
        if next_tp[isot] > 255:
            _bad("too many tile-parts")
        if p + 2 <= e and _be(d, p, 2) == 0xFFD9:
            break
    if p + 2 != e:
        _bad("data after EOC")
    for t in range(nt):
        if next_tp[t] == 0:
            _bad("tile without a tile-part")
        if total[t] and total[t] != next_tp[t]:
            _bad("fewer tile-parts than the tile announces")
    return P


# ---------------------------------------------------------------------------------------------------------------- geometry
class Precinct:
    pass


def geometry(P):
    """-> tiles[t][c][r] = list of Precinct (raster order), each with .bands (jr.Band with a block grid and two tag trees) and .X / .Y,
    the canvas position at which the position-first orders visit it.  A block's x, y, w, h are its rectangle in the component plane
    (image coordinates): each tile-component owns its rectangle, its sub-bands laid out inside it as the transform reads them."""
    out = []
    nblocks = 0
    Lv = P.levels
    for t, (tx0, ty0, tx1, ty1) in enumerate(P.tiles):
        comps = []
        for c in range(P.C):
            res = []
            for r in range(Lv + 1):
                sh = Lv - r
                rx0, ry0, rx1, ry1 = _cdiv(tx0, 1 << sh), _cdiv(ty0, 1 << sh), _cdiv(tx1, 1 << sh), _cdiv(ty1, 1 << sh)
                ppx, ppy = P.pp[r]
                precs = []
                if rx1 > rx0 and ry1 > ry0:
                    gx0, gy0 = rx0 >> ppx, ry0 >> ppy
                    npx, npy = _cdiv(rx1, 1 << ppx) - gx0, _cdiv(ry1, 1 << ppy) - gy0
                    # the low-pass counts of this resolution (the size of the one below) place HL / LH / HH inside the rectangle
                    lw, lh = _cdiv(rx1, 2) - _cdiv(rx0, 2), _cdiv(ry1, 2) - _cdiv(ry0, 2)
                    xe, ye = min(P.cbw.bit_length() - 1, ppx - 1 if r else ppx), min(P.cbh.bit_length() - 1, ppy - 1 if r else ppy)
                    for py in range(npy):
                        for px in range(npx):
                            Q = Precinct()
                            Q.c, Q.r = c, r
                            Q.X = tx0 if px == 0 and rx0 % (1 << ppx) else ((gx0 + px) << ppx) << sh
                            Q.Y = ty0 if py == 0 and ry0 % (1 << ppy) else ((gy0 + py) << ppy) << sh
                            Q.bands = []
                            for orient in ((0,) if r == 0 else (1, 2, 3)):
                                xob, yob = orient & 1, orient >> 1
                                if r == 0:
                                    bx0, by0, bx1, by1 = rx0, ry0, rx1, ry1
                                    qx0, qy0, qw, qh = (gx0 + px) << ppx, (gy0 + py) << ppy, 1 << ppx, 1 << ppy
                                else:
                                    nbl = sh + 1
                                    bx0, bx1 = _cdiv(tx0 - (xob << (nbl - 1)), 1 << nbl), _cdiv(tx1 - (xob << (nbl - 1)), 1 << nbl)
                                    by0, by1 = _cdiv(ty0 - (yob << (nbl - 1)), 1 << nbl), _cdiv(ty1 - (yob << (nbl - 1)), 1 << nbl)
                                    qx0, qy0, qw, qh = ((gx0 + px) << ppx) >> 1, ((gy0 + py) << ppy) >> 1, 1 << (ppx - 1), 1 << (ppy - 1)
                                ax0, ay0, ax1, ay1 = max(qx0, bx0), max(qy0, by0), min(qx0 + qw, bx1), min(qy0 + qh, by1)
                                B = jr.Band()
                                B.orient = orient
                                B.mb = P.mb[3 * r - 3 + orient if r else 0]
                                B.blocks = []
                                if ax1 > ax0 and ay1 > ay0:
                                    cx0, cy0 = ax0 >> xe, ay0 >> ye
                                    B.nx, B.ny = _cdiv(ax1, 1 << xe) - cx0, _cdiv(ay1, 1 << ye) - cy0
                                else:
                                    cx0 = cy0 = B.nx = B.ny = 0
                                for by in range(B.ny):
                                    for bx in range(B.nx):
                                        K = jr.Block()
                                        K.c, K.r, K.orient, K.bx, K.by, K.tile = c, r, orient, bx, by, t
                                        kx0, ky0 = max((cx0 + bx) << xe, ax0), max((cy0 + by) << ye, ay0)
                                        kx1, ky1 = min((cx0 + bx + 1) << xe, ax1), min((cy0 + by + 1) << ye, ay1)
                                        K.x = tx0 - P.X0 + (lw if r and xob else 0) + kx0 - bx0
                                        K.y = ty0 - P.Y0 + (lh if r and yob else 0) + ky0 - by0
                                        K.w, K.h = kx1 - kx0, ky1 - ky0
                                        K.mb, K.zbp, K.passes, K.segs, K.included, K.lblock = B.mb, 0, 0, [], False, 3
                                        B.blocks.append(K)
                                nblocks += len(B.blocks)
                                if nblocks > MAX_BLOCKS:
                                    _out("more code-blocks than the decoder takes")
                                B.incl, B.zbpt = jr.TagTree(B.nx, B.ny), jr.TagTree(B.nx, B.ny)
                                Q.bands.append(B)
                            precs.append(Q)
                res.append(precs)
            comps.append(res)
        out.append(comps)
    return out


def packet_order(P, comps):
    """the packets of one tile as (layer, Precinct), in the progression order"""
    precs = [(Q, i) for c in range(P.C) for r in range(P.levels + 1) for i, Q in enumerate(comps[c][r])]
    Ly = range(P.layers)
    if P.order == 0:
        precs.sort(key=lambda qi: (qi[0].r, qi[0].c, qi[1]))
        return [(l, Q) for l in Ly for Q, _ in precs]
    if P.order == 1:
        precs.sort(key=lambda qi: (qi[0].r, qi[0].c, qi[1]))
        return [(l, Q) for r in range(P.levels + 1) for l in Ly for Q, _ in precs if Q.r == r]
    if P.order == 2:
        precs.sort(key=lambda qi: (qi[0].r, qi[0].Y, qi[0].X, qi[0].c))
    elif P.order == 3:
        precs.sort(key=lambda qi: (qi[0].Y, qi[0].X, qi[0].c, qi[0].r))
    else:
        precs.sort(key=lambda qi: (qi[0].c, qi[0].Y, qi[0].X, qi[0].r))
    return [(l, Q) for Q, _ in precs for l in Ly]


def tier2(d, P, tiles):
    P.packet_ends = [[] for _ in tiles]   # per tile: the offset in the file at which each packet ends (tests/jp2_tiles_cases.py cuts there)
    for t, comps in enumerate(tiles):
        parts = [(a, b) for tt, a, b in P.parts if tt == t]
        part = 0
        pos, pend = parts[0]
        for layer, Q in packet_order(P, comps):
            while pos == pend and part + 1 < len(parts):
                part += 1
                pos, pend = parts[part]
            bio = jr.Bits(d, pos, pend)
            got = []
            if bio.bit():
                for B in Q.bands:
                    for K in B.blocks:
                        inc = bio.bit() if K.included else B.incl.decode(bio, K.bx, K.by, layer + 1)
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
                        n = jr._npasses(bio)
                        while bio.bit():
                            K.lblock += 1
                            if K.lblock > 32:
                                _bad("Lblock out of range")
                        K.passes += n
                        if K.passes > 3 * (K.mb - K.zbp) - 2:
                            _bad("more coding passes than the bit-planes hold")
                        got.append((K, bio.bits(K.lblock + n.bit_length() - 1)))
            pos = bio.align()
            for K, ln in got:
                if ln > pend - pos:
                    _bad("segment length outside the tile-part")
                if len(K.segs) >= MAX_LAYERS:
                    _bad("too many segments")
                K.segs.append((pos, ln))
                pos += ln
            P.packet_ends[t].append(pos)
        while pos == pend and part + 1 < len(parts):
            part += 1
            pos, pend = parts[part]
        if pos != pend or part + 1 != len(parts):
            _bad("data left over after the last packet")


# ---------------------------------------------------------------------------------------------------------------- transforms
def _mirror(idx, n):
    """the neighbours of the positions idx in a line of n >= 2 samples; one outside the line is replaced by the other one"""
    return np.where(idx > 0, idx - 1, idx + 1), np.where(idx + 1 < n, idx + 1, idx - 1)


def idwt53_1d(a, cas):
    """Inverse 5/3 along axis 1 of an int [m, n] array, low-pass samples first, for a line whose first canvas coordinate has parity cas.
    Sample i is a low-pass sample where i + cas is even, and the i >> 1-th of its kind either way.  A lone low-pass sample is copied; a
    lone high-pass sample is halved toward zero, as OpenJPEG's `/= 2` does."""
    n = a.shape[1]
    a = a.astype(np.int64)
    if n == 1:
        return a.copy() if cas == 0 else np.sign(a) * (np.abs(a) // 2)
    sn = (n + 1 - cas) // 2
    x = np.empty_like(a)
    low, high = np.arange(cas, n, 2), np.arange(1 - cas, n, 2)
    x[:, low] = a[:, :sn]
    x[:, high] = a[:, sn:]
    l, r = _mirror(low, n)
    x[:, low] = x[:, low] - ((x[:, l] + x[:, r] + 2) >> 2)
    l, r = _mirror(high, n)
    x[:, high] = x[:, high] + ((x[:, l] + x[:, r]) >> 1)
    return x


def idwt97_1d(a, cas):
    """Inverse 9/7 along axis 1 of a float32 [m, n] array (n >= 2), low-pass samples first; the steps go by canvas parity"""
    n = a.shape[1]
    sn = (n + 1 - cas) // 2
    x = np.empty_like(a)
    x[:, cas::2] = a[:, :sn] * ir.K_LOW
    x[:, 1 - cas::2] = a[:, sn:] * ir.K_HIGH
    for step, c in enumerate(ir.LIFT):
        idx = np.arange((step + cas) & 1, n, 2)
        l, r = _mirror(idx, n)
        x[:, idx] = x[:, idx] - (x[:, l] + x[:, r]) * c
    return x


def inverse_dwt_tile(plane, P, tile):
    """rebuilds the tile-component whose canvas corners are `tile` inside its rectangle of the component plane"""
    tx0, ty0, tx1, ty1 = tile
    view = plane[ty0 - P.Y0:ty1 - P.Y0, tx0 - P.X0:tx1 - P.X0]
    one = idwt97_1d if P.irreversible else idwt53_1d
    for r in range(1, P.levels + 1):
        sh = P.levels - r
        rx0, ry0, rx1, ry1 = _cdiv(tx0, 1 << sh), _cdiv(ty0, 1 << sh), _cdiv(tx1, 1 << sh), _cdiv(ty1, 1 << sh)
        rw, rh = rx1 - rx0, ry1 - ry0
        if rw == 0 or rh == 0:
            continue
        t = one(view[:rh, :rw], rx0 & 1).astype(plane.dtype)
        view[:rh, :rw] = one(np.ascontiguousarray(t.T), ry0 & 1).T


def decode(data, flags=TILES | IRREVERSIBLE, tier1=True):
    d = bytes(data)
    if not flags & TILES:
        return ir.decode(d, tier1) if flags & IRREVERSIBLE else jr.decode(d, tier1)
    info = [0] * 8
    try:
        s, e, box = jr.find_codestream(d)
        P = parse_headers(d, s, e, box, info, bool(flags & IRREVERSIBLE))
        tiles = geometry(P)
        tier2(d, P, tiles)
        if not tier1:
            return 0, "", info, None
        planes = np.zeros((P.C, P.H, P.W), np.float32 if P.irreversible else np.int32)
        for t, comps in enumerate(tiles):
            for c in range(P.C):
                for r, precs in enumerate(comps[c]):
                    for Q in precs:
                        for B in Q.bands:
                            for K in B.blocks:
                                if not K.passes:
                                    continue
                                blob = b"".join(d[o:o + n] for o, n in K.segs)
                                if P.irreversible:
                                    hs = F(0.5) * P.step[3 * r - 3 + B.orient if r else 0]
                                    v = ir.tier1_half_units(blob, K.w, K.h, K.orient, K.mb - K.zbp, K.passes).astype(np.float32) * hs
                                else:
                                    v = jr.tier1_block(blob, K.w, K.h, K.orient, K.mb - K.zbp, K.passes)
                                planes[c, K.y:K.y + K.h, K.x:K.x + K.w] = v
                inverse_dwt_tile(planes[c], P, P.tiles[t])
        if P.irreversible:
            rgb = ir.finish(planes, P.mct)
        else:
            if P.mct:
                y, u, v = planes[0], planes[1], planes[2]
                g = y - ((u + v) >> 2)
                planes = np.stack([v + g, g, u + g])
            rgb = np.clip(planes + 128, 0, 255).astype(np.uint8)
        if P.C == 1:
            rgb = np.repeat(rgb, 3, axis=0)
        return 0, "", info, np.ascontiguousarray(rgb.transpose(1, 2, 0))
    except jr.Refuse as r:
        return r.status, r.reason, info, None


def probe(data, flags=TILES | IRREVERSIBLE):
    st, reason, info, _ = decode(data, flags, tier1=False)
    return st, reason, info


_REF = {}


def reference(data, flags=TILES | IRREVERSIBLE):
    """decode(data, flags), computed once per distinct file of a test session -> (status, reason, info, rgb)"""
    got = _REF.get((data, flags))
    if got is None:
        got = _REF[(data, flags)] = decode(data, flags)
    return got
