"""A test-side VP8L (lossless WebP) writer for the streams libwebp's encoder never writes: forced predictor modes, block sizes, transform
orders, palettes of any size, colour caches of any size, simple and maximal-length prefix codes, repeat codes across alphabet boundaries,
entropy images with many groups, and backward references of chosen length, distance and distance code.

Nothing it writes is trusted: tests decode every file with Pillow and take Pillow's pixels as the expectation (webp_cases.py)."""
import heapq
import struct

import numpy as np

CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
# (dx, dy) of the 120 short distance codes: distance = dy * width + dx, at least 1
PLANE = [(0, 1), (1, 0), (1, 1), (-1, 1), (0, 2), (2, 0), (1, 2), (-1, 2), (2, 1), (-2, 1), (2, 2), (-2, 2), (0, 3), (3, 0), (1, 3), (-1, 3),
         (3, 1), (-3, 1), (2, 3), (-2, 3), (3, 2), (-3, 2), (0, 4), (4, 0), (1, 4), (-1, 4), (4, 1), (-4, 1), (3, 3), (-3, 3), (2, 4), (-2, 4),
         (4, 2), (-4, 2), (0, 5), (3, 4), (-3, 4), (4, 3), (-4, 3), (5, 0), (1, 5), (-1, 5), (5, 1), (-5, 1), (2, 5), (-2, 5), (5, 2), (-5, 2),
         (4, 4), (-4, 4), (3, 5), (-3, 5), (5, 3), (-5, 3), (0, 6), (6, 0), (1, 6), (-1, 6), (6, 1), (-6, 1), (2, 6), (-2, 6), (6, 2), (-6, 2),
         (4, 5), (-4, 5), (5, 4), (-5, 4), (3, 6), (-3, 6), (6, 3), (-6, 3), (0, 7), (7, 0), (1, 7), (-1, 7), (5, 5), (-5, 5), (7, 1), (-7, 1),
         (4, 6), (-4, 6), (6, 4), (-6, 4), (2, 7), (-2, 7), (7, 2), (-7, 2), (3, 7), (-3, 7), (7, 3), (-7, 3), (5, 6), (-5, 6), (6, 5), (-6, 5),
         (8, 0), (4, 7), (-4, 7), (7, 4), (-7, 4), (8, 1), (8, 2), (6, 6), (-6, 6), (8, 3), (5, 7), (-5, 7), (7, 5), (-7, 5), (8, 4), (6, 7),
         (-6, 7), (7, 6), (-7, 6), (8, 5), (7, 7), (-7, 7), (8, 6), (8, 7)]
assert len(PLANE) == 120 and len(set(PLANE)) == 120


def plane_distance(code, width):
    """pixel distance of distance code `code` (1-based, as the stream carries it after the prefix rule)"""
    if code > 120:
        return code - 120
    dx, dy = PLANE[code - 1]
    return max(1, dy * width + dx)


def code_for_distance(dist):
    return dist + 120


class BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.v |= value << self.n
        self.n += nbits

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def huffman_lengths(hist, maxlen=15):
    """code lengths (<= maxlen) for the used symbols of a histogram; a single used symbol gets length 1"""
    hist = list(hist)
    used = [s for s, c in enumerate(hist) if c]
    lens = [0] * len(hist)
    if len(used) <= 1:
        for s in used:
            lens[s] = 1
        return lens
    while True:
        heap = [(hist[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        depth = dict.fromkeys(used, 0)
        while len(heap) > 1:
            c0, k0, m0 = heapq.heappop(heap)
            c1, k1, m1 = heapq.heappop(heap)
            for s in m0 + m1:
                depth[s] += 1
            heapq.heappush(heap, (c0 + c1, min(k0, k1), m0 + m1))
        if max(depth.values()) <= maxlen:
            break
        hist = [(c + 1) // 2 if c else 0 for c in hist]   # flatten and retry
    for s in used:
        lens[s] = depth[s]
    return lens


def canonical_codes(lens):
    codes = [0] * len(lens)
    code = 0
    for l in range(1, 16):
        for s, sl in enumerate(lens):
            if sl == l:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


class Code:
    """one prefix code: lengths -> how its symbols are written"""

    def __init__(self, lens):
        self.lens = list(lens)
        self.codes = canonical_codes(self.lens)
        self.lone = sum(1 for l in self.lens if l) == 1

    def put(self, bw, sym):
        l = self.lens[sym]
        assert l, "symbol %d has no code" % sym
        if self.lone:
            return
        c = self.codes[sym]
        for i in range(l - 1, -1, -1):
            bw.put((c >> i) & 1, 1)


def write_code(bw, lens, style="auto", rle=True, max_symbol=False):
    """style: 'simple' (at most two symbols below 256, lengths all 1), 'normal' (through the code-length code), 'auto'.
    rle: use the repeat codes 16 / 17 / 18; max_symbol: write the count of code-length symbols explicitly."""
    used = [s for s, l in enumerate(lens) if l]
    simple_ok = 1 <= len(used) <= 2 and all(lens[s] == 1 for s in used) and used[-1] < 256
    if style == "simple" or (style == "auto" and simple_ok):
        assert simple_ok
        bw.put(1, 1)
        bw.put(len(used) - 1, 1)
        if used[0] < 2:
            bw.put(0, 1), bw.put(used[0], 1)
        else:
            bw.put(1, 1), bw.put(used[0], 8)
        if len(used) == 2:
            bw.put(used[1], 8)
        return Code(lens)
    # the run of code-length symbols
    n = len(lens)
    if max_symbol:
        while n > 0 and lens[n - 1] == 0:
            n -= 1
        if n < 2 or (rle and len(set(lens[:n])) == 1):   # (the count is written as count - 2: too few symbols to say so)
            n, max_symbol = len(lens), False
    toks = []   # (symbol, extra value, extra bits)
    i, prev = 0, 8
    while i < n:
        l = lens[i]
        run = 1
        while i + run < n and lens[i + run] == l:
            run += 1
        if rle and l == 0 and run >= 3:
            r = min(run, 138)
            toks.append((17, r - 3, 3) if r <= 10 else (18, r - 11, 7))
            i += r
        elif rle and l == prev and run >= 3:
            r = min(run, 6)
            toks.append((16, r - 3, 2))
            i += r
        else:
            toks.append((l, 0, 0))
            if l:
                prev = l
            i += 1
    hist = [0] * 19
    for t in toks:
        hist[t[0]] += 1
    cl = huffman_lengths(hist, 7)
    ncl = 19
    while ncl > 4 and cl[CL_ORDER[ncl - 1]] == 0:
        ncl -= 1
    bw.put(0, 1)
    bw.put(ncl - 4, 4)
    for k in range(ncl):
        bw.put(cl[CL_ORDER[k]], 3)
    clcode = Code(cl)
    if max_symbol:
        count = len(toks)
        assert count >= 2, count
        nbits = 2
        while count - 2 >= (1 << nbits):
            nbits += 2
        bw.put(1, 1), bw.put((nbits - 2) // 2, 3), bw.put(count - 2, nbits)
    else:
        bw.put(0, 1)
    for s, ev, eb in toks:
        clcode.put(bw, s)
        if eb:
            bw.put(ev, eb)
    return Code(lens)


def prefix_encode(v):
    """length or distance code value (>= 1) -> (prefix symbol, extra bits, extra value)"""
    v -= 1
    if v < 4:
        return v, 0, 0
    hb = v.bit_length() - 1
    second = (v >> (hb - 1)) & 1
    extra = hb - 1
    return 2 * hb + second, extra, v & ((1 << extra) - 1)


def cache_key(argb, bits):
    return ((0x1E35A7BD * argb) & 0xFFFFFFFF) >> (32 - bits)


def tokens_greedy(px, width, cache_bits=0, lz=True, min_match=3):
    """a plain tokeniser: literals, cache hits, and copies from the pixel above / to the left / a few rows up"""
    px = [int(p) for p in px]
    n = len(px)
    toks = []
    cache = {} if cache_bits else None
    pos = 0

    def insert(p):
        if cache is not None:
            cache[cache_key(p, cache_bits)] = p

    while pos < n:
        best, bestd = 0, 0
        if lz:
            for d in (1, width, 2, width + 1, width - 1, 2 * width, 3, 4):
                if 1 <= d <= pos:
                    l = 0
                    while pos + l < n and l < 4096 and px[pos + l] == px[pos + l - d]:
                        l += 1
                    if l > best:
                        best, bestd = l, d
        if best >= min_match:
            toks.append(("C", best, code_for_distance(bestd)))
            for k in range(best):
                insert(px[pos + k])
            pos += best
            continue
        p = px[pos]
        if cache is not None and cache.get(cache_key(p, cache_bits)) == p:
            toks.append(("K", p))
        else:
            toks.append(("L", p))
        insert(p)
        pos += 1
    return toks


def write_image(bw, toks, width, height, cache_bits=0, level0=False, meta=None, code_opts=None, force_lens=None):
    """one entropy-coded image.  toks: ('L', argb) literal, ('K', argb) the colour-cache index that holds argb (a literal if none does),
    ('C', length, distance code) a backward reference.  meta: None or (bits, list of group indices, one per block) (level0 only).
    code_opts: keyword arguments of write_code by alphabet index (0 green .. 4 distance), or for all when a plain dict of keywords;
    force_lens: {(group, alphabet): lengths} instead of lengths from the histogram (they must cover the symbols used)."""
    n = width * height
    bw.put(1 if cache_bits else 0, 1)
    if cache_bits:
        bw.put(cache_bits, 4)
    mbits, mw, mlist, ngroups = 0, 0, None, 1
    if level0:
        bw.put(1 if meta else 0, 1)
        if meta:
            mbits, mlist = meta
            mw = (width + (1 << mbits) - 1) >> mbits
            mh = (height + (1 << mbits) - 1) >> mbits
            assert len(mlist) == mw * mh
            bw.put(mbits - 2, 3)
            write_image(bw, [("L", 0xFF000000 | (g << 8)) for g in mlist], mw, mh)
            ngroups = max(mlist) + 1
    else:
        assert not meta
    # pass 1: simulate the decoder, resolve cache tokens, gather the symbols per group
    csize = (1 << cache_bits) if cache_bits else 0
    sizes = (280 + csize, 256, 256, 256, 40)
    out = [0] * n
    cache = [0] * csize
    syms = []   # (group, [(alphabet, symbol) | ('x', value, bits)])
    hists = [[[0] * s for s in sizes] for _ in range(ngroups)]
    pos = 0
    for t in toks:
        assert pos < n, "tokens past the image"
        y, x = divmod(pos, width)
        g = mlist[(y >> mbits) * mw + (x >> mbits)] if mlist else 0
        rec = []
        if t[0] == "C":
            _, length, dcode = t
            dist = plane_distance(dcode, width)
            assert dist <= pos and length <= n - pos, (pos, dist, length)
            ls, leb, lev = prefix_encode(length)
            ds, deb, dev = prefix_encode(dcode)
            rec = [(0, 256 + ls), ("x", lev, leb), (4, ds), ("x", dev, deb)]
            for k in range(length):
                out[pos + k] = out[pos + k - dist]
                if csize:
                    cache[cache_key(out[pos + k], cache_bits)] = out[pos + k]
            pos += length
        else:
            p = t[1] & 0xFFFFFFFF
            if t[0] == "K" and csize and cache[cache_key(p, cache_bits)] == p:
                rec = [(0, 280 + cache_key(p, cache_bits))]
            elif t[0] == "I":   # a raw cache index
                rec = [(0, 280 + t[1])]
                p = cache[t[1]]
            else:
                rec = [(0, (p >> 8) & 255), (1, (p >> 16) & 255), (2, p & 255), (3, p >> 24)]
            out[pos] = p
            if csize:
                cache[cache_key(p, cache_bits)] = p
            pos += 1
        for r in rec:
            if r[0] != "x":
                hists[g][r[0]][r[1]] += 1
        syms.append((g, rec))
    assert pos == n, "tokens cover %d of %d pixels" % (pos, n)
    # the codes
    codes = []
    for g in range(ngroups):
        row = []
        for a in range(5):
            lens = (force_lens or {}).get((g, a))
            if lens is None:
                h = hists[g][a]
                if not any(h):
                    h = list(h)
                    h[0] = 1   # an unused alphabet still needs a code: a lone symbol 0
                lens = huffman_lengths(h)
            else:
                lens = list(lens) + [0] * (sizes[a] - len(lens))
            opts = {}
            if code_opts:
                opts = code_opts.get(a, {}) if any(isinstance(k, int) for k in code_opts) else code_opts
            row.append(write_code(bw, lens, **opts))
        codes.append(row)
    for g, rec in syms:
        for r in rec:
            if r[0] == "x":
                if r[2]:
                    bw.put(r[1], r[2])
            else:
                codes[g][r[0]].put(bw, r[1])
    return out


def _sub(a, b):
    return (((a | 0x00FF00FF) - (b & 0xFF00FF00)) & 0xFF00FF00) | (((a | 0xFF00FF00) - (b & 0x00FF00FF)) & 0x00FF00FF)


def _avg2(a, b):
    return (((a ^ b) & 0xFEFEFEFE) >> 1) + (a & b)


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _ch(p):
    return [(p >> s) & 255 for s in (24, 16, 8, 0)]


def _pack(c):
    return (c[0] << 24) | (c[1] << 16) | (c[2] << 8) | c[3]


def predict(mode, L, T, TL, TR):
    if mode == 0 or mode > 13:
        return 0xFF000000
    if mode < 5:
        return (L, T, TR, TL)[mode - 1]
    if mode == 5:
        return _avg2(_avg2(L, TR), T)
    if mode == 6:
        return _avg2(L, TL)
    if mode == 7:
        return _avg2(L, T)
    if mode == 8:
        return _avg2(TL, T)
    if mode == 9:
        return _avg2(T, TR)
    if mode == 10:
        return _avg2(_avg2(L, TL), _avg2(T, TR))
    l, t, c = _ch(L), _ch(T), _ch(TL)
    if mode == 11:
        d = sum(abs(l[k] - c[k]) - abs(t[k] - c[k]) for k in range(4))
        return T if d <= 0 else L
    if mode == 12:
        return _pack([_clip(l[k] + t[k] - c[k]) for k in range(4)])
    a = _ch(_avg2(L, T))
    return _pack([_clip(a[k] + int((a[k] - c[k]) / 2)) for k in range(4)])


def fwd_predictor(px, w, h, bits, modes):
    """residuals of px under the per-block modes (list of subsize(w) x subsize(h) values 0..15)"""
    sw = (w + (1 << bits) - 1) >> bits
    res = list(px)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if y == 0:
                pred = 0xFF000000 if x == 0 else px[i - 1]
            elif x == 0:
                pred = px[i - w]
            else:
                pred = predict(modes[(y >> bits) * sw + (x >> bits)], px[i - 1], px[i - w], px[i - w - 1], px[i - w + 1])
            res[i] = _sub(px[i], pred)
    return res


def _s8(v):
    return v - 256 if v & 128 else v


def fwd_cross(px, w, h, bits, elems):
    """elems: per block (green_to_red, green_to_blue, red_to_blue), each 0..255"""
    sw = (w + (1 << bits) - 1) >> bits
    res = list(px)
    for y in range(h):
        for x in range(w):
            g2r, g2b, r2b = elems[(y >> bits) * sw + (x >> bits)]
            p = px[y * w + x]
            g, r = _s8((p >> 8) & 255), (p >> 16) & 255
            nr = (r - ((_s8(g2r) * g) >> 5)) & 255
            nb = ((p & 255) - ((_s8(g2b) * g) >> 5) - ((_s8(r2b) * _s8(r)) >> 5)) & 255
            res[y * w + x] = (p & 0xFF00FF00) | (nr << 16) | nb
    return res


def fwd_green(px):
    return [(p & 0xFF00FF00) | ((((p >> 16) - (p >> 8)) & 255) << 16) | ((p - (p >> 8)) & 255) for p in px]


def write_vp8l(width, height, argb, transforms=(), cache_bits=0, meta=None, lz=True, toks=None, alpha=False, sub_cache_bits=0,
               code_opts=None, force_lens=None, vp8x=False, extra_chunks=()):
    """-> file bytes.  argb: width * height words (with a ('palette', colours) transform: palette indices instead; an index may lie past
    the palette).  transforms, in stream order: ('predictor', bits, modes) | ('cross', bits, elems) | ('green',) | ('palette', colours).
    toks: explicit tokens for the ARGB stream instead of the tokeniser's (then argb is ignored and no transform may follow a palette).
    sub_cache_bits: colour cache of the sub-resolution images."""
    bw = BitWriter()
    bw.put(0x2F, 8), bw.put(width - 1, 14), bw.put(height - 1, 14), bw.put(1 if alpha else 0, 1), bw.put(0, 3)
    px = [int(p) & 0xFFFFFFFF for p in argb] if argb is not None else None
    xs = width
    for t in transforms:
        bw.put(1, 1)
        if t[0] == "predictor":
            bits, modes = t[1], t[2]
            bw.put(0, 2), bw.put(bits - 2, 3)
            sw, sh = (xs + (1 << bits) - 1) >> bits, (height + (1 << bits) - 1) >> bits
            assert len(modes) == sw * sh
            sub = [0xFF000000 | (m << 8) for m in modes]
            write_image(bw, tokens_greedy(sub, sw, sub_cache_bits), sw, sh, sub_cache_bits)
            if px is not None:
                px = fwd_predictor(px, xs, height, bits, modes)
        elif t[0] == "cross":
            bits, elems = t[1], t[2]
            bw.put(1, 2), bw.put(bits - 2, 3)
            sw, sh = (xs + (1 << bits) - 1) >> bits, (height + (1 << bits) - 1) >> bits
            assert len(elems) == sw * sh
            sub = [0xFF000000 | (e[2] << 16) | (e[1] << 8) | e[0] for e in elems]
            write_image(bw, tokens_greedy(sub, sw, sub_cache_bits), sw, sh, sub_cache_bits)
            if px is not None:
                px = fwd_cross(px, xs, height, bits, elems)
        elif t[0] == "green":
            bw.put(2, 2)
            if px is not None:
                px = fwd_green(px)
        else:
            colours = [int(c) & 0xFFFFFFFF for c in t[1]]
            nc = len(colours)
            bw.put(3, 2), bw.put(nc - 1, 8)
            deltas = [colours[0]] + [_sub(colours[i], colours[i - 1]) for i in range(1, nc)]
            write_image(bw, tokens_greedy(deltas, nc, sub_cache_bits), nc, 1, sub_cache_bits)
            bits = 0 if nc > 16 else 1 if nc > 4 else 2 if nc > 2 else 3
            if px is not None:
                pw = (xs + (1 << bits) - 1) >> bits
                per, bpp = 1 << bits, 8 >> bits
                packed = [0] * (pw * height)
                for y in range(height):
                    for x in range(xs):
                        packed[y * pw + (x >> bits)] |= (px[y * xs + x] & ((1 << bpp) - 1)) << ((x & (per - 1)) * bpp)
                px = [0xFF000000 | (v << 8) for v in packed]
                xs = pw
            else:
                xs = (xs + (1 << bits) - 1) >> bits
    bw.put(0, 1)
    if toks is None:
        toks = tokens_greedy(px, xs, cache_bits, lz)
    write_image(bw, toks, xs, height, cache_bits, True, meta, code_opts, force_lens)
    payload = bw.bytes()
    return riff(payload, width, height, vp8x, extra_chunks, alpha)


def chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def riff(vp8l_payload, width, height, vp8x=False, extra_chunks=(), alpha=False):
    """extra_chunks: (tag, payload, before the image?)"""
    body = b""
    if vp8x:
        flags = (0x10 if alpha else 0)
        for tag, _, _ in extra_chunks:
            flags |= {b"EXIF": 0x08, b"XMP ": 0x04, b"ICCP": 0x20}.get(tag, 0)
        w, h = width - 1, height - 1
        body += chunk(b"VP8X", bytes([flags, 0, 0, 0, w & 255, (w >> 8) & 255, w >> 16, h & 255, (h >> 8) & 255, h >> 16]))
        for tag, payload, before in extra_chunks:
            if before:
                body += chunk(tag, payload)
    body += chunk(b"VP8L", vp8l_payload)
    if vp8x:
        for tag, payload, before in extra_chunks:
            if not before:
                body += chunk(tag, payload)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body
