"""Plain-Python restatement of the lossless WebP (VP8L) reader behind lumina_ocr_webp_probe / lumina_ocr_webp_decode
(csrc/webp_parse.h, csrc/webp_dec.h): the same container walk, the same statuses, the same refusals.

    probe(data)  -> (status, info, reason)      status 0 read / -1 corrupt or irregular / -2 valid WebP that is not read
    decode(data) -> (status, rgb uint8 [H, W, 3] or None)

Nothing here is a yardstick: every expectation of the tests is Pillow's (libwebp's) own decode; this file only says which files the
device reader must accept and which it must refuse, so that the device can be held to it status for status."""
import numpy as np

MAX_PIXELS = 1 << 26      # width x height the reader takes (-2 beyond): 8192 x 8192; 16384 x 1 and 1 x 16384 are far inside
MAX_GROUPS = 4096         # prefix-code groups an entropy image may name (-2 beyond; libwebp's encoder stays below 2600)
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
CODE_TO_PLANE = bytes.fromhex(
    "180717192806272916 1a262a38053739151b363a252b48044749141c353b464a242c58454b343c03"
    "5759131d565a232d444c555b333d68026769121e666a222e545c434d656b323e78017779535d111f"
    "646c424e767a212f757b313f636d525e00747c414f1020626e30737d515f40727e616f50717f6070".replace(" ", ""))
assert len(CODE_TO_PLANE) == 120 and len(set(CODE_TO_PLANE)) == 120


class Corrupt(Exception):
    pass


class Unread(Exception):
    pass


def _le32(b, o):
    return b[o] | (b[o + 1] << 8) | (b[o + 2] << 16) | (b[o + 3] << 24)


def probe_span(data):
    """-> (status, info dict, reason, (offset, length) of the VP8L payload or None)"""
    info = dict(width=0, height=0, alpha=0, vp8x=0, exif=0, xmp=0)
    n = len(data)
    if n < 12 or data[:4] != b"RIFF" or data[8:12] != b"WEBP":
        return -1, info, "not a RIFF / WEBP file", None
    riff = _le32(data, 4)
    if riff + 8 > n:
        return -1, info, "RIFF size past the file", None
    if riff + 8 < n:
        return -1, info, "bytes after the RIFF payload", None
    if riff & 1:
        return -1, info, "odd RIFF size", None
    chunks = []
    p = 12
    while p < n:
        if p + 8 > n:
            return -1, info, "chunk header past the file", None
        size = _le32(data, p + 4)
        if size > 0x7FFFFFFF or p + 8 + size + (size & 1) > n:
            return -1, info, "chunk past the file", None
        chunks.append((bytes(data[p:p + 4]), p + 8, size))
        p += 8 + size + (size & 1)
    if not chunks:
        return -1, info, "no chunk", None
    span = None
    canvas = None
    refused = None
    tag0, off0, size0 = chunks[0]
    if tag0 == b"VP8X":
        info["vp8x"] = 1
        if size0 != 10:
            return -1, info, "VP8X chunk of another size than 10", None
        if data[off0] & 0xC1:
            return -1, info, "reserved VP8X flag bits set", None
        if data[off0] & 0x02:
            refused = "animated WebP"
        canvas = (1 + (data[off0 + 4] | (data[off0 + 5] << 8) | (data[off0 + 6] << 16)),
                  1 + (data[off0 + 7] | (data[off0 + 8] << 8) | (data[off0 + 9] << 16)))
        for tag, off, size in chunks[1:]:
            if tag == b"VP8X":
                return -1, info, "second VP8X chunk", None
            if tag == b"VP8L":
                if span is not None:
                    return -1, info, "second VP8L chunk", None
                span = (off, size)
            elif tag == b"VP8 ":
                refused = refused or "lossy WebP (VP8)"
            elif tag == b"ALPH":
                refused = refused or "lossy WebP with an ALPH chunk"
            elif tag in (b"ANIM", b"ANMF"):
                refused = refused or "animated WebP"
            elif tag == b"EXIF":
                info["exif"] = 1
            elif tag == b"XMP ":
                info["xmp"] = 1
    elif tag0 == b"VP8L":
        if len(chunks) != 1:
            return -1, info, "chunks after the image of a file without VP8X", None
        span = (off0, size0)
    elif tag0 == b"VP8 ":
        if len(chunks) != 1:
            return -1, info, "chunks after the image of a file without VP8X", None
        return -2, info, "lossy WebP (VP8)", None
    else:
        return -1, info, "first chunk is neither VP8X, VP8L nor VP8", None
    if refused:
        return -2, info, refused, None
    if span is None:
        return -1, info, "no image chunk", None
    off, size = span
    if size < 5 or data[off] != 0x2F:
        return -1, info, "VP8L signature byte is not 0x2F", None
    v = _le32(data, off + 1)
    if v >> 29:
        return -1, info, "VP8L version is not 0", None
    info["width"], info["height"], info["alpha"] = 1 + (v & 0x3FFF), 1 + ((v >> 14) & 0x3FFF), (v >> 28) & 1
    if canvas is not None and canvas != (info["width"], info["height"]):
        return -1, info, "VP8X canvas differs from the VP8L header", None
    if info["width"] * info["height"] > MAX_PIXELS:
        return -2, info, "more than 2^26 pixels", None
    if size >= 1 << 28:
        return -2, info, "VP8L chunk of 256 MB or more", None
    return 0, info, "", span


def probe(data):
    rc, info, reason, _ = probe_span(data)
    return rc, info, reason


class _Bits:
    """LSB-first reader; bits past the end read as 0 and make the stream corrupt once consumed"""

    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.n = 8 * len(data)
        self.pos = 0

    def read(self, k):
        r = (self.v >> self.pos) & ((1 << k) - 1)
        self.pos += k
        return r

    def check(self):
        if self.pos > self.n:
            raise Corrupt("read past the chunk")


def _build(lens):
    """canonical code of these lengths -> (lone symbol or -1, count per length, symbols sorted by (length, value))"""
    cnt = [0] * 16
    for l in lens:
        cnt[l] += 1
    syms = [s for l in range(1, 16) for s in range(len(lens)) if lens[s] == l]
    if not syms:
        raise Corrupt("code without symbols")
    if len(syms) == 1:
        if cnt[15]:
            raise Corrupt("lone symbol of length 15")
        return syms[0], cnt, syms
    left = 1
    for l in range(1, 16):
        left = 2 * left - cnt[l]
        if left < 0:
            raise Corrupt("over-subscribed code")
    if left:
        raise Corrupt("incomplete code")
    return -1, cnt, syms


def _sym(br, tree):
    lone, cnt, syms = tree
    if lone >= 0:
        return lone
    code = first = index = 0
    v = br.v >> br.pos
    for l in range(1, 16):
        code |= (v >> (l - 1)) & 1
        c = cnt[l]
        if code - first < c:
            br.pos += l
            return syms[index + code - first]
        index += c
        first = (first + c) << 1
        code <<= 1
    raise Corrupt("unused code")   # (a complete code has none: unreachable)


def _read_code(br, size):
    lens = [0] * size
    if br.read(1):
        two = br.read(1)
        s0 = br.read(8 if br.read(1) else 1)
        if s0 >= size:
            raise Corrupt("simple code: symbol outside the alphabet")
        lens[s0] = 1
        if two:
            s1 = br.read(8)
            if s1 >= size or s1 == s0:
                raise Corrupt("simple code: second symbol outside the alphabet or equal to the first")
            lens[s1] = 1
    else:
        ncl = br.read(4) + 4
        cl = [0] * 19
        for i in range(ncl):
            cl[CL_ORDER[i]] = br.read(3)
        cltree = _build(cl)
        maxsym = size
        if br.read(1):
            nb = 2 + 2 * br.read(3)
            maxsym = 2 + br.read(nb)
            if maxsym > size:
                raise Corrupt("max_symbol past the alphabet")
        sym, prev = 0, 8
        while sym < size and maxsym > 0:
            maxsym -= 1
            c = _sym(br, cltree)
            br.check()
            if c < 16:
                lens[sym] = c
                sym += 1
                if c:
                    prev = c
            else:
                rep = br.read((2, 3, 7)[c - 16]) + (3, 3, 11)[c - 16]
                if sym + rep > size:
                    raise Corrupt("repeat past the alphabet")
                if c == 16:
                    lens[sym:sym + rep] = [prev] * rep
                sym += rep
    br.check()
    return _build(lens)


def _prefix(br, s):
    if s < 4:
        return s + 1
    extra = (s - 2) >> 1
    return ((2 + (s & 1)) << extra) + br.read(extra) + 1


def _subsize(n, bits):
    return (n + (1 << bits) - 1) >> bits


def _image(br, w, h, level0):
    """one entropy-coded image (the ARGB stream or a sub-resolution image) -> list of w * h ARGB words"""
    cb = 0
    if br.read(1):
        cb = br.read(4)
        if not 1 <= cb <= 11:
            raise Corrupt("colour-cache bits outside 1..11")
    meta, mbits, mw, ngroups = None, 0, 0, 1
    if level0 and br.read(1):
        mbits = br.read(3) + 2
        mw = _subsize(w, mbits)
        meta = [(p >> 8) & 0xFFFF for p in _image(br, mw, _subsize(h, mbits), False)]
        ngroups = max(meta) + 1
        if ngroups > MAX_GROUPS:
            raise Unread("more than 4096 prefix-code groups")
    br.check()
    sizes = (280 + ((1 << cb) if cb else 0), 256, 256, 256, 40)
    groups = [[_read_code(br, s) for s in sizes] for _ in range(ngroups)]
    n = w * h
    out = [0] * n
    cache = [0] * (1 << cb) if cb else None
    shift = 32 - cb
    pos = 0
    while pos < n:
        if meta is None:
            g = groups[0]
        else:
            y = pos // w
            g = groups[meta[(y >> mbits) * mw + ((pos - y * w) >> mbits)]]
        s = _sym(br, g[0])
        if s < 256:
            r = _sym(br, g[1])
            b = _sym(br, g[2])
            a = _sym(br, g[3])
            p = (a << 24) | (r << 16) | (s << 8) | b
            out[pos] = p
            if cache is not None:
                cache[((0x1E35A7BD * p) & 0xFFFFFFFF) >> shift] = p
            pos += 1
        elif s < 280:
            length = _prefix(br, s - 256)
            dcode = _prefix(br, _sym(br, g[4]))
            if dcode > 120:
                dist = dcode - 120
            else:
                c = CODE_TO_PLANE[dcode - 1]
                dist = max(1, (c >> 4) * w + 8 - (c & 15))
            if dist > pos or length > n - pos:
                raise Corrupt("copy before the first or past the last pixel")
            if dist >= length:
                out[pos:pos + length] = out[pos - dist:pos - dist + length]
            else:
                period = out[pos - dist:pos]
                out[pos:pos + length] = (period * (length // dist + 1))[:length]
            if cache is not None:
                for p in out[pos:pos + length]:
                    cache[((0x1E35A7BD * p) & 0xFFFFFFFF) >> shift] = p
            pos += length
        else:
            p = cache[s - 280]
            out[pos] = p
            cache[((0x1E35A7BD * p) & 0xFFFFFFFF) >> shift] = p
            pos += 1
        br.check()
    return out


def _add(a, b):
    return (((a & 0xFF00FF00) + (b & 0xFF00FF00)) & 0xFF00FF00) | (((a & 0x00FF00FF) + (b & 0x00FF00FF)) & 0x00FF00FF)


def _avg2(a, b):
    return (((a ^ b) & 0xFEFEFEFE) >> 1) + (a & b)


def _clip(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _predict(mode, L, T, TL, TR):
    if mode == 0 or mode > 13:
        return 0xFF000000
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 3:
        return TR
    if mode == 4:
        return TL
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
    if mode == 11:
        d = 0
        for sh in (24, 16, 8, 0):
            t, l, c = (T >> sh) & 255, (L >> sh) & 255, (TL >> sh) & 255
            d += abs(l - c) - abs(t - c)
        return T if d <= 0 else L
    r = 0
    if mode == 12:
        for sh in (24, 16, 8, 0):
            r |= _clip(((L >> sh) & 255) + ((T >> sh) & 255) - ((TL >> sh) & 255)) << sh
        return r
    A = _avg2(L, T)
    for sh in (24, 16, 8, 0):
        a, b = (A >> sh) & 255, (TL >> sh) & 255
        r |= _clip(a + int((a - b) / 2)) << sh   # (the division truncates towards zero)
    return r


def _inv_predictor(d, w, h, bits, sub):
    sw = _subsize(w, bits)
    d[0] = _add(d[0], 0xFF000000)
    for x in range(1, w):
        d[x] = _add(d[x], d[x - 1])
    for y in range(1, h):
        row = y * w
        d[row] = _add(d[row], d[row - w])
        srow = (y >> bits) * sw
        for x in range(1, w):
            i = row + x
            mode = (sub[srow + (x >> bits)] >> 8) & 15
            d[i] = _add(d[i], _predict(mode, d[i - 1], d[i - w], d[i - w - 1], d[i - w + 1]))


def _s8(v):
    return v - 256 if v & 128 else v


def _s8v(v):
    return (v & 255).astype(np.uint8).view(np.int8).astype(np.int64)


def _inv_cross(d, w, h, bits, sub):
    """(whole-array arithmetic: the same per-pixel rule as the loops elsewhere in this file)"""
    sw = _subsize(w, bits)
    ys, xs = np.mgrid[0:h, 0:w]
    m = np.array(sub, dtype=np.int64)[(ys >> bits) * sw + (xs >> bits)].reshape(-1)
    p = np.array(d, dtype=np.int64)
    g = _s8v(p >> 8)
    r = (((p >> 16) & 255) + ((_s8v(m) * g) >> 5)) & 255
    b = ((p & 255) + ((_s8v(m >> 8) * g) >> 5) + ((_s8v(m >> 16) * _s8v(r)) >> 5)) & 255
    d[:] = ((p & 0xFF00FF00) | (r << 16) | b).tolist()


def _inv_green(d):
    p = np.array(d, dtype=np.int64)
    g = (p >> 8) & 255
    d[:] = ((p & 0xFF00FF00) | ((((p >> 16) + g) & 255) << 16) | ((p + g) & 255)).tolist()


def _inv_palette(d, w, h, bits, pal):
    """d: h rows of subsize(w, bits) words -> h rows of w words"""
    pw = _subsize(w, bits)
    bpp = 8 >> bits
    mask = (1 << bpp) - 1
    per = 1 << bits
    ys, xs = np.mgrid[0:h, 0:w]
    idx = (((np.array(d, dtype=np.int64)[ys * pw + (xs >> bits)] >> 8) & 255) >> ((xs & (per - 1)) * bpp)) & mask
    table = np.zeros(256, dtype=np.int64)   # an index past the palette gives 0
    table[:len(pal)] = pal
    return table[idx].reshape(-1).tolist()


def decode_argb(payload, w, h):
    br = _Bits(payload)
    br.pos = 40
    transforms = []
    seen = set()
    xs = w
    while br.read(1):
        t = br.read(2)
        if t in seen:
            raise Corrupt("a transform repeated")
        seen.add(t)
        if t < 2:
            bits = br.read(3) + 2
            transforms.append((t, xs, bits, _image(br, _subsize(xs, bits), _subsize(h, bits), False)))
        elif t == 2:
            transforms.append((2, xs, 0, None))
        else:
            nc = br.read(8) + 1
            bits = 0 if nc > 16 else 1 if nc > 4 else 2 if nc > 2 else 3
            pal = _image(br, nc, 1, False)
            for i in range(1, nc):
                pal[i] = _add(pal[i], pal[i - 1])
            transforms.append((3, xs, bits, pal))
            xs = _subsize(xs, bits)
        br.check()
    d = _image(br, xs, h, True)
    for t, tw, bits, sub in reversed(transforms):
        if t == 0:
            _inv_predictor(d, tw, h, bits, sub)
        elif t == 1:
            _inv_cross(d, tw, h, bits, sub)
        elif t == 2:
            _inv_green(d)
        else:
            d = _inv_palette(d, tw, h, bits, sub)
    return d


def decode(data):
    data = bytes(data)
    rc, info, _, span = probe_span(data)
    if rc:
        return rc, None
    w, h = info["width"], info["height"]
    try:
        d = decode_argb(data[span[0]:span[0] + span[1]], w, h)
    except Corrupt:
        return -1, None
    except Unread:
        return -2, None
    a = np.array(d, dtype=np.uint32).reshape(h, w)
    return 0, np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255], axis=-1).astype(np.uint8)
