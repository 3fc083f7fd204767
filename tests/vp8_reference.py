"""A plain-Python restatement of the whole lossy-WebP (VP8 key frame) decode with its acceptance rules, written from the format and
from libwebp's behaviour, not from csrc/vp8_dec.h: byte-wise boolean decoder, flat bytearrays, the loop filter and the transforms in
Python integers.  decode(data) -> (status, reason, pixels): status 0 with uint8 [H, W, 3] pixels, which tests/test_vp8_reference.py holds
to Pillow's; or -1 / -2 with a reason from the lists of the README row (pixels None).  It decides the damage sweep: the host build and the
device must give its status file for file.  The constant tables are those of csrc/vp8_tables.h (tests/test_vp8_tables.py holds them to
libwebp's); the container walk of lossless files is webp_reference.probe."""
import functools
import struct

import numpy as np

import vp8_writer as W
import webp_reference as wr

T = W.T
DCQ, ACQ, ZIGZAG, BANDS = T["vp8_dc_q"], T["vp8_ac_q"], T["vp8_zigzag"], T["vp8_bands"]
COEF_DEFAULT, COEF_UPDATE, BMODE_P, TREE, CATS = W.COEF_DEFAULT, W.COEF_UPDATE, W.BMODE_P, W.TREE, W.CATS
MAX_BLOCK_SUM, MAX_Y2_SUM = 19000, 32764
MAX_PIXELS, MAX_CHUNK = 1 << 26, 1 << 28

R_PAST_FIRST = "read past the end of the first partition"
R_PAST_TOKEN = "read past the end of a token partition"
R_FF = "partition begins outside the boolean coder's interval"
R_BOUND = "block beyond the coefficient bound"
DECODE_REASONS = (R_PAST_FIRST, R_PAST_TOKEN, R_FF, R_BOUND)
PROBE_REASONS_1 = (
    "VP8 chunk shorter than the frame tag", "VP8 inter frame", "VP8 profile above 3", "VP8 show_frame is 0", "VP8 start code is not 9d 01 2a",
    "VP8 frame of zero width or height", "VP8 first partition past the chunk", "VP8 partition-size table past the chunk",
    "VP8 token partition past the chunk", "VP8 last token partition is empty", "VP8 frame header past the first partition",
    "VP8 first partition begins outside the boolean coder's interval", "second VP8 chunk", "both a VP8 and a VP8L chunk",
    "VP8X canvas differs from the VP8 frame header")
PROBE_REASONS_2 = ("lossy WebP with an ALPH chunk", "animated WebP", "more than 2^26 pixels", "VP8 chunk of 256 MB or more")


class Bool:
    """the boolean decoder: a byte is loaded only when a decision needs it; `over` bit 0: a byte was needed that the partition does not
    have; bit 1: the partition begins with 0xFF (the code value lies outside the interval)"""
    __slots__ = ("s", "pos", "end", "value", "range", "bits", "over")

    def __init__(self, s, start, end):
        self.s, self.pos, self.end, self.value, self.range, self.bits = s, start, end, 0, 255, -8
        self.over = 2 if start < end and s[start] == 0xFF else 0

    def bit(self, prob):
        if self.bits < 0:
            if self.pos < self.end:
                self.value = (self.value << 8) | self.s[self.pos]
                self.pos += 1
            else:
                self.over |= 1
                self.value <<= 8
            self.bits += 8
        split = ((self.range - 1) * prob) >> 8
        if (self.value >> self.bits) > split:
            self.range -= split + 1
            self.value -= (split + 1) << self.bits
            b = 1
        else:
            self.range = split + 1
            b = 0
        shift = 8 - self.range.bit_length()
        if shift > 0:
            self.range <<= shift
            self.bits -= shift
        return b

    def get(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit(128)
        return v

    def signed(self, n):
        v = self.get(n)
        return -v if self.bit(128) else v


def _clip(v, hi):
    return 0 if v < 0 else hi if v > hi else v


@functools.lru_cache(maxsize=64)
def _parse_first_partition(s, part0):
    """the frame header and every macroblock's modes from the first partition s[10:10 + part0] (cached: most damaged files of a sweep
    share it) -> (frame dict, reason or None)"""
    w, h = (s[6] | (s[7] << 8)) & 0x3FFF, (s[8] | (s[9] << 8)) & 0x3FFF
    mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
    b = Bool(s, 10, 10 + part0)
    if b.over:
        return None, "VP8 first partition begins outside the boolean coder's interval"
    b.get(2)
    F = dict(width=w, height=h, mbw=mbw, mbh=mbh)
    quant, fstr, absolute, update_map, seg_p = [0] * 4, [0] * 4, 1, 0, [255] * 3
    use_segment = b.get(1)
    if use_segment:
        update_map = b.get(1)
        if b.get(1):
            absolute = b.get(1)
            quant = [b.signed(7) if b.get(1) else 0 for _ in range(4)]
            fstr = [b.signed(6) if b.get(1) else 0 for _ in range(4)]
        if update_map:
            seg_p = [b.get(8) if b.get(1) else 255 for _ in range(3)]
    simple, level, sharp, use_delta = b.get(1), b.get(6), b.get(3), b.get(1)
    ref0 = mode0 = 0
    if use_delta and b.get(1):
        ref = [b.signed(6) if b.get(1) else 0 for _ in range(4)]
        mode = [b.signed(6) if b.get(1) else 0 for _ in range(4)]
        ref0, mode0 = ref[0], mode[0]
    F["filter"] = 0 if level == 0 else 1 if simple else 2
    F["parts"] = 1 << b.get(2)
    base_q = b.get(7)
    d = [b.signed(4) if b.get(1) else 0 for _ in range(5)]
    F["dq"], F["fs"] = [], []
    for i in range(4):
        q = (quant[i] + (0 if absolute else base_q)) if use_segment else base_q
        y2ac = (ACQ[_clip(q + d[2], 127)] * 101581) >> 16
        F["dq"].append((DCQ[_clip(q + d[0], 127)], ACQ[_clip(q, 127)], 2 * DCQ[_clip(q + d[1], 127)], max(y2ac, 8),
                        DCQ[_clip(q + d[3], 117)], ACQ[_clip(q + d[4], 127)]))
        row = []
        for i4 in (0, 1):
            lv = (fstr[i] + (0 if absolute else level)) if use_segment else level
            if use_delta:
                lv += ref0 + (mode0 if i4 else 0)
            lv = _clip(lv, 63)
            if not F["filter"] or lv == 0:
                row.append((0, 0, 0))
                continue
            il = lv
            if sharp > 0:
                il >>= 2 if sharp > 4 else 1
                il = min(il, 9 - sharp)
            il = max(il, 1)
            row.append((2 * lv + il, il, 2 if lv >= 40 else 1 if lv >= 15 else 0))
        F["fs"].append(row)
    b.get(1)
    F["probs"] = [b.get(8) if b.bit(COEF_UPDATE[i]) else COEF_DEFAULT[i] for i in range(1056)]
    use_skip = b.get(1)
    skip_p = b.get(8) if use_skip else 0
    F["use_skip"] = use_skip
    if b.over:
        return None, "VP8 frame header past the first partition"
    F["after_header"] = (b.pos, b.value, b.range, b.bits)
    # the modes
    top = [0] * (4 * mbw)
    mbs = []
    for y in range(mbh):
        left = [0] * 4
        for x in range(mbw):
            seg = 0
            if update_map:
                seg = (2 + b.bit(seg_p[2])) if b.bit(seg_p[0]) else b.bit(seg_p[1])
            skip = b.bit(skip_p) if use_skip else 0
            if b.bit(145):
                ym = (1 if b.bit(128) else 3) if b.bit(156) else (2 if b.bit(163) else 0)
                sub = None
                top[4 * x:4 * x + 4] = [ym] * 4
                left = [ym] * 4
            else:
                ym, sub = None, [0] * 16
                for by in range(4):
                    for bx in range(4):
                        pr = (top[4 * x + bx] * 10 + left[by]) * 9
                        i = TREE[b.bit(BMODE_P[pr])]
                        while i > 0:
                            i = TREE[2 * i + b.bit(BMODE_P[pr + i])]
                        sub[4 * by + bx] = top[4 * x + bx] = left[by] = -i
            uv = 0 if not b.bit(142) else 2 if not b.bit(114) else 1 if b.bit(183) else 3
            mbs.append((seg, skip, ym, sub, uv))
        if b.over:
            F["modes_reason"] = R_PAST_FIRST
            break
    F["mbs"] = mbs
    return F, None


def probe(data):
    """-> (status, info, reason), the restatement of lumina_ocr_webp_probe_lossy: info = width, height, alpha, vp8x, exif, xmp, lossy,
    partitions; on a lossy file of status 0 also the payload offset and length (keys off, len)"""
    rc, info, reason = wr.probe(data)
    info = dict(info, lossy=0, partitions=0)
    if rc != -2 or reason != "lossy WebP (VP8)":
        return rc, info, reason
    if info["vp8x"]:
        have, lossless, refused, p = 0, 0, None, 30
        while p < len(data):
            tag, size = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
            if tag == b"VP8 ":
                if have:
                    return -1, info, "second VP8 chunk"
                have, off, ln = 1, p + 8, size
            elif tag == b"VP8L":
                lossless = 1
            elif tag == b"ALPH":
                refused = refused or "lossy WebP with an ALPH chunk"
            elif tag in (b"ANIM", b"ANMF"):
                refused = refused or "animated WebP"
            p += 8 + size + (size & 1)
        if lossless:
            return -1, info, "both a VP8 and a VP8L chunk"
        if refused:
            return -2, info, refused
    else:
        off, ln = 20, struct.unpack("<I", data[16:20])[0]
    s = bytes(data[off:off + ln])
    if ln < 10:
        return -1, info, "VP8 chunk shorter than the frame tag"
    tag = s[0] | (s[1] << 8) | (s[2] << 16)
    if tag & 1:
        return -1, info, "VP8 inter frame"
    if ((tag >> 1) & 7) > 3:
        return -1, info, "VP8 profile above 3"
    if not (tag >> 4) & 1:
        return -1, info, "VP8 show_frame is 0"
    part0 = tag >> 5
    if s[3:6] != b"\x9d\x01\x2a":
        return -1, info, "VP8 start code is not 9d 01 2a"
    w, h = (s[6] | (s[7] << 8)) & 0x3FFF, (s[8] | (s[9] << 8)) & 0x3FFF
    if w == 0 or h == 0:
        return -1, info, "VP8 frame of zero width or height"
    if part0 > ln - 10:
        return -1, info, "VP8 first partition past the chunk"
    # (the order of the checks is the device's: the boolean-coded header is read up to the partition count, then the table is checked)
    F, why = _parse_first_partition(s[:10 + part0], part0)
    if why == "VP8 first partition begins outside the boolean coder's interval":
        return -1, info, why
    parts = F["parts"] if F else _parts_only(s, part0)
    start = 10 + part0
    if ln - start < 3 * (parts - 1):
        return -1, info, "VP8 partition-size table past the chunk"
    p, table = start + 3 * (parts - 1), []
    for k in range(parts - 1):
        size = s[start + 3 * k] | (s[start + 3 * k + 1] << 8) | (s[start + 3 * k + 2] << 16)
        if size > ln - p:
            return -1, info, "VP8 token partition past the chunk"
        table.append((p, p + size))
        p += size
    if p >= ln:
        return -1, info, "VP8 last token partition is empty"
    table.append((p, ln))
    if why:
        return -1, info, why
    info.update(width=w, height=h, alpha=0)
    if info["vp8x"]:
        cw = 1 + (data[24] | (data[25] << 8) | (data[26] << 16))
        ch = 1 + (data[27] | (data[28] << 8) | (data[29] << 16))
        if (cw, ch) != (w, h):
            return -1, info, "VP8X canvas differs from the VP8 frame header"
    if w * h > MAX_PIXELS:
        return -2, info, "more than 2^26 pixels"
    if ln >= MAX_CHUNK:
        return -2, info, "VP8 chunk of 256 MB or more"
    info.update(lossy=1, partitions=parts, off=off, len=ln, table=table, part0=part0)
    return 0, info, ""


def _parts_only(s, part0):
    """the partition count of a header that reads past its partition later on (zeros are fed, as the device feeds them)"""
    b = Bool(s, 10, 10 + part0)
    b.get(2)
    if b.get(1):
        um = b.get(1)
        if b.get(1):
            b.get(1)
            for n in (7,) * 4 + (6,) * 4:
                if b.get(1):
                    b.signed(n)
        if um:
            for _ in range(3):
                if b.get(1):
                    b.get(8)
    b.get(10)
    if b.get(1) and b.get(1):
        for _ in range(8):
            if b.get(1):
                b.signed(6)
    return 1 << b.get(2)


def _coeffs(b, probs, t, ctx, dcq, acq, n, out, base):
    """-> (position after the last non-zero coefficient, sum of |dequantised values|)"""
    tb = t * 264
    p = tb + (BANDS[n] * 3 + ctx) * 11
    total = 0
    while n < 16:
        if not b.bit(probs[p]):
            return n, total
        while not b.bit(probs[p + 1]):
            n += 1
            p = tb + BANDS[n] * 33
            if n == 16:
                return 16, total
        nxt = tb + BANDS[n + 1] * 33
        if not b.bit(probs[p + 2]):
            v, pn = 1, nxt + 11
        else:
            if not b.bit(probs[p + 3]):
                v = 2 if not b.bit(probs[p + 4]) else 3 + b.bit(probs[p + 5])
            elif not b.bit(probs[p + 6]):
                if not b.bit(probs[p + 7]):
                    v = 5 + b.bit(159)
                else:
                    v = 7 + 2 * b.bit(165)
                    v += b.bit(145)
            else:
                b1 = b.bit(probs[p + 8])
                cat = 2 * b1 + b.bit(probs[p + 9 + b1])
                v = 0
                for pr in CATS[cat]:
                    v = 2 * v + b.bit(pr)
                v += 3 + (8 << cat)
            pn = nxt + 22
        c = v * (acq if n else dcq)
        total += c
        out[base + ZIGZAG[n]] = -c if b.bit(128) else c
        p = pn
        n += 1
    return 16, total


def _tokens(F, s, table):
    """-> (coefficients per macroblock (list of 384 or None), non-zero masks, inner flags), or a reason"""
    mbw, mbh, parts, probs = F["mbw"], F["mbh"], F["parts"], F["probs"]
    readers = [Bool(s, a, e) for a, e in table]
    if any(r.over for r in readers[:min(parts, mbh)]):
        return R_FF
    tnz, tdc = [0] * mbw, [0] * mbw
    coefs, masks, inner = [], [], []
    bad = False
    for y in range(mbh):
        b = readers[y & (parts - 1)]
        lnz = ldc = 0
        for x in range(mbw):
            seg, skip, ym, sub, uv = F["mbs"][y * mbw + x]
            i4 = sub is not None
            if F["use_skip"] and skip:
                tnz[x] = lnz = 0
                if not i4:
                    tdc[x] = ldc = 0
                coefs.append(None); masks.append(0); inner.append(1 if i4 else 0)
                continue
            q = F["dq"][seg]
            c = [0] * 384
            first, t = 0, 3
            if not i4:
                y2 = [0] * 16
                nz, s2 = _coeffs(b, probs, 1, tdc[x] + ldc, q[2], q[3], 0, y2, 0)
                tdc[x] = ldc = 1 if nz > 0 else 0
                bad |= s2 > MAX_Y2_SUM
                if nz > 0:
                    tmp = [0] * 16
                    for i in range(4):
                        a0, a1, a2, a3 = y2[i] + y2[12 + i], y2[4 + i] + y2[8 + i], y2[4 + i] - y2[8 + i], y2[i] - y2[12 + i]
                        tmp[i], tmp[8 + i], tmp[4 + i], tmp[12 + i] = a0 + a1, a0 - a1, a3 + a2, a3 - a2
                    for i in range(4):
                        dc = tmp[4 * i] + 3
                        a0, a1, a2, a3 = dc + tmp[4 * i + 3], tmp[4 * i + 1] + tmp[4 * i + 2], tmp[4 * i + 1] - tmp[4 * i + 2], dc - tmp[4 * i + 3]
                        c[64 * i], c[64 * i + 16], c[64 * i + 32], c[64 * i + 48] = (a0 + a1) >> 3, (a3 + a2) >> 3, (a0 - a1) >> 3, (a3 - a2) >> 3
                first, t = 1, 0
            mask = 0
            tn, ln = tnz[x], lnz
            new_t = new_l = 0
            for by in range(4):
                for bx in range(4):
                    k = 4 * by + bx
                    ctx = ((ln >> by) & 1) + ((tn >> bx) & 1)
                    nz, total = _coeffs(b, probs, t, ctx, q[0], q[1], first, c, 16 * k)
                    bad |= total + (abs(c[16 * k]) if first else 0) > MAX_BLOCK_SUM
                    f = 1 if nz > first else 0
                    ln = (ln & ~(1 << by)) | (f << by)
                    tn = (tn & ~(1 << bx)) | (f << bx)
                    if nz > 1 or c[16 * k]:
                        mask |= 1 << k
            for ch in (0, 1):
                for by in range(2):
                    for bx in range(2):
                        k = 16 + 4 * ch + 2 * by + bx
                        bt, bl = 4 + 2 * ch + bx, 4 + 2 * ch + by
                        ctx = ((ln >> bl) & 1) + ((tn >> bt) & 1)
                        nz, total = _coeffs(b, probs, 2, ctx, q[4], q[5], 0, c, 16 * k)
                        bad |= total > MAX_BLOCK_SUM
                        f = 1 if nz > 0 else 0
                        ln = (ln & ~(1 << bl)) | (f << bl)
                        tn = (tn & ~(1 << bt)) | (f << bt)
                        if nz > 1 or c[16 * k]:
                            mask |= 1 << k
            tnz[x], lnz = tn, ln
            coefs.append(c); masks.append(mask); inner.append(1 if (i4 or mask) else 0)
        if b.over:
            return R_PAST_TOKEN
        if bad:
            return R_BOUND
    return coefs, masks, inner


def _c8(v):
    return 0 if v < 0 else 255 if v > 255 else v


def _m1(a):
    return ((a * 20091) >> 16) + a


def _m2(a):
    return (a * 35468) >> 16


def _store(P, st, x0, y0, pred, c, base):
    if c is None:
        for j in range(4):
            o = (y0 + j) * st + x0
            P[o:o + 4] = bytes(pred[4 * j:4 * j + 4])
        return
    t = [0] * 16
    for i in range(4):
        a, bb = c[base + i] + c[base + 8 + i], c[base + i] - c[base + 8 + i]
        cc, d = _m2(c[base + 4 + i]) - _m1(c[base + 12 + i]), _m1(c[base + 4 + i]) + _m2(c[base + 12 + i])
        t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3] = a + d, bb + cc, bb - cc, a - d
    for i in range(4):
        dc = t[i] + 4
        a, bb = dc + t[8 + i], dc - t[8 + i]
        cc, d = _m2(t[4 + i]) - _m1(t[12 + i]), _m1(t[4 + i]) + _m2(t[12 + i])
        o = (y0 + i) * st + x0
        P[o] = _c8(pred[4 * i] + ((a + d) >> 3)); P[o + 1] = _c8(pred[4 * i + 1] + ((bb + cc) >> 3))
        P[o + 2] = _c8(pred[4 * i + 2] + ((bb - cc) >> 3)); P[o + 3] = _c8(pred[4 * i + 3] + ((a - d) >> 3))


def _px(P, st, x, y):
    return 127 if y < 0 else 129 if x < 0 else P[y * st + x]


def _pred_mb(P, st, mx, my, n, mode, bx, by):
    x0, y0 = mx + 4 * bx, my + 4 * by
    if mode == 0:
        if mx == 0 and my == 0:
            dc = 128
        else:
            total = 0
            sh = 4 if n == 16 else 3
            if my > 0:
                total += sum(P[(my - 1) * st + mx:(my - 1) * st + mx + n])
            if mx > 0:
                total += sum(P[(my + i) * st + mx - 1] for i in range(n))
            dc = (total + n) >> (sh + 1) if (mx > 0 and my > 0) else (total + (n >> 1)) >> sh
        return [dc] * 16
    if mode == 2:
        return [_px(P, st, x0 + i, my - 1) for i in range(4)] * 4
    if mode == 3:
        return [v for j in range(4) for v in [_px(P, st, mx - 1, y0 + j)] * 4]
    tl = _px(P, st, mx - 1, my - 1)
    tp = [_px(P, st, x0 + i, my - 1) for i in range(4)]
    return [_c8(tp[i] + _px(P, st, mx - 1, y0 + j) - tl) for j in range(4) for i in range(4)]


def _a3(a, b, c):
    return (a + 2 * b + c + 2) >> 2


def _a2(a, b):
    return (a + b + 1) >> 1


def _pred_sub(P, st, mx, my, last, mode, bx, by):
    x0, y0 = mx + 4 * bx, my + 4 * by
    I, J, K, L = (_px(P, st, x0 - 1, y0 + i) for i in range(4))
    X = _px(P, st, x0 - 1, y0 - 1)
    A, B, C, D = (_px(P, st, x0 + i, y0 - 1) for i in range(4))
    ty = my - 1 if (by == 0 or bx == 3) else y0 - 1
    E, F, G, H = (_px(P, st, mx + 15 if (bx == 3 and last) else x0 + 4 + i, ty) for i in range(4))
    e = [L, K, J, I, X, A, B, C, D, E, F, G, H]
    p = [0] * 16
    if mode == 0:
        return [(A + B + C + D + I + J + K + L + 4) >> 3] * 16
    if mode == 1:
        return [_c8(e[5 + i] + e[3 - j] - X) for j in range(4) for i in range(4)]
    if mode == 2:
        return [_a3(X, A, B), _a3(A, B, C), _a3(B, C, D), _a3(C, D, E)] * 4
    if mode == 3:
        return [v for r in (_a3(X, I, J), _a3(I, J, K), _a3(J, K, L), _a3(K, L, L)) for v in [r] * 4]
    if mode == 4:
        return [_a3(e[3 - j + i], e[4 - j + i], e[5 - j + i]) for j in range(4) for i in range(4)]
    if mode == 6:
        return [_a3(e[5 + i + j], e[6 + i + j], e[min(i + j + 7, 12)]) for j in range(4) for i in range(4)]

    def put(v, *xy):
        for x, y in xy:
            p[4 * y + x] = v
    if mode == 5:
        put(_a2(X, A), (0, 0), (1, 2)); put(_a2(A, B), (1, 0), (2, 2)); put(_a2(B, C), (2, 0), (3, 2)); put(_a2(C, D), (3, 0))
        put(_a3(K, J, I), (0, 3)); put(_a3(J, I, X), (0, 2)); put(_a3(I, X, A), (0, 1), (1, 3)); put(_a3(X, A, B), (1, 1), (2, 3))
        put(_a3(A, B, C), (2, 1), (3, 3)); put(_a3(B, C, D), (3, 1))
    elif mode == 7:
        put(_a2(A, B), (0, 0)); put(_a2(B, C), (1, 0), (0, 2)); put(_a2(C, D), (2, 0), (1, 2)); put(_a2(D, E), (3, 0), (2, 2))
        put(_a3(A, B, C), (0, 1)); put(_a3(B, C, D), (1, 1), (0, 3)); put(_a3(C, D, E), (2, 1), (1, 3)); put(_a3(D, E, F), (3, 1), (2, 3))
        put(_a3(E, F, G), (3, 2)); put(_a3(F, G, H), (3, 3))
    elif mode == 9:
        put(_a2(I, J), (0, 0)); put(_a2(J, K), (2, 0), (0, 1)); put(_a2(K, L), (2, 1), (0, 2))
        put(_a3(I, J, K), (1, 0)); put(_a3(J, K, L), (3, 0), (1, 1)); put(_a3(K, L, L), (3, 1), (1, 2))
        put(L, (3, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3))
    else:
        put(_a2(I, X), (0, 0), (2, 1)); put(_a2(J, I), (0, 1), (2, 2)); put(_a2(K, J), (0, 2), (2, 3)); put(_a2(L, K), (0, 3))
        put(_a3(A, B, C), (3, 0)); put(_a3(X, A, B), (2, 0)); put(_a3(I, X, A), (1, 0), (3, 1)); put(_a3(J, I, X), (1, 1), (3, 2))
        put(_a3(K, J, I), (1, 2), (3, 3)); put(_a3(L, K, J), (1, 3))
    return p


def _filter_line(P, o, s, thresh, it, hev, kind):
    """kind 0: simple; 1: a macroblock edge of the normal filter; 2: an inner edge"""
    p1, p0, q0, q1 = P[o - 2 * s], P[o - s], P[o], P[o + s]
    if 4 * abs(p0 - q0) + abs(p1 - q1) > 2 * thresh + 1:
        return
    sc1 = lambda v: -128 if v < -128 else 127 if v > 127 else v
    sc2 = lambda v: -16 if v < -16 else 15 if v > 15 else v
    if kind:
        p3, p2, q2, q3 = P[o - 4 * s], P[o - 3 * s], P[o + 2 * s], P[o + 3 * s]
        if abs(p3 - p2) > it or abs(p2 - p1) > it or abs(p1 - p0) > it or abs(q3 - q2) > it or abs(q2 - q1) > it or abs(q1 - q0) > it:
            return
    if kind == 0 or abs(p1 - p0) > hev or abs(q1 - q0) > hev:
        a = 3 * (q0 - p0) + sc1(p1 - q1)
        P[o - s], P[o] = _c8(p0 + sc2((a + 3) >> 3)), _c8(q0 - sc2((a + 4) >> 3))
    elif kind == 2:
        a = 3 * (q0 - p0)
        a1, a2 = sc2((a + 4) >> 3), sc2((a + 3) >> 3)
        a3 = (a1 + 1) >> 1
        P[o - 2 * s], P[o - s], P[o], P[o + s] = _c8(p1 + a3), _c8(p0 + a2), _c8(q0 - a1), _c8(q1 - a3)
    else:
        a = sc1(3 * (q0 - p0) + sc1(p1 - q1))
        a1, a2, a3 = (27 * a + 63) >> 7, (18 * a + 63) >> 7, (9 * a + 63) >> 7
        P[o - 3 * s], P[o - 2 * s], P[o - s] = _c8(p2 + a3), _c8(p1 + a2), _c8(p0 + a1)
        P[o], P[o + s], P[o + 2 * s] = _c8(q0 - a1), _c8(q1 - a2), _c8(q2 - a3)


def _filter_mb(F, planes, x, y, fs, inner):
    limit, il, hev = fs
    if not limit:
        return
    simple = F["filter"] == 1
    for P, st, n in planes[:1] if simple else planes:
        o0 = (n * y) * st + n * x
        if x > 0:
            for i in range(n):
                _filter_line(P, o0 + i * st, 1, limit + 4, il, hev, 0 if simple else 1)
        if inner:
            for e in range(4, n, 4):
                for i in range(n):
                    _filter_line(P, o0 + i * st + e, 1, limit, il, hev, 0 if simple else 2)
        if y > 0:
            for i in range(n):
                _filter_line(P, o0 + i, st, limit + 4, il, hev, 0 if simple else 1)
        if inner:
            for e in range(4, n, 4):
                for i in range(n):
                    _filter_line(P, o0 + e * st + i, st, limit, il, hev, 0 if simple else 2)


def _rgb(F, Y, U, V):
    w, h, ys, uvs = F["width"], F["height"], 16 * F["mbw"], 8 * F["mbw"]
    y = np.frombuffer(bytes(Y), np.uint8).reshape(-1, ys)[:h, :w].astype(np.int64)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    xs, yy = np.arange(w), np.arange(h)
    cx, cy = xs >> 1, yy >> 1
    nx = np.clip(np.where(xs & 1, cx + 1, cx - 1), 0, cw - 1)
    ny = np.clip(np.where(yy & 1, cy + 1, cy - 1), 0, ch - 1)
    out = []
    for C in (U, V):
        c = np.frombuffer(bytes(C), np.uint8).reshape(-1, uvs)[:ch, :cw].astype(np.int64)
        out.append((9 * c[cy][:, cx] + 3 * c[cy][:, nx] + 3 * c[ny][:, cx] + c[ny][:, nx] + 8) >> 4)
    u, v = out
    yk = (y * 19077) >> 8
    clip = lambda t: np.where((t & ~16383) == 0, t >> 6, np.where(t < 0, 0, 255))
    r = clip(yk + ((v * 26149) >> 8) - 14234)
    g = clip(yk - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708)
    b = clip(yk + ((u * 33050) >> 8) - 17685)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


def decode(data):
    """-> (status, reason, uint8 [H, W, 3] or None); a lossless file gives webp_reference's decode"""
    rc, info, reason = probe(data)
    if rc:
        return rc, reason, None
    if not info["lossy"]:
        rc, px = wr.decode(data)
        return rc, "", px
    s = bytes(data[info["off"]:info["off"] + info["len"]])
    F, _ = _parse_first_partition(s[:10 + info["part0"]], info["part0"])
    if "modes_reason" in F:
        return -1, F["modes_reason"], None
    tok = _tokens(F, s, info["table"])
    if isinstance(tok, str):
        return -1, tok, None
    coefs, masks, inner = tok
    mbw, mbh = F["mbw"], F["mbh"]
    ys, uvs = 16 * mbw, 8 * mbw
    Y, U, V = bytearray(ys * 16 * mbh), bytearray(uvs * 8 * mbh), bytearray(uvs * 8 * mbh)
    for y in range(mbh):
        for x in range(mbw):
            i = y * mbw + x
            seg, skip, ym, sub, uv = F["mbs"][i]
            c, mask = coefs[i], masks[i]
            for k in range(16):
                bx, by = k & 3, k >> 2
                pred = _pred_mb(Y, ys, 16 * x, 16 * y, 16, ym, bx, by) if sub is None else _pred_sub(Y, ys, 16 * x, 16 * y, x == mbw - 1, sub[k], bx, by)
                _store(Y, ys, 16 * x + 4 * bx, 16 * y + 4 * by, pred, c if (mask >> k) & 1 else None, 16 * k)
            for k in range(8):
                P = U if k < 4 else V
                bx, by = k & 1, (k >> 1) & 1
                pred = _pred_mb(P, uvs, 8 * x, 8 * y, 8, uv, bx, by)
                _store(P, uvs, 8 * x + 4 * bx, 8 * y + 4 * by, pred, c if (mask >> (16 + k)) & 1 else None, 16 * (16 + k))
    if F["filter"]:
        planes = [(Y, ys, 16), (U, uvs, 8), (V, uvs, 8)]
        for y in range(mbh):
            for x in range(mbw):
                i = y * mbw + x
                seg, skip, ym, sub, uv = F["mbs"][i]
                _filter_mb(F, planes, x, y, F["fs"][seg][1 if sub is not None else 0], inner[i])
    return 0, "", _rgb(F, Y, U, V)
