"""A test-side VP8 key-frame writer in the manner of webp_writer.py: a boolean encoder that emits chosen frame-header fields, chosen
modes and chosen quantised coefficient levels, so that the tests reach what libwebp's encoder never writes (the simple filter, sharpness,
loop-filter deltas, 2 / 4 / 8 token partitions, segment data without a map and the reverse, every mode on every border, every token
category, coefficient-probability updates, scale / colour-space / clamp bits).  No rate control, no prediction search: the pictures are
whatever the chosen modes and levels decode to, and the expectation is Pillow's decode of the file.

The tables are read from csrc/vp8_tables.h (tests/test_vp8_tables.py holds those to libwebp's)."""
import re
import struct
from pathlib import Path

import numpy as np

_HEADER = Path(__file__).resolve().parent.parent / "ocr-system_amd" / "csrc" / "vp8_tables.h"


def _tables():
    out = {}
    for m in re.finditer(r"VP8_HD int (\w+)\(int i\) \{\s*constexpr (\w+) t\[(\d+)\] = \{([^}]*)\}", _HEADER.read_text()):
        out[m.group(1)] = [int(v) for v in m.group(4).replace("\n", " ").split(",") if v.strip()]
    return out


T = _tables()
COEF_DEFAULT, COEF_UPDATE, BMODE_P, TREE = T["vp8_coef_default"], T["vp8_coef_update"], T["vp8_bmode_proba"], T["vp8_bmode_tree"]
BANDS, CATS = T["vp8_bands"], [T["vp8_cat3"][:-1], T["vp8_cat4"][:-1], T["vp8_cat5"][:-1], T["vp8_cat6"][:-1]]
DC, TM, VE, HE = 0, 1, 2, 3   # the four 16x16 / chroma modes; 4x4 sub-modes are 0..9 (DC TM VE HE RD VR LD VL HD HU)


def _tree_paths():
    """mode -> [(probability index, bit)]: node i reads prob[i] and goes on at tree[2 i + bit] (the root is node 0)"""
    paths = {}

    def rec(i, path):
        for bit in (0, 1):
            nxt = TREE[2 * i + bit]
            if nxt <= 0:
                paths[-nxt] = path + [(i, bit)]
            else:
                rec(nxt, path + [(i, bit)])
    rec(0, [])
    return paths


BMODE_PATHS = _tree_paths()


class BoolEncoder:
    """exact integers: `low` carries 8 + nbits bits of the code value"""
    def __init__(self):
        self.low, self.range, self.nbits = 0, 255, 0

    def put(self, prob, bit):
        split = 1 + (((self.range - 1) * prob) >> 8)
        if bit:
            self.low += split
            self.range -= split
        else:
            self.range = split
        while self.range < 128:
            self.range <<= 1
            self.low <<= 1
            self.nbits += 1

    def value(self, v, n):
        for k in range(n - 1, -1, -1):
            self.put(128, (v >> k) & 1)

    def signed(self, v, n):
        self.value(abs(v), n)
        self.put(128, 1 if v < 0 else 0)

    def optional_signed(self, v, n):
        """a flag and the value, or the flag alone for None"""
        self.put(128, 0 if v is None else 1)
        if v is not None:
            self.signed(v, n)

    def bytes(self):
        total = 8 + self.nbits
        pad = (-total) % 8
        return (self.low << pad).to_bytes((total + pad) // 8, "big")


def _put_large(e, p, v):
    if v <= 4:
        e.put(p[3], 0)
        if v == 2:
            e.put(p[4], 0)
        else:
            e.put(p[4], 1); e.put(p[5], v - 3)
    elif v <= 10:
        e.put(p[3], 1); e.put(p[6], 0)
        if v <= 6:
            e.put(p[7], 0); e.put(159, v - 5)
        else:
            e.put(p[7], 1); e.put(165, (v - 7) >> 1); e.put(145, (v - 7) & 1)
    else:
        cat = 0 if v <= 18 else 1 if v <= 34 else 2 if v <= 66 else 3
        assert v <= 2114
        e.put(p[3], 1); e.put(p[6], 1)
        e.put(p[8], cat >> 1); e.put(p[9 + (cat >> 1)], cat & 1)
        extra, tab = v - (3 + (8 << cat)), CATS[cat]
        for k, pr in enumerate(tab):
            e.put(pr, (extra >> (len(tab) - 1 - k)) & 1)


def _put_coeffs(e, probs, t, ctx, first, levels):
    """levels: 16 quantised levels in zig-zag order; -> 1 if any level from `first` on is non-zero"""
    P = lambda n, c: probs[((t * 8 + BANDS[n]) * 3 + c) * 11:((t * 8 + BANDS[n]) * 3 + c) * 11 + 11]
    last = max([k for k in range(first, 16) if levels[k]] or [-1])
    n, p = first, P(first, ctx)
    while n < 16:
        if n > last:
            e.put(p[0], 0)
            break
        e.put(p[0], 1)
        while levels[n] == 0:
            e.put(p[1], 0)
            n += 1
            p = P(n, 0)
        e.put(p[1], 1)
        v = abs(levels[n])
        if v == 1:
            e.put(p[2], 0)
        else:
            e.put(p[2], 1)
            _put_large(e, p, v)
        e.put(128, 1 if levels[n] < 0 else 0)
        n += 1
        p = P(n, 1 if v == 1 else 2)
    return 1 if last >= first else 0


def write_vp8(width, height, mbs, *, base_q=40, dq=(None,) * 5, segments=None, simple=False, level=0, sharpness=0, lf_delta=None,
              log2_parts=0, skip_prob=None, coef_updates=None, color_space=0, clamp=0, scale=(0, 0), profile=0, vp8x=False, extra_chunks=()):
    """mbs: one dict per macroblock in raster order: seg (0..3), skip (0 / 1, used with skip_prob), i4 (0 / 1), ymode or sub (16 modes),
    uvmode, and the levels (absent: zero): y2 (16), y (16 x 16), u (4 x 16), v (4 x 16), each block in zig-zag order.
    segments: None or dict(update_map, probs (3, None = 255), data = None or dict(absolute, quant (4, None = absent), level (4))).
    lf_delta: None or dict(update, ref (4, None = no update), mode (4)).  -> the RIFF / WEBP file"""
    mbw, mbh = (width + 15) >> 4, (height + 15) >> 4
    assert len(mbs) == mbw * mbh
    h = BoolEncoder()
    h.put(128, color_space); h.put(128, clamp)
    update_map = 0
    h.put(128, 1 if segments else 0)
    seg_p = [255, 255, 255]
    if segments:
        update_map = 1 if segments.get("update_map") else 0
        h.put(128, update_map)
        data = segments.get("data")
        h.put(128, 1 if data else 0)
        if data:
            h.put(128, data["absolute"])
            for v in data["quant"]:
                h.optional_signed(v, 7)
            for v in data["level"]:
                h.optional_signed(v, 6)
        if update_map:
            for k, v in enumerate(segments.get("probs", (None,) * 3)):
                h.put(128, 0 if v is None else 1)
                if v is not None:
                    h.value(v, 8)
                    seg_p[k] = v
    h.put(128, 1 if simple else 0); h.value(level, 6); h.value(sharpness, 3)
    h.put(128, 1 if lf_delta else 0)
    if lf_delta:
        h.put(128, 1 if lf_delta["update"] else 0)
        if lf_delta["update"]:
            for v in list(lf_delta["ref"]) + list(lf_delta["mode"]):
                h.optional_signed(v, 6)
    h.value(log2_parts, 2)
    h.value(base_q, 7)
    for v in dq:
        h.optional_signed(v, 4)
    h.put(128, 0)   # refresh flag
    probs = list(COEF_DEFAULT)
    coef_updates = coef_updates or {}
    for i in range(1056):
        if i in coef_updates:
            h.put(COEF_UPDATE[i], 1); h.value(coef_updates[i], 8)
            probs[i] = coef_updates[i]
        else:
            h.put(COEF_UPDATE[i], 0)
    h.put(128, 0 if skip_prob is None else 1)
    if skip_prob is not None:
        h.value(skip_prob, 8)
    # modes (first partition) and tokens
    nparts = 1 << log2_parts
    parts = [BoolEncoder() for _ in range(nparts)]
    top_modes = [DC] * (4 * mbw)
    tnz_y, tnz_u, tnz_v, tdc = [0] * (4 * mbw), [0] * (2 * mbw), [0] * (2 * mbw), [0] * mbw
    zero = [0] * 16
    for my in range(mbh):
        left_modes = [DC] * 4
        lnz_y, lnz_u, lnz_v, ldc = [0] * 4, [0] * 2, [0] * 2, 0
        e = parts[my & (nparts - 1)]
        for mx in range(mbw):
            m = mbs[my * mbw + mx]
            if update_map:
                s = m.get("seg", 0)
                h.put(seg_p[0], s >> 1); h.put(seg_p[1 + (s >> 1)], s & 1)
            skip = m.get("skip", 0) if skip_prob is not None else 0
            if skip_prob is not None:
                h.put(skip_prob, skip)
            i4 = m.get("i4", 0)
            h.put(145, 0 if i4 else 1)
            if not i4:
                ym = m.get("ymode", DC)
                h.put(156, 1 if ym in (TM, HE) else 0)
                if ym in (TM, HE):
                    h.put(128, 1 if ym == TM else 0)
                else:
                    h.put(163, 1 if ym == VE else 0)
                top_modes[4 * mx:4 * mx + 4] = [ym] * 4
                left_modes = [ym] * 4
            else:
                for by in range(4):
                    for bx in range(4):
                        mode = m["sub"][4 * by + bx]
                        pr = (top_modes[4 * mx + bx] * 10 + left_modes[by]) * 9
                        for node, bit in BMODE_PATHS[mode]:
                            h.put(BMODE_P[pr + node], bit)
                        top_modes[4 * mx + bx] = left_modes[by] = mode
            uv = m.get("uvmode", DC)
            h.put(142, 0 if uv == DC else 1)
            if uv != DC:
                h.put(114, 0 if uv == VE else 1)
                if uv != VE:
                    h.put(183, 1 if uv == TM else 0)
            # tokens
            if skip:
                tnz_y[4 * mx:4 * mx + 4] = [0] * 4; lnz_y = [0] * 4
                tnz_u[2 * mx:2 * mx + 2] = [0] * 2; lnz_u = [0] * 2
                tnz_v[2 * mx:2 * mx + 2] = [0] * 2; lnz_v = [0] * 2
                if not i4:
                    tdc[mx] = ldc = 0
                continue
            first, t = 0, 3
            if not i4:
                nz = _put_coeffs(e, probs, 1, tdc[mx] + ldc, 0, m.get("y2", zero))
                tdc[mx] = ldc = nz
                first, t = 1, 0
            ylev = m.get("y", [zero] * 16)
            for by in range(4):
                for bx in range(4):
                    nz = _put_coeffs(e, probs, t, lnz_y[by] + tnz_y[4 * mx + bx], first, ylev[4 * by + bx])
                    lnz_y[by] = tnz_y[4 * mx + bx] = nz
            for lev, tn, ln in ((m.get("u", [zero] * 4), tnz_u, lnz_u), (m.get("v", [zero] * 4), tnz_v, lnz_v)):
                for by in range(2):
                    for bx in range(2):
                        nz = _put_coeffs(e, probs, 2, ln[by] + tn[2 * mx + bx], 0, lev[2 * by + bx])
                        ln[by] = tn[2 * mx + bx] = nz
    first_part = h.bytes()
    tokens = [p.bytes() for p in parts]
    tag = 0 | (profile << 1) | (1 << 4) | (len(first_part) << 5)
    frame = struct.pack("<I", tag)[:3] + b"\x9d\x01\x2a" + struct.pack("<HH", width | (scale[0] << 14), height | (scale[1] << 14))
    frame += first_part + b"".join(struct.pack("<I", len(t))[:3] for t in tokens[:-1]) + b"".join(tokens)
    chunks = [(b"VP8 ", frame)]
    if vp8x:
        chunks = [(b"VP8X", bytes([0, 0, 0, 0]) + struct.pack("<I", width - 1)[:3] + struct.pack("<I", height - 1)[:3])] + chunks
    chunks += list(extra_chunks)
    body = b"WEBP" + b"".join(t + struct.pack("<I", len(d)) + d + (b"\0" if len(d) & 1 else b"") for t, d in chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def random_levels(rng, density=0.25, big=0.02):
    """16 levels in zig-zag order: mostly zero, small values, and in a share `big` of the blocks one value of a higher token category"""
    lev = [0] * 16
    for k in range(16):
        if rng.random() < density:
            v = int(rng.integers(1, 4))
            lev[k] = -v if rng.random() < 0.5 else v
    if rng.random() < big:
        v = int(rng.choice([4, 5, 6, 7, 10, 11, 18, 19, 34, 35, 66, 67, 150]))
        lev[int(rng.integers(0, 16))] = -v if rng.random() < 0.5 else v
    return lev


def random_mb(rng, i4=None, skip_allowed=False, segs=1, density=0.2, big=0.1):
    m = {"seg": int(rng.integers(0, segs)), "uvmode": int(rng.integers(0, 4))}
    m["i4"] = int(rng.integers(0, 2)) if i4 is None else i4
    if m["i4"]:
        m["sub"] = [int(v) for v in rng.integers(0, 10, 16)]
    else:
        m["ymode"] = int(rng.integers(0, 4))
        m["y2"] = random_levels(rng, density, big)
    if skip_allowed and rng.random() < 0.3:
        m["skip"] = 1
        return m
    if rng.random() < 0.15:
        return m   # coded, with every level zero
    m["y"] = [random_levels(rng, density, big) if rng.random() < 0.7 else [0] * 16 for _ in range(16)]
    if not m["i4"]:
        for b in m["y"]:
            b[0] = 0   # (position 0 is not coded in a 16x16-mode macroblock)
    m["u"] = [random_levels(rng, density, big) for _ in range(4)]
    m["v"] = [random_levels(rng, density, big) for _ in range(4)]
    return m
