"""A seeded corpus of damaged and hostile JPEG files for the decoder tests (tests/test_jpegdec_damaged.py on the CPU,
tests/test_gpu_jpegdec_damaged.py on the device).  Everything is generated at test time from the seeded files of jpeg_cases.py and
from a small hand-written baseline encoder below; nothing binary is committed.  corpus() -> [(name, bytes)], names stable.

The contract under test: a decoder that accepts a file (status 0) gives Pillow's pixels byte for byte; every other file is left
to Pillow.  So the corpus aims at the places where "accept" and "Pillow's answer" can drift apart: Huffman tables libjpeg refuses,
scans that run out of data or carry extra, restart markers out of step with the restart interval, coefficients beyond the range
where libjpeg-turbo's C and SIMD inverse DCTs agree, and marker-level damage around the scan."""
import struct

import numpy as np

from jpeg_cases import CASES, make_file

BASES = ["n420_q95", "n422_q75", "n444_q95", "grey_text", "rst1_420", "rstrow_420"]
N_FLIPS = 100


def base_file(name: str) -> bytes:
    return make_file(next(c for c in CASES if c[0] == name))


# ---- marker walking ------------------------------------------------------------------------------------------------------
def segments(data: bytes):
    """Header segments up to and including SOS: [(marker, start, end)], start = offset of the 0xFF, end = one past the payload."""
    out, p = [], 2
    while p + 4 <= len(data):
        assert data[p] == 0xFF
        m = data[p + 1]
        ln = struct.unpack(">H", data[p + 2:p + 4])[0]
        out.append((m, p, p + 2 + ln))
        p += 2 + ln
        if m == 0xDA:
            break
    return out


def scan_range(data: bytes):
    """(first byte of the entropy-coded data, offset of the final EOI)"""
    sos = [s for s in segments(data) if s[0] == 0xDA][0]
    assert data[-2:] == b"\xff\xd9"
    return sos[2], len(data) - 2


def replace_segment(data: bytes, marker: int, payload: bytes, nth: int = 0) -> bytes:
    seg = [s for s in segments(data) if s[0] == marker][nth]
    return data[:seg[1]] + bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload + data[seg[2]:]


def payload(data: bytes, marker: int, nth: int = 0) -> bytes:
    seg = [s for s in segments(data) if s[0] == marker][nth]
    return data[seg[1] + 4:seg[2]]


def huff_tables(data: bytes):
    """Every Huffman table in the DHT segments: [(tc, th, bits[16], vals)] in file order."""
    out = []
    for m, a, b in segments(data):
        if m != 0xC4:
            continue
        s, i = data[a + 4:b], 0
        while i < len(s):
            tc, th = s[i] >> 4, s[i] & 15
            bits = list(s[i + 1:i + 17])
            n = sum(bits)
            out.append((tc, th, bits, bytes(s[i + 17:i + 17 + n])))
            i += 17 + n
    return out


def dht_payload(tables) -> bytes:
    return b"".join(bytes([tc << 4 | th]) + bytes(bits) + vals for tc, th, bits, vals in tables)


def with_tables(data: bytes, tables) -> bytes:
    """data with all its DHT segments replaced by ONE DHT segment, just before SOF, holding `tables`."""
    segs = segments(data)
    pl = dht_payload(tables)
    head = bytearray(data[:2])
    for m, a, b in segs:
        if m == 0xC4:
            continue
        if m in (0xC0, 0xC1):
            head += b"\xff\xc4" + struct.pack(">H", len(pl) + 2) + pl
        head += data[a:b]
    return bytes(head) + data[segs[-1][2]:]


def insert_after_soi(data: bytes, seg: bytes) -> bytes:
    return data[:2] + seg + data[2:]


def app14(transform: int) -> bytes:
    pl = b"Adobe" + struct.pack(">HHHB", 100, 0, 0, transform)
    return b"\xff\xee" + struct.pack(">H", len(pl) + 2) + pl


# ---- a small baseline encoder for crafted coefficient streams --------------------------------------------------------------
def _canonical(lengths):
    """symbols grouped by code length -> (bits[16], vals, {symbol: (code, length)})"""
    bits, vals, codes, code = [0] * 16, [], {}, 0
    for l in range(1, 17):
        for sym in lengths.get(l, []):
            codes[sym] = (code, l)
            vals.append(sym)
            bits[l - 1] += 1
            code += 1
        code <<= 1
    return bits, bytes(vals), codes


# DC: categories 0..11, every code 4 bits long; AC: EOB, ZRL and every (run, size 1..15) as 8-bit codes (242 of 256: valid)
_DC = _canonical({4: list(range(12))})
_AC = _canonical({8: [0x00, 0xF0] + [r << 4 | s for r in range(16) for s in range(1, 16)]})


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        for i in range(n - 1, -1, -1):
            self.acc = (self.acc << 1) | ((v >> i) & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                if self.acc == 0xFF:
                    self.out.append(0)
                self.acc, self.n = 0, 0

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _category(v):
    return 0 if v == 0 else int(abs(v)).bit_length()


def _bits_of(v, s):
    return v if v >= 0 else v + (1 << s) - 1


def encode_grey_blocks(blocks, w: int, h: int, q: int = 1, raw_tokens=None) -> bytes:
    """A grey baseline JPEG from quantised coefficient blocks (int [nblk, 64] in ZIG-ZAG order; DC absolute), one block per MCU,
    every quantiser step = q.  raw_tokens: {block index: [(run, size, value) | 'EOB' | 'ZRL']} replaces that block's AC coding, so
    streams no conforming encoder writes (a zero run past the block end ...) can be made."""
    dcb, dcv, dcc = _DC
    acb, acv, acc = _AC
    bw = _BitWriter()
    pred = 0
    for i, blk in enumerate(blocks):
        d = int(blk[0]) - pred
        pred = int(blk[0])
        s = _category(d)
        bw.put(*dcc[s])
        if s:
            bw.put(_bits_of(d, s), s)
        toks = raw_tokens.get(i) if raw_tokens else None
        if toks is None:
            toks, run = [], 0
            last = max([k for k in range(1, 64) if blk[k]] or [0])
            for k in range(1, last + 1):
                if blk[k] == 0:
                    run += 1
                    continue
                while run > 15:
                    toks.append("ZRL")
                    run -= 16
                toks.append((run, _category(int(blk[k])), int(blk[k])))
                run = 0
            if last < 63:
                toks.append("EOB")
        for t in toks:
            if t == "EOB":
                bw.put(*acc[0x00])
            elif t == "ZRL":
                bw.put(*acc[0xF0])
            else:
                r, s, v = t
                bw.put(*acc[r << 4 | s])
                bw.put(_bits_of(v, s), s)
    scan = bw.flush()
    dqt = b"\x00" + bytes([q]) * 64
    dht = bytes([0x00]) + bytes(dcb) + dcv + bytes([0x10]) + bytes(acb) + acv
    sof = bytes([8]) + struct.pack(">HH", h, w) + bytes([1, 1, 0x11, 0])
    sos = bytes([1, 1, 0x00, 0, 63, 0])
    seg = lambda m, p: bytes([0xFF, m]) + struct.pack(">H", len(p) + 2) + p
    return b"\xff\xd8" + seg(0xDB, dqt) + seg(0xC4, dht) + seg(0xC0, sof) + seg(0xDA, sos) + scan + b"\xff\xd9"


def _blocks(n):
    return np.zeros((n, 64), np.int64)


def crafted():
    out = []
    w = 8 * 40
    b = _blocks(40)
    b[:, 0] = np.arange(1, 41) * 2047                    # DC differences of +2047: the running value passes int16 after 16 blocks
    out.append(("craft_dc_accumulates_past_int16", encode_grey_blocks(b, w, 8)))
    b = _blocks(40)
    b[:, 0] = [2047 * min(k, 39 - k) // 2 for k in range(40)]   # up and back down: peak ~20000, ends near 0
    out.append(("craft_dc_up_and_down", encode_grey_blocks(b, w, 8)))
    for x in (300, 511, 512, -512, -513):                # one DC-only block, q = 8: the sample before the +128 is x
        b = _blocks(2)
        b[0, 0] = x
        out.append(("craft_idct_out_%d" % x, encode_grey_blocks(b, 16, 8, q=8)))
    b = _blocks(2)
    b[0, 5] = 20000                                      # |coefficient x q| > 16383 with q = 1
    out.append(("craft_coef_20000_q1", encode_grey_blocks(b, 16, 8)))
    b = _blocks(2)
    b[0, 3] = 1000                                       # 1000 x 255: the de-quantised value overflows 16 bits
    out.append(("craft_dequant_overflow_q255", encode_grey_blocks(b, 16, 8, q=255)))
    b = _blocks(2)
    b[0, 0] = 40
    out.append(("craft_zrl_to_64", encode_grey_blocks(b, 16, 8, raw_tokens={0: [(0, 2, 3)] * 47 + ["ZRL"]})))        # ends exactly at 64
    out.append(("craft_zrl_past_63", encode_grey_blocks(b, 16, 8, raw_tokens={0: [(0, 2, 3)] * 50 + ["ZRL"]})))
    out.append(("craft_run_past_63", encode_grey_blocks(b, 16, 8, raw_tokens={0: [(0, 2, 3)] * 55 + [(12, 1, 1)]})))
    rng = np.random.default_rng(77)
    b = _blocks(24)
    b[:, 0] = rng.integers(-60, 60, 24)
    b[:, 1:12] = rng.integers(-20, 21, (24, 11))
    out.append(("craft_clean_control", encode_grey_blocks(b, 8 * 6, 8 * 4)))   # a plain crafted file: must be ACCEPTED
    return out


# ---- header mutations -----------------------------------------------------------------------------------------------------
def header_mutations():
    out = []
    n420, grey, rst1 = base_file("n420_q95"), base_file("grey_text"), base_file("rst1_420")
    tabs = huff_tables(n420)
    dc0 = next(i for i, t in enumerate(tabs) if t[0] == 0 and t[1] == 0)
    ac0 = next(i for i, t in enumerate(tabs) if t[0] == 1 and t[1] == 0)

    def with_table(i, bits, vals):
        t = list(tabs)
        t[i] = (t[i][0], t[i][1], list(bits), bytes(vals))
        return with_tables(n420, t)

    na = len(tabs[ac0][3])
    out.append(("hdr_dht_roundtrip", with_tables(n420, tabs)))                       # the rebuilt segment itself: must be accepted
    out.append(("hdr_dht_dc_oversub_len1", with_table(dc0, [12] + [0] * 15, tabs[dc0][3][:12].ljust(12, b"\x00"))))
    out.append(("hdr_dht_dc_full_space", with_table(dc0, [1] * 10 + [2] + [0] * 5, bytes(range(12)))))   # Kraft sum exactly 1: all-ones code
    out.append(("hdr_dht_dc_symbol_16", with_table(dc0, tabs[dc0][2], tabs[dc0][3][:-1] + b"\x10")))
    ac_bits = [0] * 16
    ac_bits[6] = na                                                                  # na (> 128) codes of 7 bits
    out.append(("hdr_dht_ac_oversub_len7", with_table(ac0, ac_bits, tabs[ac0][3])))
    out.append(("hdr_dht_ac_oversub_len1", with_table(ac0, [3] + tabs[ac0][2][1:], tabs[ac0][3] + b"\x01\x02\x03")))
    t = list(tabs)
    t[ac0] = (1, 0, [0] * 14 + [45, 255], tabs[ac0][3] + bytes(300 - na))            # counts summing to 300
    out.append(("hdr_dht_count_over_256", with_tables(n420, t)))
    t = list(tabs)
    t.append(t.pop(ac0))
    pl = dht_payload(t)
    out.append(("hdr_dht_count_past_segment", replace_segment(with_tables(n420, t), 0xC4, pl[:-7])))   # last table's values cut short

    dqt = payload(n420, 0xDB)
    out.append(("hdr_dqt_short", replace_segment(n420, 0xDB, dqt[:-10])))
    q16 = b"".join(bytes([0x10 | (dqt[i] & 15)]) + b"".join(struct.pack(">H", v) for v in dqt[i + 1:i + 65]) for i in range(0, len(dqt), 65))
    out.append(("hdr_dqt_16bit_same_values", replace_segment(n420, 0xDB, q16)))
    big = b"".join(bytes([0x10 | (dqt[i] & 15)]) + b"".join(struct.pack(">H", min(65535, v * 300)) for v in dqt[i + 1:i + 65]) for i in range(0, len(dqt), 65))
    out.append(("hdr_dqt_16bit_large", replace_segment(n420, 0xDB, big)))

    sof = payload(n420, 0xC0)
    out.append(("hdr_sof_zero_width", replace_segment(n420, 0xC0, sof[:3] + b"\x00\x00" + sof[5:])))
    out.append(("hdr_sof_zero_height", replace_segment(n420, 0xC0, sof[:1] + b"\x00\x00" + sof[3:])))
    out.append(("hdr_sof_too_short", replace_segment(n420, 0xC0, sof[:-2])))
    out.append(("hdr_sof_too_long", replace_segment(n420, 0xC0, sof + b"\x00")))
    out.append(("hdr_sof_ids_012", replace_segment(n420, 0xC0, sof[:6] + bytes([0]) + sof[7:9] + bytes([1]) + sof[10:12] + bytes([2]) + sof[13:])))
    sos = payload(n420, 0xDA)
    out.append(("hdr_sos_missing_dc_table", replace_segment(n420, 0xDA, sos[:2] + bytes([0x30 | (sos[2] & 15)]) + sos[3:])))
    out.append(("hdr_sos_missing_ac_table", replace_segment(n420, 0xDA, sos[:4] + bytes([(sos[4] & 0xF0) | 3]) + sos[5:])))

    out.append(("hdr_dri_zero", replace_segment(rst1, 0xDD, b"\x00\x00")))
    out.append(("hdr_dri_double", replace_segment(rst1, 0xDD, struct.pack(">H", 2 * struct.unpack(">H", payload(rst1, 0xDD))[0]))))
    out.append(("hdr_dri_long", replace_segment(rst1, 0xDD, payload(rst1, 0xDD) + b"\x00")))
    out.append(("hdr_dri_without_markers", insert_after_soi(n420, b"\xff\xdd\x00\x04\x00\x02")))

    for tr in (0, 1, 2):
        out.append(("hdr_adobe_grey_t%d" % tr, insert_after_soi(grey, app14(tr))))
        out.append(("hdr_adobe_rgb_t%d" % tr, insert_after_soi(n420, app14(tr))))
    sof_g = [s for s in segments(grey) if s[0] == 0xC0][0]
    out.append(("hdr_adobe_grey_after_sof", grey[:sof_g[2]] + app14(0) + grey[sof_g[2]:]))

    rng = np.random.default_rng(99)
    out.append(("tail_missing_eoi", n420[:-2]))
    out.append(("tail_two_eoi", n420 + b"\xff\xd9"))
    out.append(("tail_junk_after_eoi", n420 + bytes(rng.integers(0, 255, 200, dtype=np.uint8))))   # (no 0xFF in the junk)
    out.append(("tail_ff_before_eoi", n420[:-2] + b"\xff\xff\xd9"))
    out.append(("tail_eoi_inside_junk", n420 + b"\x12\x34\xff\xd9\x56"))
    return out


# ---- scan mutations -------------------------------------------------------------------------------------------------------
def _markers(data, a, e):
    """offsets of the RSTn markers in data[a:e]"""
    return [i for i in range(a, e - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]


def scan_mutations(base: str):
    data = base_file(base)
    a, e = scan_range(data)
    rng = np.random.default_rng(sum(map(ord, base)))
    out = []
    for k in range(N_FLIPS):
        b = bytearray(data)
        for _ in range(int(rng.integers(1, 4))):
            bit = int(rng.integers(0, (e - a) * 8))
            b[a + bit // 8] ^= 0x80 >> (bit % 8)
        out.append(("%s_flip%03d" % (base, k), bytes(b)))
    for k, cut in enumerate(sorted(int(x) for x in rng.integers(a + 1, e, 6))):
        out.append(("%s_trunc%d" % (base, k), data[:cut]))
        out.append(("%s_trunc%d_eoi" % (base, k), data[:cut] + b"\xff\xd9"))
    stuffed = [i for i in range(a, e - 1) if data[i] == 0xFF and data[i + 1] == 0x00]
    for k, i in enumerate(stuffed[:: max(1, len(stuffed) // 3)][:3]):
        out.append(("%s_bare_ff%d" % (base, k), data[:i + 1] + data[i + 2:]))
    rst = _markers(data, a, e)
    if rst:
        picks = [rst[0], rst[len(rst) // 2], rst[-1]]
        for k, i in enumerate(picks):
            out.append(("%s_rst_dup%d" % (base, k), data[:i + 2] + data[i:i + 2] + data[i + 2:]))
            out.append(("%s_rst_drop%d" % (base, k), data[:i] + data[i + 2:]))
            out.append(("%s_rst_renum%d" % (base, k), data[:i + 1] + bytes([0xD0 | ((data[i + 1] + 1) & 7)]) + data[i + 2:]))
            nxt = rst[rst.index(i) + 1] if i != rst[-1] else e
            mid = (i + 2 + nxt) // 2
            while data[mid - 1] == 0xFF:
                mid += 1
            out.append(("%s_rst_insert_mid%d" % (base, k), data[:mid] + bytes([0xFF, data[i + 1]]) + data[mid:]))
        out.append(("%s_rst_extra_at_end" % base, data[:e] + bytes([0xFF, 0xD0 | ((data[rst[-1] + 1] + 1) & 7)]) + data[e:]))
    return out


def corpus():
    out = header_mutations() + crafted()
    for b in BASES:
        out += scan_mutations(b)
    names = [n for n, _ in out]
    assert len(names) == len(set(names))
    return out


def clean_files():
    """The undamaged bases, by name."""
    return [(b, base_file(b)) for b in BASES]
