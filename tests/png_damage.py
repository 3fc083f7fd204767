"""Seeded damaged PNG files for the device decoder's acceptance rule (status 0 => Pillow decodes the file to the same bytes).

corpus() -> [(base name, case name, bytes)].  Bit flips and truncations all over the IDAT data of seven bases, zlib header damage,
hand-written DEFLATE streams (BTYPE 3, bad NLEN, over-subscribed and incomplete trees, symbols 286/287 and 30/31, distances too far
back, short / long output), Adler-32 damage, bytes after it, filter bytes 5..255, palette indices past PLTE, chunks between or after
the IDATs and a missing IEND."""
import struct
import zlib

import numpy as np

import png_cases as pc


class Bits:
    """LSB-first DEFLATE bit writer; Huffman codes are given MSB-first (as RFC 1951 lists them)."""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def code(self, code, nbits):
        self.put(int(format(code, f"0{nbits}b")[::-1], 2) if nbits else 0, nbits)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def fixed_lit(b: Bits, sym: int):
    if sym < 144:
        b.code(0x30 + sym, 8)
    elif sym < 256:
        b.code(0x190 + sym - 144, 9)
    elif sym < 280:
        b.code(sym - 256, 7)
    else:
        b.code(0xC0 + sym - 280, 8)


def zwrap(deflate: bytes, data: bytes, cmf=0x78, flg=None) -> bytes:
    if flg is None:
        flg = (31 - (cmf * 256) % 31) % 31
    return bytes([cmf, flg]) + deflate + struct.pack(">I", zlib.adler32(data))


def grey_png(zdata: bytes, w: int, h: int) -> bytes:
    return pc.SIG + pc.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + pc.chunk(b"IDAT", zdata) + pc.chunk(b"IEND", b"")


def crafted():
    """Hand-written streams for a 4x2 grey page (filtered data: 2 rows of [0, a, b, c, d])."""
    data = bytes([0, 10, 20, 30, 40, 0, 10, 20, 30, 40])
    out = []

    def fixed(syms, final=1, extra=None):
        b = Bits()
        b.put(final, 1); b.put(1, 2)
        for s in syms:
            if isinstance(s, tuple):   # (length symbol, extra bits, dist code, dist extra)
                fixed_lit(b, s[0]); b.put(*s[1]); b.code(s[2], 5); b.put(*s[3])
            else:
                fixed_lit(b, s)
        if extra:
            extra(b)
        return b.bytes()

    good = fixed(list(data[:5]) + [(259, (0, 0), 4, (0, 1))] + [256])   # length 5 (sym 259), distance 5 (code 4, extra 0)
    out.append(("craft_good_fixed", grey_png(zwrap(good, data), 4, 2)))
    out.append(("craft_btype3", grey_png(zwrap(bytes([0x07]) + good[1:], data), 4, 2)))
    # stored block with a bad NLEN
    st = bytes([1]) + struct.pack("<HH", len(data), (~len(data)) & 0xFFFF) + data
    out.append(("craft_stored_ok", grey_png(zwrap(st, data), 4, 2)))
    out.append(("craft_stored_bad_nlen", grey_png(zwrap(bytes([1]) + struct.pack("<HH", len(data), 0x1234) + data, data), 4, 2)))
    # symbols 286 / 287 and distance codes 30 / 31 in a fixed block
    for s in (286, 287):
        out.append((f"craft_sym{s}", grey_png(zwrap(fixed(list(data[:5]) + [s, 256]), data), 4, 2)))
    for dcode in (30, 31):
        out.append((f"craft_dist{dcode}", grey_png(zwrap(fixed(list(data[:5]) + [(259, (0, 0), dcode, (0, 0))] + [256]), data), 4, 2)))
    # a distance past the bytes produced so far
    out.append(("craft_dist_too_far", grey_png(zwrap(fixed(list(data[:3]) + [(259, (0, 0), 4, (1, 1)), 30, 40, 256]), data), 4, 2)))
    # a distance beyond the declared window (CINFO 0: 256 bytes) on a 600-byte page
    big = bytes([0] + [7] * 299) * 2
    b2 = Bits(); b2.put(1, 1); b2.put(1, 2)
    for v in big[:300]:
        fixed_lit(b2, v)
    fixed_lit(b2, 285); b2.code(16, 5); b2.put(43, 7)   # length 258, distance 300 (code 16: 257 + 43)
    fixed_lit(b2, 269); b2.put(0, 2); b2.code(16, 5); b2.put(43, 7)   # length 19: 300 + 258 + 19 = 577
    for v in big[577:]:
        fixed_lit(b2, v)
    fixed_lit(b2, 256)
    for cinfo, name in ((0, "craft_window_256"), (7, "craft_window_32k")):
        cmf = 0x08 | (cinfo << 4)
        out.append((name, pc.SIG + pc.chunk(b"IHDR", struct.pack(">IIBBBBB", 299, 2, 8, 0, 0, 0, 0)) +
                    pc.chunk(b"IDAT", zwrap(b2.bytes(), big, cmf=cmf)) + pc.chunk(b"IEND", b"")))
    # dynamic headers: over-subscribed / incomplete code-length codes and literal trees
    def dynamic(cl_lens, hlit=257, hdist=1, body=None):
        b = Bits()
        b.put(1, 1); b.put(2, 2); b.put(hlit - 257, 5); b.put(hdist - 1, 5); b.put(len(cl_lens) - 4, 4)
        for v in cl_lens:
            b.put(v, 3)
        if body:
            body(b)
        return b.bytes() + bytes(8)
    out.append(("craft_cl_oversubscribed", grey_png(zwrap(dynamic([1, 1, 1, 1]), data), 4, 2)))
    out.append(("craft_cl_incomplete", grey_png(zwrap(dynamic([0, 0, 0, 1]), data), 4, 2)))
    out.append(("craft_cl_empty", grey_png(zwrap(dynamic([0, 0, 0, 0]), data), 4, 2)))
    out.append(("craft_hlit_287", grey_png(zwrap(dynamic([2, 2, 2, 2], hlit=287), data), 4, 2)))
    out.append(("craft_hdist_31", grey_png(zwrap(dynamic([2, 2, 2, 2], hdist=31), data), 4, 2)))
    def all_len8(b):   # every code length "8" (code 1 in the code-length code {0:'0', 8:'1'}) -> 258 codes of length 8: over-subscribed
        for _ in range(258):
            b.code(1, 1)
    out.append(("craft_lit_oversubscribed", grey_png(zwrap(dynamic([0, 0, 0, 1, 1], body=all_len8), data), 4, 2)))
    def incomplete_lit(b):   # 3 literal codes of length 2 (0, 1, 256) + rest 0: incomplete, and more than one code
        for i in range(258):
            b.code(1 if i in (0, 1, 256) else 0, 1)
    out.append(("craft_lit_incomplete", grey_png(zwrap(dynamic([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], body=incomplete_lit), data), 4, 2)))
    # short and long output
    out.append(("craft_short_output", grey_png(zlib.compress(data[:-1]), 4, 2)))
    out.append(("craft_long_output", grey_png(zlib.compress(data + b"\x00"), 4, 2)))
    return out


def _idat_range(png: bytes):
    p, first, last = 8, None, None
    while p + 8 <= len(png):
        n = struct.unpack(">I", png[p:p + 4])[0]
        if png[p + 4:p + 8] == b"IDAT":
            first = p + 8 if first is None else first
            last = p + 8 + n
        p += 12 + n
    return first, last


def _fix_crc(png: bytes) -> bytes:
    """recompute every chunk CRC (damage inside IDAT then reaches the decoder, not the CRC check)"""
    out, p = bytearray(png[:8]), 8
    while p + 8 <= len(png):
        n = struct.unpack(">I", png[p:p + 4])[0]
        body = png[p + 4:p + 8 + n]
        out += png[p:p + 8 + n] + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)
        p += 12 + n
    return bytes(out + png[p:])


def bases():
    rng = np.random.default_rng(7)
    h, w = 24, 40
    rgb = pc.page_samples(rng, h, w, 3)
    grey = pc.page_samples(rng, h, w, 1)
    return {
        "rgb": pc.write_png(rgb, w, h, 8, 2, filters="random"),
        "rgba": pc.write_png(pc.page_samples(rng, h, w, 4), w, h, 8, 6, filters="random"),
        "grey": pc.write_png(grey, w, h, 8, 0, filters="random"),
        "grey2": pc.write_png(pc.page_samples(rng, h, w, 1, 3), w, h, 2, 0, filters="random"),
        "pal4": pc.write_png(pc.page_samples(rng, h, w, 1, 11), w, h, 4, 3, plte=rng.integers(0, 256, 36, dtype=np.uint8).tobytes(), filters="random"),
        "la_fixed": pc.write_png(pc.page_samples(rng, h, w, 2), w, h, 8, 4, filters="random", strategy=zlib.Z_FIXED),
        "rgb_stored": pc.write_png(rgb, w, h, 8, 2, level=0),
    }


def corpus():
    rng = np.random.default_rng(99)
    out = []
    for bname, base in bases().items():
        out.append((bname, "undamaged", base))
        z0, z1 = _idat_range(base)
        zlen = z1 - z0
        # bit flips across the whole zlib stream (header, blocks, Adler-32)
        for k, off in enumerate(sorted(set(np.linspace(0, zlen - 1, 48).astype(int).tolist()))):
            b = bytearray(base)
            b[z0 + off] ^= 1 << int(rng.integers(0, 8))
            out.append((bname, f"flip_{off}", _fix_crc(bytes(b))))
        # truncations of the IDAT payload (chunk length fixed up) and of the file
        for off in sorted(set(np.linspace(0, zlen - 1, 12).astype(int).tolist())):
            zd = base[z0:z1][:off]
            out.append((bname, f"trunc_idat_{off}", base[:z0 - 8] + pc.chunk(b"IDAT", zd) + pc.chunk(b"IEND", b"")))
        for off in (len(base) - 1, len(base) - 12, z1 - 3, z0 + 5):
            out.append((bname, f"trunc_file_{off}", base[:off]))
        zd = base[z0:z1]
        head = base[:z0 - 8]
        mk = lambda z: head + pc.chunk(b"IDAT", z) + pc.chunk(b"IEND", b"")
        out.append((bname, "zlib_cm7", mk(bytes([(zd[0] & 0xF0) | 7, zd[1]]) + zd[2:])))
        out.append((bname, "zlib_fcheck", mk(bytes([zd[0], zd[1] ^ 1]) + zd[2:])))
        cmf = 0x78; flg = 0x20; flg += (31 - (cmf * 256 + flg) % 31) % 31
        out.append((bname, "zlib_fdict", mk(bytes([cmf, flg]) + zd[2:])))
        out.append((bname, "zlib_cinfo8", mk(bytes([0x88, (31 - (0x88 * 256) % 31) % 31]) + zd[2:])))
        out.append((bname, "adler_bad", mk(zd[:-1] + bytes([zd[-1] ^ 0x40]))))
        out.append((bname, "after_adler", mk(zd + b"\x00")))
        out.append((bname, "chunk_between_idat", head + pc.chunk(b"IDAT", zd[:len(zd) // 2]) + pc.chunk(b"tEXt", b"a\x00b") + pc.chunk(b"IDAT", zd[len(zd) // 2:]) + pc.chunk(b"IEND", b"")))
        out.append((bname, "chunk_after_idat", head + pc.chunk(b"IDAT", zd) + pc.chunk(b"tEXt", b"a\x00b") + pc.chunk(b"IEND", b"")))
        out.append((bname, "missing_iend", head + pc.chunk(b"IDAT", zd)))
        out.append((bname, "iend_bad_crc", head + pc.chunk(b"IDAT", zd) + b"\x00\x00\x00\x00IEND\x00\x00\x00\x00"))
        out.append((bname, "after_iend", base + b"\x00"))
        out.append((bname, "ihdr_bad_crc", base[:29] + bytes([base[29] ^ 1]) + base[30:]))
        # filter bytes 5..255: re-filter the inflated data
        raw = bytearray(zlib.decompress(zd))
        ihdr = struct.unpack(">IIBBBBB", base[16:29])
        rb = (ihdr[0] * pc.CHANNELS[ihdr[3]] * ihdr[2] + 7) // 8
        for fb in (5, 6, 17, 128, 255):
            r = bytearray(raw)
            r[(rb + 1) * int(rng.integers(0, ihdr[1]))] = fb
            out.append((bname, f"filter_{fb}", mk(zlib.compress(bytes(r)))))
    # palette index past PLTE: a 4-bit palette page with 12 entries, one index raised to 12..15
    rng2 = np.random.default_rng(3)
    s = pc.page_samples(rng2, 10, 9, 1, 11)
    plte = rng2.integers(0, 256, 36, dtype=np.uint8).tobytes()
    out.append(("pal4", "pal_ok", pc.write_png(s, 9, 10, 4, 3, plte=plte)))
    for v in (12, 15):
        s2 = s.copy(); s2[4, 8] = v
        out.append(("pal4", f"pal_index_{v}", pc.write_png(s2, 9, 10, 4, 3, plte=plte)))
    s8 = pc.page_samples(rng2, 10, 9, 1, 99)
    plte8 = rng2.integers(0, 256, 300, dtype=np.uint8).tobytes()
    s8b = s8.copy(); s8b[9, 0] = 100
    out.append(("pal8", "pal8_ok", pc.write_png(s8, 9, 10, 8, 3, plte=plte8)))
    out.append(("pal8", "pal8_index_100", pc.write_png(s8b, 9, 10, 8, 3, plte=plte8)))
    for name, data in crafted():
        out.append(("crafted", name, data))
    return out
