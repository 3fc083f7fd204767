"""Scanned-TIFF cases for the strip decoders (csrc/lzw.hip), the container reader (utils/tiff_pages.py) and the provider's TIFF path: a
small TIFF container writer of its own (II / MM, any tag set, strips given as bytes) so that the tests control byte order, RowsPerStrip,
FillOrder, Photometric, Predictor and Orientation; strip payloads from Pillow / libtiff or from the restatement's encoders
(tests/tiff_reference.py).  The expected pixels of every case are Pillow's Image.open(file) (frame k) .convert('RGB')."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

import tiff_reference as tr
from pdf_cases import pack_bits

NONE, G4, LZW, DEFLATE, PACKBITS = 1, 4, 5, 8, 32773


# ---- the container writer ----
def _entry(E, tag, typ, values, blobs, base):
    """one 12-byte IFD entry; values longer than 4 bytes go to `blobs` (placed at base + their offset)"""
    fmt = {1: "B", 3: "H", 4: "I"}[typ]
    raw = struct.pack(E + "%d%s" % (len(values), fmt), *values)
    if len(raw) <= 4:
        return struct.pack(E + "HHI", tag, typ, len(values)) + raw.ljust(4, b"\0")
    off = base + len(blobs)
    blobs += raw + (b"\0" if len(raw) & 1 else b"")
    return struct.pack(E + "HHI", tag, typ, len(values)) + struct.pack(E + "I", off)


def tiff_file(frames, big_endian=False, magic=42) -> bytes:
    """frames: dicts with `strips` (list of bytes) and `tags` {tag: value | list | (type, list)}; StripOffsets (273) and
    StripByteCounts (279) are filled in unless the frame gives them.  SHORT is used for values below 65536, else LONG."""
    E = ">" if big_endian else "<"
    out = bytearray((b"MM" if big_endian else b"II") + struct.pack(E + "HI", magic, 8))
    for k, fr in enumerate(frames):
        strips = [bytes(s) for s in fr.get("strips", [])]
        tags = dict(fr["tags"])
        ifd_at = len(out)
        n = len(set(tags) | ({273, 279} if strips else set()))
        base = ifd_at + 2 + 12 * n + 4          # blobs, then the strips
        # two passes: the first sizes the blobs so the strip offsets are known
        offsets = None
        for _ in range(2):
            t = dict(tags)
            if strips:
                t.setdefault(279, (4, [len(s) for s in strips]))
                t.setdefault(273, (4, offsets or [0] * len(strips)))
            blobs = bytearray()
            entries = b""
            for tag in sorted(t):
                v = t[tag]
                if isinstance(v, tuple):
                    typ, vals = v
                else:
                    vals = list(v) if isinstance(v, (list, np.ndarray)) else [v]
                    typ = 3 if all(0 <= int(x) < 65536 for x in vals) else 4
                entries += _entry(E, tag, typ, [int(x) for x in vals], blobs, base)
            at = base + len(blobs)
            offsets = []
            for s in strips:
                offsets.append(at)
                at += len(s) + (len(s) & 1)
        body = bytearray(struct.pack(E + "H", n) + entries)
        end = at
        nxt = fr.get("next", end if k + 1 < len(frames) else 0)
        body += struct.pack(E + "I", nxt) + blobs
        for s in strips:
            body += s + (b"\0" if len(s) & 1 else b"")
        out += body
        assert len(out) == end, (len(out), end)
    return bytes(out)


def base_tags(width, height, comp, photo, bits=8, spp=1, rps=None, extra=None):
    t = {256: width, 257: height, 258: [bits] * spp, 259: comp, 262: photo, 277: spp}
    if rps is not None:
        t[278] = rps
    t.update(extra or {})
    return t


# ---- strip payloads ----
def split_rows(rows: bytes, rb: int, height: int, rps: int):
    return [rows[r * rb:min(height, r + rps) * rb] for r in range(0, height, rps)]


def encode_strips(rows: bytes, rb: int, height: int, rps: int, comp: int):
    enc = {NONE: bytes, LZW: tr.lzw_encode, PACKBITS: tr.packbits_encode, DEFLATE: zlib.compress}[comp]
    return [enc(s) for s in split_rows(rows, rb, height, rps)]


def predict(rows: np.ndarray, comps: int) -> np.ndarray:
    a = rows.astype(np.int32).reshape(rows.shape[0], -1, comps)
    d = a.copy()
    d[:, 1:] -= a[:, :-1]
    return (d & 255).astype(np.uint8).reshape(rows.shape)


def libtiff_strips(im: Image.Image, compression: str, tiffinfo=None):
    """save with Pillow / libtiff -> (the file, its strips, RowsPerStrip)"""
    bio = io.BytesIO()
    im.save(bio, "TIFF", compression=compression, tiffinfo=tiffinfo or None)
    data = bio.getvalue()
    t = Image.open(io.BytesIO(data)).tag_v2
    return data, [data[o:o + c] for o, c in zip(t[273], t[279])], t.get(278, im.size[1])


def pillow_rgb(data: bytes, frame: int = 0) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    im.seek(frame)
    return np.asarray(im.convert("RGB"))


# ---- pictures ----
def noise(h, w, c=1, seed=7, top=256):
    a = np.random.default_rng(seed).integers(0, top, (h, w * c), dtype=np.uint8)
    return a


def text_like(h, w, seed=3):
    """dark strokes on a light ground with a little noise: long and short LZW strings"""
    rng = np.random.default_rng(seed)
    a = np.full((h, w), 240, np.uint8)
    for _ in range(h * w // 40):
        y, x = rng.integers(0, h), rng.integers(0, w)
        a[y:y + rng.integers(1, 3), x:x + rng.integers(1, 9)] = rng.integers(0, 60)
    a[rng.random((h, w)) < 0.02] = 200
    return a


def smooth_rgb(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 3 + y) & 255, (x + y * 2) & 255, (x * y) & 255], axis=2).astype(np.uint8).reshape(h, w * 3)


PALETTE16 = [((i * 4111) & 0xFFFF, (i * 9001 + 77) & 0xFFFF, (65535 - i * 257) & 0xFFFF) for i in range(256)]


def colormap(bits):
    k = 1 << bits
    return [PALETTE16[i][c] for c in range(3) for i in range(k)]


# ---- the fixed case list of the strip decoders ----
def make_case(name, rows, width, comp, photo=1, bits=8, spp=1, rps=None, predictor=1, strips=None, big_endian=False, extra=None):
    """rows: uint8 [H][row bytes] of packed samples (before the predictor).  -> dict(name, file, height, width, rps, params, palette,
    strips): what the C ABI needs, beside the file Pillow opens."""
    h, rb = rows.shape
    rps_eff = min(rps or h, h)
    stored = predict(rows, spp) if predictor == 2 else rows
    if strips is None:
        strips = encode_strips(stored.tobytes(), rb, h, rps_eff, comp)
    tags = base_tags(width, h, comp, photo, bits, spp, rps, extra)
    if predictor != 1:
        tags[317] = predictor
    if photo == 3:
        tags[320] = colormap(bits)
    data = tiff_file([dict(strips=strips, tags=tags)], big_endian)
    pal = None
    if photo == 3:
        k = 1 << bits
        pal = bytearray(768)
        for i in range(k):
            pal[3 * i:3 * i + 3] = bytes(v // 256 for v in PALETTE16[i])
        pal = bytes(pal)
    return dict(name=name, file=data, height=h, width=width, rps=rps_eff, palette=pal, strips=strips,
                params=(comp, predictor, spp, bits, int(photo == 3), int(photo == 0), 0))


_CASES = None


def strip_cases():
    """name -> case; every one a file Pillow opens.  Built once."""
    global _CASES
    if _CASES is not None:
        return _CASES
    C = {}

    def add(c):
        C[c["name"]] = c

    # 40 x 300 8-bit noise in one LZW strip, as libtiff writes it: 12-bit codes and table-full Clears
    a = noise(40, 300)
    _, strips, _ = libtiff_strips(Image.fromarray(a), "tiff_lzw", {278: 40})
    add(make_case("lzw_noise_40x300_libtiff", a, 300, LZW, strips=strips))
    add(make_case("lzw_noise_40x300_own", a, 300, LZW))
    # 64 x 331 all-white / all-black 1-bit: KwKwK chains, strings far longer than 64 bytes, 5 pad bits a row
    for nm, v in (("white", 1), ("black", 0)):
        add(make_case("lzw_1bit_%s_64x331" % nm, pack_bits(np.full((64, 331), v, np.uint8), 1), 331, LZW, bits=1))
    add(make_case("lzw_1x1", np.array([[173]], np.uint8), 1, LZW))
    add(make_case("lzw_width1_37", noise(37, 1, seed=9), 1, LZW))
    add(make_case("lzw_257rows_rps64", text_like(257, 50), 50, LZW, rps=64))
    add(make_case("lzw_grey2_331", pack_bits(noise(21, 331, seed=11, top=4), 2), 331, LZW, bits=2))
    add(make_case("lzw_grey4_331", pack_bits(noise(21, 331, seed=12, top=16), 4), 331, LZW, bits=4))
    add(make_case("lzw_pal4_331", pack_bits(noise(21, 331, seed=13, top=16), 4), 331, LZW, photo=3, bits=4))
    add(make_case("lzw_pal8_331", noise(21, 331, seed=14), 331, LZW, photo=3))
    add(make_case("lzw_grey_pred2", text_like(33, 130, seed=5), 130, LZW, predictor=2, rps=13))
    add(make_case("lzw_rgb_pred2", smooth_rgb(33, 130), 130, LZW, photo=2, spp=3, predictor=2, rps=13))
    add(make_case("lzw_rgb", smooth_rgb(20, 77), 77, LZW, photo=2, spp=3, rps=7))
    add(make_case("lzw_miniswhite_1bit", pack_bits(np.random.default_rng(15).random((30, 331)) < 0.1, 1), 331, LZW, photo=0, bits=1))
    add(make_case("lzw_miniswhite_2bit", pack_bits(noise(11, 331, seed=22, top=4), 2), 331, LZW, photo=0, bits=2))
    add(make_case("lzw_miniswhite_4bit", pack_bits(noise(11, 331, seed=23, top=16), 4), 331, LZW, photo=0, bits=4))
    add(make_case("lzw_miniswhite_8bit", text_like(30, 90, seed=6), 90, LZW, photo=0))
    # a strip cut right after its last needed code (no EOI), and one followed by other bytes
    t = text_like(24, 100, seed=8)
    add(make_case("lzw_no_eoi", t, 100, LZW, strips=[tr.lzw_encode(t.tobytes(), eoi=False)]))
    add(make_case("lzw_trailing_bytes", t, 100, LZW, strips=[tr.lzw_encode(t.tobytes()) + b"\x00\x01II*\x00 bytes after the data"]))
    # PackBits: literals, repeats of 128 bytes, the 128 header (skipped in a TIFF)
    p = np.concatenate([noise(3, 300, seed=16), np.full((2, 300), 77, np.uint8), text_like(5, 300, seed=17)])
    add(make_case("packbits_mixed", p, 300, PACKBITS, rps=4))
    enc = tr.packbits_encode(p.tobytes())
    add(make_case("packbits_with_128_headers", p, 300, PACKBITS, strips=[b"\x80" + enc[:301] + b"\x80\x80" + enc[301:]]))
    add(make_case("packbits_1bit", pack_bits(np.random.default_rng(18).random((40, 331)) < 0.05, 1), 331, PACKBITS, bits=1, rps=16))
    add(make_case("raw_grey", noise(19, 67, seed=19), 67, NONE, rps=5))
    add(make_case("raw_rgb_mm", smooth_rgb(19, 67), 67, NONE, photo=2, spp=3, rps=8, big_endian=True))
    add(make_case("raw_pal2", pack_bits(noise(9, 331, seed=20, top=4), 2), 331, NONE, photo=3, bits=2))
    add(make_case("raw_pal1", pack_bits(noise(9, 331, seed=21, top=2), 1), 331, NONE, photo=3, bits=1))
    _CASES = C
    return C


def damaged(data: bytes, strip_at: int, strip_len: int, count: int, seed: int):
    """`count` copies of the file with one byte of its strip xor-ed with a seeded non-zero value at a seeded position"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b = bytearray(data)
        b[strip_at + int(rng.integers(0, strip_len))] ^= int(rng.integers(1, 256))
        out.append(bytes(b))
    return out


def damage_sets():
    """[(name, case, [damaged files])]: the noise and a text-like page in one libtiff LZW strip, one byte of the strip changed at 24
    seeded positions each"""
    out = []
    for name, a, seed in (("noise", noise(40, 300), 101), ("text", text_like(64, 300, seed=4), 202)):
        _, strips, _ = libtiff_strips(Image.fromarray(a), "tiff_lzw", {278: a.shape[0]})
        c = make_case("damage_" + name, a, a.shape[1], LZW, strips=strips)
        at = c["file"].index(strips[0])
        out.append((name, c, damaged(c["file"], at, len(strips[0]), 24, seed)))
    return out


def hostile_strips(total: int):
    """name -> (codec, strip): streams that must not decode to `total` bytes"""
    C, E = tr.CLEAR, tr.EOI
    return {
        "code_past_table": (LZW, tr.pack_codes([(C, 9), (65, 9), (66, 9), (400, 9)] + [(65, 9)] * 40)),
        "eoi_early": (LZW, tr.pack_codes([(C, 9), (65, 9), (258, 9), (E, 9)] + [(65, 9)] * 40)),
        "all_ones": (LZW, b"\xff" * 300),
        "empty": (LZW, b""),
        "clear_only": (LZW, tr.pack_codes([(C, 9)] * 200)),
        "table_full_no_clear": (LZW, tr.pack_codes([(C, 9)] + [(c, b) for c, b in tr.lzw_codes(bytes(np.random.default_rng(5).integers(0, 256, 8000, dtype=np.uint8)))[1:]
                                                                 if c != C][:4200])),
        "packbits_repeat_at_last_byte": (PACKBITS, bytes([3, 1, 2, 3, 4, 254])),
        "packbits_literal_past_input": (PACKBITS, bytes([127]) + bytes(50)),
        "packbits_empty": (PACKBITS, b""),
        "raw_short": (NONE, bytes(total - 1)),
    }


# ---- frames for the reader and the provider ----
REVERSE = bytes(int("{:08b}".format(i)[::-1], 2) for i in range(256))


def g4_frame(bitmap: np.ndarray, photo=0, fill_order=1, rps=None, extra=None):
    """bitmap: bool [H][W], True = black.  Group 4 strips from libtiff (which codes black runs as such whatever the photometric)."""
    h, w = bitmap.shape
    im = Image.fromarray(np.where(bitmap, 0, 255).astype(np.uint8)).convert("1")
    _, strips, got_rps = libtiff_strips(im, "group4", {278: rps or h, 262: photo})
    assert got_rps == (rps or h)
    if fill_order == 2:
        strips = [s.translate(REVERSE) for s in strips]
    tags = base_tags(w, h, G4, photo, 1, 1, rps, extra)
    if fill_order != 1:
        tags[266] = fill_order
    return dict(strips=strips, tags=tags)


def frame(rows, width, comp, photo=1, bits=8, spp=1, rps=None, predictor=1, extra=None):
    """a frame of tiff_file from packed rows (see make_case)"""
    h, rb = rows.shape
    stored = predict(rows, spp) if predictor == 2 else rows
    tags = base_tags(width, h, comp, photo, bits, spp, rps, extra)
    if predictor != 1:
        tags[317] = predictor
    if photo == 3:
        tags[320] = colormap(bits)
    return dict(strips=encode_strips(stored.tobytes(), rb, h, min(rps or h, h), comp), tags=tags)


def tiled_frame(h=32, w=48):
    """one 8-bit grey page stored as 16 x 16 tiles (uncompressed): outside the reader's subset, inside Pillow's"""
    a = text_like(h, w, seed=77)
    tiles = [a[y:y + 16, x:x + 16].tobytes() for y in range(0, h, 16) for x in range(0, w, 16)]
    tags = base_tags(w, h, NONE, 1)
    tags.update({322: 16, 323: 16, 325: (4, [256] * len(tiles))})
    return dict(tiles=tiles, tags=tags), a


def tiff_file_with_tiles(frames, big_endian=False) -> bytes:
    """tiff_file for frames of which some carry `tiles` (TileOffsets 324 patched in after the layout is known)"""
    plain = []
    for fr in frames:
        if "tiles" in fr:
            t = dict(fr["tags"])
            t[324] = (4, [0] * len(fr["tiles"]))
            plain.append(dict(strips=[], tags=t, _tiles=fr["tiles"]))
        else:
            plain.append(fr)
    # tile data goes behind the whole chain; two passes give the offsets
    body = tiff_file([{k: v for k, v in f.items() if k != "_tiles"} for f in plain], big_endian)
    at = len(body)
    tail = b""
    for f in plain:
        if "_tiles" in f:
            offs = []
            for t in f["_tiles"]:
                offs.append(at + len(tail))
                tail += t
            f["tags"][324] = (4, offs)
    body = tiff_file([{k: v for k, v in f.items() if k != "_tiles"} for f in plain], big_endian)
    assert len(body) == at
    return body + tail


def libtiff_frame(rows, width, photo=1, spp=1, rps=None, predictor=1, compression="tiff_lzw", comp=LZW, extra=None):
    """frame() with the strips coded by libtiff (the restatement's own LZW encoder is slow on whole pages)"""
    h = rows.shape[0]
    im = Image.fromarray(rows.reshape(h, width, 3) if spp == 3 else rows)
    info = {278: rps or h}
    if predictor != 1:
        info[317] = predictor
    _, strips, got = libtiff_strips(im, compression, info)
    assert got == (rps or h)
    tags = base_tags(width, h, comp, photo, 8, spp, rps, extra)
    if predictor != 1:
        tags[317] = predictor
    return dict(strips=strips, tags=tags)
