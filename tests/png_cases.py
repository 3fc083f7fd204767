"""Seeded PNG test files for the device PNG decoder (nothing binary is committed: every file is written here).

cases() -> [(name, png bytes, expected probe rc)].  Pillow writes every mode it can at compress_level 0..9 and optimize=True; a small
numpy writer covers what Pillow will not produce: forced filters, split IDAT chunks, zlib strategies and window sizes, 2/4-bit grey,
short palettes, tRNS, eXIf orientations, Adam7 and 16-bit files (those two must be refused with -2)."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(ctype: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    a, b, c = a.astype(np.int16), b.astype(np.int16), c.astype(np.int16)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)).astype(np.uint8)


def filter_rows(rows: np.ndarray, bpp: int, filters) -> bytes:
    """rows: uint8 [H, rowbytes] (packed samples) -> the filtered scanlines with their filter bytes."""
    h, rb = rows.shape
    out = bytearray()
    prev = np.zeros(rb, np.uint8)
    for y in range(h):
        cur = rows[y]
        ft = int(filters[y])
        left = np.concatenate([np.zeros(bpp, np.uint8), cur[:-bpp]]) if rb > bpp else np.zeros(rb, np.uint8)
        ul = np.concatenate([np.zeros(bpp, np.uint8), prev[:-bpp]]) if rb > bpp else np.zeros(rb, np.uint8)
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - left
        elif ft == 2:
            f = cur - prev
        elif ft == 3:
            f = cur - ((left.astype(np.uint16) + prev) >> 1).astype(np.uint8)
        else:
            f = cur - _paeth(left, prev, ul)
        out.append(ft)
        out += f.astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def pack_rows(samples: np.ndarray, depth: int) -> np.ndarray:
    """samples uint [H, W*channels] at `depth` bits -> packed rows uint8 [H, rowbytes] (sub-byte rows end mid-byte, zero padded)."""
    if depth == 8:
        return samples.astype(np.uint8)
    if depth == 16:
        return samples.astype(">u2").view(np.uint8).reshape(samples.shape[0], -1)
    bits = np.unpackbits(samples.astype(np.uint8)[..., None], axis=-1)[..., 8 - depth:].reshape(samples.shape[0], -1)
    return np.packbits(bits, axis=-1)


def write_png(samples, width, height, depth, ct, filters=None, plte=None, trns=None, exif=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY,
              wbits=15, idat_split=None, interlace=0, zdata=None, extra_before=b"", tail=None, seed=0):
    rows = pack_rows(samples, depth)
    bpp = max(1, CHANNELS[ct] * depth // 8)
    rng = np.random.default_rng(seed)
    if filters is None:
        filters = np.zeros(height, np.int64)
    elif isinstance(filters, int):
        filters = np.full(height, filters)
    elif filters == "random":
        filters = rng.integers(0, 5, height)
    raw = filter_rows(rows, bpp, filters)
    if zdata is None:
        c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
        zdata = c.compress(raw) + c.flush()
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, ct, 0, 0, interlace)) + extra_before
    if exif is not None:
        out += chunk(b"eXIf", exif)
    if plte is not None:
        out += chunk(b"PLTE", plte)
    if trns is not None:
        out += chunk(b"tRNS", trns)
    if idat_split is None:
        out += chunk(b"IDAT", zdata)
    else:
        parts, k = [], 0
        for n in idat_split(len(zdata)):
            parts.append(zdata[k:k + n]); k += n
        parts.append(zdata[k:])
        out += b"".join(chunk(b"IDAT", p) for p in parts)
    out += chunk(b"IEND", b"") if tail is None else tail
    return out


def exif_orientation(o: int) -> bytes:
    return b"MM\x00\x2a" + struct.pack(">I", 8) + struct.pack(">H", 1) + struct.pack(">HHIHH", 0x0112, 3, 1, o, 0) + struct.pack(">I", 0)


def with_text(data: bytes, key: bytes, value: bytes) -> bytes:
    """the same file with a tEXt chunk (before IDAT)"""
    p = data.index(b"IDAT") - 4
    return data[:p] + chunk(b"tEXt", key + b"\x00" + value) + data[p:]


def text_orientation_files(page_image):
    """orientation 6 carried only by a tEXt chunk: a "Raw profile type exif" hex dump, or an XMP tiff:Orientation (Pillow's getexif()
    reads both; neither sets info["exif"])"""
    ex = b"Exif\x00\x00" + exif_orientation(6)
    raw = ("\nexif\n%8d\n" % len(ex) + ex.hex()).encode()
    xmp = (b'<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#">'
           b'<rdf:Description xmlns:tiff="http://ns.adobe.com/tiff/1.0/" tiff:Orientation="6"/></rdf:RDF></x:xmpmeta>')
    page = pil_bytes(page_image)
    return {"raw_profile": with_text(page, b"Raw profile type exif", raw), "xmp": with_text(page, b"XML:com.adobe.xmp", xmp)}


def page_samples(rng, h, w, ch, maxv=255, smooth=True):
    """Text-like content: a smooth background with random strokes, so that every filter type has work to do."""
    if not smooth:
        return rng.integers(0, maxv + 1, (h, w * ch))
    y, x = np.mgrid[0:h, 0:w]
    base = ((x * 3 + y * 5) % (maxv + 1))[..., None].repeat(ch, -1).astype(np.int64)
    mask = rng.random((h, w)) < 0.2
    base[mask] = rng.integers(0, maxv + 1, (int(mask.sum()), ch))
    return base.reshape(h, w * ch)


def pil_bytes(im, **kw) -> bytes:
    b = io.BytesIO()
    im.save(b, "PNG", **kw)
    return b.getvalue()


def cases():
    rng = np.random.default_rng(20261016)
    out = []
    # ---- Pillow writes: every mode, compress_level 0..9, optimize ----
    h, w = 37, 53
    rgb = page_samples(rng, h, w, 3).astype(np.uint8).reshape(h, w, 3)
    pil = {
        "rgb": Image.fromarray(rgb, "RGB"),
        "rgba": Image.fromarray(np.dstack([rgb, rng.integers(0, 256, (h, w), dtype=np.uint8)]), "RGBA"),
        "l": Image.fromarray(rgb[..., 0], "L"),
        "la": Image.fromarray(np.dstack([rgb[..., 0], rgb[..., 1]]), "LA"),
        "1": Image.fromarray(rgb[..., 0] > 128).convert("1"),
        "p": Image.fromarray(rgb, "RGB").quantize(200),
    }
    for name, im in pil.items():
        for lvl in range(10):
            out.append((f"pil_{name}_z{lvl}", pil_bytes(im, compress_level=lvl), 0))
        out.append((f"pil_{name}_opt", pil_bytes(im, optimize=True), 0))
    for bits in (1, 2, 4):
        p = Image.fromarray(rgb, "RGB").quantize(1 << bits)
        out.append((f"pil_p{bits}", pil_bytes(p, bits=bits), 0))
    p = pil["p"].copy()
    p.info["transparency"] = 3
    out.append(("pil_p_trns", pil_bytes(p, transparency=3), 0))
    # ---- numpy writer: every colour type / depth, every filter forced, random filters ----
    for ct, depths in ((0, (1, 2, 4, 8)), (2, (8,)), (3, (1, 2, 4, 8)), (4, (8,)), (6, (8,))):
        for d in depths:
            ch = CHANNELS[ct]
            for hh, ww in ((29, 45), (1, 1), (17, 1), (9, 7)):
                maxv = (1 << d) - 1
                s = page_samples(rng, hh, ww, ch, maxv)
                plte = None
                if ct == 3:
                    npal = 1 << d
                    plte = rng.integers(0, 256, 3 * npal, dtype=np.uint8).tobytes()
                for filt in (0, 1, 2, 3, 4, "random"):
                    out.append((f"np_ct{ct}_d{d}_{hh}x{ww}_f{filt}", write_png(s, ww, hh, d, ct, filters=filt, plte=plte, seed=hh + ww), 0))
    base = page_samples(rng, 61, 83, 3)
    mk = lambda **kw: write_png(base, 83, 61, 8, 2, filters="random", **kw)
    # IDAT splits
    out.append(("split_1byte", mk(idat_split=lambda n: [1] * (n - 1)), 0))
    out.append(("split_zero_len", mk(idat_split=lambda n: [0, 5, 0, 0, n // 2 - 5, 0]), 0))
    # zlib strategies and window sizes
    for sname, st in (("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("filtered", zlib.Z_FILTERED)):
        out.append((f"zlib_{sname}", mk(strategy=st), 0))
    for wb in range(9, 16):
        out.append((f"zlib_wbits{wb}", write_png(page_samples(rng, 120, 200, 3), 200, 120, 8, 2, filters="random", wbits=wb), 0))
    # stored blocks over 64 KB; distance-1 runs of length 258
    big = page_samples(rng, 150, 200, 3, smooth=False)
    out.append(("stored_big", write_png(big, 200, 150, 8, 2, level=0), 0))
    flat = np.full((90, 300 * 3), 200)
    out.append(("dist1_runs", write_png(flat, 300, 90, 8, 2, level=9), 0))
    out.append(("dist1_runs_rle", write_png(flat, 300, 90, 8, 2, strategy=zlib.Z_RLE), 0))
    # odd widths, sub-byte rows that end mid-byte
    for ww in (3, 5, 13, 31):
        for d in (1, 2, 4):
            s = page_samples(rng, 11, ww, 1, (1 << d) - 1)
            out.append((f"subbyte_g{d}_w{ww}", write_png(s, ww, 11, d, 0, filters="random"), 0))
    # a short PLTE (indices stay below it), tRNS in grey / RGB / palette files
    s = rng.integers(0, 5, (23, 19))
    out.append(("short_plte", write_png(s, 19, 23, 8, 3, plte=rng.integers(0, 256, 15, dtype=np.uint8).tobytes(), filters="random"), 0))
    out.append(("trns_grey", write_png(page_samples(rng, 21, 22, 1), 22, 21, 8, 0, trns=b"\x00\x07"), 0))
    out.append(("trns_rgb", write_png(page_samples(rng, 21, 22, 3), 22, 21, 8, 2, trns=b"\x00\x01\x00\x02\x00\x03"), 0))
    out.append(("trns_pal", write_png(s, 19, 23, 8, 3, plte=rng.integers(0, 256, 15, dtype=np.uint8).tobytes(), trns=b"\x00\x80\xff"), 0))
    out.append(("trns_grey1", write_png(rng.integers(0, 2, (9, 30)), 30, 9, 1, 0, trns=b"\x00\x01"), 0))
    # eXIf orientations
    for o in (1, 3, 6, 8):
        out.append((f"exif_o{o}", write_png(page_samples(rng, 33, 47, 3), 47, 33, 8, 2, filters="random", exif=exif_orientation(o)), 0))
    # outside the subset: Adam7 and 16 bit
    s16 = rng.integers(0, 65536, (13, 17 * 3))
    out.append(("rgb16", write_png(s16, 17, 13, 16, 2), -2))
    out.append(("grey16", write_png(rng.integers(0, 65536, (13, 17)), 17, 13, 16, 0), -2))
    out.append(("rgba16", write_png(rng.integers(0, 65536, (13, 17 * 4)), 17, 13, 16, 6), -2))
    out.append(("adam7", _adam7(rng), -2))
    return out


def _adam7(rng) -> bytes:
    """An interlaced 8-bit grey file (the seven passes filtered with filter 0)."""
    h, w = 15, 13
    img = rng.integers(0, 256, (h, w)).astype(np.uint8)
    raw = bytearray()
    for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = img[y0::dy, x0::dx]
        if sub.size == 0:
            continue
        for row in sub:
            raw.append(0)
            raw += row.tobytes()
    return SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 1)) + chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b"")


def pillow_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
