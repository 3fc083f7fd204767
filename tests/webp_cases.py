"""WebP test files: intact lossless files from Pillow's encoder and from the test-side writer (webp_writer.py), the refused kinds, and the
damage sweep.  The expectation of every intact case is Pillow's own decode of the file: pillow_rgb(data)."""
import functools
import io

import numpy as np
from PIL import Image, ImageDraw

import webp_writer as W


def pillow_rgb(data):
    """Pillow's pixels, or None where Pillow raises"""
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert("RGB"))
    except Exception:
        return None


def text_tile(w, h, seed=0, noise=0.0):
    rng = np.random.default_rng(seed)
    im = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(im)
    words = "the quick brown fox jumps over a lazy dog 0123456789 lossless webp page".split()
    for y in range(1, h, 11):
        d.text((2, y), " ".join(rng.permutation(words)[:6]), fill=(0, 0, 0))
    a = np.array(im)
    if noise:
        m = rng.random((h, w)) < noise
        a[m] = rng.integers(0, 256, (int(m.sum()), 3))
    return a


def _save(im, **kw):
    b = io.BytesIO()
    im.save(b, "WEBP", **kw)
    return b.getvalue()


def _as_mode(a, mode, seed):
    im = Image.fromarray(a)
    if mode == "RGBA":
        im = im.convert("RGBA")
        im.putalpha(Image.fromarray(np.random.default_rng(seed).integers(0, 256, a.shape[:2], dtype=np.uint8)))
        return im
    if mode == "P":
        return im.quantize(23)
    return im.convert(mode)


# (libwebp's encoder stops at 16383; the writer's cases below reach 16384)
SHAPES = ((1, 1), (1, 16383), (16383, 1), (5, 3), (63, 9), (64, 9), (65, 9), (129, 7), (40, 130), (200, 300))   # (width, height)
MODES = ("RGB", "RGBA", "L", "P", "1")


@functools.lru_cache(maxsize=None)
def pillow_cases():
    """[(name, file bytes)]: lossless=True at method 0 / 4 / 6 x quality 0 / 75 / 100 in modes RGB, RGBA (exact), L, P, 1, at every shape
    (method 6 with quality 100 at the seven small shapes only; the 200 x 300 tile at four of the pairs)"""
    out = []
    for si, (w, h) in enumerate(SHAPES):
        base = text_tile(w, h, si, 0.02) if (w, h) == (200, 300) else None
        for mode in MODES:
            for method in (0, 4, 6):
                for quality in (0, 75, 100):
                    if method == 6 and quality == 100 and w * h >= 16383:
                        continue   # (the encoder's exhaustive search takes 2-3 s a file there; the small shapes have the pair)
                    if base is not None and (method, quality) not in ((0, 0), (0, 100), (4, 75), (6, 0)):
                        continue   # (the one large tile: every method and every quality once; the restatement takes seconds a file)
                    seed = si * 1000 + method * 10 + quality
                    if base is not None:
                        a = base
                    elif w * h >= 16383:   # the long lines: runs, a ramp and noise
                        rng = np.random.default_rng(seed)
                        a = np.repeat(rng.integers(0, 256, (256, 3), dtype=np.uint8), 64, axis=0)[:16383].reshape(h, w, 3)
                        a = a.copy()
                        a.reshape(-1, 3)[5000:9000] = rng.integers(0, 256, (4000, 3))
                    else:
                        rng = np.random.default_rng(seed)
                        a = text_tile(w, h, seed, 0.05) if quality == 75 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                    out.append(("pillow-%dx%d-%s-m%d-q%d" % (w, h, mode, method, quality),
                                _save(_as_mode(a, mode, seed), lossless=True, method=method, quality=quality, exact=True)))
    return out


def _argb(a, alpha=None):
    a = a.astype(np.uint32)
    al = np.full(a.shape[:2], 255, np.uint32) if alpha is None else alpha.astype(np.uint32)
    return ((al << 24) | (a[..., 0] << 16) | (a[..., 1] << 8) | a[..., 2]).reshape(-1).tolist()


def _smooth(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 9 + y * 3) & 255, (x * 2 + y * 11 + 40) & 255, (x * y + 7) & 255], axis=-1).astype(np.uint8)
    m = rng.random((h, w)) < 0.2
    a[m] = rng.integers(0, 256, (int(m.sum()), 3))
    return a


def _sub(n, bits):
    return (n + (1 << bits) - 1) >> bits


def _copy_tokens(w, h, copies, seed, lead=None):
    """literals up to `lead` pixels, then the (length, distance code) copies with a literal between them, literals, and a last copy of
    distance 1 that crosses a row boundary and ends on the last pixel"""
    rng = np.random.default_rng(seed)
    n = w * h
    lit = lambda: ("L", int(rng.integers(0, 1 << 32)))
    toks = [lit() for _ in range(lead if lead is not None else w + 9)]
    pos = len(toks)
    for length, dcode in copies:
        toks.append(("C", length, dcode))
        toks.append(lit())
        pos += length + 1
    tail = w + 3
    assert pos <= n - tail, (pos, n)
    toks += [lit() for _ in range(n - tail - pos)]
    toks.append(("C", tail, W.code_for_distance(1)))
    return toks


@functools.lru_cache(maxsize=None)
def writer_cases():
    """[(name, file bytes)]: the streams libwebp's encoder never writes"""
    out = []
    D = W.code_for_distance
    # every predictor mode on every block of a 3 x 3 block grid (edges and corners included), block bits 2
    a = _argb(_smooth(11, 10, 1), np.random.default_rng(2).integers(0, 256, (10, 11)))
    for m in range(16):
        out.append(("predictor-mode%d" % m, W.write_vp8l(11, 10, a, [("predictor", 2, [m] * 9)], alpha=True)))
    out.append(("predictor-mixed", W.write_vp8l(19, 13, _argb(_smooth(19, 13, 3)), [("predictor", 2, [(k * 7 + 3) & 15 for k in range(5 * 4)])])))
    big = _argb(_smooth(70, 9, 4))
    out.append(("predictor-bits9", W.write_vp8l(70, 9, big, [("predictor", 9, [11])])))
    out.append(("cross-bits9", W.write_vp8l(70, 9, big, [("cross", 9, [(200, 17, 250)])])))
    rng = np.random.default_rng(5)
    el = lambda k: [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(k)]
    out.append(("cross-bits2", W.write_vp8l(70, 9, big, [("cross", 2, el(18 * 3))])))
    out.append(("green-alone", W.write_vp8l(70, 9, big, [("green",)])))
    out.append(("no-transform-no-lz", W.write_vp8l(70, 9, big, lz=False)))
    # all transforms, several orders (the sub-resolution images with a colour cache of their own in one of them)
    pm = lambda w, h, b: [int(v) for v in rng.integers(0, 14, _sub(w, b) * _sub(h, b))]
    out.append(("order-gpc", W.write_vp8l(70, 9, big, [("green",), ("predictor", 3, pm(70, 9, 3)), ("cross", 2, el(18 * 3))], cache_bits=4)))
    out.append(("order-pcg", W.write_vp8l(70, 9, big, [("predictor", 2, pm(70, 9, 2)), ("cross", 3, el(9 * 2)), ("green",)], sub_cache_bits=3)))
    out.append(("order-cgp", W.write_vp8l(70, 9, big, [("cross", 4, el(5)), ("green",), ("predictor", 4, pm(70, 9, 4))], cache_bits=1)))
    idx = [int(v) for v in rng.integers(0, 7, 45 * 9)]
    pal7 = [int(v) for v in rng.integers(0, 1 << 32, 7)]
    out.append(("order-all4-palette-first", W.write_vp8l(45, 9, idx, [("palette", pal7), ("predictor", 2, pm(23, 9, 2)), ("cross", 2, el(6 * 3)), ("green",)],
                                                        cache_bits=5, alpha=True)))
    out.append(("order-all4-palette-last", W.write_vp8l(45, 9, idx, [("green",), ("cross", 2, el(12 * 3)), ("predictor", 2, pm(45, 9, 2)), ("palette", pal7)])))
    out.append(("order-all4-palette-mid", W.write_vp8l(45, 9, idx, [("predictor", 3, pm(45, 9, 3)), ("palette", pal7), ("green",), ("cross", 2, el(6 * 3))])))
    # palettes: every bundling, widths that are no multiple of the bundle, an index past the palette
    for nc in (1, 2, 3, 4, 16, 17, 256):
        pal = [int(v) for v in rng.integers(0, 1 << 32, nc)]
        ix = [int(v) for v in rng.integers(0, nc, 13 * 5)]
        out.append(("palette-%d" % nc, W.write_vp8l(13, 5, ix, [("palette", pal)], alpha=True)))
        if nc in (1, 3, 17):
            ix2 = list(ix)
            for k in range(0, len(ix2), 4):
                ix2[k] = {1: 1, 3: 3, 17: 200}[nc]
            out.append(("palette-%d-index-past" % nc, W.write_vp8l(13, 5, ix2, [("palette", pal)], alpha=True)))
    # colour caches
    tile = _argb(text_tile(64, 24, 6, 0.05))
    for cb in (0, 1, 10, 11):
        out.append(("cache-%d" % cb, W.write_vp8l(64, 24, tile, cache_bits=cb, lz=cb != 10)))
    # simple codes of one and two symbols; the same through the code-length code (a lone symbol)
    two = [0xFF000000 | (int(v) << 8) for v in rng.integers(0, 2, 9 * 7) * 255]
    out.append(("simple-codes", W.write_vp8l(9, 7, two, lz=False)))
    out.append(("lone-symbol-normal", W.write_vp8l(9, 7, [0xFF102030] * 63, lz=False, code_opts=dict(style="normal"))))
    out.append(("two-symbols-normal-maxsym", W.write_vp8l(9, 7, two, lz=False, code_opts=dict(style="normal", max_symbol=True))))
    # a code of maximal length: red 0..15 with lengths 1, 2, ..., 14, 15, 15
    ramp = [0xFF000000 | (int(v) << 16) | (int(g) << 8) for v, g in zip(rng.integers(0, 16, 300), rng.integers(0, 256, 300))]
    ramp[:16] = [0xFF000000 | (v << 16) for v in range(16)]
    out.append(("length-15", W.write_vp8l(20, 15, ramp, lz=False, force_lens={(0, 1): list(range(1, 16)) + [15]})))
    # repeat codes that run across the green / length (256) and length / cache (280) boundaries
    lens = [9] * 240 + [8] * 32 + [3, 4, 4, 5] + [6] * 8
    out.append(("repeat-across-boundaries", W.write_vp8l(64, 24, tile, cache_bits=2, force_lens={(0, 0): lens})))
    out.append(("no-rle-maxsym", W.write_vp8l(64, 24, tile, cache_bits=2, code_opts=dict(rle=False, max_symbol=True))))
    # an entropy image with 400 groups
    a80 = _argb(_smooth(80, 80, 7))
    out.append(("groups-400", W.write_vp8l(80, 80, a80, meta=(2, list(range(400))), cache_bits=3)))
    out.append(("groups-sparse", W.write_vp8l(70, 9, big, meta=(3, [(k * 5) % 11 for k in range(9 * 2)]), transforms=[("green",)])))
    # copies: lengths 1, 64, 65, 4096; distances 1, 2, 63, 64, 65; crossing rows; ending on the last pixel
    cp = [(1, D(1)), (64, D(2)), (65, D(63)), (4096, D(64)), (300, D(65)), (64, D(1)), (1, D(64)), (65, D(65)), (64, D(63)), (130, D(3)), (7, D(70))]
    out.append(("copies", W.write_vp8l(70, 75, None, toks=_copy_tokens(70, 75, cp, 8), cache_bits=6, alpha=True)))
    out.append(("copies-no-cache", W.write_vp8l(70, 75, None, toks=_copy_tokens(70, 75, cp, 9))))
    # every short distance code, at a width where none clamps and at one where many clamp to 1
    out.append(("plane-codes-w20", W.write_vp8l(20, 30, None, toks=_copy_tokens(20, 30, [(2, k) for k in range(1, 121)], 10, lead=170), cache_bits=4)))
    out.append(("plane-codes-w4", W.write_vp8l(4, 120, None, toks=_copy_tokens(4, 120, [(2, k) for k in range(1, 121)], 11, lead=40))))
    # the longest lines the format has: 16384 x 1 and 1 x 16384
    line = np.repeat(rng.integers(0, 256, (256, 3), dtype=np.uint8), 64, axis=0)
    line[3000:6000] = rng.integers(0, 256, (3000, 3))
    la = _argb(line.reshape(1, 16384, 3))
    out.append(("wide-16384x1", W.write_vp8l(16384, 1, la, [("predictor", 4, [5] * 1024), ("green",)], cache_bits=7)))
    out.append(("tall-1x16384", W.write_vp8l(1, 16384, la, [("predictor", 5, [9] * 512), ("cross", 2, [(7, 250, 40)] * 4096)], cache_bits=3)))
    # containers
    exif = b"Exif\0\0MM\0*\0\0\0\x08\0\x01\x01\x12\0\x03\0\0\0\x01\0\x06\0\0\0\0\0\0"
    out.append(("vp8x-plain", W.write_vp8l(70, 9, big, [("green",)], vp8x=True)))
    out.append(("vp8x-chunks", W.write_vp8l(70, 9, big, [("green",)], vp8x=True, alpha=True,
                                            extra_chunks=[(b"ICCP", b"not a profile", True), (b"EXIF", exif, False), (b"abcd", b"odd", False)])))
    return out


@functools.lru_cache(maxsize=None)
def intact_cases():
    return pillow_cases() + writer_cases()


@functools.lru_cache(maxsize=None)
def refused_cases():
    """[(name, file bytes)]: valid WebP the device does not read (status -2)"""
    a = text_tile(40, 30, 12, 0.02)
    rgba = _as_mode(a, "RGBA", 12)
    frames = [Image.fromarray(a), Image.fromarray(255 - a)]
    b = io.BytesIO()
    frames[0].save(b, "WEBP", save_all=True, append_images=frames[1:], lossless=True, duration=100)
    return [("lossy", _save(Image.fromarray(a), quality=80)), ("lossy-alpha", _save(rgba, quality=80)), ("animated", b.getvalue())]


@functools.lru_cache(maxsize=None)
def sweep_bases():
    """the two files of about 1 KB the damage sweep is made from"""
    a = text_tile(96, 40, 13, 0.004)
    f1 = _save(Image.fromarray(a), lossless=True)
    rng = np.random.default_rng(14)
    b = _argb(text_tile(32, 20, 15, 0.02))
    f2 = W.write_vp8l(32, 20, b, [("predictor", 3, [int(v) for v in rng.integers(0, 14, 4 * 3)]), ("cross", 4, [(3, 250, 9)] * 4), ("green",)],
                      cache_bits=5, meta=(4, [k % 3 for k in range(2 * 2)]), vp8x=True)
    return [("pillow-text", f1), ("writer-transforms", f2)]


def flip(data, bit):
    d = bytearray(data)
    d[bit >> 3] ^= 1 << (bit & 7)
    return bytes(d)


def sweep():
    """yields (name, kind, file bytes): every single-bit flip and every truncation of the two base files"""
    for name, data in sweep_bases():
        for bit in range(8 * len(data)):
            yield "%s-flip%d" % (name, bit), "flip", flip(data, bit)
        for n in range(len(data)):
            yield "%s-cut%d" % (name, n), "cut", data[:n]


def sweep_sample(n, seed):
    """n files of the sweep, drawn without replacement"""
    files = list(sweep())
    pick = np.random.default_rng(seed).choice(len(files), n, replace=False)
    return [files[int(k)] for k in sorted(pick)]


@functools.lru_cache(maxsize=None)
def sweep_reference():
    """[(name, kind, file bytes, restatement status, restatement pixels or None)] over the whole sweep (computed once per process)"""
    import webp_reference as R
    out = []
    for name, kind, data in sweep():
        rc, px = R.decode(data)
        out.append((name, kind, data, rc, px))
    return out
