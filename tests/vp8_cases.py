"""Lossy WebP (VP8) test files: intact files from Pillow's encoder and from the test-side writer (vp8_writer.py), the refused kinds,
the files just beyond the coefficient bound, and the damage sweep of two files.  The
expectation of every intact case is Pillow's own decode of the file: pillow_rgb(data).

The reconstruction kernel (csrc/vp8dec.hip, vp8_recon) handles 16 macroblocks of a diagonal at a time; the case "pillow-1056x272" is
66 macroblocks wide (more than twice that) and 17 high."""
import functools
import io
import struct

import numpy as np
from PIL import Image

import vp8_writer as W
from webp_cases import flip, pillow_rgb, text_tile   # noqa: F401  (re-exported)

RECON_MBS = 16   # macroblocks of a diagonal the reconstruction kernel handles at a time
WIDE = (1056, 272)


def _save(im, **kw):
    b = io.BytesIO()
    im.save(b, "WEBP", **kw)
    return b.getvalue()


def _picture(w, h, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "text":
        return text_tile(w, h, seed, 0.02)
    # smooth ramps with edges and a few noisy patches: every kind of macroblock
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([(x * 3 + y) & 255, (x + y * 5 + 40) & 255, ((x * y) >> 3) & 255], axis=-1).astype(np.uint8)
    a[(x // 23 + y // 17) % 3 == 0] = (250, 250, 245)
    m = rng.random((h, w)) < 0.03
    a[m] = rng.integers(0, 256, (int(m.sum()), 3))
    return a


SHAPES = ((1, 1), (16, 16), (17, 17), (15, 33), (33, 15), (48, 48), (1, 40), (40, 1), (130, 70), (200, 300), (16383, 16), (16, 16383), WIDE)
QUALITIES = (0, 50, 80, 95, 100)
METHODS = (0, 4, 6)


@functools.lru_cache(maxsize=None)
def pillow_cases():
    """[(name, file bytes)]: quality 0 / 50 / 80 / 95 / 100 x method 0 / 4 / 6 in modes RGB and L at the small shapes; the two
    16383-pixel strips and the wide case once per quality (methods in turn), RGB"""
    out = []
    for si, (w, h) in enumerate(SHAPES):
        large = w * h >= 200000   # (the two 16383-pixel strips and the wide case run once per quality; 200 x 300 has the whole matrix)
        for mode in ("RGB", "L"):
            for qi, quality in enumerate(QUALITIES):
                for method in METHODS:
                    if large and (mode != "RGB" or method != METHODS[qi % 3]):
                        continue
                    seed = si * 1000 + method * 10 + quality
                    kind = "text" if (w, h) == (200, 300) else ("noise" if (quality == 100 and not large) else "mixed")
                    im = Image.fromarray(_picture(w, h, seed, kind)).convert(mode)
                    out.append(("pillow-%dx%d-%s-m%d-q%d" % (w, h, mode, method, quality), _save(im, quality=quality, method=method)))
    return out


def _chunks(data):
    """[(tag, payload)] of a RIFF / WEBP file"""
    out, p = [], 12
    while p < len(data):
        size = struct.unpack("<I", data[p + 4:p + 8])[0]
        out.append((data[p:p + 4], data[p + 8:p + 8 + size]))
        p += 8 + size + (size & 1)
    return out


def riff(chunks):
    body = b"WEBP" + b"".join(t + struct.pack("<I", len(d)) + d + (b"\0" if len(d) & 1 else b"") for t, d in chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def vp8x(flags, w, h):
    return (b"VP8X", bytes([flags, 0, 0, 0]) + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3])


EXIF6 = b"MM\0*\0\0\0\x08\0\x01\x01\x12\0\x03\0\0\0\x01\0\x06\0\0\0\0\0\0"   # orientation 6


@functools.lru_cache(maxsize=None)
def container_cases():
    """[(name, file bytes)]: the lossy chunk inside VP8X with ICCP, EXIF and unknown chunks; non-zero scale bits"""
    a = _picture(40, 30, 21, "mixed")
    bare = _save(Image.fromarray(a), quality=70)
    (tag, vp8), = _chunks(bare)
    assert tag == b"VP8 "
    out = [("vp8x-plain", riff([vp8x(0, 40, 30), (b"VP8 ", vp8)])),
           ("vp8x-chunks", riff([vp8x(0x28, 40, 30), (b"ICCP", b"not a profile"), (b"VP8 ", vp8), (b"EXIF", EXIF6), (b"abcd", b"odd")]))]
    s = bytearray(vp8)
    s[7] |= 0x40; s[9] |= 0x80   # the scale bits, which libwebp ignores
    out.append(("scale-bits", riff([(b"VP8 ", bytes(s))])))
    return out


def _grid(w, h, seed, **kw):
    rng = np.random.default_rng(seed)
    return [W.random_mb(rng, **kw) for _ in range(((w + 15) >> 4) * ((h + 15) >> 4))]


@functools.lru_cache(maxsize=None)
def writer_cases():
    """[(name, file bytes)]: the streams libwebp's encoder never writes (tests/vp8_writer.py), all decoded by Pillow"""
    out = []
    add = lambda name, w, h, mbs, **kw: out.append((name, W.write_vp8(w, h, mbs, **kw)))
    # every 16x16 / chroma mode and every 4x4 sub-mode on every border, corner and interior macroblock (3 x 3), with residuals
    for m in range(4):
        mbs = _grid(40, 40, 100 + m, i4=0)
        for mb in mbs:
            mb["ymode"] = mb["uvmode"] = m
        add("mode16-%d" % m, 40, 40, mbs, base_q=30)
    for sm in range(10):
        mbs = _grid(48, 48, 110 + sm, i4=1)
        for mb in mbs:
            mb["sub"] = [sm] * 16
        add("submode-%d" % sm, 48, 48, mbs, base_q=30)
    for k in range(6):
        add("modes-mixed-%d" % k, 70, 50, _grid(70, 50, 130 + k), base_q=10 + 12 * k, level=8 * k)
    # loop filters: simple and normal, levels, sharpness, deltas
    for lv in (1, 14, 15, 39, 40, 63):
        add("simple-level%d" % lv, 50, 40, _grid(50, 40, 200 + lv), simple=True, level=lv, base_q=60)
        add("normal-level%d" % lv, 50, 40, _grid(50, 40, 300 + lv), level=lv, base_q=60)
    for sh in (1, 4, 5, 7):
        add("sharpness-%d" % sh, 50, 40, _grid(50, 40, 400 + sh), level=40, sharpness=sh, base_q=70)
        add("sharpness-%d-simple" % sh, 50, 40, _grid(50, 40, 410 + sh), simple=True, level=25, sharpness=sh, base_q=70)
    add("lf-delta-no-update", 50, 40, _grid(50, 40, 420), level=30, base_q=60, lf_delta=dict(update=0))
    add("lf-delta-positive", 50, 40, _grid(50, 40, 421), level=30, base_q=60, lf_delta=dict(update=1, ref=(10, None, 5, None), mode=(20, 3, None, None)))
    add("lf-delta-negative", 50, 40, _grid(50, 40, 422), level=30, base_q=60, lf_delta=dict(update=1, ref=(-12, None, None, -63), mode=(-15, None, None, 7)))
    add("lf-delta-to-zero", 50, 40, _grid(50, 40, 423), level=10, base_q=60, lf_delta=dict(update=1, ref=(-3, None, None, None), mode=(-20, None, None, None)))
    add("lf-delta-to-63", 50, 40, _grid(50, 40, 424), simple=True, level=50, base_q=60, lf_delta=dict(update=1, ref=(40, None, None, None), mode=(63, None, None, None)))
    # token partitions, on pictures with fewer and with more macroblock rows than partitions
    for lp in (1, 2, 3):
        add("parts-%d-rows3" % (1 << lp), 40, 40, _grid(40, 40, 500 + lp), log2_parts=lp, base_q=50, level=12)
        add("parts-%d-rows11" % (1 << lp), 36, 170, _grid(36, 170, 510 + lp), log2_parts=lp, base_q=50, level=12, simple=lp == 2)
    # segments
    seg = lambda **kw: dict(kw)
    add("segments-delta", 70, 50, _grid(70, 50, 600, segs=4, density=0.08, big=0), base_q=60, level=20,
        segments=seg(update_map=1, probs=(120, 200, 60), data=dict(absolute=0, quant=(-60, 20, None, 67), level=(-20, 43, None, 10))))
    add("segments-absolute", 70, 50, _grid(70, 50, 601, segs=4, density=0.08, big=0), base_q=60, level=20, simple=True,
        segments=seg(update_map=1, probs=(None, 100, None), data=dict(absolute=1, quant=(0, 127, 30, None), level=(0, 63, None, 33))))
    add("segments-map-only", 70, 50, _grid(70, 50, 602, segs=4), base_q=60, level=20, segments=seg(update_map=1, probs=(90, 90, 90), data=None))
    add("segments-data-only", 70, 50, _grid(70, 50, 603, density=0.08, big=0), base_q=60, level=20,
        segments=seg(update_map=0, data=dict(absolute=0, quant=(25, 1, 2, 3), level=(9, 1, 2, 3))))
    add("segments-levels-clipped", 70, 50, _grid(70, 50, 604, segs=4), base_q=60, level=30,
        segments=seg(update_map=1, probs=(128, 128, 128), data=dict(absolute=0, quant=(None,) * 4, level=(-30, -63, 33, 63))))
    # quantisers: every delta at both clip ends
    add("quant-low-clip", 40, 40, _grid(40, 40, 700), base_q=3, dq=(-15, -15, -15, -15, -15))
    add("quant-high-clip", 40, 40, _grid(40, 40, 701, density=0.08, big=0), base_q=120, dq=(15, 15, 15, 15, 15))
    add("quant-mixed", 40, 40, _grid(40, 40, 702), base_q=64, dq=(7, -8, None, 15, -15))
    # the skip probability: absent with all-zero macroblocks present and the filter on; present with skipped macroblocks of both kinds
    mbs = _grid(70, 50, 800)
    for k in (0, 3, 7, 8, 12, 19):
        mbs[k] = dict(i4=0, ymode=k % 4, uvmode=(k + 1) % 4)
    add("no-skip-prob-zero-mbs", 70, 50, mbs, base_q=40, level=35)
    add("no-skip-prob-zero-mbs-simple", 70, 50, mbs, base_q=40, level=35, simple=True)
    add("skip-prob", 70, 50, _grid(70, 50, 801, skip_allowed=True), base_q=40, level=35, skip_prob=150)
    add("skip-prob-simple", 70, 50, _grid(70, 50, 802, skip_allowed=True), base_q=40, level=20, simple=True, skip_prob=40)
    # tokens: each category with its extremes, EOB at every position, the largest cat6 value inside the coefficient bound
    vals = [1, 2, 3, 4, 5, 6, 7, 10, 11, 18, 19, 34, 35, 66, 67, 300]
    mbs = []
    for k in range(9):
        y = [[0] * 16 for _ in range(16)]
        for b in range(16):
            y[b][(b + k) % 16] = vals[(b + 3 * k) % 16] * (-1 if (b + k) & 1 else 1)   # the last non-zero level at every position
        mbs.append(dict(i4=1, sub=[(b + k) % 10 for b in range(16)], y=y, u=[[vals[k], 0, -vals[15 - k]] + [0] * 13] * 4, v=[[0] * 15 + [2]] * 4))
    add("token-categories", 48, 48, mbs, base_q=10)
    # steps at base_q 6: 10 / 10 / 20 / 15.  A block sum of exactly 19000, and a Y2 sum of 1638 * 20 = 32760 <= 32764
    inside = [dict(i4=1, sub=[0] * 16, y=[[1900] + [0] * 15] + [[0] * 16] * 15), dict(i4=0, ymode=0, y2=[1638] + [0] * 15)]
    add("bound-inside", 32, 16, inside, base_q=6)
    # coefficient-probability updates
    add("coef-updates", 70, 50, _grid(70, 50, 900), base_q=40, coef_updates={i: (i * 37 + 11) % 255 + 1 for i in range(0, 1056, 5)})
    # header bits libwebp ignores, a higher profile, the VP8X container
    add("scale-colour-clamp-bits", 40, 40, _grid(40, 40, 901), base_q=40, color_space=1, clamp=1, scale=(1, 3))
    add("profile-3-vp8x", 40, 40, _grid(40, 40, 902), base_q=40, profile=3, vp8x=True, level=10)
    return out


@functools.lru_cache(maxsize=None)
def bound_cases():
    """[(name, file bytes, status)]: just beyond the coefficient bound (Pillow reads them; the device refuses them)"""
    y_beyond = [dict(i4=1, sub=[0] * 16, y=[[1901] + [0] * 15] + [[0] * 16] * 15)]
    y2_beyond = [dict(i4=0, ymode=0, y2=[1639] + [0] * 15)]
    return [("bound-block-beyond", W.write_vp8(16, 16, y_beyond, base_q=6), -1), ("bound-y2-beyond", W.write_vp8(16, 16, y2_beyond, base_q=6), -1)]


@functools.lru_cache(maxsize=None)
def intact_cases():
    return pillow_cases() + container_cases() + writer_cases()


@functools.lru_cache(maxsize=None)
def refused_cases():
    """[(name, file bytes, status)]"""
    a = _picture(40, 30, 22, "mixed")
    bare = _save(Image.fromarray(a), quality=80)
    (_, vp8), = _chunks(bare)
    rgba = Image.fromarray(a).convert("RGBA")
    rgba.putalpha(Image.fromarray(np.random.default_rng(3).integers(0, 256, a.shape[:2], dtype=np.uint8)))
    frames = [Image.fromarray(a), Image.fromarray(255 - a)]
    b = io.BytesIO()
    frames[0].save(b, "WEBP", save_all=True, append_images=frames[1:], quality=80, duration=100)
    lossless = _chunks(_save(Image.fromarray(a), lossless=True))[0][1]
    inter = bytearray(vp8); inter[0] |= 1
    hidden = bytearray(vp8); hidden[0] &= ~0x10
    return [("lossy-alpha", _save(rgba, quality=80), -2), ("animated", b.getvalue(), -2),
            ("inter-frame", riff([(b"VP8 ", bytes(inter))]), -1), ("show-frame-0", riff([(b"VP8 ", bytes(hidden))]), -1),
            ("vp8-and-vp8l", riff([vp8x(0, 40, 30), (b"VP8 ", vp8), (b"VP8L", lossless)]), -1),
            ("canvas-mismatch", riff([vp8x(0, 41, 30), (b"VP8 ", vp8)]), -1)]


@functools.lru_cache(maxsize=None)
def sweep_bases():
    """the two files of about 1 KB the damage sweep is made from: Pillow at quality 50, and the writer with 2 partitions, the simple
    filter and segments"""
    f2 = W.write_vp8(64, 48, _grid(64, 48, 77, segs=4, skip_allowed=True), base_q=45, level=22, simple=True, log2_parts=1, skip_prob=90,
                     segments=dict(update_map=1, probs=(100, 150, 80), data=dict(absolute=0, quant=(-20, 10, None, 25), level=(5, -10, None, 20))))
    return [("pillow-q50", _save(Image.fromarray(text_tile(64, 48, 13, 0.004)), quality=50)), ("writer-parts2-simple-segments", f2)]


def sweep():
    """yields (name, kind, file bytes): every single-bit flip and every truncation of the two base files"""
    for name, data in sweep_bases():
        for bit in range(8 * len(data)):
            yield "%s-flip%d" % (name, bit), "flip", flip(data, bit)
        for n in range(len(data)):
            yield "%s-cut%d" % (name, n), "cut", data[:n]


def sweep_sample(n, seed):
    files = list(sweep())
    pick = np.random.default_rng(seed).choice(len(files), n, replace=False)
    return [files[int(k)] for k in sorted(pick)]


@functools.lru_cache(maxsize=None)
def sweep_reference():
    """[(name, kind, file bytes, restatement status, reason, pixels or None)] over the whole sweep (computed once per process)"""
    import vp8_reference as R
    return [(name, kind, data) + R.decode(data) for name, kind, data in sweep()]


# what the restatement accepts of the sweep (Pillow 12.2 / libwebp 1.6 wrote the first file): flips, truncations
SWEEP_ACCEPTED = {"flip": 17319, "cut": 0}
