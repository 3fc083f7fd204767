"""Seeded JPEG 2000 files for the device decoder, written by Pillow (OpenJPEG).  The expected pixels of a file are always
Image.open(BytesIO(file)).convert('RGB').

intact() -> [(name, bytes)]: the files the decoder reads (status 0).   refused() -> [(name, bytes, word of the reason)]: valid files
outside the subset (-2).   damage_bases() / damage_sweep(): the three files of the damage tests and every damaged variant of them."""
import io

import numpy as np
from PIL import Image


def content(kind, h, w, mode, seed=0):
    """uint8 [h, w] (L) or [h, w, 3] (RGB)"""
    rng = np.random.default_rng(seed)
    ch = 3 if mode == "RGB" else 1
    if kind == "white":
        a = np.full((h, w, ch), 255, np.uint8)
    elif kind == "flat0":
        a = np.zeros((h, w, ch), np.uint8)
    elif kind == "flat255":
        a = np.full((h, w, ch), 255, np.uint8)
    elif kind == "noise":
        a = rng.integers(0, 256, (h, w, ch), dtype=np.uint8)
    elif kind == "page":   # a light ground with dark strokes and a little noise: what a scan looks like to the coder
        a = np.full((h, w, ch), 236, np.int32) + rng.integers(-3, 4, (h, w, ch))
        for _ in range(max(2, h * w // 400)):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            if rng.integers(0, 2):
                a[y:y + 2, x:x + int(rng.integers(2, 12))] = rng.integers(0, 60, ch)
            else:
                a[y:y + int(rng.integers(2, 9)), x:x + 2] = rng.integers(0, 60, ch)
        a = np.clip(a, 0, 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    return a[:, :, 0] if ch == 1 else a


def write(arr, **opts):
    im = Image.fromarray(arr)
    b = io.BytesIO()
    im.save(b, "JPEG2000", **opts)
    return b.getvalue()


def expected(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def text_page(h=300, w=420, seed=5):
    from lumina_ocr import synth
    return synth.synth_page(h, w, seed, n_lines=6)[0]


def intact():
    out = []

    def add(name, kind, h, w, mode, seed=1, **opts):
        opts.setdefault("irreversible", False)
        out.append((name, write(content(kind, h, w, mode, seed), **opts)))

    # sides
    add("s1x1_L", "noise", 1, 1, "L", num_resolutions=1)
    add("s1x1_RGB", "noise", 1, 1, "RGB", num_resolutions=1)
    add("s1x7_RGB", "noise", 1, 7, "RGB", num_resolutions=1)
    add("s5x3_L_r1", "noise", 5, 3, "L", num_resolutions=1)
    add("s5x3_RGB_r2", "noise", 5, 3, "RGB", num_resolutions=2)
    for h, w in ((63, 65), (64, 64), (65, 63), (129, 64), (100, 130)):
        add(f"s{h}x{w}_RGB", "page", h, w, "RGB", seed=h)
        add(f"s{h}x{w}_L", "page", h, w, "L", seed=w)
    # resolutions (7 = six decomposition levels)
    for nr in (1, 2, 3, 6, 7):
        add(f"res{nr}_RGB", "page", 100, 130, "RGB", seed=10 + nr, num_resolutions=nr)
        add(f"res{nr}_L_noise", "noise", 129, 64, "L", seed=20 + nr, num_resolutions=nr)
    # code-block sizes
    for cb in ((4, 4), (8, 64), (64, 8), (32, 32), (64, 64)):
        add(f"cb{cb[0]}x{cb[1]}_RGB", "page", 63, 65, "RGB", seed=30 + cb[0], codeblock_size=cb, num_resolutions=3)
        add(f"cb{cb[0]}x{cb[1]}_L", "noise", 65, 63, "L", seed=31 + cb[1], codeblock_size=cb, num_resolutions=3)
    # component transform
    for mct in (0, 1):
        add(f"mct{mct}", "noise", 64, 64, "RGB", seed=40, mct=mct)
        add(f"mct{mct}_page", "page", 100, 130, "RGB", seed=41, mct=mct)
    # progression orders, two layers
    for prog in ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL"):
        add(f"prog_{prog}", "page", 63, 65, "RGB", seed=50, progression=prog, quality_layers=[10, 2], num_resolutions=4)
        add(f"prog_{prog}_L", "noise", 65, 63, "L", seed=51, progression=prog, quality_layers=[10, 2], num_resolutions=3, codeblock_size=(16, 16))
    # lossy 5/3: blocks that stop early
    for mode in ("RGB", "L"):
        add(f"layers_rate_{mode}", "page", 100, 130, mode, seed=60, quality_layers=[40, 20, 5])
        add(f"layers_rate_noise_{mode}", "noise", 64, 64, mode, seed=61, quality_layers=[40, 20, 5])
        add(f"layers_db_{mode}", "page", 100, 130, mode, seed=62, quality_mode="dB", quality_layers=[30, 40])
        add(f"layers_db_noise_{mode}", "noise", 63, 65, mode, seed=63, quality_mode="dB", quality_layers=[30, 40])
    # container and markers
    add("no_jp2_RGB", "page", 63, 65, "RGB", seed=70, no_jp2=True)
    add("no_jp2_L", "page", 65, 63, "L", seed=71, no_jp2=True)
    add("plt_RGB", "page", 63, 65, "RGB", seed=72, plt=True)
    add("plt_layers_L", "page", 65, 63, "L", seed=73, plt=True, quality_layers=[20, 4])
    # contents
    for kind in ("white", "flat0", "flat255", "noise"):
        add(f"c_{kind}_RGB", kind, 64, 64, "RGB", seed=80)
        add(f"c_{kind}_L", kind, 65, 63, "L", seed=81)
    page = text_page()
    out.append(("text_page_RGB", write(page, irreversible=False)))
    out.append(("text_page_L_layers", write(page[:, :, 1].copy(), irreversible=False, quality_layers=[20, 5])))
    return out


def refused():
    a = content("page", 100, 130, "RGB", 3)
    return [
        ("irreversible", write(a, irreversible=True), "9/7"),
        ("tiles", write(a, irreversible=False, tile_size=(64, 64)), "tile"),
        ("precincts", write(a, irreversible=False, precinct_size=(64, 64)), "precinct"),
        ("codeblock_128x32", write(a, irreversible=False, codeblock_size=(128, 32)), "code-block side"),
        ("rgba", write(np.dstack([a, a[:, :, :1]]), irreversible=False), "cdef"),
        ("i16", write(content("noise", 40, 33, "L", 4).astype(np.uint16) * 257, irreversible=False), "bit depth"),
    ]


def damage_bases():
    return [
        ("rgb_layers", write(content("page", 33, 40, "RGB", 90), irreversible=False, quality_layers=[10, 2], num_resolutions=3)),
        ("grey_lossless", write(content("page", 64, 64, "L", 91), irreversible=False)),
        ("rgb_rlcp_cb8", write(content("page", 40, 33, "RGB", 92), irreversible=False, progression="RLCP", codeblock_size=(8, 8))),
    ]


def data_start(data):
    """offset of the first byte after the first SOD marker (the end of the headers)"""
    return data.index(b"\xff\x93") + 2


def damage_sweep(base):
    """[(name, bytes)]: every single-bit flip of the headers, every 7th bit of the data, truncation at every 16th byte."""
    out = []
    hdr = data_start(base)
    for bit in range(hdr * 8):
        b = bytearray(base)
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((f"h{bit}", bytes(b)))
    for bit in range(hdr * 8, len(base) * 8, 7):
        b = bytearray(base)
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((f"d{bit}", bytes(b)))
    for n in range(0, len(base), 16):
        out.append((f"t{n}", base[:n]))
    return out


_REF = {}


def reference(data):
    """jp2_reference.decode(data), computed once per distinct file of a test session -> (status, reason, info, rgb)"""
    import jp2_reference as jr
    got = _REF.get(data)
    if got is None:
        got = _REF[data] = jr.decode(data)
    return got


_SWEEP = []


def full_sweep():
    """[(base name, case name, bytes)] over the three bases, built once"""
    if not _SWEEP:
        for bname, base in damage_bases():
            _SWEEP.extend((bname, name, data) for name, data in damage_sweep(base))
    return _SWEEP


def sweep_sample(count, seed):
    """a seeded sample of the sweep, in sweep order"""
    sweep = full_sweep()
    pick = np.random.default_rng(seed).choice(len(sweep), size=count, replace=False)
    return [sweep[int(i)] for i in sorted(pick)]
