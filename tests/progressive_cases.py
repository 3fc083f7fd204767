"""Progressive JPEG files for the decoder tests (CPU: the restatement tests/progressive_reference.py against Pillow; GPU: the device
against Pillow).  Pillow writes most of them at test time from seeded images; the scan scripts Pillow cannot write are re-emitted from
a Pillow file's coefficients by progressive_reference.write_progressive.  Every expected value is Pillow's decode of the file."""
import functools
import io

import numpy as np
from PIL import Image

import progressive_reference as pr
from jpeg_cases import _image, pil_decode  # noqa: F401  (pil_decode: re-exported for the tests)

SAMPLING = {"grey": None, "444": 0, "422": 1, "420": 2}
SIZES = [(1, 1), (8, 8), (17, 13), (37, 53), (100, 75), (333, 211)]   # sides that are no multiple of 8 or of the MCU: the component raster differs from the padded grid
KINDS = ["noise", "smooth", "text"]
QUALITIES = [5, 50, 90, 100]


def _pillow_cases():
    out, k = [], 0
    for si, (w, h) in enumerate(SIZES):
        for mi, mode in enumerate(SAMPLING):
            kind = KINDS[(si + 2 * mi) % 3]
            if kind == "text" and min(w, h) < 37:   # (the text synthesiser needs room)
                kind = "noise"
            q = QUALITIES[(si + mi) % 4]
            out.append(("%s_%dx%d_%s_q%d" % (mode, w, h, kind, q), kind, w, h, 100 + k, dict(quality=q), mode))
            k += 1
    for mode in ("grey", "420", "444"):
        out.append(("%s_37x53_rstblocks3" % mode, "noise", 37, 53, 100 + k, dict(quality=90, restart_marker_blocks=3), mode))
        out.append(("%s_100x75_rstrows1" % mode, "text", 100, 75, 101 + k, dict(quality=50, restart_marker_rows=1), mode))
        k += 2
    out.append(("422_333x211_q100_rstrows1", "noise", 333, 211, 100 + k, dict(quality=100, restart_marker_rows=1), "422"))
    return out


# (name, kind, w, h, seed, save kwargs, "grey" | "444" | "422" | "420")
PILLOW = _pillow_cases()
WHITE = ("white_1032x1024_grey", "white", 1032, 1024, 0, dict(quality=90), "grey")        # 16512 blocks, all AC zero: one EOB run of category 14
NOISE_VGA = ("noise_640x480_420_q95", "noise", 640, 480, 7, dict(quality=95), "420")      # scans of several 256-byte chunks
BASE_420 = ("base_37x53_420", "noise", 37, 53, 4, dict(quality=90), "420")                # the 37 x 53 4:2:0 file of the damage sweep and the writer scripts
BASE_444 = ("base_100x75_444", "text", 100, 75, 5, dict(quality=85), "444")


def pillow_file(case) -> bytes:
    name, kind, w, h, seed, kw, mode = case
    arr = np.full((h, w, 3), 255, np.uint8) if kind == "white" else _image(kind, w, h, seed)
    im = Image.fromarray(arr)
    kw = dict(kw)
    if mode == "grey":
        im = im.convert("L")
    else:
        kw["subsampling"] = SAMPLING[mode]
    buf = io.BytesIO()
    im.save(buf, format="JPEG", progressive=True, **kw)
    return buf.getvalue()


def _ac(comps, bands, ah, al):
    return [((c,), lo, hi, ah, al) for c in comps for lo, hi in bands]


ALL = (0, 1, 2)
# name -> (base case, script [(components, Ss, Se, Ah, Al)], restart interval per scan or None, all tables before the first scan)
SCRIPTS = {
    "spectral_only": (BASE_420, [(ALL, 0, 0, 0, 0)] + _ac(ALL, [(1, 5), (6, 63)], 0, 0), None, False),
    "depth_3_2_1_0": (BASE_444, [(ALL, 0, 0, 0, 3)] + _ac(ALL, [(1, 63)], 0, 3) + [(ALL, 0, 0, 3, 2)] + _ac(ALL, [(1, 63)], 3, 2)
                      + [(ALL, 0, 0, 2, 1)] + _ac(ALL, [(1, 63)], 2, 1) + [(ALL, 0, 0, 1, 0)] + _ac(ALL, [(1, 63)], 1, 0), None, False),
    "dc_per_component": (BASE_420, [((0,), 0, 0, 0, 1), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 1)] + _ac(ALL, [(1, 63)], 0, 0)
                         + [((2,), 0, 0, 1, 0), ((0,), 0, 0, 1, 0)], None, False),
    "bands_1_2_9_63": (BASE_444, [(ALL, 0, 0, 0, 0)] + _ac(ALL, [(1, 1), (2, 2), (3, 9), (10, 63)], 0, 0), None, False),
    "tables_first": (BASE_420, [(ALL, 0, 0, 0, 1)] + _ac(ALL, [(1, 5)], 0, 1) + _ac(ALL, [(6, 63)], 0, 1) + [(ALL, 0, 0, 1, 0)]
                     + _ac(ALL, [(1, 63)], 1, 0), None, True),
    "restart_single_component": (BASE_420, [((0,), 0, 0, 0, 1), ((1, 2), 0, 0, 0, 1)] + _ac(ALL, [(1, 63)], 0, 2) + _ac(ALL, [(1, 63)], 2, 1)
                                 + [((0,), 0, 0, 1, 0), ((1, 2), 0, 0, 1, 0)] + _ac(ALL, [(1, 63)], 1, 0),
                                 [2, 1, 3, 1, 2, 4, 3, 1, 5, 2, 3, 2, 1], False),
}


@functools.lru_cache(maxsize=None)
def script_file(name: str) -> bytes:
    base, script, restarts, tables_first = SCRIPTS[name]
    fr, coefs = pr.decode(pillow_file(base))
    return pr.write_progressive(fr, coefs, script, restarts, tables_first)


@functools.lru_cache(maxsize=None)
def all_files():
    """[(name, width, height, file bytes)] of every case: Pillow's files, the two large ones, the writer's scripts."""
    out = [(c[0], c[2], c[3], pillow_file(c)) for c in PILLOW + [WHITE, NOISE_VGA, BASE_420, BASE_444]]
    for name, (base, _, _, _) in SCRIPTS.items():
        out.append((name, base[2], base[3], script_file(name)))
    return out


def grey_script_file() -> bytes:
    """A grey file re-emitted with a restart interval in every scan (single-component DC and AC scans of a one-component frame)."""
    fr, coefs = pr.decode(pillow_file(PILLOW[12]))   # grey 37 x 53
    assert fr.ncomp == 1
    return pr.write_progressive(fr, coefs, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)], [4, 3, 5])


def drop_last_scans(data: bytes, k: int) -> bytes:
    """The file with its last k scans (and their tables) cut off and EOI appended: Pillow decodes it, short of full precision."""
    keep = pr.parse(data).scans[-k - 1]
    return data[:keep["off"] + len(keep["data"])] + b"\xff\xd9"


def cut_inside_last_scan(data: bytes) -> bytes:
    last = pr.parse(data).scans[-1]
    return data[:last["off"] + len(last["data"]) // 2] + b"\xff\xd9"


def swap_ah(data: bytes) -> bytes:
    """The last scan's Ah (1 in Pillow's script) raised to 2: not the successor of the coefficients' last scan."""
    last = pr.parse(data).scans[-1]
    p = last["off"] - 1
    assert data[p] == 0x10
    return data[:p] + b"\x21" + data[p + 1:]


def damage_corpus():
    """[(name, bytes)]: the 37 x 53 4:2:0 file undamaged, with flips in its JFIF density bytes, 300 single-bit flips and 120 truncations"""
    base = pillow_file(BASE_420)
    assert base[6:11] == b"JFIF\0"
    rng = np.random.default_rng(20241)
    out = [("clean", base)]
    for pos in (14, 15, 16, 17):                                   # JFIF X / Y density: no decoder reads them
        out.append(("density_%d" % pos, base[:pos] + bytes([base[pos] ^ 0x04]) + base[pos + 1:]))
    for k in range(300):                                           # single-bit flips anywhere in the file
        pos, bit = int(rng.integers(2, len(base) - 2)), int(rng.integers(0, 8))
        out.append(("flip_%d_%d" % (pos, bit), base[:pos] + bytes([base[pos] ^ (1 << bit)]) + base[pos + 1:]))
    for k in range(60):                                            # truncations, with and without an EOI after the cut
        pos = int(rng.integers(20, len(base) - 2))
        out.append(("cut_%d" % pos, base[:pos]))
        out.append(("cut_eoi_%d" % pos, base[:pos] + b"\xff\xd9"))
    return out


def repeated_first_scan_file() -> bytes:
    """The spectral_only file with its first DC scan sent twice, the second time with every DC value 7 higher: libjpeg decodes the scans in
    file order without a warning and the later one wins (-> the file, and the file the later scan alone would give)."""
    base, script, _, _ = SCRIPTS["spectral_only"]
    fr, coefs = pr.decode(pillow_file(base))
    plain = pr.write_progressive(fr, coefs, script)
    raised = [c.copy() for c in coefs]
    for c in raised:
        c[:, :, 0] += 7
    other = pr.write_progressive(fr, raised, script)
    a, b = pr.parse(plain).scans[0], pr.parse(other).scans[0]
    dht = other.index(b"\xff\xc4")                      # the second copy's first scan with its tables: DHT ... SOS ... data
    return plain[:a["off"] + len(a["data"])] + other[dht:b["off"] + len(b["data"])] + plain[a["off"] + len(a["data"]):], other
