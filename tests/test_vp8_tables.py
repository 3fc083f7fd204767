"""CPU: the constant tables of csrc/vp8_tables.h against the read-only data of Pillow's bundled libwebp, where that library is present
(the pixels of tests/test_vp8_sanitized.py are the check that counts in any case).  Skips where Pillow links a system libwebp."""
import glob
import os
import re
import struct
from pathlib import Path

import PIL
import pytest

HEADER = Path(__file__).resolve().parent.parent / "ocr-system_amd" / "csrc" / "vp8_tables.h"
SIZES = {"vp8_coef_default": 1056, "vp8_coef_update": 1056, "vp8_bmode_proba": 900, "vp8_bmode_tree": 18, "vp8_dc_q": 128, "vp8_ac_q": 128,
         "vp8_zigzag": 16, "vp8_bands": 17, "vp8_cat3": 4, "vp8_cat4": 5, "vp8_cat5": 6, "vp8_cat6": 12}


def tables():
    text = HEADER.read_text()
    out = {}
    for m in re.finditer(r"VP8_HD int (\w+)\(int i\) \{\s*constexpr (\w+) t\[(\d+)\] = \{([^}]*)\}", text):
        out[m.group(1)] = (m.group(2), [int(v) for v in m.group(4).replace("\n", " ").split(",") if v.strip()])
    return out


def test_tables_have_their_sizes():
    t = tables()
    assert {k: len(v) for k, (_, v) in t.items()} == SIZES
    assert t["vp8_coef_default"][1][33:44] == [253, 136, 254, 255, 228, 219, 128, 128, 128, 128, 128]


def test_tables_are_libwebps():
    libs = glob.glob(os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs", "libwebp-*.so*"))
    if not libs:
        pytest.skip("Pillow has no bundled libwebp here")
    blob = Path(libs[0]).read_bytes()
    for name, (ctype, values) in tables().items():
        raw = struct.pack("<%dH" % len(values), *values) if ctype == "uint16_t" else bytes(v & 255 for v in values)
        assert raw in blob, name
