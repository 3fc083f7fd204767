"""GPU: the device PNG decoder on the damaged corpus of tests/png_damage.py, graded file for file against Pillow: status 0 implies that
Pillow decodes the file to identical bytes, and every undamaged base is accepted.  Prints the acceptance count per base."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_damage
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu


def _pillow(data):
    try:
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    except Exception:
        return None


# the cases each rule of the acceptance rule exists to refuse, with the status it gives (several of them Pillow decodes: the device is
# stricter on purpose, and dropping a check must fail here)
MUST_REFUSE = {
    "adler_bad": -1, "after_adler": -1, "missing_iend": -1, "iend_bad_crc": -1, "ihdr_bad_crc": -1,
    "after_iend": -2, "chunk_after_idat": -2, "chunk_between_idat": -2,
    "zlib_cm7": -1, "zlib_fcheck": -1, "zlib_fdict": -1, "zlib_cinfo8": -1,
    "filter_5": -1, "filter_6": -1, "filter_17": -1, "filter_128": -1, "filter_255": -1,
    "pal_index_12": -1, "pal_index_15": -1, "pal8_index_100": -1,
    "craft_btype3": -1, "craft_stored_bad_nlen": -1, "craft_sym286": -1, "craft_sym287": -1, "craft_dist30": -1, "craft_dist31": -1,
    "craft_dist_too_far": -1, "craft_window_256": -1, "craft_cl_oversubscribed": -1, "craft_cl_incomplete": -1, "craft_cl_empty": -1,
    "craft_hlit_287": -1, "craft_hdist_31": -1, "craft_lit_oversubscribed": -1, "craft_lit_incomplete": -1,
    "craft_short_output": -1, "craft_long_output": -1,
}


def test_accepted_damaged_files_equal_pillow(engine):
    corpus = png_damage.corpus()
    groups = {}
    for base, name, data in corpus:
        rc, info = Engine.png_probe(data)
        groups.setdefault((info["height"], info["width"]) if info["width"] > 0 and info["height"] > 0 else (1, 1), []).append((base, name, data))
    accepted, total, wrong = {}, {}, []
    for (h, w), group in groups.items():
        if h * w > 1 << 24:
            continue
        out, status = engine.png_decode([d for _, _, d in group], h, w)
        torch.cuda.synchronize()
        for k, (base, name, data) in enumerate(group):
            total[base] = total.get(base, 0) + 1
            if name in ("undamaged", "pal_ok", "pal8_ok", "craft_good_fixed", "craft_stored_ok", "craft_window_32k"):
                assert status[k] == 0, (base, name, status[k])
            if name in MUST_REFUSE or name.startswith("trunc_"):
                want_rc = MUST_REFUSE.get(name, -1)
                if status[k] != want_rc:
                    wrong.append((base, name, "status %d, expected %d" % (status[k], want_rc)))
            if status[k] != 0:
                continue
            accepted[base] = accepted.get(base, 0) + 1
            want = _pillow(data)
            if want is None or want.shape != (h, w, 3) or not np.array_equal(out[k].cpu().numpy(), want):
                wrong.append((base, name))
    print("device acceptance per base: " + ", ".join("%s %d/%d" % (b, accepted.get(b, 0), total[b]) for b in total))
    assert not wrong, wrong
    assert sum(total.values()) == len(corpus)
