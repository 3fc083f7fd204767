"""GPU: the device JPEG decoder (csrc/jpegdec.hip) on the damaged and hostile corpus of tests/jpeg_damage.py.

The contract: status 0 => byte-identical to Pillow; anything else is left to Pillow (the provider falls back to it).  The device
must accept exactly the files the oracle accepts (tests/test_jpegdec_damaged.py holds the oracle to every SIMD choice of Pillow),
leave every refused page unwritten, keep its clean neighbours in the same batch exact, give the same statuses through the
asynchronous entry point, and still decode cleanly afterwards.  Set LUMINA_JPEG_DAMAGE_STATS to a file name to get the per-base
acceptance counts as JSON."""
import io
import json
import os
from collections import defaultdict

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_damage as jd
from jpeg_cases import pil_decode
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
BATCH = 64
CLEAN_AT = (0, 21, 42, 63)          # fixed positions of the clean neighbours in every batch


def _clean(w, h):
    rng = np.random.default_rng(w * 7919 + h)
    buf = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=90)
    return buf.getvalue()


def _oracle_accepts(data):
    from oracle import jpeg as oj
    if oj.info(data)[0] != 0:
        return None
    try:
        return oj.decode(data)
    except ValueError:
        return None


def _pil(data):
    try:
        return pil_decode(data)
    except OSError:                 # Pillow cannot decode it at all
        return None


def _base_of(name):
    return next((b for b in jd.BASES if name.startswith(b + "_")), name.split("_")[0])


@pytest.fixture(scope="module")
def batches():
    """[(h, w, [(name, bytes)] of <= 64 with clean files at CLEAN_AT)] — the corpus grouped by the size its header declares"""
    groups = defaultdict(list)
    for name, data in jd.corpus():
        rc, info = Engine.jpeg_probe(data)
        size = (info["height"], info["width"]) if info["width"] > 0 and info["height"] > 0 else (48, 64)
        groups[size].append((name, data))
    out = []
    per = BATCH - len(CLEAN_AT)
    for (h, w), items in sorted(groups.items()):
        clean = _clean(w, h)
        for i in range(0, len(items), per):
            chunk = list(items[i:i + per])
            for p in CLEAN_AT:
                if p <= len(chunk):
                    chunk.insert(p, ("clean_%dx%d" % (w, h), clean))
            out.append((h, w, chunk))
    return out


def test_device_accepts_what_the_oracle_accepts_and_equals_pillow(engine, batches):
    stats = defaultdict(lambda: [0, 0])                # base -> [device accepted, entries]
    mismatched, written, wrong = [], [], []
    for h, w, items in batches:
        files = [d for _, d in items]
        out = torch.full((len(files), h, w, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        out, status = engine.jpeg_decode(files, h, w, out=out)
        torch.cuda.synchronize()
        pages = out.cpu().numpy()
        for k, (name, data) in enumerate(items):
            if name.startswith("clean_"):
                assert status[k] == 0 and np.array_equal(pages[k], pil_decode(data)), (name, k, status[k])
                continue
            want = _oracle_accepts(data)
            st = stats[_base_of(name)]
            st[1] += 1
            st[0] += status[k] == 0
            if status[k] == 0 and not (np.array_equal(pages[k], _pil(data)) and (want is None or np.array_equal(pages[k], want))):
                wrong.append(name)
            if (status[k] == 0) != (want is not None):
                mismatched.append((name, status[k]))
            if status[k] != 0 and not (pages[k] == SENTINEL).all():
                written.append((name, status[k]))
    path = os.environ.get("LUMINA_JPEG_DAMAGE_STATS")
    if path:
        with open(path, "w") as f:
            json.dump({b: dict(accepted=a, entries=n) for b, (a, n) in sorted(stats.items())}, f, indent=1)
    assert not wrong, "%d accepted, but not Pillow's (or the oracle's) pixels: %s" % (len(wrong), wrong[:20])
    assert not mismatched, "%d: device and oracle accept different files (name, device status): %s" % (len(mismatched), mismatched[:20])
    assert not written, "refused pages were written: %s" % written[:20]
    for b in jd.BASES:
        assert 0 < stats[b][0] < stats[b][1], (b, stats[b])       # refusal did not become "refuse everything"


def test_async_decode_gives_the_same_statuses_and_pages(engine, batches):
    for h, w, items in batches:
        files = [d for _, d in items]
        ref, st_ref = engine.jpeg_decode(files, h, w)
        passes = max(len(f) for f in files) // 1024 + 4                # a chunk decoder is exact after (its index + 1) passes
        out = torch.full((len(files), h, w, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        out, st = engine.jpeg_decode_async(files, h, w, out=out, passes=passes)
        torch.cuda.synchronize()
        assert st.tolist() == st_ref, [(items[k][0], a, b) for k, (a, b) in enumerate(zip(st.tolist(), st_ref)) if a != b]
        for k, s in enumerate(st_ref):
            if s == 0:
                assert torch.equal(out[k], ref[k]), items[k][0]
            else:
                assert bool((out[k] == SENTINEL).all()), items[k][0]


def test_clean_decode_after_the_corpus_is_still_exact(engine, batches):
    for h, w, items in batches[:3]:
        engine.jpeg_decode([d for _, d in items], h, w)
    base = jd.base_file("rstrow_420")
    clean = [base, _clean(256, 192), base]
    out, status = engine.jpeg_decode(clean, 192, 256)
    torch.cuda.synchronize()
    assert status == [0, 0, 0]
    for k, f in enumerate(clean):
        assert np.array_equal(out[k].cpu().numpy(), pil_decode(f)), k


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    yield s
    s.cleanup()


@pytest.mark.parametrize("name", ["hdr_dht_dc_oversub_len1", "rstrow_420_rst_dup1"])
def test_provider_gives_the_host_result_for_damaged_uploads(service, name):
    """An upload the device must refuse goes through process_image_sync exactly as with device_jpeg=False (Pillow decodes it)."""
    data = dict(jd.corpus())[name]
    s = service
    s.device_jpeg = False
    host = s.process_image_sync(data)
    s.device_jpeg = True
    dev = s.process_image_sync(data)
    for field in ("success", "error", "layout_boxes", "markdown", "processed_image_bytes", "image_width", "image_height"):
        assert getattr(dev, field) == getattr(host, field), field
