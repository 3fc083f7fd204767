"""CPU: the plain-Python restatement of the lossless-WebP reader (tests/webp_reference.py) against Pillow (libwebp).  On every intact
case, from Pillow's encoder and from the test-side writer, it gives Pillow's bytes.  Over the damage sweep (every single-bit flip and every
truncation of two files of about 1 KB) every file it accepts decodes to Pillow's bytes, so it accepts none where Pillow raises; it refuses
every truncation; and it still accepts at least a quarter of the flips, so the sweep cannot pass by refusing everything."""
import io

import numpy as np
from PIL import Image

import webp_cases as wc
import webp_reference as wr
import webp_writer as ww


def test_every_writer_file_is_valid_for_pillow():
    for name, data in wc.writer_cases():
        assert wc.pillow_rgb(data) is not None, name


def test_writer_covers_the_longest_lines_and_the_code_tables():
    shapes = {wr.probe(data)[1]["width"]: wr.probe(data)[1]["height"] for _, data in wc.writer_cases()}
    assert shapes.get(16384) == 1 and shapes.get(1) == 16384
    # the writer's table of the 120 short distance codes and the restatement's were written down apart; Pillow arbitrates through the
    # plane-codes cases, and the two must agree
    for k in range(120):
        c = wr.CODE_TO_PLANE[k]
        assert (8 - (c & 15), c >> 4) == ww.PLANE[k], k


def test_intact_cases_equal_pillow():
    cases = wc.intact_cases()
    assert len(cases) > 450
    for name, data in cases:
        rc, got = wr.decode(data)
        assert rc == 0, (name, rc)
        assert np.array_equal(got, wc.pillow_rgb(data)), name


def test_refused_cases():
    for name, data in wc.refused_cases():
        assert wr.decode(data)[0] == -2, name
        assert wc.pillow_rgb(data) is not None, name   # (valid files: Pillow reads them)


def test_rgba_is_not_premultiplied():
    """convert('RGB') of an exact RGBA file is the stored RGB"""
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (7, 9, 4), dtype=np.uint8)
    b = io.BytesIO()
    Image.fromarray(a, "RGBA").save(b, "WEBP", lossless=True, exact=True)
    rc, got = wr.decode(b.getvalue())
    assert rc == 0 and np.array_equal(got, a[..., :3]) and np.array_equal(wc.pillow_rgb(b.getvalue()), a[..., :3])


def test_byte_after_the_riff_payload_is_refused():
    """Pillow reads such a file; a strict reader need not, so the restatement (and the device) answer -1: the file goes to Pillow."""
    data = wc.sweep_bases()[0][1] + b"\0"
    assert wc.pillow_rgb(data) is not None
    rc, _, reason = wr.probe(data)
    assert rc == -1 and reason == "bytes after the RIFF payload"


def test_damage_sweep():
    sweep = wc.sweep_reference()
    flips = [s for s in sweep if s[1] == "flip"]
    cuts = [s for s in sweep if s[1] == "cut"]
    assert len(flips) == 8 * sum(len(d) for _, d in wc.sweep_bases()) and len(cuts) == sum(len(d) for _, d in wc.sweep_bases())
    assert all(rc != 0 for _, _, _, rc, _ in cuts), "a truncated file was accepted"
    accepted = 0
    for name, kind, data, rc, px in sweep:
        if rc == 0:
            want = wc.pillow_rgb(data)
            assert want is not None, "accepted where Pillow raises: " + name
            assert np.array_equal(px, want), name
            accepted += 1
    print("accepted %d of %d flips, 0 of %d truncations" % (accepted, len(flips), len(cuts)))
    assert accepted >= len(flips) / 4, (accepted, len(flips))
