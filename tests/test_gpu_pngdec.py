"""GPU: the device PNG decoder (csrc/pngdec.hip, through lumina_ocr_png_decode) vs Pillow's Image.open(f).convert('RGB'), byte for
byte: every seeded file of tests/png_cases.py (every supported colour type and bit depth, Pillow at compress_level 0..9 and optimize,
forced and random filters, split IDATs, zlib strategies and window sizes, stored blocks over 64 KB, distance-1 runs, tiny and odd sizes,
short palettes, tRNS, eXIf), mixed batches, refused pages left untouched, a 64-page A4 batch and the engine's buffer lifetimes."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as pc
from lumina_ocr import synth
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu

CASES = pc.cases()


def _by_size(cases):
    groups = {}
    for name, data, rc in cases:
        _, info = Engine.png_probe(data)
        groups.setdefault((info["height"], info["width"]), []).append((name, data, rc))
    return groups


def test_every_case_equals_pillow(engine):
    """One call per size: each file's status is its probe's, and every accepted page equals Pillow's decode byte for byte."""
    n_ok = 0
    for (h, w), group in _by_size(CASES).items():
        out, status = engine.png_decode([d for _, d, _ in group], h, w)
        torch.cuda.synchronize()
        for k, (name, data, rc) in enumerate(group):
            assert status[k] == rc, (name, status[k], rc)
            if rc == 0:
                got, want = out[k].cpu().numpy(), pc.pillow_rgb(data)
                if not np.array_equal(got, want):
                    d = np.argwhere(got != want)
                    raise AssertionError("%s: %d of %d values differ, first at %s: got %s want %s" % (name, len(d), got.size, d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])]))
                n_ok += 1
    assert n_ok == sum(1 for c in CASES if c[2] == 0)


def test_mixed_batch_with_refused_pages_left_untouched(engine):
    """One call: RGB, palette, grey 1-bit, RGBA, a 16-bit page (-2), a corrupt one (-1) and one of another size (-4).  Refused pages
    keep the sentinel the output was filled with."""
    rng = np.random.default_rng(5)
    h, w = 40, 57
    ims = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
           Image.fromarray(synth.synth_page(h, w, 3, n_lines=2)[0]).quantize(16),
           Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8) > 100).convert("1"),
           Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "RGBA")]
    files = [pc.pil_bytes(im) for im in ims]
    files.append(pc.write_png(rng.integers(0, 65536, (h, w * 3)), w, h, 16, 2))
    bad = bytearray(files[0]); bad[-20] ^= 0xFF
    files.append(bytes(bad))
    files.append(pc.pil_bytes(Image.fromarray(rng.integers(0, 256, (h + 1, w, 3), dtype=np.uint8))))
    out = torch.full((len(files), h, w, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.png_decode(files, h, w, out=out)
    torch.cuda.synchronize()
    assert status[:4] == [0, 0, 0, 0] and status[4] == -2 and status[5] == -1 and status[6] == -4, status
    for k in range(4):
        assert np.array_equal(out[k].cpu().numpy(), pc.pillow_rgb(files[k])), k
    for k in range(4, 7):
        assert bool((out[k] == 77).all()), k


def test_a4_batch_of_64(engine):
    """64 A4 pages at 200 dpi written by Pillow (RGB, grey and palette pages) in one call: ≈ 380 MB of filtered scanlines, one sub-batch
    (the sub-batch loop is test_sub_batches_reuse_the_staging_buffer's)."""
    h, w = 2339, 1654
    base = synth.synth_page(h, w, 77, n_lines=40)[0]
    files = []
    for k in range(64):
        page = np.roll(base, 37 * k, axis=0)
        im = Image.fromarray(page)
        im = im.convert("L") if k % 3 == 1 else (im.quantize(8) if k % 3 == 2 else im)
        files.append(pc.pil_bytes(im, compress_level=1 + k % 9))
    out, status = engine.png_decode(files, h, w)
    torch.cuda.synchronize()
    assert status == [0] * 64
    for k in (0, 1, 2, 31, 62, 63):
        assert np.array_equal(out[k].cpu().numpy(), pc.pillow_rgb(files[k])), k


def test_sub_batches_reuse_the_staging_buffer():
    """png_sub_batch_mb = 1: eleven distinct pages (RGB ≈ 0.6 MB of filtered scanlines, grey and 4-bit palette less) split into
    several sub-batches of one or more files, each refilling the pinned staging buffer and the workspace; a refused page in the middle
    stays untouched.  Every decoded page must equal Pillow's."""
    eng = Engine(0)
    eng.set_option("png_sub_batch_mb", 1)
    rng = np.random.default_rng(31)
    h, w = 400, 500
    files = []
    for k in range(11):
        im = Image.fromarray(synth.synth_page(h, w, 200 + k, n_lines=6)[0])
        im = im.convert("L") if k % 3 == 1 else (im.quantize(16) if k % 3 == 2 else im)
        files.append(pc.pil_bytes(im, compress_level=1 + k % 9))
    files[5] = pc.write_png(rng.integers(0, 65536, (h, w * 3)), w, h, 16, 2)   # -2
    out = torch.full((len(files), h, w, 3), 91, dtype=torch.uint8, device="cuda")
    out, status = eng.png_decode(files, h, w, out=out)
    torch.cuda.synchronize()
    assert status == [0] * 5 + [-2] + [0] * 5, status
    for k, f in enumerate(files):
        if k == 5:
            assert bool((out[k] == 91).all())
        else:
            assert np.array_equal(out[k].cpu().numpy(), pc.pillow_rgb(f)), k
    eng.close()


def test_decodes_around_a_resize_that_grows_its_buffer_then_close():
    """The PNG decoder's pinned staging buffer and the resize's device intermediate belong to the engine: growing the one must leave
    the other alone.  Decode, resize a batch that grows the intermediate, decode twice more, close."""
    eng = Engine(0)
    rng = np.random.default_rng(29)
    w, h = 320, 240
    files = [pc.pil_bytes(Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)), compress_level=k) for k in (1, 6, 9)]
    want = [pc.pillow_rgb(f) for f in files]

    def decode_and_check():
        out, status = eng.png_decode(files, h, w)
        torch.cuda.synchronize()
        assert status == [0, 0, 0]
        for k in range(3):
            assert np.array_equal(out[k].cpu().numpy(), want[k]), k

    decode_and_check()
    pages = torch.from_numpy(rng.integers(0, 256, (4, 600, 800, 3), dtype=np.uint8)).cuda()
    resized = eng.resize_lanczos(pages, 300, 700)
    torch.cuda.synchronize()
    assert resized.shape == (4, 300, 700, 3)
    decode_and_check()
    decode_and_check()
    eng.close()
