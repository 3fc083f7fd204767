"""GPU: progressive JPEG files through lumina_ocr_jpeg_probe_progressive / lumina_ocr_jpeg_decode_progressive (csrc/jpegdec.hip) against
Pillow, byte for byte: every case of tests/progressive_cases.py (Pillow's own progressive files in every sampling, odd and tiny
sizes, restart intervals, an EOB run of category 14, scans of many chunks, and the scan scripts only the test-side writer can emit),
a mixed batch, the answers of the old entries, and the refusals.  Reference: Image.open in
/root/reference/backend/utils/image_preprocessing.py:57-75."""
import numpy as np
import pytest
import torch

import progressive_cases as pc
from jpeg_cases import CASES, UNSUPPORTED, make_file, pil_decode
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu

FILES = pc.all_files()
SENTINEL = 0xA5


def _same(name, got, want):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ, first at %s: got %s want %s" % (name, len(d), got.size, d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])]))


@pytest.mark.parametrize("name", [f[0] for f in FILES])
def test_device_decode_equals_pillow(engine, name):
    _, w, h, data = next(f for f in FILES if f[0] == name)
    rc, info = Engine.jpeg_probe_progressive(data)
    assert rc == 0 and (info["width"], info["height"]) == (w, h) and info["progressive"]
    out, status = engine.jpeg_decode_progressive([data], h, w)
    torch.cuda.synchronize()
    assert status == [0]
    _same(name, out[0].cpu().numpy(), pil_decode(data))


def test_grey_file_with_a_restart_interval_in_every_scan(engine):
    data = pc.grey_script_file()
    out, status = engine.jpeg_decode_progressive([data], 53, 37)
    torch.cuda.synchronize()
    assert status == [0]
    _same("grey_script", out[0].cpu().numpy(), pil_decode(data))


def test_mixed_batch_reports_per_page_and_leaves_refused_pages_alone(engine):
    """Three different progressive files, a baseline file, the CMYK file and a file of another size in one call (all 37 x 53 but the last)."""
    by_name = {f[0]: f[3] for f in FILES}
    prog = [by_name["420_37x53_noise_q90"], by_name["restart_single_component"], by_name["grey_37x53_rstblocks3"]]
    base = make_file(CASES[4])                                   # odd422, 37 x 53, sequential
    name, kind, _, _, seed, kw, mode = UNSUPPORTED[1]
    cmyk = make_file((name, kind, 37, 53, seed, kw, mode))
    other = by_name["444_100x75_noise_q50"]
    files = [prog[0], base, cmyk, prog[1], other, prog[2]]
    out = torch.full((6, 53, 37, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    out, status = engine.jpeg_decode_progressive(files, 53, 37, out=out)
    torch.cuda.synchronize()
    assert status == [0, 0, -2, 0, -4, 0], status
    pages = out.cpu().numpy()
    for k in (0, 3, 5):
        _same("page %d" % k, pages[k], pil_decode(files[k]))
    ref, st = engine.jpeg_decode([base], 53, 37)
    torch.cuda.synchronize()
    assert st == [0] and np.array_equal(pages[1], ref[0].cpu().numpy()) and np.array_equal(pages[1], pil_decode(base))
    assert (pages[2] == SENTINEL).all() and (pages[4] == SENTINEL).all()       # refused pages are not written


def test_old_entries_keep_their_answer_for_a_progressive_file(engine):
    _, w, h, data = next(f for f in FILES if f[0] == "420_37x53_noise_q90")
    assert Engine.jpeg_probe(data)[0] == -2
    out = torch.full((1, h, w, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    out, status = engine.jpeg_decode([data], h, w, out=out)
    torch.cuda.synchronize()
    assert status == [-2] and bool((out == SENTINEL).all())
    _, st = engine.jpeg_decode_async([data], h, w)
    torch.cuda.synchronize()
    assert st.tolist() == [-2]


def test_refusals(engine):
    data = pc.pillow_file(pc.BASE_420)
    cases = [(pc.drop_last_scans(data, 1), -2), (pc.drop_last_scans(data, 4), -2), (pc.cut_inside_last_scan(data), -1), (pc.swap_ah(data), -1), (data, 0),
             (pc.repeated_first_scan_file()[0], -2)]       # a complete coefficient sent again as a first scan: libjpeg lets the later scan win
    files = [f for f, _ in cases]
    for f, want in cases:
        if want in (-2, 0) or f is cases[3][0]:
            assert Engine.jpeg_probe_progressive(f)[0] == want      # the header tells; a cut inside the data shows on the device only
    out = torch.full((len(files), 53, 37, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    out, status = engine.jpeg_decode_progressive(files, 53, 37, out=out)
    torch.cuda.synchronize()
    assert status == [w for _, w in cases], status
    pages = out.cpu().numpy()
    assert all((pages[k] == SENTINEL).all() for k in (0, 1, 2, 3, 5))
    _same("clean neighbour", pages[4], pil_decode(data))
