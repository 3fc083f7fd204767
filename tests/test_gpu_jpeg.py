"""GPU parity (bit-exact, integer work): the device JPEG encoder vs the pinned C oracle and vs Pillow — the encoder the
reference calls in compress_for_azure (/root/reference/backend/utils/image_preprocessing.py:526-538)."""
import ctypes
import hashlib
import io

import numpy as np
import pytest
import torch

import jpeg_edge_inputs as J
from lumina_ocr import synth

pytestmark = pytest.mark.gpu


def _images(n, h, w, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    return np.stack([synth.synth_page(h, w, seed + i, n_lines=max(2, h // 40))[0] for i in range(n)])


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 8, 8), (3, 37, 53), (1, 64, 48), (2, 17, 31), (1, 100, 75), (2, 250, 333)])
@pytest.mark.parametrize("quality", [95, 50])
def test_coefficients_match_oracle(engine, shape, quality):
    from oracle import jpeg as oj
    n, h, w = shape
    imgs = _images(n, h, w, 11, "noise")
    got = engine.jpeg_coefficients(torch.from_numpy(imgs).cuda(), quality).cpu().numpy()
    zz = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
    for i in range(n):
        ref = oj.coefficients(imgs[i], quality)[:, :, zz]      # oracle: natural order -> zig-zag
        assert np.array_equal(got[i], ref), (shape, quality, i)


@pytest.mark.parametrize("case", [(1, 1, 1, "noise"), (2, 8, 8, "noise"), (3, 37, 53, "noise"), (2, 100, 75, "noise"), (2, 250, 333, "page"),
                                  (2, 640, 448, "page"), (1, 1000, 707, "page")])
@pytest.mark.parametrize("quality", [95, 85, 30])
def test_files_match_oracle_and_pillow(engine, case, quality):
    from PIL import Image
    from oracle import jpeg as oj
    n, h, w, kind = case
    imgs = _images(n, h, w, 23, kind)
    out, sizes = engine.jpeg_encode(torch.from_numpy(imgs).cuda(), quality)
    out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
    for i in range(n):
        assert sizes[i] > 0
        got = out[i, : sizes[i]].tobytes()
        assert got == oj.encode(imgs[i], quality), (case, quality, i)
        b = io.BytesIO()
        Image.fromarray(imgs[i]).save(b, format="JPEG", quality=quality, optimize=True)
        assert got == b.getvalue(), (case, quality, i)


def test_too_small_output_reports_negative_size(engine):
    imgs = _images(1, 200, 300, 5, "noise")
    out, sizes = engine.jpeg_encode(torch.from_numpy(imgs).cuda(), 95, max_bytes=4096)
    assert int(sizes[0]) < 0


@pytest.mark.parametrize("quality", [95, 30])
def test_standard_table_mode_matches_pillow(engine, quality):
    """optimize=0: the Annex K.3 tables — the reference's size probe `image.save(buffer, 'JPEG', quality=min_quality)` (:548)."""
    from PIL import Image
    from oracle import jpeg as oj
    imgs = _images(2, 123, 211, 31, "page")
    out, sizes = engine.jpeg_encode(torch.from_numpy(imgs).cuda(), quality, optimize=False)
    out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
    for i in range(2):
        b = io.BytesIO()
        Image.fromarray(imgs[i]).save(b, format="JPEG", quality=quality)
        got = out[i, : sizes[i]].tobytes()
        assert got == b.getvalue() and got == oj.encode(imgs[i], quality, optimize=False)


def test_compress_for_azure_device_mirrors_the_reference_loop(engine):
    """Quality loop 95 -> 30 and the resize fallback (image_preprocessing.py:495-557) on the device vs the same loop run with PIL."""
    from PIL import Image
    from lumina_ocr.utils.image_preprocessing import ImagePreprocessor
    pre = ImagePreprocessor(engine=engine)
    rng = np.random.default_rng(8)
    page = synth.synth_page(400, 560, 3, n_lines=10)[0]
    noisy = np.clip(page.astype(np.int16) + rng.normal(0, 12, page.shape), 0, 255).astype(np.uint8)
    batch = np.stack([page, noisy])
    dev = torch.from_numpy(batch).cuda()
    full = [len(pre.compress_for_azure(Image.fromarray(b))) for b in batch]
    for target in (2.0, max(full) * 0.7 / 2 ** 20, min(full) * 0.45 / 2 ** 20, 0.004):   # fits / lower quality / mixed / resize fallback
        got = pre.compress_for_azure_device(dev, target_size_mb=target)
        for i in range(2):
            ref = pre.compress_for_azure(Image.fromarray(batch[i]), target_size_mb=target)
            assert got[i] == ref, (target, i, len(got[i]), len(ref))


# ---- regimes that noise and text pages never enter (tests/jpeg_edge_inputs.py; tests/test_jpeg_edge_inputs.py proves on the CPU that every
# input has the property it is named after, and that the oracle equals Pillow on all of them) ----
def _pillow(img, quality, optimize=True):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=quality, optimize=optimize)
    return b.getvalue()


def _device_files(engine, imgs, quality, optimize=True, max_bytes=2 * 1024 * 1024):
    out, sizes = engine.jpeg_encode(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), quality, max_bytes=max_bytes, optimize=optimize)
    out, sizes = out.cpu().numpy(), sizes.cpu().numpy()
    assert (sizes > 0).all(), sizes
    return [out[i, : sizes[i]].tobytes() for i in range(len(imgs))]


@pytest.fixture(scope="module")
def edge_pages():
    return {name: build() for name, build in J.INPUTS.items()}


@pytest.mark.parametrize("setting", J.SETTINGS, ids=lambda s: "q%d_%s" % (s[0], "opt" if s[1] else "std"))
@pytest.mark.parametrize("name", list(J.INPUTS))
def test_edge_inputs_match_oracle_and_pillow(engine, edge_pages, name, setting):
    from oracle import jpeg as oj
    quality, optimize = setting
    img = edge_pages[name]
    ref = oj.encode(img, quality, optimize=optimize)
    if name in J.FLAT_INPUTS and optimize:
        assert max(J.dht_symbol_counts(ref).values()) <= 2                  # (the regime: tables of one or two symbols)
    if name == "ff_dense" and setting == J.FF_SETTING:
        stream = J.unstuffed_scan(ref)
        assert J.ff_border_hits(stream) and b"\xff\xff\xff" in stream      # 0xFF on both sides of a piece border, and a run of three
    if name == "deep_huffman" and setting == (J.DEEP_QUALITY, True):
        lengths = J.dht_lengths(ref)[0x10]                                  # 22 symbols in a chain (22 deep before limiting): lengths 1, 2, .. and a
        assert lengths.sum() == 22 and lengths[15] >= 2 and (lengths[:10] == 1).all()      # crowd at 16 bits that only the limiter can make
    if quality < 24:
        assert int(J.dqt_tables(ref)[0].max()) == 255                       # clamped quantisers
    got = _device_files(engine, img[None], quality, optimize)[0]
    assert got == ref, (name, setting, len(got), len(ref))
    assert got == _pillow(img, quality, optimize), (name, setting)
    if optimize and quality in (100, 1):
        coefs = engine.jpeg_coefficients(torch.from_numpy(img[None]).cuda(), quality).cpu().numpy()[0]
        want = oj.coefficients(img, quality)
        if quality == 100 and name == "blocks8":
            assert J.dc_categories(want, *img.shape[:2]).max() == 11
        if quality == 100 and name == "checkerboard":
            assert J.max_ac_size(want) == 10
        assert np.array_equal(coefs, want[:, :, J.ZIGZAG]), (name, quality)


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_mixed_batch_is_per_page(engine, order):
    """Tables, bit offsets, piece counts and sizes are per page: a blank page next to a busy one must not see its neighbour."""
    from oracle import jpeg as oj
    h, w = 200, 300
    pages = [J.flat(h, w, 255), J.colour_noise(h, w), J.checkerboard(h, w), synth.synth_page(h, w, 23, n_lines=5)[0], J.flat(h, w, 0)]
    if order == "reversed":
        pages = pages[::-1]
    batch = np.stack(pages)
    for quality in (95, 30):
        refs = [oj.encode(p, quality) for p in pages]
        busy, blank = J.unstuffed_scan(refs[1 if order == "forward" else 3]), J.unstuffed_scan(refs[0])
        assert len(busy) > 3 * J.PIECE and len(blank) < J.PIECE // 8                # (busy: several pieces of stream; blank: a fraction of one)
        together = _device_files(engine, batch, quality)
        alone = [_device_files(engine, p[None], quality)[0] for p in pages]
        for i in range(len(pages)):
            assert together[i] == alone[i], (order, quality, i)
            assert together[i] == refs[i], (order, quality, i)


@pytest.mark.parametrize("case", [("page", 95), ("blank", 30)], ids=lambda c: "%s_q%d" % c)
def test_production_size_page(engine, case):
    """2000 x 1414, what the default pre-processing hands over: ~66000 blocks, hundreds of 4096-byte pieces per page."""
    from oracle import jpeg as oj
    kind, quality = case
    h, w = 2000, 1414
    img = synth.synth_page(h, w, 23, n_lines=50)[0] if kind == "page" else J.blank_text_page(h, w)
    ref = oj.encode(img, quality)
    assert len(J.unstuffed_scan(ref)) > (100 if kind == "page" else 1) * J.PIECE
    got = _device_files(engine, img[None], quality, max_bytes=4 * 1024 * 1024)[0]
    sha = lambda b: hashlib.sha256(b).hexdigest()
    assert len(got) == len(ref) and sha(got) == sha(ref)
    assert sha(got) == sha(_pillow(img, quality))


def _encode_raw(engine, imgs, quality, out_stride, room):
    """lumina_ocr_jpeg_encode itself with an exact out_stride (Engine.jpeg_encode rounds it up to 1024), on a buffer of n * out_stride + room
    bytes filled with a sentinel -> (the n rows, the bytes after them, sizes)"""
    n, h, w, _ = imgs.shape
    dev = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    out = torch.full((n * out_stride + room,), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    rc = engine.lib.lumina_ocr_jpeg_encode(engine._h, dev.data_ptr(), n, h, w, int(quality), 1, out.data_ptr(), ctypes.c_size_t(out_stride),
                                           sizes.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, engine.lib.lumina_ocr_last_error(engine._h)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[: n * out_stride].reshape(n, out_stride), o[n * out_stride:], sizes.cpu().numpy()


def test_exact_fit_and_needed_length(engine):
    """sizes is the file length when the file fits out_stride exactly, -(needed length) when it does not; no byte past a page's
    out_stride is written either way."""
    from oracle import jpeg as oj
    img = np.random.default_rng(31).integers(0, 256, (123, 211, 3), dtype=np.uint8)
    ref = oj.encode(img, 95)
    s = len(_device_files(engine, img[None], 95)[0])
    assert s == len(ref) and s > 3 * J.PIECE
    room = 8192
    rows, tail, sizes = _encode_raw(engine, img[None], 95, s, room)
    assert int(sizes[0]) == s and rows[0].tobytes() == ref and (tail == 0xA5).all()
    for stride in (s - 1, 1):
        rows, tail, sizes = _encode_raw(engine, img[None], 95, stride, room)
        assert int(sizes[0]) == -s, (stride, int(sizes[0]))
        assert (tail == 0xA5).all(), stride
    # two pages, only the second fits: its file is whole, the first reports its own length, the sentinel after both rows is untouched
    small = J.flat(123, 211, 255)
    ref_small = oj.encode(small, 95)
    stride = 1000
    assert len(ref_small) < stride < s
    for pages, refs in (([img, small], [ref, ref_small]), ([small, img], [ref_small, ref])):
        rows, tail, sizes = _encode_raw(engine, np.stack(pages), 95, stride, room)
        for i in range(2):
            if len(refs[i]) <= stride:
                assert int(sizes[i]) == len(refs[i]) and rows[i, : sizes[i]].tobytes() == refs[i], i
                assert (rows[i, sizes[i]:] == 0xA5).all(), i
            else:
                assert int(sizes[i]) == -len(refs[i]), i
        assert (tail == 0xA5).all()
