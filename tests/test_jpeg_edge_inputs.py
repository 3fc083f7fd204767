"""CPU: the inputs of tests/jpeg_edge_inputs.py on the sequential definition.  For every input and every (quality, optimize) pair that
tests/test_gpu_jpeg.py encodes on the device, the C oracle equals Pillow byte for byte, and every input really has the property it
was built for — so the GPU test cannot pass on pages that never enter the regime they are named after."""
import io

import numpy as np
import pytest

import jpeg_edge_inputs as J


@pytest.fixture(scope="module")
def pages():
    return {name: build() for name, build in J.INPUTS.items()}


def _pillow(img, quality, optimize):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="JPEG", quality=quality, optimize=optimize)
    return b.getvalue()


@pytest.mark.parametrize("name", list(J.INPUTS))
def test_oracle_equals_pillow(pages, name):
    from oracle import jpeg as oj
    img = pages[name]
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    for quality, optimize in J.SETTINGS:
        assert oj.encode(img, quality, optimize=optimize) == _pillow(img, quality, optimize), (name, quality, optimize)


def test_builders_are_deterministic():
    for name in ("blank_text_page", "grey_noise", "ff_dense", "deep_huffman"):
        assert np.array_equal(J.INPUTS[name](), J.INPUTS[name]()), name


@pytest.mark.parametrize("name", J.FLAT_INPUTS)
def test_flat_pages_give_tables_of_at_most_two_symbols(pages, name):
    from oracle import jpeg as oj
    img = pages[name]
    assert (img == img[0, 0]).all()
    for quality in J.QUALITIES:
        counts = J.dht_symbol_counts(oj.encode(img, quality))
        assert sorted(counts) == [0x00, 0x01, 0x10, 0x11]
        assert all(1 <= n <= 2 for n in counts.values()), (name, quality, counts)
        assert counts[0x10] == 1 and counts[0x11] == 1 and counts[0x01] == 1          # AC tables: EOB alone; chroma DC: category 0 alone


def test_one_ink_pixel_and_grey_noise_tables(pages):
    from oracle import jpeg as oj
    counts = J.dht_symbol_counts(oj.encode(pages["one_ink_pixel"], 95))
    assert counts[0x10] > 2 and counts[0x00] <= 3                    # one busy block among flat ones
    for quality in J.QUALITIES:
        counts = J.dht_symbol_counts(oj.encode(pages["grey_noise"], quality))
        assert counts[0x11] == 1 and counts[0x01] == 1, (quality, counts)       # chroma: a single symbol per table
    assert J.dht_symbol_counts(oj.encode(pages["grey_noise"], 100))[0x10] > 10


def test_maximum_swing_patterns_reach_the_largest_categories(pages):
    from oracle import jpeg as oj
    for name in ("blocks8", "mcus16"):
        h, w = pages[name].shape[:2]
        assert J.dc_categories(oj.coefficients(pages[name], 100), h, w).max() == 11, name
    for name in ("checkerboard", "vertical_stripes", "horizontal_stripes"):
        assert J.max_ac_size(oj.coefficients(pages[name], 100)) == 10, name
    c = oj.coefficients(pages["saturated_stripes"], 100)
    assert int(np.abs(c[:, 4:, 1:]).max()) >= 256                    # chroma AC of size 9 and more


def test_low_qualities_clamp_quantisers_at_255(pages):
    from oracle import jpeg as oj
    for quality in (1, 10, 23):
        tabs = J.dqt_tables(oj.encode(pages["checkerboard"], quality))
        assert len(tabs) == 2 and int(tabs[0].max()) == 255, quality
        assert int(tabs[1].max()) == (255 if quality <= 10 else 215), quality
    # 23 is the last quality that clamps: at 24 the scale factor is 5000 // 24 = 208 and the largest luma entry (121 * 208 + 50) // 100 = 252
    assert [int(t.max()) for t in J.dqt_tables(oj.encode(pages["checkerboard"], 24))] == [252, 206]
    assert all(int(t.max()) == 1 for t in J.dqt_tables(oj.encode(pages["checkerboard"], 100)))


def test_ff_dense_stream_has_its_bytes_where_stated(pages):
    from oracle import jpeg as oj
    img = pages["ff_dense"]
    assert img.shape[0] <= 200 and img.shape[1] <= 300
    tile = oj.coefficients(J.ff_tile(J.FF_TILE_SEED), 100)[0][:, J.ZIGZAG]
    assert int(tile[1, 0]) - int(tile[0, 0]) == 1023 and not tile[1, 1:16].any() and 128 <= abs(int(tile[1, 16])) <= 255
    quality, optimize = J.FF_SETTING
    assert (quality, optimize) in J.SETTINGS
    data = oj.encode(img, quality, optimize=optimize)
    stream = J.unstuffed_scan(data)
    hits = J.ff_border_hits(stream)
    assert hits and hits[0] >= 1 and len(stream) > J.PIECE * (hits[0] + 1), (hits, len(stream))
    assert stream[J.PIECE * hits[0] - 1] == 0xFF and stream[J.PIECE * hits[0]] == 0xFF
    assert b"\xff\xff\xff" in stream
    assert stream.count(b"\xff") > 0.02 * len(stream)
    _, p0, p1 = J.segments(data)
    assert p1 - p0 == len(stream) + stream.count(b"\xff")


def test_deep_huffman_page_is_22_deep(pages):
    from oracle import jpeg as oj
    img = pages["deep_huffman"]
    assert img.shape[0] <= 512 and img.shape[1] <= 512 and J.DEEP_QUALITY in J.QUALITIES
    hist = J.luma_ac_histogram(oj.coefficients(img, J.DEEP_QUALITY))
    want = np.zeros(256, np.int64)
    for run, val, count in J._deep_symbols():
        want[(run << 4) + (1 if val == 1 else 2)] = count
    want[0] = 4096
    assert np.array_equal(hist, want)                                # the designed coefficients survive the rounding to pixels
    assert J.huffman_depth(hist) >= 22
    # the text page the suite already encodes is 18 deep at quality 95: the limiter runs there, but barely
    data = oj.encode(img, J.DEEP_QUALITY)
    assert J.dht_symbol_counts(data)[0x10] == 22
