"""GPU: PDF /FlateDecode image streams (csrc/pngdec.hip, through lumina_ocr_flate_image_decode) against the source arrays: predictors 1,
2 and 10..15 with all five row filters mixed, grey at 1, 2, 4 and 8 bits, RGB, indexed colour at 1, 2, 4 and 8 bits, /Decode [1 0], stored /
fixed / dynamic deflate blocks, and corrupt streams.  One mixed batch per size; width 3 makes a packed row a part of one byte."""
import zlib

import numpy as np
import pytest
import torch

import pdf_cases as pc

pytestmark = pytest.mark.gpu

SIZES = [(61, 37), (128, 64), (3, 37)]   # (width, height)


def _rgb_of_grey(g):
    return np.repeat(g[:, :, None], 3, axis=2).astype(np.uint8)


def _cases(w, h):
    """[(name, stream, (predictor, components, bits, indexed, invert), palette, expected RGB or None, expected status)]"""
    rng = np.random.default_rng(w * 1000 + h)
    g = rng.integers(0, 256, (h, w), dtype=np.uint8)
    g[:, : w // 2] = np.sort(g[:, : w // 2], axis=1)   # (some structure: back-references and a dynamic block worth building)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgb[h // 2:] = rgb[h // 2 - 1]
    flat = rgb.reshape(h, -1)
    bw = rng.integers(0, 2, (h, w), dtype=np.uint8)
    i4, i8 = rng.integers(0, 16, (h, w)), rng.integers(0, 200, (h, w))
    lut4, lut8 = rng.integers(0, 256, (16, 3), dtype=np.uint8), rng.integers(0, 256, (200, 3), dtype=np.uint8)
    g2, g4, i1, i2 = rng.integers(0, 4, (h, w)), rng.integers(0, 16, (h, w)), rng.integers(0, 2, (h, w)), rng.integers(0, 4, (h, w))
    lut1, lut2 = rng.integers(0, 256, (2, 3), dtype=np.uint8), rng.integers(0, 256, (4, 3), dtype=np.uint8)

    def pal(lut):
        return np.concatenate([lut, np.repeat(lut[-1:], 256 - len(lut), axis=0)]).tobytes()
    bits1, bits4 = pc.pack_bits(bw, 1), pc.pack_bits(i4, 4)
    mixed = [0, 1, 2, 3, 4]
    out = []

    def add(name, raw, params, palette, want, kind="dynamic", status=0):
        out.append((name, pc.deflate(raw, kind), params, palette, want, status))
    for kind in ("stored", "fixed", "dynamic"):
        add("grey8_p1_" + kind, g.tobytes(), (1, 1, 8, 0, 0), None, _rgb_of_grey(g), kind)
    add("grey8_p2", pc.tiff_predict_rows(g, 1), (2, 1, 8, 0, 0), None, _rgb_of_grey(g))
    add("rgb8_p1", flat.tobytes(), (1, 3, 8, 0, 0), None, rgb)
    add("rgb8_p2", pc.tiff_predict_rows(flat, 3), (2, 3, 8, 0, 0), None, rgb, "fixed")
    for pred in range(10, 16):
        types = mixed[pred - 10:] + mixed[:pred - 10]
        add("rgb8_p%d" % pred, pc.png_filter_rows(flat, 3, types), (pred, 3, 8, 0, 0), None, rgb)
    add("grey8_p15", pc.png_filter_rows(g, 1, mixed), (15, 1, 8, 0, 0), None, _rgb_of_grey(g), "stored")
    add("grey8_invert", g.tobytes(), (1, 1, 8, 0, 1), None, _rgb_of_grey(255 - g))
    add("grey1_p1", bits1.tobytes(), (1, 1, 1, 0, 0), None, _rgb_of_grey(bw * 255))
    add("grey1_invert", bits1.tobytes(), (1, 1, 1, 0, 1), None, _rgb_of_grey(255 - bw * 255))
    add("grey1_p12", pc.png_filter_rows(bits1, 1, mixed), (12, 1, 1, 0, 0), None, _rgb_of_grey(bw * 255))
    # grey at 2 and 4 bits maps as v * 85 and v * 17 (v * 255 / (2^bits - 1)); indexed colour below 4 bits
    for bits, v, scale in ((2, g2, 85), (4, g4, 17)):
        packed = pc.pack_bits(v, bits)
        add("grey%d_p1" % bits, packed.tobytes(), (1, 1, bits, 0, 0), None, _rgb_of_grey(v * scale), "stored")
        add("grey%d_invert" % bits, packed.tobytes(), (1, 1, bits, 0, 1), None, _rgb_of_grey(255 - v * scale))
        add("grey%d_p13" % bits, pc.png_filter_rows(packed, 1, mixed), (13, 1, bits, 0, 0), None, _rgb_of_grey(v * scale))
    add("indexed1", pc.pack_bits(i1, 1).tobytes(), (1, 1, 1, 1, 0), pal(lut1), lut1[i1])
    add("indexed2", pc.pack_bits(i2, 2).tobytes(), (1, 1, 2, 1, 0), pal(lut2), lut2[i2])
    add("indexed2_p11", pc.png_filter_rows(pc.pack_bits(i2, 2), 1, mixed), (11, 1, 2, 1, 0), pal(lut2), lut2[i2], "fixed")
    add("indexed4", bits4.tobytes(), (1, 1, 4, 1, 0), pal(lut4), lut4[i4])
    add("indexed4_p15", pc.png_filter_rows(bits4, 1, mixed), (15, 1, 4, 1, 0), pal(lut4), lut4[i4])
    add("indexed8", i8.astype(np.uint8).tobytes(), (1, 1, 8, 1, 0), pal(lut8), lut8[i8])
    add("indexed8_p2", pc.tiff_predict_rows(i8.astype(np.uint8), 1), (2, 1, 8, 1, 0), pal(lut8), lut8[i8])
    # corrupt: a wrong Adler-32, a short stream, one row too few, one byte too many, a PNG filter byte of 5
    good = pc.deflate(flat.tobytes())
    out.append(("wrong_adler", good[:-1] + bytes([good[-1] ^ 1]), (1, 3, 8, 0, 0), None, None, -1))
    out.append(("short_stream", good[:len(good) * 2 // 3], (1, 3, 8, 0, 0), None, None, -1))
    add("row_missing", flat[:-1].tobytes(), (1, 3, 8, 0, 0), None, None, status=-1)
    add("byte_extra", flat.tobytes() + b"\x00", (1, 3, 8, 0, 0), None, None, status=-1)
    bad_filter = bytearray(pc.png_filter_rows(g, 1, [0])); bad_filter[(w + 1) * (h // 2)] = 5
    add("filter_byte_5", bytes(bad_filter), (15, 1, 8, 0, 0), None, None, status=-1)
    # outside the subset
    add("rgb_4bit", flat.tobytes(), (1, 3, 4, 0, 0), None, None, status=-2)
    add("tiff_predictor_1bit", bits1.tobytes(), (2, 1, 1, 0, 0), None, None, status=-2)
    add("predictor_3", g.tobytes(), (3, 1, 8, 0, 0), None, None, status=-2)
    add("intact_neighbour", g.tobytes(), (1, 1, 8, 0, 0), None, _rgb_of_grey(g))
    return out


@pytest.mark.parametrize("w,h", SIZES)
def test_mixed_batch_equals_source(engine, w, h):
    cases = _cases(w, h)
    kinds = {(c[1][2] >> 1) & 3 for c in cases}   # BTYPE of each stream's first block
    assert kinds >= {0, 1, 2}, "stored, fixed and dynamic blocks are all in the batch"
    out, status = engine.flate_image_decode([c[1] for c in cases], h, w, [c[2] for c in cases], [c[3] for c in cases])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for k, (name, _, _, _, want, st) in enumerate(cases):
        assert status[k] == st, (name, status[k], st)
        if want is not None:
            assert np.array_equal(got[k], want), name


def test_single_stream_without_palettes_argument(engine):
    w, h = SIZES[0]
    g = np.random.default_rng(1).integers(0, 256, (h, w), dtype=np.uint8)
    out, status = engine.flate_image_decode([zlib.compress(g.tobytes())], h, w, [(1, 1, 8, 0, 0)])
    assert status == [0] and np.array_equal(out[0].cpu().numpy(), _rgb_of_grey(g))
    # an indexed stream without its palette is outside the subset, not a fault
    assert engine.flate_image_decode([zlib.compress(g.tobytes())], h, w, [(1, 1, 8, 1, 0)])[1] == [-2]


def test_predictor_2_rows_beyond_the_grid(engine):
    """pd_tiff_predict runs min(height, 1024) work-groups a stream and takes the rows beyond them by a grid stride: 65 x 1030 grey and
    RGB (width 65: one full chunk of 64 pixels and a carry into a chunk of one), stored blocks, every row different"""
    w, h = 65, 1030
    rng = np.random.default_rng(1030)
    g, rgb = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    streams = [pc.deflate(pc.tiff_predict_rows(g, 1), "stored"), pc.deflate(pc.tiff_predict_rows(rgb.reshape(h, -1), 3), "stored")]
    out, status = engine.flate_image_decode(streams, h, w, [(2, 1, 8, 0, 0), (2, 3, 8, 0, 0)])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert status == [0, 0]
    for k, want in enumerate((_rgb_of_grey(g), rgb)):
        rows = np.flatnonzero((got[k] != want).any(axis=(1, 2)))
        assert rows.size == 0, (k, rows[:8])
