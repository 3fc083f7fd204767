"""GPU: the strip decoders (csrc/lzw.hip, through lumina_ocr_strip_image_decode) on the fixed case list of tests/tiff_cases.py: status 0
and pixels equal to Pillow's Image.open(file).convert('RGB') and to the integer restatement (tests/tiff_reference.py); a mixed batch;
hostile strips among good neighbours, whose status must be exactly the restatement's and whose neighbours must stay intact; and a damage
sweep (one byte of an LZW strip changed): device status == restatement status, and status 0 => Pillow's own decode of the damaged file.
No case is skipped: the payloads that come from libtiff are what Pillow itself was built with."""
import numpy as np
import pytest
import torch
from PIL import features

import tiff_cases as tc
import tiff_reference as tr

pytestmark = pytest.mark.gpu


def _decode(engine, pages, h, w, rps, params, palettes=None):
    out, status = engine.strip_image_decode(pages, h, w, rps, params, palettes)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status


@pytest.mark.parametrize("name", list(tc.strip_cases()))
def test_case_equals_pillow_and_restatement(engine, name):
    c = tc.strip_cases()[name]
    got, status = _decode(engine, [c["strips"]], c["height"], c["width"], c["rps"], [c["params"]], [c["palette"]])
    assert status == [0]
    want = tc.pillow_rgb(c["file"])
    rst, ref, _, ctr = tr.decode_page(c["strips"], c["height"], c["width"], c["rps"], c["params"], c["palette"])
    assert rst == 0 and np.array_equal(ref, want)
    assert np.array_equal(got[0], want)
    if name.startswith("lzw_noise_40x300"):   # the case is only worth its name if the stream gets there
        assert ctr[0]["widest"] == 12 and ctr[0]["clears"] >= 2 and len(c["strips"]) == 1
    if name == "lzw_noise_40x300_libtiff":
        assert features.check("libtiff")


def test_mixed_batch_of_codecs_in_one_call(engine):
    h, w, rps = 40, 300, 16
    pages = [tc.noise(h, w, seed=31), tc.text_like(h, w, seed=32), tc.noise(h, w, seed=33), tc.text_like(h, w, seed=34), tc.noise(h, w, seed=35, top=3)]
    comps = [tc.LZW, tc.PACKBITS, tc.NONE, tc.LZW, tc.PACKBITS]
    cases = [tc.make_case("m%d" % k, a, w, comp, rps=rps, predictor=2 if k == 3 else 1, photo=0 if k == 1 else 1) for k, (a, comp) in enumerate(zip(pages, comps))]
    got, status = _decode(engine, [c["strips"] for c in cases], h, w, rps, [c["params"] for c in cases])
    assert status == [0] * 5
    for k, c in enumerate(cases):
        assert np.array_equal(got[k], tc.pillow_rgb(c["file"])), k


def test_hostile_strips_among_good_neighbours(engine):
    h, w = 40, 300
    good = tc.noise(h, w, seed=41)
    good_rgb = np.repeat(good[:, :, None], 3, axis=2)
    g = tc.make_case("good", good, w, tc.LZW)
    gp = tc.make_case("goodp", good, w, tc.PACKBITS)
    hostile = tc.hostile_strips(h * w)
    pages, params, want = [g["strips"]], [g["params"]], [0]
    for name, (codec, strip) in hostile.items():
        pages += [[strip], gp["strips"] if len(pages) % 4 == 1 else g["strips"]]
        params += [(codec, 1, 1, 8, 0, 0, 0), gp["params"] if len(params) % 4 == 1 else g["params"]]
        st = tr.decode_strip(strip, h * w, codec)[0]
        assert st != 0, name
        want += [st, 0]
    got, status = _decode(engine, pages, h, w, h, params)
    assert status == want
    for k, st in enumerate(want):
        if st == 0:
            assert np.array_equal(got[k], good_rgb), k


def test_hostile_strip_inside_a_page_and_wrong_strip_count(engine):
    h, w, rps = 40, 300, 8
    a = tc.noise(h, w, seed=42)
    c = tc.make_case("p", a, w, tc.LZW, rps=rps)
    bad = list(c["strips"])
    bad[2] = tc.hostile_strips(rps * w)["eoi_early"][1]
    odd = list(c["strips"])
    odd[4] = b"\x00\x01" + odd[4][2:]       # does not start with Clear: -2 wins over the -1 of strip 2
    odd[2] = bad[2]
    pages = [c["strips"], bad, odd, c["strips"][:-1], c["strips"]]
    got, status = _decode(engine, pages, h, w, rps, [c["params"]] * 5)
    assert status == [0, -1, -2, -2, 0] == [tr.decode_page(p, h, w, rps, c["params"])[0] for p in pages]
    want = np.repeat(a[:, :, None], 3, axis=2)
    assert np.array_equal(got[0], want) and np.array_equal(got[4], want)


def test_unsupported_parameters_are_minus_two(engine):
    c = tc.strip_cases()["lzw_grey_pred2"]
    p = c["params"]
    variants = [p, (7,) + p[1:], p[:1] + (3,) + p[2:], p[:2] + (2,) + p[3:], p[:3] + (16,) + p[4:], p[:4] + (1,) + p[5:], p[:5] + (1, 0)]
    got, status = _decode(engine, [c["strips"]] * len(variants), c["height"], c["width"], c["rps"], variants)
    #   ok, codec 7, predictor 3, two components, 16 bits, indexed without a palette, (invert is fine with one component)
    assert status == [0, -2, -2, -2, -2, -2, 0]
    assert np.array_equal(got[0], tc.pillow_rgb(c["file"]))


def test_sub_batches(engine):
    """png_sub_batch_mb = 1: seven 300 x 300 RGB pages of 0.27 MB of packed rows each are split into three sub-batches"""
    h, w, rps = 300, 300, 13
    cases = [tc.make_case("s%d" % k, tc.smooth_rgb(h, w) + np.uint8(k), w, tc.LZW, photo=2, spp=3, rps=rps, predictor=2) for k in range(7)]
    engine.set_option("png_sub_batch_mb", 1)
    try:
        got, status = _decode(engine, [c["strips"] for c in cases], h, w, rps, [c["params"] for c in cases])
    finally:
        engine.set_option("png_sub_batch_mb", 768)
    assert status == [0] * 7
    for k, c in enumerate(cases):
        assert np.array_equal(got[k], (tc.smooth_rgb(h, w) + np.uint8(k)).reshape(h, w, 3)), k
    assert np.array_equal(got[3], tc.pillow_rgb(cases[3]["file"]))


@pytest.mark.parametrize("which", [0, 1])
def test_damage_sweep(engine, which):
    name, c, files = tc.damage_sets()[which]
    at, n = c["file"].index(c["strips"][0]), len(c["strips"][0])
    strips = [f[at:at + n] for f in files]
    got, status = _decode(engine, [[s] for s in strips], c["height"], c["width"], c["rps"], [c["params"]] * len(files))
    ref = [tr.decode_page([s], c["height"], c["width"], c["rps"], c["params"])[0] for s in strips]
    print(name, "device", status, "restatement", ref)
    assert status == ref
    for k, f in enumerate(files):
        if status[k] == 0:
            assert np.array_equal(got[k], tc.pillow_rgb(f)), (name, k)


def test_rows_of_part_of_a_byte(engine):
    """width 3: a packed row is 3, 6 or 12 bits.  Grey at 1, 2 and 4 bits with and without MinIsWhite and indexed colour at 1, 2 and 4
    bits, uncompressed, against the source arrays (v * 255, v * 85, v * 17; the palette's high bytes).  The same sample formats at
    width 331, against Pillow, are test_case_equals_pillow_and_restatement's lzw_1bit_*, lzw_grey2_331, lzw_grey4_331,
    lzw_miniswhite_1bit / _2bit / _4bit, raw_pal1, raw_pal2 and lzw_pal4_331: they are not repeated here."""
    w, h = 3, 37
    rng = np.random.default_rng(337)
    pal = np.array([[v // 256 for v in rgb] for rgb in tc.PALETTE16], np.uint8)
    cases, want = [], []
    for bits, scale in ((1, 255), (2, 85), (4, 17)):
        v = rng.integers(0, 1 << bits, (h, w))
        for photo in (1, 0, 3):
            cases.append(tc.make_case("w3_%d_%d" % (bits, photo), tc.pack_bits(v, bits), w, tc.NONE, photo=photo, bits=bits, rps=16))
            grey = (v * scale if photo == 1 else 255 - v * scale).astype(np.uint8)
            want.append(pal[v] if photo == 3 else np.repeat(grey[:, :, None], 3, axis=2))
    got, status = _decode(engine, [c["strips"] for c in cases], h, w, 16, [c["params"] for c in cases], [c["palette"] for c in cases])
    assert status == [0] * len(cases)
    for k, c in enumerate(cases):
        assert np.array_equal(got[k], want[k]), c["name"]
        assert np.array_equal(want[k], tc.pillow_rgb(c["file"])), c["name"]   # (the source mapping is Pillow's)


def test_predictor_2_rows_beyond_the_grid(engine):
    """pd_tiff_predict (the row stage shared with the Flate images) runs min(height, 1024) work-groups a page and takes the rows beyond
    them by a grid stride; no other predictor-2 case has more than 300 rows.  65 x 1030 grey and RGB, uncompressed in one strip, against
    the source arrays (Pillow is no reference here: libtiff ignores Predictor outside LZW and Deflate)."""
    w, h = 65, 1030
    rng = np.random.default_rng(1031)
    g, rgb = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    cases = [tc.make_case("p2_grey", g, w, tc.NONE, predictor=2), tc.make_case("p2_rgb", rgb.reshape(h, -1), w, tc.NONE, photo=2, spp=3, predictor=2)]
    assert all(len(c["strips"]) == 1 and c["rps"] == h for c in cases)
    for c, want in zip(cases, (np.repeat(g[:, :, None], 3, axis=2), rgb)):     # (one component and three: a call has one shape of page, not one of sample)
        got, status = _decode(engine, [c["strips"]], h, w, h, [c["params"]])
        assert status == [0]
        rows = np.flatnonzero((got[0] != want).any(axis=(1, 2)))
        assert rows.size == 0, (c["name"], rows[:8])
