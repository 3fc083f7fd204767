"""GPU: stem.conv3 with the 3x3/s2 max pool in its epilogue (conv_ring_kernel<0,false,true,4>: resident work-groups walk overlapping
16x32 conv tiles, 7x15 pooled pixels each; raw packed bf16 values pooled with integer maxima, ReLU once on the pooled values, the
horizontal maximum taken with DPP lane shifts, the out-of-map mask only in tiles on the map's border) against the un-fused pair
conv + maxpool_kernel (fuse_pool = 0; conv_big_min = 1 so that the un-fused conv sums in the same chunk order), bit for bit.

Every comparison runs with keep_taps = 2 and looks at the tap stem.pool and at the probability map.  Three weight sets: the dense
seeded detector; the same with stem.conv3 turned into a pass-through of its 32 inputs (the pooled tensor then IS a pooled copy of
stem12's output); and "dead channels" — dense, but channels 0..15 carry a bias of -1e3 and channels 16..31 the negated centre-tap
pass-through, so that whole pooling windows hold nothing but negative values and zeros: the fused result there must be +0."""
import numpy as np
import pytest
import torch

from lumina_ocr import synth

pytestmark = pytest.mark.gpu

POOL_TH, POOL_TW = 7, 15        # pooled pixels of one tile
WGS_PER_CU = 2                  # resident work-groups per CU of the ring kernels


@pytest.fixture(scope="module")
def passthrough_det_weights(dense_det_weights):
    w = {k: v.copy() for k, v in dense_det_weights.items()}
    w3 = np.zeros_like(w["stem.conv3.w"])          # OHWI [64, 3, 3, 32]
    for c in range(32):
        w3[c, 1, 1, c] = 1.0
    w["stem.conv3.w"] = w3
    w["stem.conv3.b"] = np.zeros_like(w["stem.conv3.b"])
    return w


@pytest.fixture(scope="module")
def dead_det_weights(dense_det_weights):
    w = {k: v.copy() for k, v in dense_det_weights.items()}
    w3, b3 = w["stem.conv3.w"].copy(), w["stem.conv3.b"].copy()
    b3[:16] = -1e3                                  # dense weights, every value far below zero
    w3[16:32] = 0.0
    for c in range(16, 32):
        w3[c, 1, 1, c] = -1.0                       # minus a ReLU output: negative or zero
    b3[16:32] = 0.0
    w["stem.conv3.w"], w["stem.conv3.b"] = w3, b3
    return w


@pytest.fixture(scope="module", params=["dense", "passthrough", "dead"])
def weights(request, dense_det_weights, passthrough_det_weights, dead_det_weights):
    return {"dense": dense_det_weights, "passthrough": passthrough_det_weights, "dead": dead_det_weights}[request.param]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(engine, pages, fused, taps):
    engine.set_option("fuse_pool", 1 if fused else 0)
    prob = engine.det_forward(pages).clone()
    torch.cuda.synchronize()
    out = {"prob": prob.view(torch.int16).cpu().numpy()}
    for name in taps:
        out[name] = _bits(engine.read_tap(name))
    return out


def _compare(engine, weights, pages_np):
    """-> (fused, un-fused) after asserting that stem.pool and the probability map are the same bits"""
    pages = torch.from_numpy(np.ascontiguousarray(pages_np)).cuda()
    engine.load_det(weights)
    engine.set_option("keep_taps", 2)
    engine.set_option("conv_big_min", 1)            # the un-fused stem.conv3 sums in the fused kernel's chunk order; the fused one takes the
    try:                                            # ring kernel at any setting, and the layers behind both see the same setting
        got = _run(engine, pages, True, ["stem.pool"])
        ref = _run(engine, pages, False, ["stem.conv3", "stem.pool"])
    finally:
        engine.set_option("fuse_pool", 1)
        engine.set_option("conv_big_min", 1024)
        engine.set_option("keep_taps", 0)
    for name in ["stem.pool", "prob"]:
        assert got[name].shape == ref[name].shape, name
        if not np.array_equal(got[name], ref[name]):
            d = np.argwhere(got[name] != ref[name])
            raise AssertionError("tap %s differs at %d of %d values, first %s" % (name, len(d), got[name].size, d[0].tolist()))
    assert ref["stem.pool"].any()
    return got, ref


def _assert_dead_channels(weights, dead_det_weights, got):
    if weights is dead_det_weights:
        pool = got["stem.pool"]
        assert not pool[..., :32].any(), "a window of negative values / zeros must pool to +0 (bit pattern 0x0000)"
        assert pool[..., 32:].any()


def _text_pages(b, h, w, seed):
    return np.stack([synth.synth_page(h, w, seed + i, n_lines=max(3, h // 40))[0] for i in range(b)])


def _pooled(h, w):
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    return hp // 4, wp // 4


def _tiles(b, h, w):
    hq, wq = _pooled(h, w)
    return b * (-(-hq // POOL_TH)) * (-(-wq // POOL_TW))


@pytest.mark.parametrize("shape", [(1, 33, 35), (3, 96, 130)], ids=lambda s: "b%d_%dx%d" % s)
def test_few_tiles(engine, weights, dead_det_weights, shape):
    """(1, 33, 35): pooled 16 x 16, 3 x 2 = 6 tiles — fewer than one work-group per XCD slot, XCDs 6 and 7 get none;
    (3, 96, 130): 3 pages of 4 x 3 tiles, ragged both ways."""
    b, h, w = shape
    if shape == (1, 33, 35):
        assert _pooled(h, w) == (16, 16) and _tiles(b, h, w) == 6
    got, _ = _compare(engine, weights, _text_pages(b, h, w, 151))
    _assert_dead_channels(weights, dead_det_weights, got)


def test_whole_tiles(engine, weights, dead_det_weights):
    """(1, 224, 480): pooled 56 x 120 = 8 x 8 whole tiles, no ragged edge: the only masked conv pixels are row / column -1."""
    assert _pooled(224, 480) == (56, 120) and 56 % POOL_TH == 0 and 120 % POOL_TW == 0
    got, _ = _compare(engine, weights, _text_pages(1, 224, 480, 161))
    _assert_dead_channels(weights, dead_det_weights, got)


def test_borders_and_numpy_pool(engine, weights, dead_det_weights):
    """(1, 447, 901): pooled 112 x 232 — 16 tile rows of 7 exactly, the last tile column holds 7 of 15 pooled columns; the page's
    valid area ends inside the padding.  Also: the 3x3/s2 maximum (pad 1) recomputed in numpy from the UN-FUSED tap stem.conv3 must
    equal the fused stem.pool — a check that does not go through maxpool_kernel (bf16 values are exact in float32)."""
    assert _pooled(447, 901) == (112, 232) and 232 % POOL_TW == 7
    got, ref = _compare(engine, weights, _text_pages(1, 447, 901, 171))
    _assert_dead_channels(weights, dead_det_weights, got)
    conv = ref["stem.conv3"].view(np.float32)                      # [1, 224, 464, 64], ReLU output
    n, hc, wc, c = conv.shape
    hq, wq = (hc - 1) // 2 + 1, (wc - 1) // 2 + 1
    pad = np.full((n, 2 * hq + 1, 2 * wq + 1, c), -np.inf, np.float32)
    pad[:, 1:hc + 1, 1:wc + 1] = conv
    want = np.full((n, hq, wq, c), -np.inf, np.float32)
    for dy in range(3):
        for dx in range(3):
            want = np.maximum(want, pad[:, dy:dy + 2 * hq:2, dx:dx + 2 * wq:2])
    assert want.shape == got["stem.pool"].shape
    assert np.array_equal(_bits(want), got["stem.pool"])


def test_long_walk_with_page_crossings_and_ragged_xcd_ranges(engine, weights, dead_det_weights):
    """9 pages of 1000 x 700 in one launch: pooled 256 x 176, 37 x 12 tiles a page, 3,996 in all.  Each XCD owns a contiguous
    range of 500 tiles (the last one 496) walked by its resident work-groups: every work-group walks several tiles, the ranges
    cross from one page into the next, and no range is a whole number of rounds."""
    b, h, w = 9, 1000, 700
    tiles, cus = _tiles(b, h, w), torch.cuda.get_device_properties(0).multi_processor_count
    assert _pooled(h, w) == (256, 176) and tiles == 37 * 12 * 9 == 3996
    per_xcd, wgs = -(-tiles // 8), cus // 8 * WGS_PER_CU
    last = tiles - 7 * per_xcd
    assert per_xcd >= 3 * wgs and last >= 3 * wgs                  # every work-group walks at least three tiles
    assert per_xcd % wgs != 0 and last % wgs != 0                  # the last round of every range is not full
    assert per_xcd % (tiles // b) != 0                             # range boundaries are not page boundaries: walks cross pages
    base = synth.synth_page(h, w, 61, n_lines=24)[0]
    pages = np.stack([np.roll(base, (37 * i, 53 * i), axis=(0, 1)) for i in range(b)])    # nine different pages from one rendering
    engine.set_option("det_sub_batch", 16)          # all nine pages in one launch
    got, _ = _compare(engine, weights, pages)
    _assert_dead_channels(weights, dead_det_weights, got)


def test_every_byte_value(engine, weights, dead_det_weights):
    """Seeded uniform random bytes instead of rendered text, one page that is all 0 and one that is all 255: every lane and
    register position of a tile carries a value of its own, so a lane shift that fetched the wrong neighbour could not hide
    behind the flat background of a rendered page."""
    rng = np.random.default_rng(191)
    pages = rng.integers(0, 256, size=(4, 250, 201, 3), dtype=np.uint8)
    pages[2] = 0
    pages[3] = 255
    for c in range(3):
        assert len(np.unique(pages[:2, :, :, c])) == 256
    got, _ = _compare(engine, weights, pages)
    _assert_dead_channels(weights, dead_det_weights, got)
