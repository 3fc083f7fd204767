"""GPU: the persistent stem.conv1 + stem.conv2 kernel (stem12_kernel: resident work-groups walk the tiles, words of the next tile
requested under conv2 of the current one, word descriptors rebuilt when an image's base is aligned differently, dword gather +
byte permutes for conv1's operand, epilogue in registers) against the two-kernel path (fuse_stem = 0), bit for bit.

Every comparison runs with keep_taps = 2 and fuse_pool = 0 and looks at the taps stem.conv3 and stem.pool and at the
probability map.  Two weight sets: the dense seeded detector, and the same with stem.conv3 turned into a pass-through of its
first 32 input channels (w[c, 1, 1, c] = 1, bias 0): stem12's output is a ReLU output (>= 0), so channels 0..31 of the tap
stem.conv3 ARE the kernel's output tensor, not something a further convolution has blurred."""
import numpy as np
import pytest
import torch

from lumina_ocr import synth

pytestmark = pytest.mark.gpu

TAPS = ["stem.conv3", "stem.pool"]
TILE_H, TILE_W = 8, 32          # output pixels of one stem12 tile (half resolution)
MAX_WGS_PER_CU = 8              # upper bound of the kernel's resident work-groups per CU


@pytest.fixture(scope="module")
def passthrough_det_weights(dense_det_weights):
    w = {k: v.copy() for k, v in dense_det_weights.items()}
    w3 = np.zeros_like(w["stem.conv3.w"])          # OHWI [64, 3, 3, 32]
    for c in range(32):
        w3[c, 1, 1, c] = 1.0
    w["stem.conv3.w"] = w3
    w["stem.conv3.b"] = np.zeros_like(w["stem.conv3.b"])
    return w


@pytest.fixture(scope="module", params=["dense", "passthrough"])
def weights(request, dense_det_weights, passthrough_det_weights):
    return dense_det_weights if request.param == "dense" else passthrough_det_weights


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(engine, pages, fuse_stem):
    engine.set_option("fuse_stem", fuse_stem)
    prob = engine.det_forward(pages).clone()
    torch.cuda.synchronize()
    out = {"prob": prob.view(torch.int16).cpu().numpy()}
    for name in TAPS:
        out[name] = _bits(engine.read_tap(name))
    return out


def _compare(engine, weights, pages_np):
    pages = torch.from_numpy(np.ascontiguousarray(pages_np)).cuda()
    engine.load_det(weights)
    engine.set_option("keep_taps", 2)
    engine.set_option("fuse_pool", 0)
    try:
        got = _run(engine, pages, 1)
        ref = _run(engine, pages, 0)
    finally:
        engine.set_option("fuse_stem", 1)
        engine.set_option("fuse_pool", 1)
        engine.set_option("keep_taps", 0)
    for name in TAPS + ["prob"]:
        assert got[name].shape == ref[name].shape, name
        if not np.array_equal(got[name], ref[name]):
            d = np.argwhere(got[name] != ref[name])
            raise AssertionError("tap %s differs at %d of %d values, first %s" % (name, len(d), got[name].size, d[0].tolist()))
    return ref


def _text_pages(b, h, w, seed):
    return np.stack([synth.synth_page(h, w, seed + i, n_lines=max(3, h // 40))[0] for i in range(b)])


def _tiles(b, h, w):
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    return b * (-(-(hp // 2) // TILE_H)) * (-(-(wp // 2) // TILE_W))


@pytest.mark.parametrize("shape", [(1, 33, 35), (3, 96, 130)], ids=lambda s: "b%d_%dx%d" % s)
def test_fewer_tiles_than_work_groups(engine, weights, shape):
    """Four tiles (and a tensor whose byte count is odd: its last word is read byte by byte), and 54 tiles: the grid is the
    tile count, no work-group walks."""
    b, h, w = shape
    assert _tiles(b, h, w) < torch.cuda.get_device_properties(0).multi_processor_count
    ref = _compare(engine, weights, _text_pages(b, h, w, 51))
    assert ref["stem.conv3"].any()


def test_long_walk_with_page_crossings_and_a_ragged_last_round(engine, weights):
    """9 pages of 1000 x 700: 64 x 11 tiles a page, 6,336 in all — every work-group walks at least three tiles whatever the
    kernel's work-groups per CU (<= 8), walks cross from one page into the next, and the last round is not full."""
    b, h, w = 9, 1000, 700
    tiles, cus = _tiles(b, h, w), torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles == 9 * 64 * 11
    assert tiles >= 3 * cus * MAX_WGS_PER_CU
    for k in range(1, MAX_WGS_PER_CU + 1):
        assert tiles % (cus * k) != 0, k
    base = synth.synth_page(h, w, 61, n_lines=24)[0]
    pages = np.stack([np.roll(base, (37 * i, 53 * i), axis=(0, 1)) for i in range(b)])    # nine different pages from one rendering
    engine.set_option("det_sub_batch", 16)          # all nine pages in one launch
    _compare(engine, weights, pages)


@pytest.mark.parametrize("w", [200, 203, 202, 201], ids=lambda w: "pitch_mod4_%d" % (3 * w % 4))
def test_alignment_classes(engine, weights, w):
    """Row pitch 3 * W = 0, 1, 2, 3 (mod 4) at H = 250, two pages each: the words of consecutive rows start at every offset, and
    where the page size is no multiple of 4 the second page's base is aligned differently from the first one's."""
    assert 3 * w % 4 == {200: 0, 203: 1, 202: 2, 201: 3}[w]
    _compare(engine, weights, _text_pages(2, 250, w, 71))


def test_borders(engine, weights):
    """(1, 447, 901): the half-resolution map is 224 x 464, so the last tile column is half empty; the page's last row and
    column (446, 900) end inside the padded input, where the halo must read as zero."""
    _compare(engine, weights, _text_pages(1, 447, 901, 81))


def test_every_byte_value(engine, weights):
    """Seeded uniform random bytes instead of rendered text (every byte value in every channel and word position), one page
    that is all 0 and one that is all 255."""
    rng = np.random.default_rng(91)
    pages = rng.integers(0, 256, size=(4, 250, 201, 3), dtype=np.uint8)
    pages[2] = 0
    pages[3] = 255
    for c in range(3):
        assert len(np.unique(pages[:2, :, :, c])) == 256
    _compare(engine, weights, pages)
