"""GPU parity (bit-exact) of the tiled pre-processing kernels at the edges of their tiles, against oracle.preprocess (itself checked
byte for byte against Pillow and the golden vectors).  The shapes follow the tile constants of ocr-system_amd/csrc/resize.hip:
  vertical Lanczos   VT_R = 16 output rows x VT_XB = 1008 row bytes (336 px), <= 9 taps or <= VKMAX = 16 taps, 60 KB LDS gate
  horizontal Lanczos HR = 8 rows x HX = 256 output pixels, <= 9 taps or <= HKMAX = 12 taps, segment <= HPXMAX = 400 input pixels
  enhance            EN_R = 16 rows x EN_XB = 1008 row bytes (4 waves x 63 words)
  gray sum           four pixels (three aligned words) per thread, bytewise head and tail"""
import numpy as np
import pytest
import torch

from oracle import preprocess as P

pytestmark = pytest.mark.gpu


def _rand(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _view_at(x, off):
    """x's bytes as a device tensor that starts `off` bytes into an allocation."""
    big = torch.from_numpy(np.concatenate([np.zeros(off, np.uint8), x.reshape(-1)])).cuda()
    return big[off:].view(*x.shape)


def _check_resize(engine, x, oh, ow, offsets=(0,)):
    want = [P.resize_lanczos(x[k], ow, oh) for k in range(x.shape[0])]
    for off in offsets:
        got = engine.resize_lanczos(_view_at(x, off), oh, ow).cpu().numpy()
        for k in range(x.shape[0]):
            assert np.array_equal(got[k], want[k]), (x.shape, oh, ow, off, k)


def _enhance_ref(x, contrast, sharpness):
    y = P.enhance_contrast(x, contrast) if contrast != 1.0 else x
    return P.enhance_sharpness(y, sharpness) if sharpness != 1.0 else y


def _check_enhance(engine, x, contrast=1.2, sharpness=1.1, offsets=(0,)):
    want = [_enhance_ref(x[k], contrast, sharpness) for k in range(x.shape[0])]
    for off in offsets:
        got = engine.enhance(_view_at(x, off), contrast, sharpness).cpu().numpy()
        for k in range(x.shape[0]):
            assert np.array_equal(got[k], want[k]), (x.shape, contrast, sharpness, off, k)


# (n, h, w, out_h): the width stays, so only the vertical pass runs.  Down-scale by about 1.17 (9 taps, the A4 ratio) unless noted.
V_CASES = [
    (1, 19, 335, 16),    # one tile of rows; 1005 row bytes (1 mod 4), just under one strip
    (1, 18, 336, 15),    # one tile - 1; exactly one strip, rows word aligned
    (2, 20, 337, 17),    # one tile + 1; 1011 bytes: 3 bytes spill into a second strip; page starts misaligned
    (1, 39, 338, 33),    # two tiles + 1; 1014 bytes (2 mod 4)
    (1, 8, 673, 7),      # less than one tile; two strips + 3 bytes
    (3, 12, 50, 17),     # up-scale: 7 taps
    (1, 50, 337, 33),    # down-scale by 1.5: 11 taps, the VKMAX instantiation
    (1, 233, 41, 100),   # down-scale by 2.33: 15 taps fit the loop, but 16 output rows span about 50 input rows: past the LDS gate, fallback kernel
]


@pytest.mark.parametrize("case", V_CASES)
def test_vertical_tile_edges(engine, case):
    n, h, w, oh = case
    _check_resize(engine, _rand(h * 131 + w, (n, h, w, 3)), oh, w)


# (n, h, w, out_w): the height stays, so only the horizontal pass runs; n * h = HR * k +- 1 rows.
H_CASES = [
    (1, 7, 298, 255),    # HX - 1 outputs, 9 taps
    (3, 3, 300, 256),    # HX
    (1, 15, 301, 257),   # HX + 1
    (1, 17, 603, 515),   # 2 HX + 3
    (1, 9, 117, 100),    # the bench's ratio
    (1, 7, 351, 300),
    (1, 9, 200, 257),    # up-scale: 7 taps
    (1, 7, 100, 256),
    (1, 9, 384, 256),    # down-scale by 1.5: 11 taps, the HKMAX instantiation
    (1, 15, 386, 257),
    (1, 9, 514, 257),    # down-scale by 2: 13 taps, leaves the fast path
    (1, 7, 425, 257),    # 11 taps, but 256 outputs span more than HPXMAX input pixels: generic kernel
]


@pytest.mark.parametrize("case", H_CASES)
def test_horizontal_tile_edges(engine, case):
    n, h, w, ow = case
    _check_resize(engine, _rand(h * 977 + w, (n, h, w, 3)), h, ow)


# (h, w), three pages each: heights around EN_R and 1, 2, 3; every (w * 3) & 3; strips just under and just over EN_XB bytes
E_CASES = [(15, 335), (16, 336), (17, 337), (33, 338), (1, 337), (2, 339), (3, 673), (16, 4), (17, 1)]


@pytest.mark.parametrize("case", E_CASES)
def test_enhance_tile_edges(engine, case):
    h, w = case
    x = _rand(h * 1009 + w, (3, h, w, 3))
    x[1] = 255 if h % 2 else 0       # a saturated or an all-zero page between two random ones
    _check_enhance(engine, x)


def test_enhance_saturated_and_zero_pages(engine):
    x = np.stack([np.full((17, 337, 3), 255, np.uint8), np.zeros((17, 337, 3), np.uint8), _rand(5, (17, 337, 3))])
    _check_enhance(engine, x)
    _check_enhance(engine, x, 1.0, 1.1)


# image sizes whose byte count is 0, 1, 2 and 3 mod 4 (3 HW = 120, 45, 18, 75), and images shorter than one group of four pixels
@pytest.mark.parametrize("hw", [(5, 8), (3, 5), (2, 3), (5, 5), (1, 1), (1, 2), (1, 3), (1, 7), (37, 46)])
def test_gray_sum_sizes(engine, hw):
    h, w = hw
    _check_enhance(engine, _rand(h * 53 + w, (3, h, w, 3)), 1.2, 1.0)


def test_gray_sum_mean_on_a_rounding_boundary(engine):
    """sum(L) = HW * 128 + HW / 2 rounds to a mean of 129, one count less to 128: a single pixel missed or counted twice flips it."""
    h, w, m, ntune = 37, 46, 128, 200
    rng = np.random.default_rng(77)
    a = rng.integers(0, 256, (h * w, 3), dtype=np.uint8)
    tune = rng.permutation(h * w)[:ntune]                     # grey pixels (L = v) that bring the sum to the boundary
    a[tune] = 0
    lum = lambda p: int(((p[:, 0].astype(np.int64) * 19595 + p[:, 1].astype(np.int64) * 38470 + p[:, 2].astype(np.int64) * 7471 + 0x8000) >> 16).sum())
    need = h * w * m + h * w // 2 - lum(a)
    assert 0 <= need <= 255 * ntune
    vals = np.full(ntune, need // ntune, np.int64)
    vals[: need % ntune] += 1
    a[tune] = vals[:, None].astype(np.uint8)
    b = a.copy()
    b[tune[-1]] -= 1                                          # (need // ntune >= 1: checked by the means below)
    a, b = a.reshape(h, w, 3), b.reshape(h, w, 3)
    assert P.gray_mean(a) == m + 1 and P.gray_mean(b) == m
    _check_enhance(engine, np.stack([a, b, a]), 1.2, 1.0)


def test_misaligned_base_pointer(engine):
    """One case of each family on views that start 1, 2 and 3 bytes into an allocation."""
    _check_resize(engine, _rand(1, (2, 20, 337, 3)), 17, 337, offsets=(1, 2, 3))      # vertical
    _check_resize(engine, _rand(2, (1, 9, 301, 3)), 9, 257, offsets=(1, 2, 3))        # horizontal
    _check_enhance(engine, _rand(3, (3, 17, 337, 3)), offsets=(1, 2, 3))              # enhance
    _check_enhance(engine, _rand(4, (3, 5, 5, 3)), 1.2, 1.0, offsets=(1, 2, 3))       # gray sum
