"""The fused expand + depthwise kernel (mbconv.hip) at the batch sizes where its schedule can go wrong: a persistent grid of
G = CUs x resident work-groups, each walking the items (crop, 32-column strip) g, g + G, ..., and the four waves of a work-group
sharing a strip's expand units round-robin.

Reference: the unfused path (conv + dwconv_kernel + se_pool_kernel, fuse_mb = 0), which computes the same arithmetic in the same
order.  Every block tap and the final outputs must be EQUAL.

Sizes: N = 1 (5 recogniser items, 3 classifier items: nearly every work-group idles), N = 2 and 3 (a work-group's first item is its
last), and one N with items > 2 G and items mod G != 0 for both grids the launch can choose (2 or 3 work-groups per CU by LDS use):
every work-group loops, the last round is ragged.  The classifier runs at its own sizes: its maps are 24 / 12 / 6 / 3 rows high and
three strips wide, so the units split over the waves at other tile counts than the recogniser's."""
import numpy as np
import pytest
import torch

import cls_reference as cr
from lumina_ocr import arch
from test_gpu_rec import _crops

pytestmark = pytest.mark.gpu

REC_WIDTHS = [320, 33, 200, 77, 320, 131, 18, 250, 64, 301, 160]      # ragged, cycled (11: coprime to the 16 distinct crops)
CLS_WIDTHS = [192, 33, 1, 8, 31, 77, 150, 191, 100]
MAX_N = 1024


def _large_n(strips):
    """Smallest N <= MAX_N with N * strips > 2 G and (N * strips) mod G != 0 for G = CUs x 3 and CUs x 2."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * 3 * cus // strips + 1
    while any((n * strips) % (cus * k) == 0 for k in (2, 3)):
        n += 1
    assert n <= MAX_N, (n, cus)
    return n


def _tiled(base, widths, n):
    reps = (n + len(base) - 1) // len(base)
    crops = np.ascontiguousarray(np.concatenate([base] * reps)[:n])
    return crops, np.array([widths[i % len(widths)] for i in range(n)], np.int32)


def _both_ways(engine, forward, crops, widths, names):
    x, w = torch.from_numpy(crops).cuda(), torch.from_numpy(widths).cuda()
    outs = []
    engine.set_option("keep_taps", 1)
    try:
        for fuse in (1, 0):
            engine.set_option("fuse_mb", fuse)
            res = forward(x, w)
            torch.cuda.synchronize()
            outs.append(([engine.read_tap(k) for k in names], [r.cpu().numpy() for r in res]))
    finally:
        engine.set_option("fuse_mb", 1)
        engine.set_option("keep_taps", 0)
    for name, a, b in zip(names, outs[0][0], outs[1][0]):
        assert a.shape[0] == len(crops) and np.array_equal(a, b), name
    return outs[0][1], outs[1][1]


@pytest.fixture(scope="module")
def rec_base():
    return _crops(16, 2468)


@pytest.fixture(scope="module")
def cls_base():
    return cr.layer_crops(16, seed=41)[0]


@pytest.fixture(scope="module")
def cls_weights():
    return arch.make_cls_weights(2718)


@pytest.mark.parametrize("n", [1, 2, 3, "large"])
def test_rec_fused_equals_unfused(engine, rec_weights, rec_base, n):
    n = _large_n(5) if n == "large" else n           # 160 columns: 5 strips per crop
    crops, widths = _tiled(rec_base, REC_WIDTHS[1:] if n < 4 else REC_WIDTHS, n)      # (N = 1 runs the 33-column crop)
    engine.load_rec(rec_weights)
    fused, plain = _both_ways(engine, engine.rec_forward, crops, widths, ["rec.b%d" % i for i in range(11)])
    for name, a, b in zip(("idx", "prob"), fused, plain):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("n", [1, 2, 3, "large"])
def test_cls_fused_equals_unfused(engine, cls_weights, cls_base, n):
    n = _large_n(3) if n == "large" else n           # 96 columns: 3 strips per crop
    crops, widths = _tiled(cls_base, CLS_WIDTHS[1:] if n < 4 else CLS_WIDTHS, n)
    engine.load_cls(cls_weights)
    fused, plain = _both_ways(engine, engine.cls_forward, crops, widths, ["cls.b%d" % i for i in range(11)])
    for name, a, b in zip(("label", "score", "flip"), fused, plain):
        assert np.array_equal(a, b), name
