"""GPU: lumina_ocr_page_compose through the C ABI (Engine.page_compose) against its restatement (pdf_layers_reference.compose), byte for
byte, on the smallest canvases at which the kernel can go wrong (tables: pdf_layer_tables.py): widths around its 16-pixel store groups,
bands of rows that end inside a rectangle, pages whose first byte is not 16-byte aligned, rectangles that stick out on every side, every
kind and polarity, both sample maps, rows longer than a tile."""
import ctypes

import numpy as np
import pytest

import pdf_layer_tables as lt
import pdf_layers_reference as lr

pytestmark = pytest.mark.gpu


def run(engine, canvas_hw, n, layers):
    import torch
    dev = [(p, k, r, f, c, None if s is None else torch.from_numpy(s).cuda(), None if m is None else torch.from_numpy(m).cuda())
           for p, k, r, f, c, s, m in layers]
    out = engine.page_compose(canvas_hw, n, dev)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(engine, canvas_hw, n, layers):
    want = lr.compose(canvas_hw, n, layers)
    got = run(engine, canvas_hw, n, layers)
    assert got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=3))
        raise AssertionError("%d pixels differ, the first at page %d, y %d, x %d: got %s, want %s"
                             % (len(bad), *bad[0], got[tuple(bad[0])], want[tuple(bad[0])]))
    return got


@pytest.mark.parametrize("H", lt.HEIGHTS)
@pytest.mark.parametrize("W", lt.WIDTHS)
def test_small_canvases_every_kind(engine, W, H):
    layers = lt.small_canvas(W, H)
    assert {(l[1], l[3]) for l in layers} == {(k, f) for k in range(4) for f in range(2)}   # every kind, both polarities
    check(engine, (H, W), 2, layers)


def test_three_pages_with_0_1_and_64_layers(engine):
    layers = lt.three_pages()
    assert [sum(l[0] == p for l in layers) for p in range(3)] == [0, 1, 64]
    got = check(engine, (70, 67), 3, layers)
    assert (got[0] == 255).all()
    check(engine, (70, 67), 2, [])


def test_edges_inside_store_groups_and_row_bands(engine):
    check(engine, (70, 67), 1, lt.edges())


def test_identity_and_23_to_67_on_one_page_and_overlaps_in_both_orders(engine):
    orders = lt.orders()
    for order in orders:
        check(engine, (37, 67), 1, order)
    assert not np.array_equal(lr.compose((37, 67), 1, orders[2]), lr.compose((37, 67), 1, orders[3]))


@pytest.mark.parametrize("flip", [0, 1])
def test_alpha_edge_values(engine, flip):
    check(engine, (12, 36), 1, lt.alpha(flip))


def test_wide_rows_take_several_tiles(engine):
    check(engine, (3, 4100), 1, lt.wide())


def test_an_output_that_is_not_16_byte_aligned(engine):
    import torch
    from lumina_ocr.engine import ComposeLayer
    H, W = 5, 33
    src = lt._img(np.random.default_rng(23), H, W)
    layers = [(0, 0, (1, 0, W + 1, H), 0, (0, 0, 0), src, None), (1, 0, (0, 0, W, H), 0, (0, 0, 0), src, None)]
    want = lr.compose((H, W), 2, layers)
    dsrc = torch.from_numpy(src).cuda()
    buf = torch.zeros(2 * H * W * 3 + 16, dtype=torch.uint8, device="cuda")
    table = (ComposeLayer * 2)()
    for rec, l in zip(table, layers):
        rec.page, rec.kind, (rec.x0, rec.y0, rec.x1, rec.y1), rec.src, rec.w, rec.h = l[0], 0, l[2], dsrc.data_ptr(), W, H
    assert engine.lib.lumina_ocr_page_compose(engine._h, ctypes.addressof(table), 2, 2, H, W, buf.data_ptr() + 3, engine._stream()) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[3:3 + want.size].reshape(want.shape), want) and (got[:3] == 0).all() and (got[3 + want.size:] == 0).all()


def test_a_hostile_table_is_an_error_and_nothing_is_launched(engine):
    import torch
    from lumina_ocr.engine import EngineError
    H, W = 9, 20
    src = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    host = np.zeros((4, 4, 3), np.uint8)
    for table, twin in zip(lt.hostile(src, src[:0]), lt.hostile(host, host[:0])):
        assert not lr.compose_params_ok(twin, 1, H, W)
        with pytest.raises(EngineError, match="page_compose"):
            engine.page_compose((H, W), 1, table)
    good = (0, 0, (0, 0, 4, 4), 0, (0, 0, 0), src, None)
    with pytest.raises(EngineError, match="grouped by page"):
        engine.page_compose((H, W), 2, [(1,) + good[1:], good])
    out = engine.page_compose((H, W), 1, [good])   # the handle still works
    torch.cuda.synchronize()
    assert bool((out[0, :4, :4] == 0).all()) and bool((out[0, 4:] == 255).all())
