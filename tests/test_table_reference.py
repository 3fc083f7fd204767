"""CPU: the numpy restatement of the rule extraction (tests/table_reference.py) on hand-made masks with known answers."""
import numpy as np

from lumina_ocr import arch

import table_reference as tr

P = arch.TABLE_PARAMS
GAP, MIN_LEN, MAX_THICK = P["gap"], P["min_len"], P["max_thick"]


def page_of(ink: np.ndarray) -> np.ndarray:
    return np.where(ink[..., None], 0, 255).astype(np.uint8).repeat(3, axis=2)


def rules(ink: np.ndarray, **kw):
    _, h, v = tr.table_rules(page_of(ink), **kw)
    return h.tolist(), v.tolist()


def test_luma_threshold_is_pillows_convert_l():
    from PIL import Image
    rng = np.random.default_rng(0)
    px = rng.integers(0, 256, (40, 50, 3)).astype(np.uint8)
    grey = np.asarray(Image.fromarray(px).convert("L"))
    for t in (1, 100, 128, 255):
        assert np.array_equal(tr.ink_mask(px, t), grey < t)
    px[:] = 128
    assert not tr.ink_mask(px, 128).any() and tr.ink_mask(px, 129).all()


def test_gap_merging_at_gap_and_gap_plus_one():
    for g, expect in ((GAP, 1), (GAP + 1, 0)):
        ink = np.zeros((20, 200), bool)
        ink[5, 10:40] = True
        ink[5, 40 + g:40 + g + 40] = True      # 30 + g + 40 >= 64 only when the two runs merge
        h, v = rules(ink)
        assert len(h) == expect and v == []
        if expect:
            assert h == [[10, 5, 40 + g + 39, 5, 70 + g]]     # area counts the bridged gap (kept-run length)


def test_min_len_minus_one_and_min_len():
    for n, expect in ((MIN_LEN - 1, 0), (MIN_LEN, 1)):
        ink = np.zeros((100, 300), bool)
        ink[7, 20:20 + n] = True
        ink[3:3 + n, 250] = True
        h, v = rules(ink)
        assert (len(h), len(v)) == (expect, expect)
    assert h == [[20, 7, 20 + MIN_LEN - 1, 7, MIN_LEN]] and v == [[250, 3, 250, 3 + MIN_LEN - 1, MIN_LEN]]


def test_filled_block_is_rejected_by_area_not_by_height():
    ink = np.zeros((100, 300), bool)
    ink[10:10 + MAX_THICK, 20:220] = True        # mean thickness == max_thick: a rule
    ink[50:50 + MAX_THICK + 1, 20:220] = True    # one row more: a bar, no rule
    h, v = rules(ink)
    assert h == [[20, 10, 219, 10 + MAX_THICK - 1, 200 * MAX_THICK]] and v == []
    ink = np.zeros((200, 200), bool)
    ink[20:180, 30:170] = True                   # a photo-sized block: neither direction
    assert rules(ink) == ([], [])


def test_skewed_long_rule_is_one_rule():
    """A 1400 px rule 3 px thick at 0.4 degrees (what de-skew leaves): its bounding box is 12 px high, its mean thickness 3."""
    ink = np.zeros((100, 1500), bool)
    x = np.arange(50, 1450)
    y = 40 + np.floor((x - 50) * np.tan(np.radians(0.4))).astype(int)
    for dy in range(3):
        ink[y + dy, x] = True
    h, v = rules(ink)
    assert len(h) == 1 and v == []
    x0, y0, x1, y1, area = h[0]
    assert (x0, x1, y0, area) == (50, 1449, 40, 3 * 1400) and y1 - y0 + 1 == 12
    hv, vv = rules(np.ascontiguousarray(ink.T))
    assert hv == [] and vv == [[y0, x0, y1, x1, area]]


def test_rules_touching_the_page_edge_and_widths_off_64():
    for w in (63, 64, 65, 127, 128, 130):
        ink = np.zeros((90, w), bool) if w >= MIN_LEN else np.zeros((90, w), bool)
        ink[0, :] = True
        ink[89, w - min(w, 70):] = True
        ink[:, 0] = True
        ink[10:, w - 1] = True
        h, v = rules(ink)
        exp_h = [[0, 0, w - 1, 0, w], [w - min(w, 70), 89, w - 1, 89, min(w, 70)]] if w >= MIN_LEN else []
        assert h == exp_h and v == [[0, 0, 0, 89, 90], [w - 1, 10, w - 1, 89, 80]]
        mask, _, _ = tr.table_rules(page_of(ink))
        assert mask.shape == (90, (w + 63) // 64) and mask.dtype == np.uint64
        for r in (0, 1, 5, 20, 89):
            assert [(int(mask[r, x // 64]) >> (x % 64)) & 1 for x in range(w)] == ink[r].astype(int).tolist()
            assert int(mask[r, -1]) >> ((w - 1) % 64 + 1) == 0                                   # bits past W are 0


def test_blank_and_all_ink_pages():
    assert rules(np.zeros((70, 200), bool)) == ([], [])
    assert rules(np.ones((70, 200), bool)) == ([], [])                     # 70 rows thick: no rule either way
    assert rules(np.ones((MAX_THICK, 200), bool)) == ([[0, 0, 199, MAX_THICK - 1, 200 * MAX_THICK]], [])


def test_canonical_order():
    ink = np.zeros((300, 400), bool)
    for y, x0 in ((200, 10), (50, 300 - 64), (50, 20), (120, 100)):
        ink[y, x0:x0 + 70] = True
    for x, y0 in ((390, 10), (5, 200), (5, 20), (200, 100)):
        ink[y0:y0 + 70, x] = True
    h, v = rules(ink)
    assert [r[:2] for r in h] == [[20, 50], [236, 50], [100, 120], [10, 200]]            # by (y0, x0)
    assert [r[:2] for r in v] == [[5, 20], [5, 200], [200, 100], [390, 10]]              # by (x0, y0)
    assert h == sorted(h, key=lambda r: (r[1], r[0], r[3], r[2])) and v == sorted(v, key=lambda r: (r[0], r[1], r[2], r[3]))


def test_components_join_only_through_overlapping_kept_runs():
    ink = np.zeros((40, 400), bool)
    ink[10, 0:100] = True
    ink[11, 100:200] = True        # touches diagonally only: x-intervals do not overlap -> two rules
    ink[20, 0:100] = True
    ink[21, 99:200] = True         # one pixel of overlap -> one rule
    ink[30, 0:100] = True
    ink[31, 50:60] = True          # a short run below: not kept, so not part of the rule
    h, _ = rules(ink)
    assert h == [[0, 10, 99, 10, 100], [100, 11, 199, 11, 100], [0, 20, 199, 21, 201], [0, 30, 99, 30, 100]]


def test_pack_mask_bit_order():
    ink = np.zeros((1, 130), bool)
    ink[0, [0, 63, 64, 129]] = True
    assert [int(v) for v in tr.pack_mask(ink)[0]] == [(1 << 63) | 1, 1, 2]
