"""GPU: lumina_ocr_table_rules through the C ABI against the restatement (tests/table_reference.py): the ink mask (parity hook), both
rule lists and the counts are EQUAL — the definition is integer arithmetic with a canonical order, so there is no tolerance."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth

import table_reference as tr

pytestmark = pytest.mark.gpu

P = arch.TABLE_PARAMS


def check(engine, pages: np.ndarray, **params):
    """pages uint8 [n,H,W,3] -> the per-page (hrules, vrules) of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in ("threshold", "gap", "min_len", "max_thick")}
    cap = params.get("max_rules", P["max_rules"])
    hr, vr, cnt, mask = engine.table_rules(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), max_rules=cap, debug=True, **kw)
    torch.cuda.synchronize()
    hr, vr, cnt, mask = hr.cpu().numpy(), vr.cpu().numpy(), cnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64)
    out = []
    for i, page in enumerate(pages):
        rmask, rh, rv = tr.table_rules(page, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert (int(cnt[i, 0]), int(cnt[i, 1])) == (len(rh), len(rv)), "page %d: counts %s, restatement %s" % (i, cnt[i], (len(rh), len(rv)))
        for got, ref, name in ((hr[i], rh, "horizontal"), (vr[i], rv, "vertical")):
            n = len(ref) if len(ref) <= cap else 0      # an overflowing list is not written; rows past the count are untouched
            assert np.array_equal(got[:n], ref[:n]), "page %d: %s rules differ" % (i, name)
            assert not got[n:].any(), "page %d: %s rows past the count were written" % (i, name)
        out.append((rh, rv))
    return out


def bars_page(h: int, w: int, seed: int) -> np.ndarray:
    """Random bars of both directions (some touching the page edges, some broken by gaps of 1-4 pixels), a filled block and noise dots."""
    rng = np.random.default_rng(seed)
    pg = np.full((h, w, 3), 255, np.uint8)
    for _ in range(10):
        t, vertical = int(rng.integers(1, 7)), bool(rng.integers(0, 2))
        if vertical:
            x, y0, y1 = int(rng.integers(0, w)), int(rng.integers(0, h // 2)), int(rng.integers(h // 2, h + 1))
            pg[y0:y1, x:x + t] = int(rng.integers(0, 100))
            gy = int(rng.integers(y0, max(y0 + 1, y1 - 4)))
            pg[gy:gy + int(rng.integers(1, 5)), x:x + t] = 255
        else:
            y, x0, x1 = int(rng.integers(0, h)), int(rng.integers(0, w // 2)), int(rng.integers(w // 2, w + 1))
            pg[y:y + t, x0:x1] = int(rng.integers(0, 100))
            gx = int(rng.integers(x0, max(x0 + 1, x1 - 4)))
            pg[y:y + t, gx:gx + int(rng.integers(1, 5))] = 255
    pg[0, :] = 30; pg[h - 1, :] = 30; pg[:, 0] = 30; pg[:, w - 1] = 30      # rules on all four page edges
    by, bx = int(rng.integers(0, max(1, h - 40))), int(rng.integers(0, max(1, w - 40)))
    pg[by:by + 40, bx:bx + 40] = 0                                            # a filled block
    dots = rng.integers(0, [h, w], (200, 2))
    pg[dots[:, 0], dots[:, 1]] = 0
    return pg


@pytest.mark.parametrize("seed,thickness,noise", [(0, 2, 0.0), (1, 3, 3.0), (2, 4, 0.0), (3, 5, 3.0), (4, 0, 3.0)])
def test_table_pages(engine, seed, thickness, noise):
    pages, gts = zip(*[synth.synth_table_page(seed, n_tables=2, thickness=thickness, noise=noise, spans=bool(s)) for s in (0, 1)])
    for (rh, rv), gt in zip(check(engine, np.stack(pages)), gts):
        assert len(gt) == 2 and len(rh) >= sum(g["row_count"] + 1 for g in gt) and len(rv) >= sum(g["column_count"] + 1 for g in gt)


def test_text_pages_have_no_rules_and_ruled_pages_have_underlines(engine):
    plain = np.stack([synth.synth_page(700, 1000, s, n_lines=16)[0] for s in range(3)])
    assert all(len(rh) == 0 and len(rv) == 0 for rh, rv in check(engine, plain))
    ruled = np.stack([synth.synth_page(700, 1000, s, n_lines=16, ruled=True)[0] for s in range(3)])
    assert all(len(rh) >= 10 and len(rv) == 0 for rh, rv in check(engine, ruled))
    (rh, rv), = check(engine, synth.synth_form_page(0)[0][None])
    assert len(rh) == 0 and len(rv) == 0


def test_a4_batch_of_64_different_pages(engine):
    h, w = synth.A4_200DPI
    base = [synth.synth_table_page(s, h, w, n_tables=3, spans=bool(s & 1), noise=3.0 * (s & 2))[0] for s in range(4)]
    base += [synth.synth_page(h, w, 11, n_lines=40)[0], synth.synth_page(h, w, 12, n_lines=40, ruled=True)[0], bars_page(h, w, 13), bars_page(h, w, 14)]
    pages = np.stack([np.roll(base[i % 8], (37 * (i // 8), 53 * (i // 8)), axis=(0, 1)) for i in range(64)])
    assert len({pg.tobytes() for pg in pages}) == 64
    res = check(engine, pages)
    with_rules = [(rh.tobytes(), rv.tobytes()) for rh, rv in res if len(rh) + len(rv)]
    assert len(with_rules) == 56 and len(set(with_rules)) == 56      # every page with rules has a result of its own; the text page has none


@pytest.mark.parametrize("w", [63, 64, 65, 1414])
def test_widths(engine, w):
    pages = np.stack([bars_page(200, w, s) for s in range(3)])
    check(engine, pages)
    check(engine, np.ascontiguousarray(pages.transpose(0, 2, 1, 3)))     # the same as heights


def test_blank_and_all_ink_pages(engine):
    pages = np.stack([np.full((150, 300, 3), 255, np.uint8), np.zeros((150, 300, 3), np.uint8), np.full((150, 300, 3), 128, np.uint8)])
    res = check(engine, pages)
    assert all(len(rh) == 0 and len(rv) == 0 for rh, rv in res)
    (rh, rv), = check(engine, np.zeros((1, 10, 300, 3), np.uint8))          # 10 rows of ink: one horizontal rule, the whole page
    assert rh.tolist() == [[0, 0, 299, 9, 3000]] and len(rv) == 0


def test_overflow_reports_the_true_count(engine):
    page = synth.synth_page(700, 1000, 5, n_lines=16, ruled=True)[0]
    (rh, rv), = check(engine, page[None], max_rules=4)
    assert len(rh) > 4 and len(rv) == 0


@pytest.mark.parametrize("params", [dict(threshold=100, gap=0, min_len=20, max_thick=3, max_rules=2048),
                                    dict(threshold=200, gap=5, min_len=40, max_thick=30, max_rules=64),
                                    dict(threshold=128, gap=1, min_len=1, max_thick=1, max_rules=2048),
                                    dict(threshold=128, gap=0, min_len=300, max_thick=6, max_rules=16)])
def test_other_parameters(engine, params):
    pages = np.stack([synth.synth_page(300, 420, 2, n_lines=7, ruled=True)[0], synth.synth_table_page(6, 300, 420, rows=2, cols=2)[0], bars_page(300, 420, 7)])
    check(engine, pages, **params)


def test_zero_pages_is_a_no_op(engine):
    hr, vr, cnt = engine.table_rules(torch.zeros((0, 100, 100, 3), dtype=torch.uint8, device="cuda"))
    assert tuple(cnt.shape) == (0, 2)
