"""CPU: the restated page orientation (tests/page_orient_reference.py) and its host half (lumina_ocr/utils/page_orient.py): the profile
statistic calls every synthetic page kind right in all four rotations, blank and all-ink pages, the ratio at its boundary, the vote
rule, the np.rot90 convention of `turn`, grouping and input-order reassembly, the page_rotation mapping."""
import numpy as np
import pytest

from lumina_ocr import arch
from lumina_ocr.utils import page_orient as po

import page_orient_reference as pr

KINDS = ["text_a4", "text_small", "text_3_lines", "ruled_a4", "ruled_small", "form", "table_1", "table_2", "marks", "text_landscape"]


@pytest.fixture(scope="module")
def kinds():
    pages = pr.page_kinds()
    assert sorted(pages) == sorted(KINDS)
    return pages


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_every_page_kind_is_called_right_in_every_rotation(kinds, kind, k):
    page = np.rot90(kinds[kind], k)
    e_r, e_c = pr.energies(page)
    print(kind, k, e_r, e_c, max(e_r, e_c) / max(1, min(e_r, e_c)))
    assert pr.sideways(page) == bool(k & 1), (kind, k, e_r, e_c)
    # a quarter turn exchanges the two profiles, a half turn reverses each: the energies follow exactly
    u_r, u_c = pr.energies(kinds[kind])
    assert (e_r, e_c) == ((u_c, u_r) if k & 1 else (u_r, u_c))


def test_profiles_and_energy_by_hand():
    page = np.full((3, 4, 3), 255, np.uint8)
    page[0, :3] = 0          # row counts 3, 1, 0
    page[1, 1] = (127, 127, 127)   # L = 127 < 128: ink
    page[2, 2] = (128, 128, 128)   # L = 128: not ink
    r, c = pr.profiles(page)
    assert r.tolist() == [3, 1, 0] and c.tolist() == [1, 2, 1, 0]
    assert pr.energies(page) == (4 + 1, 1 + 1 + 1)
    assert pr.energy([5]) == 0 and pr.energy([]) == 0
    assert pr.energy([0, 65535, 0]) == 2 * 65535 * 65535     # past 32 bits


def test_blank_and_all_ink_pages_are_upright():
    for value in (255, 0):
        for shape in ((64, 100, 3), (100, 64, 3), (1, 1, 3)):
            page = np.full(shape, value, np.uint8)
            assert pr.energies(page) == (0, 0) and not pr.sideways(page)
    assert not po.is_sideways(0, 0)


def test_ratio_at_the_boundary():
    ratio = arch.PAGE_ORIENT_PARAMS["ratio"]
    assert ratio == 2 and arch.PAGE_ORIENT_PARAMS["min_lines"] == 3 and arch.PAGE_ORIENT_PARAMS["threshold"] == arch.TABLE_PARAMS["threshold"]
    for e_r in (0, 1, 7, 10 ** 6, 2 ** 47):
        assert not pr.sideways_from(e_r, 2 * e_r) and not po.is_sideways(e_r, 2 * e_r)
        assert pr.sideways_from(e_r, 2 * e_r + 1) and po.is_sideways(e_r, 2 * e_r + 1)
    assert pr.sideways_from(5, 16, ratio=3) and not pr.sideways_from(5, 15, ratio=3)
    # a page built to sit on the boundary: rows 2, 0 -> E_r = 4; columns c with E_c = 8 or 9
    page = np.full((2, 6, 3), 255, np.uint8)
    page[0, 0] = page[0, 2] = 0          # c = 1 0 1 0 0 0 -> E_c = 3, r = 2 0 -> E_r = 4
    assert pr.energies(page) == (4, 3) and not pr.sideways(page)
    tall = np.full((6, 2, 3), 255, np.uint8)
    tall[0, 0] = tall[2, 0] = tall[4, 0] = 0   # r = 1 0 1 0 1 0 -> E_r = 5, c = 3 0 -> E_c = 9
    assert pr.energies(tall) == (5, 9) and not pr.sideways(tall)
    tall[5, 0] = 0                             # r = 1 0 1 0 1 1 -> E_r = 4, c = 4 0 -> E_c = 16
    assert pr.energies(tall) == (4, 16) and pr.sideways(tall)


def test_vote_rule():
    assert not pr.vote([]) and not pr.vote([1]) and not pr.vote([1, 1])          # fewer than min_lines lines: never
    assert pr.vote([1, 1, 1]) and pr.vote([1, 1, 0]) and not pr.vote([1, 0, 0]) and not pr.vote([0, 0, 0])
    assert not pr.vote([1, 1, 0, 0]) and pr.vote([1, 1, 1, 0])                  # a tie leaves the page alone
    assert pr.vote([1, 1], min_lines=2)
    votes = np.array([[0, 0], [2, 2], [3, 2], [3, 1], [4, 2], [4, 3], [1000, 501], [1000, 500]])
    assert po.upside_down(votes).tolist() == [False, False, True, False, False, True, True, False]
    assert po.upside_down(votes).tolist() == [pr.vote([1] * f + [0] * (n - f)) for n, f in votes]
    rng = np.random.default_rng(4)
    flip, idx = rng.integers(0, 2, 200), rng.integers(-1, 7, 200)
    counts = pr.vote_counts(flip, idx, 6)
    assert counts[:, 0].sum() == ((idx >= 0) & (idx < 6)).sum() and counts[2].tolist() == [int((idx == 2).sum()), int(flip[idx == 2].sum())]


def test_turn_follows_np_rot90():
    page = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    for k in range(4):
        lying = np.rot90(page, k)
        assert np.array_equal(np.rot90(lying, (4 - k) % 4), page)     # turn = (4 - k) % 4 undoes k
    assert [po.page_rotation(t) for t in range(5)] == [0, 90, 180, 270, 0]
    # a page found at 90 degrees clockwise (np.rot90(page, -1)) is made upright by one counter-clockwise quarter: turn 1
    assert np.array_equal(np.rot90(np.rot90(page, -1), 1), page) and po.page_rotation(1) == 90


def test_grouping_and_reassembly():
    assert po.first_pass_groups([0, 0, 0]) == [(0, [0, 1, 2])]
    assert po.first_pass_groups([1, 1]) == [(1, [0, 1])]
    assert po.first_pass_groups([0, 1, 1, 0, 1]) == [(0, [0, 3]), (1, [1, 2, 4])]
    assert po.first_pass_groups([]) == []
    assert po.second_pass(0, [0, 3], [False, True]) == (2, [3], [1])
    assert po.second_pass(1, [1, 2, 4], [True, False, True]) == (3, [1, 4], [0, 2])
    assert po.second_pass(1, [5], [False]) == (3, [], [])
    # a batch of 8 in all four orientations, as the pipeline's passes would hand it back
    sideways = [0, 1, 0, 1, 1, 0, 0, 1]
    flipped = {0: [False, True, False, True], 1: [True, False, False, True]}
    parts, turns = [], {}
    for quarter, idxs in po.first_pass_groups(sideways):
        turn2, again, pos = po.second_pass(quarter, idxs, flipped[quarter])
        keep = [i for k, i in enumerate(idxs) if k not in pos]
        parts.append((keep, ["p%d" % i for i in keep]))
        parts.append((again, ["p%d" % i for i in again]))
        turns.update({i: quarter for i in keep})
        turns.update({i: turn2 for i in again})
    assert po.reassemble(8, parts) == ["p%d" % i for i in range(8)]
    assert [turns[i] for i in range(8)] == [0, 3, 2, 1, 1, 0, 2, 3]
    with pytest.raises(ValueError):
        po.reassemble(3, [([0, 1], "ab")])
    with pytest.raises(ValueError):
        po.reassemble(2, [([0, 1], "ab"), ([1], "c")])


def test_pipeline_and_provider_switches(monkeypatch):
    from lumina_ocr.pipeline import OcrPipeline, PageDetections
    from lumina_ocr.services import ocr_service as svc

    class NoCls:
        cls_loaded, num_classes = False, 6625
    with pytest.raises(ValueError, match="Engine.load_cls"):
        OcrPipeline(NoCls(), page_orient=True)

    class Cls(NoCls):
        cls_loaded = True
    with pytest.raises(ValueError, match="gather"):
        OcrPipeline(Cls(), page_orient=True, gather=object())
    off = OcrPipeline(Cls())
    assert off.page_orient is False
    with pytest.raises(ValueError):
        off.run_oriented(None)
    assert OcrPipeline(Cls(), page_orient=True).page_orient_params == arch.PAGE_ORIENT_PARAMS
    assert PageDetections(np.zeros((0, 8), np.int32), [], np.zeros(0, np.float32), np.zeros(0, np.float32)).turn is None
    monkeypatch.delenv("LUMINA_OCR_PAGE_ORIENTATION", raising=False)
    fresh = object.__new__(svc.OCRService)
    fresh._initialized = False
    svc.OCRService.__init__(fresh)
    assert fresh._use_page_orient is False
    monkeypatch.setenv("LUMINA_OCR_PAGE_ORIENTATION", "1")
    fresh._initialized = False
    svc.OCRService.__init__(fresh)
    assert fresh._use_page_orient is True and fresh._use_angle_cls is False
    # without classifier weights the option is an error result, before any GPU is touched
    fresh._allow_synthetic, fresh._cls_weights = False, ""
    fresh._det_weights = fresh._rec_weights = fresh._rec_dict = "x"
    with pytest.raises(RuntimeError, match="LUMINA_OCR_CLS_WEIGHTS"):
        fresh._ensure_engine()
