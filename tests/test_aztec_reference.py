"""CPU: the restatement of the Aztec pass (tests/aztec_reference.py) reads what the encoder of lumina_ocr/utils/aztec.py renders, in
every size, rotation and module size, up to the error capacity and the measured tilts, and nothing else."""
import numpy as np
import pytest

from lumina_ocr import arch, synth
from lumina_ocr.utils import aztec as az

import aztec_pages as AP
import aztec_reference as R

P = arch.AZTEC_PARAMS


def read(page, **kw):
    _, codes, data, finders = R.aztec(page, **kw)
    return codes, data, finders


@pytest.mark.parametrize("compact,layers", az.SYMBOLS)
def test_every_size_round_trips_at_module_three_and_seven_in_all_rotations(compact, layers):
    text = AP.payload(compact, layers)
    m = az.encode(text, compact, layers)
    for module in (3, 7):
        s = AP.side_px(compact, layers, module)
        for rotation in range(4):
            page = AP.blank(s + 20, s + 27)
            box = az.draw(page, 13, 9, m, module, rotation)
            codes, data, finders = read(page)
            assert R.texts(codes, data) == [text] and finders == 1
            ndata = az.symbol_words(text, compact, layers)[1]
            assert tuple(codes[0][:4]) == box and tuple(codes[0][4:12]) == (layers, int(compact), az.word_width(layers), ndata, 0, rotation, 0, 0)


@pytest.mark.parametrize("compact,layers,wrong", [(True, 2, 2), (True, 4, 2), (False, 4, 3), (False, 11, 3)])
def test_mode_message_errors_are_corrected_and_one_more_is_not_read_as_written(compact, layers, wrong):
    words, nd = az.symbol_words("MODE", compact, layers)
    for extra in (0, 1):
        mode = az.mode_words(compact, layers, nd)
        for i in range(wrong + extra):
            mode[2 * i] ^= 9
        s = AP.side_px(compact, layers)
        page = AP.blank(s + 20, s + 20)
        AP.put(page, 10, 10, "", compact, layers, matrix=az.matrix_of_words(compact, layers, words, nd, mode))
        codes, data, _ = read(page)
        if extra == 0:
            assert R.texts(codes, data) == ["MODE"] and int(codes[0][10]) == wrong
        else:
            assert R.texts(codes, data) != ["MODE"]


@pytest.mark.parametrize("compact,layers", AP.WIDTH_ENDS)
def test_the_block_corrects_half_its_check_words_and_one_more_error_gives_no_row(compact, layers):
    text = AP.payload(compact, layers)
    t = AP.capacity(compact, layers, text)
    s = AP.side_px(compact, layers) + 16
    page = AP.blank(s, s + 3)
    AP.put(page, 9, 8, "", compact, layers, matrix=AP.corrupted(text, compact, layers, t))
    codes, data, _ = read(page)
    assert R.texts(codes, data) == [text] and int(codes[0][8]) == t and t >= 2
    page = AP.blank(s, s + 3)
    AP.put(page, 9, 8, "", compact, layers, matrix=AP.corrupted(text, compact, layers, t + 1))
    codes, data, finders = read(page)
    assert len(codes) == 0 and finders == 1                             # no row: not a miscorrection either


@pytest.mark.parametrize("compact,layers", sorted(AP.TILTS))
def test_tilted_symbols_read(compact, layers):
    text = AP.payload(compact, layers, "TILT ")
    s = AP.side_px(compact, layers) + 44
    for x, y in ((22, 20), (25, 24)):
        page = AP.blank(s, s + 5)
        AP.put(page, x, y, text, compact, layers, 3, layers % 4)
        for a in AP.TILTS[(compact, layers)]:
            for sign in (1, -1):
                codes, data, _ = read(AP.tilted(page, sign * a))
                assert R.texts(codes, data) == [text], (x, y, sign * a)


def test_decoys_and_text_give_nothing():
    page, kinds = AP.decoys()
    codes, _, finders = read(page)
    assert len(kinds) == 11 and len(codes) == 0 and finders >= 3
    text = synth.synth_page(150, 330, 5, n_lines=5)[0]
    assert len(read(text)[0]) == 0


def test_a_dirty_quiet_ring_is_a_miss_and_the_page_edge_is_quiet():
    page = AP.blank(80, 80)
    box = AP.put(page, 10, 10, "QUIET", True, 1)
    assert R.texts(*read(page)[:2]) == ["QUIET"]
    dirty = page.copy()
    dirty[20:23, box[2] + 2:box[2] + 4] = 0
    assert len(read(dirty)[0]) == 0
    assert R.texts(*read(dirty, quiet=0)[:2]) == ["QUIET"]
    edge = AP.blank(45, 45)
    AP.put(edge, 0, 0, "EDGE", True, 1)
    assert R.texts(*read(edge)[:2]) == ["EDGE"]


def test_finder_list_overflow():
    page = AP.blank(70, 140)
    AP.put(page, 8, 8, "ONE", True, 1)
    AP.put(page, 80, 12, "TWO", True, 1)
    codes, data, finders = read(page)
    assert R.texts(codes, data) == ["ONE", "TWO"] and finders == 2
    codes, data, finders = read(page, max_finders=1)
    assert len(codes) == 0 and finders == 2
