"""CPU: the restatement of the two-stage Data Matrix pass (tests/dm_sizes_reference.py) reads what the encoder drew: the nine large
sizes in every rotation, another pitch, the cap, the error capacity of the short and the long blocks, and it leaves stage 1 alone."""
import numpy as np
import pytest

from lumina_ocr import arch, synth
from lumina_ocr.utils import datamatrix as dm

import dm_pages as DP
import dm_reference as R1
import dm_sizes_pages as LP
import dm_sizes_reference as R2

P = arch.DM_PARAMS


@pytest.mark.parametrize("side", LP.SIDES)
def test_every_size_in_every_rotation(side):
    size = LP.size_of(side)
    for rotation in range(4):
        page, box, text = LP.page_of(size, rotation)
        assert page.shape[:2] == (3 * side + 48, 3 * side + 64)
        _, rc, rd, n1 = LP.reference(page)
        assert LP.found(rc, rd) == {box: text}
        assert tuple(rc[0][4:12]) == (side, side, dm.ALL_SIZES[size][2], 0, rotation, 0, 0, 0) and not rd[0, dm.ALL_SIZES[size][2]:].any()
        assert len(R1.datamatrix(page)[1]) == 0                                # (stage 1 alone reads nothing here)
    assert LP.page_of(21)[0].shape[:2] == (240, 256) and LP.page_of(29)[0].shape[:2] == (480, 496)


def test_another_pitch():
    page, box, text = LP.page_of(22, rotation=3, module=7)
    _, rc, rd, _ = LP.reference(page)
    assert LP.found(rc, rd) == {box: text} and tuple(rc[0][4:6]) == (72, 72)


def test_144_round_trips_through_the_restatement():
    nd = dm.ALL_SIZES[29][2]
    data = [(p * 7 + p // 256) % 256 for p in range(nd)]
    page, box, _ = LP.page_of(29, 1, text="", matrix=synth.dm_matrix(synth.dm_interleave(data, 29), 29))
    _, rc, rd, _ = LP.reference(page)
    assert [tuple(r[:4]) for r in rc] == [box] and rd[0, :nd].tolist() == data and not rd[0, nd:].any()


def test_pages_of_small_symbols_equal_stage_one():
    pages = [synth.synth_dm_page(5, 300, 500, n_codes=3, text_lines=2)[0], synth.synth_dm_decoys()[0], DP.blank()]
    DP.put(pages[2], 20, 20, DP.payload(14), 14, 3, 2)
    for page in pages:
        _, c1, d1, n1 = R1.datamatrix(page)
        for cap in (52, 144):
            _, c2, d2, n2 = R2.datamatrix_sizes(page, cap)
            assert np.array_equal(c1, c2) and np.array_equal(d1, d2[:, :dm.MAX_DATA]) and not d2[:, dm.MAX_DATA:].any() and n1 == n2
    assert len(R1.datamatrix(pages[2])[1]) == 1


def mixed_page():
    page = LP.blank(240, 420)
    a = DP.put(page, 20, 30, "SMALL 24", dm.size_index(24, 24), 3, 1)
    b = synth.draw_dm(page, 200, 24, synth.dm_encode(LP.payload(21), 21), 3, 2)
    return page, a, b


def test_max_size_is_a_cap():
    page, a, b = mixed_page()
    _, c1, d1, n1 = R1.datamatrix(page)
    _, c2, d2, n2 = LP.reference(page, 52)
    assert np.array_equal(c1, c2) and np.array_equal(d1, d2[:, :dm.MAX_DATA]) and n1 == n2 and LP.found(c2, d2) == {a: "SMALL 24"}
    _, c3, d3, n3 = LP.reference(page, 64)
    assert LP.found(c3, d3) == {a: "SMALL 24", b: LP.payload(21)} and n3 == n1
    assert [tuple(r[:4]) for r in c3] == sorted((a, b), key=lambda t: (t[1], t[0]))
    big = LP.blank(104 * 3 + 48, 2 * 104 * 3 + 100)
    p96 = synth.draw_dm(big, 20, 24, synth.dm_encode(LP.payload(25), 25), 3)
    p104 = synth.draw_dm(big, 350, 24, synth.dm_encode(LP.payload(26), 26), 3)
    for cap, want in ((96, {p96: LP.payload(25)}), (103, {p96: LP.payload(25)}), (104, {p96: LP.payload(25), p104: LP.payload(26)})):
        _, rc, rd, _ = LP.reference(big, cap)
        assert LP.found(rc, rd) == want


@pytest.mark.parametrize("size,block", [(29, 9), (29, 0), (26, 5)])
def test_a_block_corrects_half_its_check_words_and_not_one_more(size, block):
    """the last block of 144 x 144 is one of its two short ones"""
    text = LP.payload(size)
    d, ec = dm.block_lengths(size)[block]
    assert (d, ec) == {(29, 9): (155, 62), (29, 0): (156, 62), (26, 5): (136, 56)}[(size, block)]
    good, box, _ = LP.page_of(size, text=text, matrix=LP.corrupted(text, size, block, ec // 2))
    bad, _, _ = LP.page_of(size, text=text, matrix=LP.corrupted(text, size, block, ec // 2 + 1))
    _, rc, rd, _ = LP.reference(good)
    assert LP.found(rc, rd) == {box: text} and int(rc[0][7]) == ec // 2
    e, = dm.read_datamatrix(rc, rd)
    assert e["errors"] == ec // 2 and e["confidence"] == 1.0 - (ec // 2) / dm.capacity_errors(size)
    _, rc, rd, _ = LP.reference(bad)
    assert text not in R2.texts(rc, rd)


def test_what_loses_the_large_symbol_leaves_stage_one_alone():
    page, a, b = mixed_page()
    touched, ring = page.copy(), page.copy()
    touched[b[1] - 4:b[1] + 2, b[2] - 1:b[2] + 5] = 0                          # ink touching the L's elbow (the symbol is turned twice: top right)
    ring[b[1] - 3:b[1] - 1, b[0] + 30:b[0] + 60] = 0                           # ink in the quiet ring, touching nothing
    for name, p in (("touched", touched), ("ring", ring)):
        _, rc, rd, _ = LP.reference(p)
        assert LP.found(rc, rd) == {a: "SMALL 24"}, name
    _, rc, rd, _ = LP.reference(ring, quiet=0)
    assert LP.found(rc, rd) == {a: "SMALL 24", b: LP.payload(21)}


def crowded_page():
    """a 24 x 24 and two 64 x 64 symbols; at max_module = 3 the large ones are candidates of stage 2 alone"""
    page = LP.blank(240, 620)
    a = DP.put(page, 20, 30, "SMALL 24", dm.size_index(24, 24), 3, 1)
    b = synth.draw_dm(page, 200, 24, synth.dm_encode(LP.payload(21), 21), 3, 2)
    c = synth.draw_dm(page, 410, 30, synth.dm_encode(LP.payload(21, "second "), 21), 3)
    return page, a, b, c


def test_a_stage_two_list_over_capacity_is_not_read_and_stage_one_is():
    page, a, b, c = crowded_page()
    kw = dict(min_module=3, max_module=3)
    ink = page[..., 0] < 128
    assert len(R1.find_candidates(ink, 3, 3)) == 1 and len(R2.large_candidates(ink, 3, 3)) == 2
    _, rc, rd, n1 = LP.reference(page, 144, max_candidates=2, **kw)
    assert LP.found(rc, rd) == {a: "SMALL 24", b: LP.payload(21), c: LP.payload(21, "second ")} and n1 == 1
    _, rc, rd, n1 = LP.reference(page, 144, max_candidates=1, **kw)
    assert LP.found(rc, rd) == {a: "SMALL 24"} and n1 == 1


@pytest.mark.parametrize("side", [64, 104, 144])
def test_tilts_read_where_both_placements_of_the_sweep_read(side):
    """upright must read: there the diagonal extremes are the exact corners"""
    made, text = LP.tilt_pages(side)
    for deg, at, page in made:
        if deg == 0.0 or (side, deg) in LP.TILT_READS:
            _, rc, rd, _ = LP.reference(page)
            assert R2.texts(rc, rd) == [text], (side, deg, at)
    assert {d for s, d in LP.TILT_READS if s == side} <= set(LP.SWEEP)
