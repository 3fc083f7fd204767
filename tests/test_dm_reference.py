"""The restatement of the Data Matrix pass (tests/dm_reference.py) on synthetic pages: every size at every rotation and two module
sizes, the error-correction limit of every block and one error more, residual skew, what looks like a symbol and is none, ink that
touches the L, and the overflow rules.  The GPU tests hold the device to this definition; these hold the definition to the symbols."""
import numpy as np
import pytest
from PIL import Image

from lumina_ocr import arch, synth
from lumina_ocr.utils import datamatrix as dm

import dm_reference as R

P = arch.DM_PARAMS


def blank(h: int, w: int) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def payload(size: int) -> str:
    return "1234" if size == 0 else ("S%d " % size + "restated / " * 24)[:dm.SIZES[size][2] - 1]


def read(page, **kw):
    _, rc, rd, n = R.datamatrix(page, **kw)
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, R.texts(rc, rd))}, rc, n


@pytest.mark.parametrize("module", [3, 7])
def test_every_size_at_every_rotation(module):
    for s in range(dm.NUM_SIZES):
        side = max(dm.SIZES[s][:2]) * module + 2 * module + 9
        for rot in range(4):
            page = blank(side, side + 5)
            box = synth.draw_dm(page, module + 2, module + 4, synth.dm_encode(payload(s), s), module, rot)
            got, rc, n = read(page)
            assert got == {box: payload(s)} and n >= 1, (s, rot)
            assert tuple(int(v) for v in rc[0][4:]) == dm.SIZES[s][:3] + (0, rot, 0, 0, 0), (s, rot)


@pytest.mark.parametrize("size", [0, 3, 8, 13, 14, 16, 20])
def test_most_errors_each_block_corrects_and_one_more_is_dropped(size):
    nb, ec = dm.SIZES[size][6], dm.SIZES[size][3] // dm.SIZES[size][6]
    for extra in (0, 1):
        cw = synth.dm_interleave(synth.dm_data_codewords(payload(size), size), size)
        total = len(cw)
        for b in range(nb):
            for i in range(ec // 2 + extra):
                cw[(total - 1 - b) - nb * 2 * i] ^= (0xFF, 0x5A, 0x01, 0x80)[i % 4]      # check and data codewords alike, every other one of the block
        page = blank(52 * 3 + 20, 52 * 3 + 24)
        box = synth.draw_dm(page, 9, 7, synth.dm_matrix(cw, size), 3)
        got, rc, n = read(page)
        assert n >= 1
        if extra:
            assert got == {}
        else:
            assert got == {box: payload(size)} and int(rc[0][7]) == nb * (ec // 2)
    assert R.rs_correct([0] * 10, 4) == ([0] * 10, 0) and R.rs_correct([0, 0, 0, 7, 0, 0, 9, 0, 0, 0], 4)[1] == 2
    assert R.rs_correct([1, 0, 0, 7, 0, 0, 9, 0, 0, 0], 4) is None


@pytest.mark.parametrize("angle", [0.5, 1.0, 2.0, -2.0])
def test_residual_skew_reads(angle):
    """The grid is affine through three corners of the L, so a tilt costs nothing but the stairs on the module edges.  Limit, not a
    promise: 52 x 52 at 3 px still reads at 3 degrees and is lost at 5 (the diagonal extremes leave the L's corners, the module
    centres the modules); the pipeline's de-skew leaves less than a degree."""
    for s, m, text in ((14, 3, payload(14)), (5, 4, payload(5)), (19, 4, payload(19))):
        page = blank(243, 243)
        synth.draw_dm(page, 40, 40, synth.dm_encode(text, s), m)
        page = np.asarray(Image.fromarray(page).rotate(angle, resample=Image.BICUBIC, fillcolor=(255, 255, 255)))
        got, rc, n = read(page)
        assert list(got.values()) == [text] and n >= 1, (s, angle)


def test_decoys_read_as_nothing():
    page, gt = synth.synth_dm_decoys()
    kinds = [g["kind"] for g in gt]
    assert kinds == ["table", "letter_l", "qr", "solid", "checkbox", "gap", "mirrored", "inverted"]
    got, rc, n = read(page)
    assert got == {} and len(rc) == 0 and n >= 6
    for g in gt:                                       # each alone: nothing either, and which of them the filter lets through to the tries
        x0, y0, x1, y1 = g["box"]
        alone = blank(*page.shape[:2])
        alone[y0:y1 + 1, x0:x1 + 1] = page[y0:y1 + 1, x0:x1 + 1]
        got, rc, n = read(alone)
        assert got == {} and (n >= 1) == (g["kind"] != "inverted" or n >= 1), g["kind"]
        if g["kind"] in ("table", "letter_l", "solid", "checkbox", "gap", "mirrored"):
            assert n >= 1, g["kind"]
    # the gap is what loses the sixth: the same symbol whole reads
    whole = blank(120, 120)
    box = synth.draw_dm(whole, 10, 10, synth.dm_encode("GAP IN THE ARM", 4), 4)
    assert read(whole)[0] == {box: "GAP IN THE ARM"}
    sym = synth.dm_encode("GAP IN THE ARM", 4)
    sym[6:9, 0] = False
    gap = blank(120, 120)
    synth.draw_dm(gap, 10, 10, sym, 4)
    assert read(gap)[0] == {} and read(gap, solid_max=3)[0] == {}


def test_ink_touching_the_l_is_a_miss_and_a_dirty_quiet_zone_too():
    page = blank(120, 160)
    box = synth.draw_dm(page, 30, 20, synth.dm_encode("TOUCHED", 3), 4)
    assert read(page)[0] == {box: "TOUCHED"}
    touched = page.copy()
    touched[box[3] - 3:box[3] + 1, 10:30] = 0          # a stroke that runs into the L's foot: the component's box is no longer the symbol's
    assert read(touched)[0] == {}
    near = page.copy()
    near[20:84, box[2] + 3:box[2] + 5] = 0             # a rule inside the quiet ring, touching nothing
    assert read(near)[0] == {} and read(near, quiet=0)[0] == {box: "TOUCHED"}
    edge = blank(64, 64)
    box = synth.draw_dm(edge, 0, 0, synth.dm_encode("EDGE", 3), 4)      # the page edge counts as quiet
    assert box == (0, 0, 63, 63) and read(edge)[0] == {box: "EDGE"}


def test_overflow_rules():
    page = blank(120, 260)
    a = synth.draw_dm(page, 10, 10, synth.dm_encode("ONE", 1), 4)
    b = synth.draw_dm(page, 130, 30, synth.dm_encode("TWO", 2), 4)
    got, rc, n = read(page)
    assert got == {a: "ONE", b: "TWO"} and n == 2 and [tuple(c[:2]) for c in rc] == [a[:2], b[:2]]       # sorted by (y0, x0)
    got, rc, n = read(page, max_candidates=1)          # more candidates than the list holds: the page is not read
    assert got == {} and n == 2
    got, rc, n = read(page, max_candidates=2)
    assert len(got) == 2
    codes, data, n = R.codes_of_ink(R.ink_mask(page, P["threshold"]))
    assert codes.shape == (2, 12) and data.shape == (2, dm.MAX_DATA) and not data[0, 5:].any() and not data[1, 8:].any()


def test_module_range_and_thresholds():
    page = blank(80, 80)
    box = synth.draw_dm(page, 8, 8, synth.dm_encode("1234", 0), 5)
    assert read(page)[0] == {box: "1234"}
    assert read(page, min_module=6)[0] == {} and read(page, max_module=4)[0] == {}
    spoiled = page.copy()
    spoiled[8:13, 13:18] = 0                           # one light clock module made dark
    got, rc, _ = read(spoiled)
    assert got == {box: "1234"} and int(rc[0][9]) == 1 and read(spoiled, timing_max=0)[0] == {}
    holed = page.copy()
    holed[28:33, 8:13] = 255                           # one module of the upright cleared (the L stays one component through the data)
    got, rc, _ = read(holed)
    assert got == {box: "1234"} and int(rc[0][10]) == 1 and read(holed, solid_max=0)[0] == {}
