"""The restatement of the QR pass (tests/qr_reference.py) reads what the encoder (lumina_ocr.synth.qr_encode / draw_qr) draws: every
version, level and mask, the module sizes, rotations and page positions the device meets, injected errors up to and past the
blocks' capacity, and nothing on pages that only look like a symbol."""
import numpy as np
import pytest

from lumina_ocr import synth
from lumina_ocr.utils import qrcodes as qr

import qr_reference as R


def blank(h: int, w: int) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def text_for(version: int, level: int, salt: int = 0) -> str:
    """A byte-mode text that fills most of the symbol."""
    n = max(1, min(qr.data_codewords(version, level) - 3, 60))
    return ("v%d%s#%d " % (version, qr.LEVELS[level], salt) + "lumina-qr/" * 8)[:n]


def read(page: np.ndarray, **kw):
    _, codes, data, nf = R.qrcodes(page, **kw)
    return codes, data, nf


def test_every_version_level_and_mask_round_trips_at_module_four():
    for version in range(1, 11):
        side = 4 * (17 + 4 * version)
        for level in range(4):
            for mask in range(8):
                page = blank(side + 24, side + 29)
                text = text_for(version, level, mask)
                box = synth.draw_qr(page, 13, 11, synth.qr_encode(text, version, level, mask), 4)
                codes, data, nf = read(page)
                assert nf == 3 and len(codes) == 1, (version, level, mask)
                assert tuple(codes[0]) == box + (version, level, mask, qr.data_codewords(version, level), 0, 0, 0, 0)
                assert R.texts(codes, data) == [text]


@pytest.mark.parametrize("module", [3, 4, 7, 12])
@pytest.mark.parametrize("version", [1, 4, 10])
def test_module_sizes(version, module):
    side = module * (17 + 4 * version)
    page = blank(side + 40, side + 47)
    text = text_for(version, 2)
    box = synth.draw_qr(page, 21, 19, synth.qr_encode(text, version, 2, 6), module)
    codes, data, _ = read(page)
    assert len(codes) == 1 and tuple(codes[0][:8]) == box + (version, 2, 6, qr.data_codewords(version, 2)) and R.texts(codes, data) == [text]


@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
def test_rotations(rotation):
    page = blank(200, 260)
    box = synth.draw_qr(page, 70, 30, synth.qr_encode("ROTATED BY %d" % (90 * rotation), 3, 1, 2), 4, rotation)
    codes, data, _ = read(page)
    assert len(codes) == 1 and tuple(codes[0][:4]) == box and int(codes[0][9]) == rotation
    assert R.texts(codes, data) == ["ROTATED BY %d" % (90 * rotation)]


@pytest.mark.parametrize("x, w", [(0, 200), (50, 200), (7, 131), (195 - 116, 195)])
def test_page_edge_word_boundary_and_ragged_width(x, w):
    """x = 0: the left edge is the page's; x = 50: the symbol straddles pixel 64; W = 131 and 195 are no multiples of 64, and at
    x = 79 of 195 the right edge is the page's."""
    page = blank(150, w)
    box = synth.draw_qr(page, x, 17, synth.qr_encode("0123456789012345", 3, 3, 7), 4)
    codes, data, _ = read(page)
    assert len(codes) == 1 and tuple(codes[0][:4]) == box and R.texts(codes, data) == ["0123456789012345"]


def test_two_symbols_in_one_row_band_give_two_reads():
    page = blank(140, 330)
    a = synth.draw_qr(page, 10, 12, synth.qr_encode("LEFT", 2, 1, 0), 4)
    b = synth.draw_qr(page, 10 + 100 + 16, 12, synth.qr_encode("RIGHT", 2, 1, 1), 4)        # the same size, the same rows, four modules apart
    codes, data, nf = read(page)
    assert nf == 6 and [tuple(c[:4]) for c in codes] == [a, b] and R.texts(codes, data) == ["LEFT", "RIGHT"]


def corrupt(version: int, level: int, mask: int, text: str, block: int, wrong: int, flip=0xFF) -> np.ndarray:
    """The symbol with the first `wrong` data codewords of one block wrong."""
    cw = synth.qr_interleave(synth.qr_data_codewords(text, version, level), version, level)
    nb = qr.block_structure(version, level)[0]
    for i in range(wrong):
        cw[i * nb + block] ^= flip if isinstance(flip, int) else flip[i % len(flip)]
    return synth.qr_matrix(cw, version, level, mask)


@pytest.mark.parametrize("version, level", [(5, 2), (10, 3), (1, 0)])
def test_errors_up_to_the_capacity_are_corrected_and_one_more_is_not_read_as_the_content(version, level):
    nb, _, _, ec = qr.block_structure(version, level)
    t, text = ec // 2, text_for(version, level)
    side = 4 * (17 + 4 * version)
    for wrong in (t, t + 1):
        page = blank(side + 30, side + 30)
        synth.draw_qr(page, 15, 15, corrupt(version, level, 4, text, nb - 1, wrong, flip=(0xFF, 0x5A, 0x01, 0x80)), 4)
        codes, data, _ = read(page)
        if wrong == t:
            assert len(codes) == 1 and int(codes[0][8]) == t and R.texts(codes, data) == [text]
        else:
            assert text not in R.texts(codes, data)
            assert len(codes) == 0                       # (these positions: the locator has no t + 1 roots, the candidate is dropped)


def test_the_second_format_copy_is_read_when_the_first_is_destroyed():
    version, level, mask = 2, 2, 5
    true = qr.format_word(level, mask)
    flips = next(f for f in range(1, 1 << 15) if 4 <= bin(f).count("1") <= 6
                 and min(bin((true ^ f) ^ w).count("1") for w in qr.FORMAT_WORDS) >= 4)       # farther than 3 from every word
    sym = synth.qr_encode("SECOND COPY", version, level, mask)
    for i, (r, c) in enumerate(qr.format_positions(version)[0]):
        if (flips >> i) & 1:
            sym[r, c] = not sym[r, c]
    page = blank(140, 150)
    synth.draw_qr(page, 20, 20, sym, 4)
    codes, data, _ = read(page)
    assert len(codes) == 1 and int(codes[0][10]) == qr.SECOND_COPY and (int(codes[0][5]), int(codes[0][6])) == (level, mask)
    assert R.texts(codes, data) == ["SECOND COPY"]
    for i, (r, c) in enumerate(qr.format_positions(version)[1]):                              # both destroyed: no read
        if (flips >> i) & 1:
            sym[r, c] = not sym[r, c]
    page = blank(140, 150)
    synth.draw_qr(page, 20, 20, sym, 4)
    assert len(read(page)[0]) == 0


def test_three_format_errors_in_the_first_copy_are_within_reach():
    sym = synth.qr_encode("3 OFF", 1, 3, 1)
    for r, c in qr.format_positions(1)[0][:3]:
        sym[r, c] = not sym[r, c]
    page = blank(120, 130)
    synth.draw_qr(page, 18, 18, sym, 4)
    codes, data, _ = read(page)
    assert len(codes) == 1 and int(codes[0][10]) == 3 and R.texts(codes, data) == ["3 OFF"]


def test_a_filled_quiet_zone_is_no_symbol():
    sym = synth.qr_encode("QUIET", 1, 1, 3)
    page = blank(140, 150)
    synth.draw_qr(page, 30, 30, sym, 4)
    assert len(read(page)[0]) == 1
    page[30:114, 30 + 84 + 4:30 + 84 + 8] = 0             # a bar in the second module beside the symbol
    assert len(read(page)[0]) == 0 and len(read(page, quiet=1)[0]) == 1


def test_decoys_give_no_reads():
    page, gt = synth.synth_qr_decoys()
    assert [g["kind"] for g in gt] == ["finder"] * 3 + ["three_finders", "mirrored", "inverted", "halftone"]
    codes, _, nf = read(page)
    assert len(codes) == 0 and nf >= 9                    # the finders are found; nothing is read from them


@pytest.mark.parametrize("kind", ["checkboxes", "radio", "code128", "text"])
def test_other_pages_give_no_reads(kind):
    if kind == "checkboxes":
        page = synth.synth_marks_page(3, h=500, w=700)[0]
    elif kind == "radio":
        page = synth.synth_radio_page(3, h=500, w=700)[0]
    elif kind == "code128":
        page = blank(120, 640)
        synth.render_barcode(page, 20, 20, synth.code128_symbols("NOT A QR CODE"), "Code128", 3, 60)
    else:
        page = synth.synth_page(400, 640, 7, n_lines=14)[0]
    assert len(read(page)[0]) == 0


def test_more_finders_than_the_list_holds_and_the_page_is_not_read():
    page = blank(140, 150)
    synth.draw_qr(page, 20, 20, synth.qr_encode("FULL", 1, 1, 0), 4)
    codes, _, nf = read(page, max_finders=2)
    assert nf == 3 and len(codes) == 0


def test_a_neighbours_finder_nearer_than_the_corners_own_partner_costs_one_try():
    page, want = synth.synth_qr_crowded_page()
    ink = R.ink_mask(page, R.P["threshold"])
    fs = R.find_finders(ink, R.P["min_module"], R.P["max_module"], R.P["centre_tol"], R.P["ring_tol"])
    corner = next(i for i, f in enumerate(fs) if abs(f[0] - 2 * 122) <= 3 and abs(f[1] - 2 * 22) <= 3)
    pairs = R.pairs_of(fs, corner)
    assert len(pairs) >= 2
    assert R.decode_candidate(ink, fs[corner], fs[pairs[0][0]], fs[pairs[0][1]], R.P["quiet"], R.P["timing_max"]) is None     # the cross pair comes first
    codes, data, _ = read(page)
    assert {tuple(int(v) for v in c[:4]): t for c, t in zip(codes, R.texts(codes, data))} == want


def tilted(module: int, version: int, degrees: float):
    """A symbol on a page turned by a small angle (bicubic, as a scanner's residual skew after the page de-skew)."""
    from PIL import Image
    side = module * (17 + 4 * version)
    page = blank(side + 80, side + 83)
    synth.draw_qr(page, 40, 40, synth.qr_encode("TILT %d" % version, version, 1, 2), module)
    return np.asarray(Image.fromarray(page).rotate(degrees, resample=Image.BICUBIC, fillcolor=(255, 255, 255))), "TILT %d" % version


@pytest.mark.parametrize("module, version", [(4, 5), (3, 10), (3, 1)])
@pytest.mark.parametrize("degrees", [0.5, -1.0, 2.0])
def test_a_small_tilt_is_read(module, version, degrees):
    """what the page de-skew leaves: a one-pixel stair on every edge (the reason the core rule is 3/4 solid, arch.QR_PARAMS)"""
    page, text = tilted(module, version, degrees)
    codes, data, nf = read(page)
    assert nf == 3 and R.texts(codes, data) == [text] and int(codes[0][8]) == 0
