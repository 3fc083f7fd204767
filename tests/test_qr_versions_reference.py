"""The restatement of the all-versions QR pass (tests/qr_versions_reference.py) reads what the encoder draws: the versions where the
code takes another path, every block structure of versions 11-40, the error capacity, the two version information copies, mixed
sizes, and stage 1's rows for small symbols."""
import numpy as np
import pytest

from lumina_ocr import synth
from lumina_ocr.utils import qrcodes as qr

import qr_reference as R1
import qr_version_cases as C
import qr_versions_reference as R
from table_reference import ink_mask


def read(page, max_version=40):
    _, rc, rd, rf = R.qrcodes(page, max_version)
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, R.texts(rc, rd))}, rc, rd, rf


@pytest.mark.parametrize("version,level", C.EIGHT)
@pytest.mark.parametrize("module", [3, 4])
def test_round_trip_through_a_page(version, level, module):
    side = qr.dimension(version) * module
    page = C.blank(side + 40 + module, side + 29 + module)
    box, text = C.put(page, 14, 15, version, level, module, rotation=(version + module) % 4)
    got, rc, rd, rf = read(page)
    assert got == {box: text} and rf == 3
    assert tuple(int(v) for v in rc[0][4:12]) == (version, level, (version + level) % 8, qr.data_codewords(version, level), 0, (version + module) % 4, 0, 0)
    assert rd.dtype == np.uint8 and rd.shape == (1, qr.MAX_DATA_ALL) and not rd[0, qr.data_codewords(version, level):].any()


@pytest.mark.parametrize("version", range(11, 41))
def test_every_block_structure_round_trips_without_an_image(version):
    for level in range(4):
        text, sym = C.symbol(version, level)
        rows = [sum(int(b) << c for c, b in enumerate(r)) for r in sym]
        data, errors = R.blocks_of_rows(rows, version, level, (version + level) % 8)
        assert errors == 0 and len(data) == qr.data_codewords(version, level)
        assert qr.codewords_text(version, data) == (text, None)


@pytest.mark.parametrize("version,level", [(40, 3), (37, 0)])
def test_error_capacity_of_the_last_block(version, level):
    nb, _, _, ec = qr.block_structure(version, level)
    for extra in (0, 1):
        text, sym = C.corrupted(version, level, nb - 1, ec // 2 + extra)
        page = C.blank()
        box, _ = C.put(page, 12, 13, version, level, sym=sym)
        got, rc, _, _ = read(page)
        assert got == ({} if extra else {box: text})
        assert extra or int(rc[0][8]) == ec // 2 == 15


def test_the_second_version_copy_reads_and_both_destroyed_do_not():
    page = C.blank()
    text, sym = C.version_copy_destroyed(14, 0, (0,))
    a = C.put(page, 20, 20, 14, 0, sym=sym)[0]
    C.put(page, 300, 300, 14, 0, sym=C.version_copy_destroyed(14, 0, (0, 1))[1])
    got, _, _, rf = read(page)
    assert got == {a: text} and rf == 6
    word = qr.version_word(14)
    for copy in (0, 1):
        drawn = sum(int(sym[pos[copy]]) << i for i, pos in enumerate(qr.version_positions(14)))
        assert bin(drawn ^ word).count("1") == (6, 0)[copy]


def test_mixed_sizes_on_one_page_and_the_version_window():
    page = C.blank()
    c, text12 = C.put(page, 20, 30, 12, 2, 4)
    d = synth.draw_qr(page, 400, 60, synth.qr_encode("SMALL NEIGHBOUR", 3, 1, 2), 4)
    assert read(page)[0] == {c: text12, d: "SMALL NEIGHBOUR"}
    assert read(page, 11)[0] == {d: "SMALL NEIGHBOUR"} == read(page, 10)[0]
    page = C.blank()
    f, text14 = C.put(page, 40, 40, 14, 1)
    assert read(page, 13)[0] == {} and read(page, 14)[0] == {f: text14}


def test_small_symbols_give_stage_ones_rows():
    for seed in (3, 4):
        page = synth.synth_qr_page(seed, h=C.H, w=C.W, n_codes=2, text_lines=3, module_px=3)[0]
        ink = ink_mask(page, R.P["threshold"])
        rc1, rd1, rf1 = R1.codes_of_ink(ink)
        rc, rd, rf = R.codes_of_ink(ink, 40)
        assert len(rc1) == 2 and rf == rf1 and np.array_equal(rc, rc1)
        assert np.array_equal(rd[:, :qr.MAX_DATA], rd1) and not rd[:, qr.MAX_DATA:].any()


@pytest.mark.parametrize("degrees", [0.5, 1.0, 2.0])
def test_tilted_pages_read(degrees):
    """25-M and 40-M at 3 px read up to two degrees of tilt; where they are lost is the README's limit, not a promise"""
    for version, h, w in ((25, C.H, C.W), (40, 640, 620)):
        page = C.blank(h, w)
        _, text = C.put(page, 44, 50, version, 1)
        got, rc, rd, _ = read(C.tilted(page, degrees))
        assert R.texts(rc, rd) == [text], (version, degrees)


def test_reach_window_holds_the_true_version():
    """a symbol at m px a module has |AB| = |AC| = 2 n m and me = 14 m in doubled pixels: its version is in reach, with neighbours"""
    for v in range(11, 41):
        n = 10 + 4 * v
        for m in (3, 5, 8):
            reach = R.versions_in_reach(2 * (2 * n * m) ** 2, 3 * 14 * m, 40)
            assert v in reach and 2 <= len(reach) <= 7, (v, m, reach)
    assert R.versions_in_reach(2 * (2 * 54 * 3) ** 2, 3 * 14 * 3, 10) == []
