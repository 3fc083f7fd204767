"""CPU: the restatement of lumina_ocr_aztec_layers (tests/aztec_layers_reference.py) reads what the encoder of lumina_ocr/utils/aztec.py
renders at the sizes where the code takes another path, at the tilts the earlier passes promise, up to the error capacity, and its
stage 1 is the restatement of lumina_ocr_aztec."""
import numpy as np
import pytest

from lumina_ocr.utils import aztec as az

import aztec_layers_pages as LP
import aztec_layers_reference as R2
import aztec_pages as AP
import aztec_reference as R1


@pytest.mark.parametrize("layers", LP.SIZES)
def test_the_six_sizes_round_trip_at_module_three(layers):
    page, box, text = LP.page_of(layers, rotation=layers % 4)
    _, codes, data, finders = LP.reference(page)
    assert R2.texts(codes, data) == [text] and finders == 1 and data.shape == (1, az.MAX_DATA_ALL) and data.dtype == np.uint16
    ndata = az.symbol_words(text, False, layers)[1]
    assert tuple(codes[0][:4]) == box and tuple(codes[0][4:12]) == (layers, 0, az.word_width(layers), ndata, 0, layers % 4, 0, 0)
    assert not data[0, ndata:].any()


def test_read_aztec_takes_large_rows_only_when_told():
    page, _, text = LP.page_of(12)
    _, codes, data, _ = LP.reference(page)
    assert int(codes[0][4]) == 12 and az.read_aztec(codes, data) == [] and az.read_aztec(codes, data, max_layers=11) == []
    assert [e["content"] for e in az.read_aztec(codes, data, max_layers=32)] == [text]
    assert [e["content"] for e in az.read_aztec(codes, data, max_layers=12)] == [text]
    e, = az.read_aztec(codes, data, max_layers=32)
    assert e["kind"] == "Aztec" and e["layers"] == 12 and e["compact"] is False and e["confidence"] == 1.0


def test_the_cap_drops_what_is_above_it_and_eleven_is_stage_one():
    page, _, text = LP.page_of(23)
    assert len(LP.reference(page, 20)[1]) == 0 and len(LP.reference(page, 22)[1]) == 0 and R2.texts(*LP.reference(page, 23)[1:3]) == [text]
    small = AP.blank(120, 330)
    AP.put(small, 8, 8, "SMALL ONE", True, 2)
    AP.put(small, 100, 12, "Full four.", False, 4, 3, 1)
    _, c1, d1, f1 = R1.aztec(small)
    for cap in (11, 32):
        _, c2, d2, f2 = LP.reference(small, cap)
        assert np.array_equal(c1, c2) and np.array_equal(d1, d2[:, :320]) and not d2[:, 320:].any() and f1 == f2 == 2 and len(c1) == 2
    decoys, _ = AP.decoys()
    assert len(LP.reference(decoys)[1]) == 0


@pytest.mark.parametrize("layers", [22, 23])
def test_the_block_corrects_half_its_check_words_and_one_more_error_gives_no_row(layers):
    text = LP.nearly_full(layers)
    t = AP.capacity(False, layers, text)
    good, _, _ = LP.page_of(layers, text=text, matrix=AP.corrupted(text, False, layers, t))
    bad, _, _ = LP.page_of(layers, text=text, matrix=AP.corrupted(text, False, layers, t + 1))
    _, codes, data, _ = LP.reference(good)
    assert R2.texts(codes, data) == [text] and int(codes[0][8]) == t
    assert len(LP.reference(bad)[1]) == 0 and LP.reference(bad)[3] == 1


def test_the_array_reed_solomon_is_the_plain_one():
    rng = np.random.RandomState(7)
    for m, nd, ec, wrong in ((10, 30, 12, 6), (10, 30, 12, 7), (12, 25, 9, 4), (12, 25, 9, 0), (12, 20, 10, 9)):
        data = [int(v) for v in rng.randint(0, 1 << m, nd)]
        block = data + az.rs_check_words(data, ec, m)
        for i in rng.permutation(len(block))[:wrong]:
            block[i] ^= int(rng.randint(1, 1 << m))
        assert R2.rs_correct(block, ec, m) == R1.rs_correct(block, ec, m)
        if wrong <= ec // 2:
            assert R2.rs_correct(block, ec, m)[1] == wrong and R2.rs_correct(block, ec, m)[0][:nd] == data


@pytest.mark.parametrize("layers,degrees", LP.TILTS)
def test_the_promised_tilts_read(layers, degrees):
    text = LP.payload(layers, "TILT ")
    page, _, _ = LP.page_of(layers, rotation=layers % 3, text=text, margin=(22, 20))
    _, codes, data, _ = LP.reference(AP.tilted(page, degrees))
    assert R2.texts(codes, data) == [text]
