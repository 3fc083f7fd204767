"""CPU: the container readers on fax-coded pages.  utils/tiff_pages.py takes Compression 2 (CCITT RLE) and 3 (Group 3) with the
parameters lumina_ocr_fax_decode wants, FillOrder 2 included, and refuses uncompressed mode and T4Options bits it does not know;
utils/pdf_pages.py hands /K and /EncodedByteAlign through.  The strips the reader returns decode, by the restatement, to Pillow's page."""
import numpy as np
import pytest
from PIL import features

import ccitt_cases as cc
import fax_cases as fc
import fax_reference as fr
import pdf_cases as pc
import tiff_cases as tc
from lumina_ocr.utils import pdf_pages as pp
from lumina_ocr.utils import tiff_pages as tp

needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="libtiff is the fax encoder of these cases")


def _restated_page(page: tp.PageImage) -> np.ndarray:
    """the page's strips through the restatement, as the provider sends them to the device: RGB u8 [H][W][3]"""
    k, align, b1, invert = page.ccitt_params()
    rows = []
    for n, strip in enumerate(page.strips):
        st, bits = fr.decode(bytes(strip), page.width, page.strip_rows(n), k, bool(align), bool(b1))
        assert st == 0, (n, st)
        rows.append(fr.to_rgb(bits, bool(invert)))
    return np.concatenate(rows)


@needs_libtiff
@pytest.mark.parametrize("mode", list(fc.MODES))
def test_reader_takes_compression_2_and_3(mode):
    comp, t4, k, align = fc.MODES[mode]
    bm = cc.bitmaps()["noise_67x40"]
    for photo in (0, 1):
        for fill_order in (1, 2):
            data = tc.tiff_file([fc.g3_frame(bm, mode, photo, fill_order, rps=7)], big_endian=fill_order == 2)
            (page,) = tp.read_pages(data)
            assert isinstance(page, tp.PageImage), page.reason
            assert (page.codec, page.width, page.height, page.rows_per_strip, len(page.strips)) == ("rle" if comp == 2 else "group3", 67, 40, 7, 6)
            assert page.ccitt_params() == (k, align, 0, int(photo == 1)) and page.fill_order == fill_order
            assert np.array_equal(_restated_page(page), tc.pillow_rgb(data)), (photo, fill_order)


def _one_strip(t4opts, comp=3, extra=None, bits=1, photo=0):
    stream = (cc.GOLDEN / "rand_65x40.1d.g3").read_bytes()
    tags = tc.base_tags(65, 40, comp, photo, bits, 1, None, extra)
    if t4opts is not None:
        tags[292] = (4, [t4opts])
    return tc.tiff_file([dict(strips=[stream], tags=tags)])


def test_t4options():
    for t4, want in ((None, 0), (0, 0), (1, 1), (4, 0), (5, 1)):
        (page,) = tp.read_pages(_one_strip(t4))
        assert isinstance(page, tp.PageImage) and page.ccitt_params() == (want, 0, 0, 0), t4
    for t4, reason in ((2, "uncompressed mode"), (3, "uncompressed mode"), (6, "uncompressed mode"), (8, "T4Options 8"), (0x10001, "T4Options 65537")):
        (page,) = tp.read_pages(_one_strip(t4))
        assert isinstance(page, tp.TiffRefused) and reason in page.reason, (t4, page.reason)
    # Compression 2 has no T4Options: the tag is not looked at
    (page,) = tp.read_pages(_one_strip(2, comp=2))
    assert isinstance(page, tp.PageImage) and page.ccitt_params() == (0, 1, 0, 0)


def test_what_is_still_refused():
    for kw, reason in ((dict(bits=8), "Group 3 / CCITT RLE that is not one bit of grey"), (dict(comp=2, bits=8), "Group 3 / CCITT RLE that is not one bit of grey"),
                       (dict(extra={317: 2}), "Predictor 2"), (dict(extra={256: 8193}), "wider than 8192"), (dict(extra={266: 3}), "FillOrder 3")):
        (page,) = tp.read_pages(_one_strip(0, **kw))
        assert isinstance(page, tp.TiffRefused) and reason in page.reason, (kw, page.reason)
    # FillOrder 2 stays what it was for the byte-oriented codecs
    (page,) = tp.read_pages(tc.tiff_file([tc.frame(np.zeros((4, 8), np.uint8), 8, tc.PACKBITS, extra={266: 2})]))
    assert isinstance(page, tp.TiffRefused) and "FillOrder 2" in page.reason


@needs_libtiff
def test_multi_page_file_with_mixed_codings():
    maps = cc.bitmaps()
    frames = [fc.g3_frame(maps["rand_65x40"], "1d", rps=7), fc.g3_frame(maps["noise_67x40"], "2d_aligned", 1, 2, rps=16),
              fc.g3_frame(maps["text_640x200"], "rle", 0, 1), tc.g4_frame(maps["begins_black_65x12"], 0, 1), fc.g3_frame(maps["rand_65x40"], "2d", 1, 1, rps=40)]
    data = tc.tiff_file(frames)
    pages = tp.read_pages(data)
    assert [type(p) for p in pages] == [tp.PageImage] * 5
    assert [p.codec for p in pages] == ["group3", "group3", "rle", "group4", "group3"]
    assert [p.ccitt_params() for p in pages] == [(0, 0, 0, 0), (1, 0, 0, 1), (0, 1, 0, 0), (-1, 0, 0, 0), (1, 0, 0, 1)]
    assert [len(p.strips) for p in pages] == [6, 3, 1, 1, 1]
    for k in (0, 1, 2, 4):
        assert np.array_equal(_restated_page(pages[k]), tc.pillow_rgb(data, k)), k


def test_pdf_page_carries_k_and_alignment():
    stream = (cc.GOLDEN / "rand_65x40.2d.g3").read_bytes()
    parms = ("<< /K 0 /Columns 65 /Rows 40 >>", "<< /K 4 /Columns 65 /Rows 40 /EndOfLine true /BlackIs1 true >>",
             "<< /K 0 /EncodedByteAlign true /Columns 65 /EndOfBlock false /DamagedRowsBeforeError 3 >>")
    doc = pc.document([{"image": pc.image_obj(65, 40, "/CCITTFaxDecode", stream, bits=1, parms=p), "box": (65, 40)} for p in parms])
    pages = pp.read_pages(doc)
    assert [p.filter for p in pages] == ["CCITTFaxDecode"] * 3
    assert [p.params for p in pages] == [{"K": 0, "EncodedByteAlign": False, "BlackIs1": False, "invert": False},
                                         {"K": 4, "EncodedByteAlign": False, "BlackIs1": True, "invert": False},
                                         {"K": 0, "EncodedByteAlign": True, "BlackIs1": False, "invert": False}]
    st, bits = fr.decode(bytes(pages[1].stream), 65, 40, 4, False, True)
    assert st == 0 and np.array_equal(bits, cc.expected_bits(cc.bitmaps()["rand_65x40"], True))
