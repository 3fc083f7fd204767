"""GPU: the Group 4 decoder (csrc/ccitt.hip, through lumina_ocr_ccitt_decode) byte-equal to the integer restatement
(tests/ccitt_reference.py) and to the source bitmaps: the committed fixtures, the libtiff-encoded cases of tests/ccitt_cases.py with and
without EOFB and with trailing bytes, both BlackIs1 values and /Decode [1 0], a mixed batch, the widest line the decoder takes, and
hostile streams, which must end with -1 and leave their neighbours intact."""
import numpy as np
import pytest
import torch
from PIL import features

import ccitt_cases as cc
import ccitt_reference as cr

pytestmark = pytest.mark.gpu
needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="libtiff is the Group 4 encoder of these cases")


def _decode(engine, streams, rows, cols, params):
    out, status = engine.ccitt_decode(streams, rows, cols, params)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status


def test_fixtures_equal_restatement_and_digests(engine):
    for name, (stream, w, h, digests) in cc.fixtures().items():
        params = [(-1, 0, b1, inv) for b1 in (0, 1) for inv in (0, 1)]
        got, status = _decode(engine, [stream] * 4, h, w, params)
        assert status == [0] * 4, (name, status)
        for k, (_, _, b1, inv) in enumerate(params):
            st, bits = cr.decode(stream, w, h, bool(b1))
            assert st == 0 and cc.sha(bits) == digests[bool(b1)]
            assert np.array_equal(got[k], cr.to_rgb(bits, bool(inv))), (name, b1, inv)


@needs_libtiff
def test_cases_equal_restatement_and_source(engine):
    """per bitmap one call: the strip as libtiff wrote it, cut after the last line (no EOFB), and followed by other bytes"""
    for name, bm in cc.bitmaps().items():
        h, w = bm.shape
        stream = cc.g4_encode(bm)
        used = cr.decode_ex(stream, w, h)[2]
        streams = [stream, stream[:(used + 7) // 8], stream + b"\x00\x01II*\x00 bytes after the data", stream]
        params = [(-1, 0, 0, 0)] * 3 + [(-4, 0, 1, 0)]
        got, status = _decode(engine, streams, h, w, params)
        assert status == [0] * 4, (name, status)
        for k in range(4):
            b1 = bool(params[k][2])
            st, bits = cr.decode(streams[k], w, h, b1)
            assert st == 0 and np.array_equal(bits, cc.expected_bits(bm, b1))
            assert np.array_equal(got[k], cr.to_rgb(bits)), (name, k)


@needs_libtiff
def test_mixed_batch_of_five_pages(engine):
    maps = cc.bitmaps()
    rng = np.random.default_rng(31)
    pages = [maps["rand_65x40"], maps["white_65x40"], maps["black_65x40"], rng.random((40, 65)) < 0.5, rng.random((40, 65)) < 0.05]
    params = [(-1, 0, 0, 0), (-1, 0, 1, 0), (-1, 0, 0, 1), (-1, 0, 1, 1), (-2, 0, 0, 0)]
    got, status = _decode(engine, [cc.g4_encode(p) for p in pages], 40, 65, params)
    assert status == [0] * 5
    for k, (bm, (_, _, b1, inv)) in enumerate(zip(pages, params)):
        assert np.array_equal(got[k], cr.to_rgb(cc.expected_bits(bm, bool(b1)), bool(inv))), k


@needs_libtiff
def test_widest_line_and_rows(engine):
    cols = cr.MAX_COLUMNS
    rng = np.random.default_rng(8)
    bm = np.repeat(rng.random((3, cols // 2)) < 0.5, 2, axis=1)
    bm[1] = (np.arange(cols) & 1) == 0   # a change at every pixel: cols changing elements on one line
    stream = cc.g4_encode(bm)
    got, status = _decode(engine, [stream], 3, cols, [(-1, 0, 0, 0)])
    assert status == [0] and np.array_equal(got[0], cr.to_rgb(cc.expected_bits(bm, False)))
    # fewer rows wanted than coded: the decoder stops after them; more: corrupt
    got, status = _decode(engine, [stream], 2, cols, [(-1, 0, 0, 0)])
    assert status == [0] and np.array_equal(got[0], cr.to_rgb(cc.expected_bits(bm[:2], False)))
    assert _decode(engine, [stream], 4, cols, [(-1, 0, 0, 0)])[1] == [-1] == [cr.decode(stream, cols, 4)[0]]


def test_unsupported_parameters_are_minus_two(engine):
    stream, w, h, _ = cc.fixtures()["rand_65x40"]
    got, status = _decode(engine, [stream] * 4, h, w, [(0, 0, 0, 0), (-1, 1, 0, 0), (3, 0, 0, 0), (-1, 0, 0, 0)])
    assert status == [-2, -2, -2, 0]
    assert np.array_equal(got[3], cr.to_rgb(cr.decode(stream, w, h)[1]))
    assert _decode(engine, [stream], 1, cr.MAX_COLUMNS + 1, [(-1, 0, 0, 0)])[1] == [-2]


def test_truncated_and_random_streams_are_minus_one_neighbours_intact(engine):
    stream, w, h, _ = cc.fixtures()["text_640x200"]
    junk = np.random.default_rng(4242).integers(0, 256, 2048, dtype=np.uint8).tobytes()
    streams = [stream, stream[:len(stream) // 2], junk, stream]
    assert [cr.decode(s, w, h)[0] for s in streams] == [0, -1, -1, 0]
    got, status = _decode(engine, streams, h, w, [(-1, 0, 0, 0)] * 4)
    assert status == [0, -1, -1, 0]
    want = cr.to_rgb(cr.decode(stream, w, h)[1])
    assert np.array_equal(got[0], want) and np.array_equal(got[3], want)
