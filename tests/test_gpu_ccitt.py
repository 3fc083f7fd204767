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


# ---- damaged streams: device == restatement on every page (the restatement's accepted streams are held to libtiff on the CPU) ----
@pytest.mark.parametrize("name", ["begins_black_65x12", "rand_65x40", pytest.param("rand_7x9", marks=needs_libtiff)])
def test_damage_sweep_equals_restatement_neighbours_intact(engine, name):
    """one call per file: every stream of cc.damage_sweep (single-bit flips and cuts at every byte length), the intact stream at every
    64th position.  Status equal to the restatement's on every page, pixels on every status-0 page, every intact page untouched."""
    stream, w, h, damaged = cc.damage_sweep(name)
    ref = cc.sweep_restatement(name)
    pages, owner = [], []   # owner: the damaged stream's index, -1 for the intact one
    for k, (_, d) in enumerate(damaged):
        if len(pages) % 64 == 0:
            pages.append(stream)
            owner.append(-1)
        pages.append(d)
        owner.append(k)
    pages.append(stream)
    owner.append(-1)
    assert all(o == -1 for o in owner[::64]) and sorted(o for o in owner if o >= 0) == list(range(len(damaged)))
    got, status = _decode(engine, pages, h, w, [(-1, 0, 0, 0)] * len(pages))
    want_status = [0 if o < 0 else ref[o][0] for o in owner]
    wrong = [(damaged[o][0] if o >= 0 else "intact", s, t) for o, s, t in zip(owner, status, want_status) if s != t]
    assert wrong == [], wrong[:10]
    intact = cr.to_rgb(cr.decode(stream, w, h)[1])
    accepted = 0
    for i, o in enumerate(owner):
        if o < 0:
            assert np.array_equal(got[i], intact), ("intact page", i)
        elif ref[o][0] == 0:
            accepted += 1
            assert np.array_equal(got[i], cr.to_rgb(ref[o][1])), damaged[o][0]
    assert accepted >= 20, accepted
    if name == "rand_65x40":   # a pass code whose b2 is the line's end (T.6: pass mode only when b2 lies left of a1): libtiff reads these two differently
        labels = [l for l, _ in damaged]
        assert [status[owner.index(labels.index("bit %d" % b))] for b in (5230, 5309)] == [-1, -1]


# ---- legal streams that libtiff never writes (cc.g4_encode_policy, pinned against libtiff's decoder on the CPU) ----
@pytest.mark.parametrize("p_horiz", [0.0, 0.3, 1.0])
def test_policy_encoder_streams_equal_source(engine, p_horiz):
    """vertical pairs recoded in horizontal mode with probability p_horiz, runs from 2560 up as repeated make-ups, with and without
    EOFB; widths around the 32-pixel words of the line stage; a line of 8192 changing elements in horizontal mode alone; a stream that
    ends on the last bit of its last byte.  Status 0 and the pixels of the source bitmap, both BlackIs1 values."""
    cases = dict(cc.policy_bitmaps())
    cases["exact_fit"], exact = cc.exact_fit_stream(p_horiz)
    for name, bm in cases.items():
        h, w = bm.shape
        with_eofb, without = (cc.g4_encode_policy(bm, np.random.default_rng(5), p_horiz, e) for e in (True, False))
        if name == "exact_fit":
            without = exact
            assert cr.decode_ex(exact, w, h)[2] == 8 * len(exact)
        streams = [with_eofb, without, without]
        params = [(-1, 0, 0, 0), (-1, 0, 0, 0), (-1, 0, 1, 0)]
        got, status = _decode(engine, streams, h, w, params)
        assert status == [0] * 3, (name, status)
        for k, (_, _, b1, _) in enumerate(params):
            assert np.array_equal(got[k], cr.to_rgb(cc.expected_bits(bm, bool(b1)))), (name, k)
