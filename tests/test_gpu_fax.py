"""GPU: the fax decoder (fx_decode of csrc/ccitt.hip, through lumina_ocr_fax_decode) byte-equal to the integer restatement
(tests/fax_reference.py): the five codings libtiff writes at the shapes where the kernel can go wrong, legal codings it never writes,
hostile streams with intact neighbours, every single-bit flip and cut of one stream in one launch, and K < 0 against
lumina_ocr_ccitt_decode."""
import numpy as np
import pytest
import torch
from PIL import features

import ccitt_cases as cc
import ccitt_reference as cr
import fax_cases as fc
import fax_reference as fr

pytestmark = pytest.mark.gpu
needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="libtiff is the fax encoder of these cases")


def _decode(engine, streams, rows, cols, params):
    out, status = engine.fax_decode(streams, rows, cols, params)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status


def _check(engine, streams, rows, cols, params, label, all_ok=True):
    """one call; every status equal to the restatement's, every accepted page's bytes too. -> the statuses"""
    got, status = _decode(engine, streams, rows, cols, params)
    for i, (s, (k, align, b1, inv, _)) in enumerate(zip(streams, params)):
        st, bits = fr.decode(s, cols, rows, k, bool(align), bool(b1))
        assert status[i] == st, (label, i, status[i], st)
        if st == 0:
            assert np.array_equal(got[i], fr.to_rgb(bits, bool(inv))), (label, i)
    if all_ok:
        assert status == [0] * len(streams), (label, status)
    return status


def test_committed_streams_equal_restatement_and_digests(engine):
    for key, (stream, w, h, k, align, digests) in fc.fixtures().items():
        params = [(k, align, b1, inv, 0) for b1 in (0, 1) for inv in (0, 1)]
        got, status = _decode(engine, [stream] * 4, h, w, params)
        assert status == [0] * 4, (key, status)
        for i, (_, _, b1, inv, _) in enumerate(params):
            st, bits = fr.decode(stream, w, h, k, bool(align), bool(b1))
            assert st == 0 and cc.sha(bits) == digests[bool(b1)]
            assert np.array_equal(got[i], fr.to_rgb(bits, bool(inv))), (key, b1, inv)


@needs_libtiff
def test_every_coding_in_one_batch_per_shape(engine):
    """widths 1, 7, 8, 9 and 65, 1728 x 3, 8192 x 2 white and black, 2700 x 4 (make-ups beyond 2560), text_640x200 (its streams cross
    the bit reader's 128-byte reload): the five codings libtiff writes in one call, and the source bitmap's pixels"""
    for name, bm in fc.intact_bitmaps().items():
        h, w = bm.shape
        streams, params = [], []
        for mode, (_, _, k, align) in fc.MODES.items():
            s = fc.g3_encode(bm, mode)
            if fr.decode(s, w, h, k, bool(align))[0] != 0:   # CCITT RLE lines of one byte: see fax_reference
                assert mode == "rle" and w < 64
                s += b"\0"
            streams.append(s)
            params.append((k, align, len(streams) & 1, (len(streams) >> 1) & 1, 0))
        got, status = _decode(engine, streams, h, w, params)
        assert status == [0] * 5, (name, status)
        for i, (_, _, b1, inv, _) in enumerate(params):
            assert np.array_equal(got[i], fr.to_rgb(cc.expected_bits(bm, bool(b1)), bool(inv))), (name, i)


@needs_libtiff
def test_rows_one_fewer_rows_more_rows_and_any_positive_k(engine):
    bm = cc.bitmaps()["rand_65x40"]
    streams = [fc.g3_encode(bm, mode) for mode in fc.MODES]
    params = [(k, align, 0, 0, 0) for _, _, k, align in fc.MODES.values()]
    for rows in (1, 17):
        got, status = _decode(engine, streams, rows, 65, params)
        assert status == [0] * 5, (rows, status)
        for i in range(5):
            assert np.array_equal(got[i], fr.to_rgb(cc.expected_bits(bm[:rows], False))), (rows, i)
    assert _check(engine, streams, 41, 65, params, "41 rows", all_ok=False) == [-1] * 5
    _check(engine, [streams[1], streams[3]], 40, 65, [(1000, 0, 0, 0, 0), (2, 0, 0, 0, 1)], "K")
    one = bm[:1]
    _check(engine, [fc.g3_encode(one, mode) for mode in fc.MODES], 1, 65, params, "one coded row")


def _eol_across_the_reload(bm):
    """a 1-D stream of `bm` whose fill puts an EOL's twelve bits across bit 1024 (the bit reader loads a new window once it is 128
    bytes into the one it holds), and the index of that line"""
    fill = [0] * bm.shape[0]
    for y in range(bm.shape[0]):
        at = len(fc.fax_encode_policy_bits(bm[:y], fill=tuple(fill[:y]) or (0,))) if y else 0
        if at > 900:
            assert at <= 1018
            fill[y] = 1018 - at
            bits = fc.fax_encode_policy_bits(bm, fill=tuple(fill))
            assert bits[1018:1030] == fc.EOL
            return cc.bits_to_bytes(bits), y
    raise AssertionError("the stream is shorter than 1024 bits")


def test_policy_encoder_streams(engine):
    """legal codings libtiff never writes: fill of 0, 1, 7, 70 and 2100 bits (longer than the reader's 256-byte window), one-dimensional
    lines anywhere in a K > 0 stream, a two-dimensional first line, runs from repeated 2560 make-ups, an RTC tail, PDF's /K 0 with
    neither EOLs nor alignment; an EOL across the reader's reload"""
    groups = {}
    for name, (bm, stream, k, align, _) in fc.policy_cases().items():
        groups.setdefault(bm.shape, []).append((name, bm, stream, k, align))
    bm = cc.bitmaps()["rand_65x40"]
    across, _ = _eol_across_the_reload(bm)
    groups[bm.shape].append(("eol_across_the_reload", bm, across, 0, 0))
    for (h, w), cases in groups.items():
        streams = [c[2] for c in cases]
        params = [(c[3], c[4], i & 1, 0, 0) for i, c in enumerate(cases)]
        got, status = _decode(engine, streams, h, w, params)
        assert status == [0] * len(cases), ([c[0] for c in cases], status)
        for i, c in enumerate(cases):
            assert np.array_equal(got[i], fr.to_rgb(cc.expected_bits(c[1], bool(i & 1)))), c[0]


def test_hostile_streams_neighbours_intact(engine):
    """truncated, junk, a short and a long line, EOLs in front of some lines only, K > 0 without EOLs, alignment with EOLs, two EOLs in
    a row, a 1 inside fill, zeros to the stream's end, a run of length 0 inside a line: -1 or -2 as the restatement says, and the
    intact streams between them decode as if alone"""
    good = (cc.GOLDEN / "rand_65x40.2d.g3").read_bytes()
    want = fr.to_rgb(fr.decode(good, 65, 40, 1)[1])
    hostile = fc.hostile_cases()
    big = {n: c for n, c in hostile.items() if (c[1], c[2]) == (65, 40)}
    assert len(big) >= 10
    streams, params, expect = [good], [(1, 0, 0, 0, 0)], [0]
    for name, (stream, _, _, k, align, st) in big.items():
        streams += [stream, good]
        params += [(k, align, 0, 0, 0), (1, 0, 0, 0, 0)]
        expect += [st, 0]
    got, status = _decode(engine, streams, 40, 65, params)
    assert status == expect, list(zip(["-"] + [n for n in big for _ in (0, 1)], status, expect))
    assert {-1, -2} <= set(status)
    for i in range(0, len(streams), 2):
        assert np.array_equal(got[i], want), i
    for name, (stream, w, h, k, align, st) in hostile.items():
        if name not in big:
            assert _decode(engine, [stream], h, w, [(k, align, 0, 0, 0)])[1] == [st], name


def test_unsupported_parameters_are_minus_two(engine):
    good = (cc.GOLDEN / "rand_65x40.1d.g3").read_bytes()
    got, status = _decode(engine, [good] * 5, 40, 65, [(0, 0, 0, 0, 2), (0, 0, 0, 0, 3), (0, 0, 0, 0, -1), (0, 0, 0, 0, 1), (0, 0, 0, 0, 0)])
    assert status == [-2, -2, -2, 0, 0]
    assert np.array_equal(got[3], got[4]) and np.array_equal(got[4], fr.to_rgb(fr.decode(good, 65, 40)[1]))
    assert _decode(engine, [good], 1, fr.MAX_COLUMNS + 1, [(0, 0, 0, 0, 0)])[1] == [-2]
    assert _decode(engine, [b""], 40, 65, [(0, 0, 0, 0, 0)])[1] == [-1]


def test_group4_through_the_new_entry_equals_ccitt_decode(engine):
    for name, (stream, w, h, _) in cc.fixtures().items():
        damaged = cc.flip_bit(stream, 40)
        streams = [stream, damaged, stream, stream]
        params4 = [(-1, 0, 0, 0), (-1, 0, 0, 0), (-3, 0, 1, 1), (-1, 1, 0, 0)]
        old, old_status = engine.ccitt_decode(streams, h, w, params4)
        new, new_status = engine.fax_decode(streams, h, w, [p + (0,) for p in params4])
        torch.cuda.synchronize()
        assert new_status == old_status and old_status[0] == 0 and old_status[2] == 0 and old_status[3] == -2, (name, old_status)
        for i, st in enumerate(old_status):
            if st == 0:
                assert torch.equal(old[i], new[i]), (name, i)
    # Group 4 and Group 3 pages in one call
    g4, w, h, _ = cc.fixtures()["rand_65x40"]
    g3 = (cc.GOLDEN / "rand_65x40.1d.g3").read_bytes()
    got, status = _decode(engine, [g4, g3, g4], h, w, [(-1, 0, 0, 0, 0), (0, 0, 0, 0, 0), (-1, 0, 0, 0, 1)])
    assert status == [0, 0, 0]
    assert all(np.array_equal(got[i], cr.to_rgb(cr.decode(g4, w, h)[1])) for i in range(3))


@needs_libtiff
def test_damage_sweep_equals_restatement_neighbours_intact(engine):
    """one call: every single-bit flip and every cut of rand_65x40's one-dimensional stream, the intact stream at every 64th place.
    Status equal to the restatement's on every page, pixels on every accepted page, every intact page untouched."""
    stream, w, h, damaged = fc.damage_sweep("rand_65x40", "1d")
    ref = fc.sweep_restatement("rand_65x40", "1d")
    pages, owner = [], []
    for k, (_, d) in enumerate(damaged):
        if len(pages) % 64 == 0:
            pages.append(stream)
            owner.append(-1)
        pages.append(d)
        owner.append(k)
    pages.append(stream)
    owner.append(-1)
    got, status = _decode(engine, pages, h, w, [(0, 0, 0, 0, 0)] * len(pages))
    want_status = [0 if o < 0 else ref[o][0] for o in owner]
    wrong = [(damaged[o][0] if o >= 0 else "intact", s, t) for o, s, t in zip(owner, status, want_status) if s != t]
    assert wrong == [], wrong[:10]
    intact = fr.to_rgb(fr.decode(stream, w, h)[1])
    accepted = 0
    for i, o in enumerate(owner):
        if o < 0:
            assert np.array_equal(got[i], intact), ("intact page", i)
        elif ref[o][0] == 0:
            accepted += 1
            assert np.array_equal(got[i], fr.to_rgb(ref[o][1])), damaged[o][0]
    assert accepted >= 1, accepted
