"""CPU: the fax restatement (tests/fax_reference.py) against source bitmaps and against libtiff's decoder: the five codings libtiff
writes, legal codings it never writes (the policy encoder of tests/fax_cases.py), the committed streams, and every single-bit flip and
cut of two bitmaps in three codings, where every stream the restatement accepts must be libtiff's picture too."""
import numpy as np
import pytest
from PIL import features

import ccitt_cases as cc
import fax_cases as fc
import fax_reference as fr

needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="libtiff is the encoder and the second decoder of these cases")


@needs_libtiff
@pytest.mark.parametrize("mode", list(fc.MODES))
def test_libtiff_streams_equal_source_and_libtiff(mode):
    comp, t4, k, align = fc.MODES[mode]
    for name, bm in fc.intact_bitmaps().items():
        h, w = bm.shape
        stream = fc.g3_encode(bm, mode)
        if fr.decode(stream, w, h, k, bool(align))[0] != 0:
            # CCITT RLE lines of one byte: the last one begins in the strip's last byte, which libtiff may misread (rand_8x6: it does)
            # and the decoder refuses (test_rle_line_in_the_strips_last_byte_is_refused); a byte behind the strip makes it regular
            assert mode == "rle" and w < 64, (name, mode)
            stream += b"\0"
        for b1 in (False, True):
            st, bits = fr.decode(stream, w, h, k, bool(align), b1)
            assert st == 0 and np.array_equal(bits, cc.expected_bits(bm, b1)), (name, b1, st)
        assert np.array_equal(fr.decode(stream, w, h, k, bool(align))[1], fc.libtiff_fax_bits(stream, w, h, comp, t4)), name
        # K is the encoder's business: any positive value reads the same stream (here: more than the number of rows)
        if k > 0:
            assert np.array_equal(fr.decode(stream, w, h, h + 5, bool(align))[1], cc.expected_bits(bm, False)), name


@needs_libtiff
@pytest.mark.parametrize("mode", list(fc.MODES))
def test_rows_smaller_and_larger_than_coded(mode):
    _, _, k, align = fc.MODES[mode]
    bm = cc.bitmaps()["rand_65x40"]
    stream = fc.g3_encode(bm, mode)
    st, bits = fr.decode(stream, 65, 17, k, bool(align))
    assert st == 0 and np.array_equal(bits, cc.expected_bits(bm[:17], False))
    assert fr.decode(stream, 65, 41, k, bool(align))[0] == -1
    # the same with an RTC behind the last line: six EOLs are no 41st line
    rtc = fc.fax_encode_policy(bm, k=k, eol=mode != "rle", align=bool(align), rtc=True)
    assert fr.decode(rtc, 65, 40, k, bool(align))[0] == 0 and fr.decode(rtc, 65, 41, k, bool(align))[0] == -1


def test_committed_streams():
    for key, (stream, w, h, k, align, digests) in fc.fixtures().items():
        for b1 in (False, True):
            st, bits = fr.decode(stream, w, h, k, bool(align), b1)
            assert st == 0 and cc.sha(bits) == digests[b1], (key, b1)


@needs_libtiff
def test_committed_streams_are_what_libtiff_writes():
    maps = cc.bitmaps()
    for name, mode in fc.FIXTURES:
        assert fc.fixtures()["%s.%s" % (name, mode)][0] == fc.g3_encode(maps[name], mode), (name, mode)


# ---- legal codings libtiff never writes ----
def test_policy_encoder_streams_equal_source_and_libtiff():
    for name, (bm, stream, k, align, tiff) in fc.policy_cases().items():
        h, w = bm.shape
        for b1 in (False, True):
            st, bits = fr.decode(stream, w, h, k, bool(align), b1)
            assert st == 0 and np.array_equal(bits, cc.expected_bits(bm, b1)), (name, st)
        if tiff is not None and features.check("libtiff"):
            assert np.array_equal(fc.libtiff_fax_bits(stream, w, h, *tiff), cc.expected_bits(bm, False)), name


def test_hostile_streams():
    for name, (stream, w, h, k, align, want) in fc.hostile_cases().items():
        assert fr.decode(stream, w, h, k, bool(align))[0] == want, name


# ---- the damage sweep ----
@needs_libtiff
@pytest.mark.parametrize("mode", fc.SWEEP_MODES)
@pytest.mark.parametrize("name", fc.SWEEP_FILES)
def test_damage_sweep_accepted_streams_equal_libtiff(name, mode):
    """every single-bit flip and every cut of libtiff's stream: whatever the restatement accepts (status 0), libtiff decodes to the
    same picture, and the comparison is not empty"""
    comp, t4, _, _ = fc.MODES[mode]
    _, w, h, damaged = fc.damage_sweep(name, mode)
    accepted, differ = 0, []
    for (label, d), (st, bits) in zip(damaged, fc.sweep_restatement(name, mode)):
        assert st in (0, -1, -2), label
        if st == 0:
            accepted += 1
            lt = fc.libtiff_fax_bits(d, w, h, comp, t4)
            if lt is None or not np.array_equal(lt, bits):
                differ.append(label)
    print("%s %s: %d of %d damaged streams accepted" % (name, mode, accepted, len(damaged)))
    assert differ == [] and accepted >= 1, (differ[:10], accepted)


@needs_libtiff
def test_rle_line_in_the_strips_last_byte_is_refused():
    """libtiff misreads its own CCITT RLE stream when the strip's last line fits in the last byte and the code before it was looked up
    across the strip's end.  Over 1500 small bitmaps: whatever the restatement accepts is the source and libtiff's picture, and the
    streams libtiff misreads exist and are all refused."""
    misread = 0
    for seed in range(1500):
        r = np.random.default_rng(seed)
        w, h = int(r.integers(1, 24)), int(r.integers(1, 4))
        bm = r.random((h, w)) < 0.5
        stream = fc.g3_encode(bm, "rle")
        st, bits = fr.decode(stream, w, h, 0, True)
        lt = fc.libtiff_fax_bits(stream, w, h, 2, None)
        wrong = not np.array_equal(lt, cc.expected_bits(bm, False))
        misread += wrong
        assert st == (-1 if wrong else st) and st in (0, -1), seed
        if st == 0:
            assert np.array_equal(bits, cc.expected_bits(bm, False)) and np.array_equal(bits, lt), seed
        else:   # refused for this reason alone: a byte behind the stream makes it regular, for the restatement and for libtiff
            st2, bits2 = fr.decode(stream + b"\0", w, h, 0, True)
            assert st2 == 0 and np.array_equal(bits2, cc.expected_bits(bm, False)), seed
            assert np.array_equal(fc.libtiff_fax_bits(stream + b"\0", w, h, 2, None), bits2), seed
    assert misread >= 5, misread
