"""CPU: the JPEG 2000 restatement against Pillow on damaged files: every single-bit flip of the headers, every 7th bit of the data
and truncation at every 16th byte of three files (33x40 RGB with 2 layers and 3 resolutions; 64x64 L lossless; 40x33 RGB, RLCP, 8x8
blocks).  Wherever the restatement answers 0 its bytes are Pillow's; wherever Pillow raises the restatement answers non-zero.  The
strictness rule has no tolerance: a class of files on which the two could differ is refused (DESIGN.md §3 lists the classes)."""
import warnings

import numpy as np
import pytest

import jp2_cases as jc

BASES = jc.damage_bases()


def test_bases_are_what_they_say():
    info = {name: jc.reference(data)[2] for name, data in BASES}
    assert info["rgb_layers"] == [40, 33, 3, 2, 2, 0, 64, 64]
    assert info["grey_lossless"][:3] == [64, 64, 1] and info["grey_lossless"][4] == 1
    assert info["rgb_rlcp_cb8"][:3] == [33, 40, 3] and info["rgb_rlcp_cb8"][5:] == [1, 8, 8]


@pytest.mark.parametrize("base", BASES, ids=[b[0] for b in BASES])
def test_intact_base(base):
    name, data = base
    status, reason, _, rgb = jc.reference(data)
    assert status == 0, reason
    assert np.array_equal(rgb, jc.expected(data))


@pytest.mark.parametrize("base", BASES, ids=[b[0] for b in BASES])
def test_sweep(base):
    bname, data = base
    sweep = jc.damage_sweep(data)
    accepted, wrong, lenient = 0, [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (Pillow's decompression-bomb warning on flipped size fields)
        for name, damaged in sweep:
            status, reason, _, rgb = jc.reference(damaged)
            try:
                exp = jc.expected(damaged)
            except Exception:
                exp = None
            if status == 0:
                accepted += 1
                if exp is None:
                    lenient.append(name)
                elif exp.shape != rgb.shape or not np.array_equal(exp, rgb):
                    wrong.append(name)
    print(f"{bname}: accepted {accepted} of {len(sweep)}")
    assert not lenient, ("accepted where Pillow raises", lenient[:10])
    assert not wrong, ("bytes differ from Pillow's", wrong[:10])
    assert 0 < accepted < len(sweep)
