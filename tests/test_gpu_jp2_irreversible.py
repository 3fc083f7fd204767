"""GPU: the 9/7 path of the device JPEG 2000 decoder (csrc/jp2dec.hip, through lumina_ocr_jp2_decode_irreversible) vs Pillow's
Image.open(f).convert('RGB'), byte for byte: every intact case of tests/jp2_irreversible_cases.py, a batch that mixes 5/3 and 9/7
files, rows and columns longer than one lifting window, the 5/3 cases through the new entry, the old entry's refusal, and a seeded
sample of the damage sweep against the restatement.  Every damaged file here has gone through the sanitized host program and the
restatement (tests/test_jp2_irreversible_sanitized.py); none is built to provoke a fault."""
import numpy as np
import pytest
import torch

import jp2_cases as jc
import jp2_irreversible_cases as ic
import jp2_irreversible_reference as ir
from lumina_ocr import synth
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu


def _by_size(files):
    groups = {}
    for name, data in files:
        _, info = Engine.jp2_probe_irreversible(data)
        groups.setdefault((info["height"], info["width"]), []).append((name, data))
    return groups


def _differs(got, want):
    d = np.argwhere(got != want)
    return "%d of %d values differ, first at %s: got %s want %s" % (len(d), got.size, d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])])


def test_every_intact_case_equals_pillow(engine):
    cases = ic.intact()
    for (h, w), group in _by_size(cases).items():
        out, status = engine.jp2_decode_irreversible([d for _, d in group], h, w)
        assert status == [0] * len(group), (h, w, status)
        for k, (name, data) in enumerate(group):
            got, want = out[k].cpu().numpy(), jc.expected(data)
            assert np.array_equal(got, want), (name, _differs(got, want))


def test_mixed_batch_of_both_transforms(engine):
    """32 distinct 96 x 128 files in one call, 5/3 and 9/7 alternating, with different level counts: both kinds equal Pillow"""
    h, w = 96, 128
    files = []
    for i in range(32):
        mode = "RGB" if i % 4 < 2 else "L"
        opts = dict(irreversible=bool(i % 2), num_resolutions=1 + i % 6)
        if i % 8 >= 4:
            opts["quality_layers"] = [30, 8] if i % 16 >= 8 else [12]
        opts["codeblock_size"] = [(64, 64), (32, 32), (16, 64)][i % 3]
        files.append(jc.write(jc.content("page" if i % 3 else "noise", h, w, mode, seed=2000 + i), **opts))
    assert len(set(files)) == 32
    out = torch.full((32, h, w, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.jp2_decode_irreversible(files, h, w, out=out)
    assert status == [0] * 32, status
    got = out.cpu().numpy()
    for k, data in enumerate(files):
        want = jc.expected(data)
        assert np.array_equal(got[k], want), (k, _differs(got[k], want))
    # the entry without the option refuses exactly the 9/7 half and leaves those slots as they were
    out2 = torch.full((32, h, w, 3), 77, dtype=torch.uint8, device="cuda")
    out2, status2 = engine.jp2_decode(files, h, w, out=out2)
    assert status2 == [-2 if i % 2 else 0 for i in range(32)]
    got2 = out2.cpu().numpy()
    for k in range(32):
        assert np.array_equal(got2[k], got[k]) if k % 2 == 0 else (got2[k] == 77).all(), k


def test_old_entry_still_refuses(engine):
    data = dict(ic.intact())["s100x130_RGB"]
    rc, info = Engine.jp2_probe(data)
    assert rc == -2 and "9/7" in info["reason"]
    out = torch.full((1, 100, 130, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.jp2_decode([data], 100, 130, out=out)
    assert status == [-2] and bool((out == 77).all())


def test_reversible_cases_through_the_new_entry(engine):
    """the 5/3 intact() files: the new call gives the bytes lumina_ocr_jp2_decode gives"""
    for (h, w), group in _by_size(jc.intact()).items():
        files = [d for _, d in group]
        a, sa = engine.jp2_decode_irreversible(files, h, w)
        b, sb = engine.jp2_decode(files, h, w)
        assert sa == sb == [0] * len(files), (h, w, sa, sb)
        assert torch.equal(a, b), (h, w)


@pytest.mark.parametrize("shape", [(300, 420), (130, 100), (58, 258)], ids=["h300w420", "h130w100", "h58w258"])
def test_lines_longer_than_a_window(engine, shape):
    """420 columns: two windows of j2_dwt97_h (256 samples) at the last level; 300 and 130 rows: six and three windows of j2_dwt97_v
    (56 rows); 420 / 100 columns: seven and two of its 64-column strips, the last one part full; 258 x 58: a second window of two
    samples, shorter than its halo, both ways.  Default rate and a layered file, RGB with the colour transform and grey."""
    h, w = shape
    page = synth.synth_page(h, w, 21, n_lines=max(1, h // 50))[0]
    files = [jc.write(page, irreversible=True), jc.write(np.ascontiguousarray(page[:, :, 1]), irreversible=True, quality_layers=[20], num_resolutions=4)]
    out, status = engine.jp2_decode_irreversible(files, h, w)
    assert status == [0, 0]
    for k, data in enumerate(files):
        got, want = out[k].cpu().numpy(), jc.expected(data)
        assert np.array_equal(got, want), (k, _differs(got, want))


def test_damage_sample_equals_restatement(engine):
    """67 files of the damage sweep, one call per base (each base has one size): the status is the restatement's, the bytes of an
    accepted file are the restatement's (which the CPU sweep holds to Pillow's), and a refused slot keeps its fill."""
    sample = ic.sweep_sample(200, seed=9700)[::3]
    sizes = {name: ir.reference(data)[2][:2] for name, data in ic.damage_bases()}
    n_ok = 0
    for bname, (w, h) in sizes.items():
        group = [(name, data) for b, name, data in sample if b == bname]
        assert group
        out = torch.full((len(group), h, w, 3), 77, dtype=torch.uint8, device="cuda")
        out, status = engine.jp2_decode_irreversible([d for _, d in group], h, w, out=out)
        got = out.cpu().numpy()
        for k, (name, data) in enumerate(group):
            st, _, info, rgb = ir.reference(data)
            if st == 0 and info[:2] != [w, h]:
                st = -4
            assert status[k] == st, (bname, name, status[k], st)
            if st == 0:
                assert np.array_equal(got[k], rgb), (bname, name, _differs(got[k], rgb))
                n_ok += 1
            else:
                assert (got[k] == 77).all(), (bname, name)
    assert n_ok >= 15
