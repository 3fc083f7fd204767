"""GPU: the device JPEG 2000 decoder (csrc/jp2dec.hip, through lumina_ocr_jp2_decode) vs Pillow's Image.open(f).convert('RGB'), byte
for byte: every intact case of tests/jp2_cases.py, a batch of 64 distinct files, a call that mixes accepted and refused files, a
700 x 1000 text page lossless and layered, and a seeded sample of the damage sweep against the restatement.  Every damaged file here
has gone through the sanitized host parser and the restatement (tests/test_jp2_parser_sanitized.py); none is built to provoke a fault."""
import numpy as np
import pytest
import torch

import jp2_cases as jc
from lumina_ocr import synth
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu


def _by_size(files):
    groups = {}
    for name, data in files:
        _, info = Engine.jp2_probe(data)
        groups.setdefault((info["height"], info["width"]), []).append((name, data))
    return groups


def _differs(got, want):
    d = np.argwhere(got != want)
    return "%d of %d values differ, first at %s: got %s want %s" % (len(d), got.size, d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])])


def test_every_intact_case_equals_pillow(engine):
    cases = jc.intact()
    for (h, w), group in _by_size(cases).items():
        out, status = engine.jp2_decode([d for _, d in group], h, w)
        assert status == [0] * len(group), (h, w, status)
        for k, (name, data) in enumerate(group):
            got, want = out[k].cpu().numpy(), jc.expected(data)
            assert np.array_equal(got, want), (name, _differs(got, want))


def test_batch_of_64(engine):
    """64 distinct 96 x 128 files in one call: L and RGB, lossless and layered, several block sizes and progression orders."""
    h, w = 96, 128
    files = []
    for i in range(64):
        mode = "RGB" if i % 2 else "L"
        opts = dict(irreversible=False)
        if i % 4 >= 2:
            opts["quality_layers"] = [30, 8] if i % 8 >= 4 else [12]
        opts["codeblock_size"] = [(64, 64), (32, 32), (16, 64)][i % 3]
        opts["progression"] = ["LRCP", "RLCP", "RPCL", "PCRL", "CPRL"][i % 5]
        files.append(jc.write(jc.content("page" if i % 3 else "noise", h, w, mode, seed=1000 + i), **opts))
    assert len(set(files)) == 64
    out, status = engine.jp2_decode(files, h, w)
    assert status == [0] * 64, status
    got = out.cpu().numpy()
    for k, data in enumerate(files):
        want = jc.expected(data)
        assert np.array_equal(got[k], want), (k, _differs(got[k], want))


def test_mixed_call_leaves_refused_slots_untouched(engine):
    h, w = 100, 130
    good_rgb = jc.write(jc.content("page", h, w, "RGB", 7), irreversible=False)
    good_l = jc.write(jc.content("noise", h, w, "L", 8), irreversible=False, quality_layers=[8])
    lossy97 = jc.write(jc.content("page", h, w, "RGB", 9), irreversible=True)
    cut = good_rgb[:len(good_rgb) // 2]
    other = jc.write(jc.content("page", h + 1, w, "RGB", 10), irreversible=False)
    files = [good_rgb, lossy97, cut, good_l, other, b"not a file"]
    out = torch.full((len(files), h, w, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.jp2_decode(files, h, w, out=out)
    assert status == [0, -2, -1, 0, -4, -1], status
    got = out.cpu().numpy()
    for k in (0, 3):
        assert np.array_equal(got[k], jc.expected(files[k])), k
    for k in (1, 2, 4, 5):
        assert (got[k] == 77).all(), k


@pytest.mark.parametrize("layers", [None, [20]], ids=["lossless", "layers20"])
def test_text_page(engine, layers):
    page = synth.synth_page(700, 1000, 11, n_lines=14)[0]
    opts = dict(irreversible=False)
    if layers:
        opts["quality_layers"] = layers
    data = jc.write(page, **opts)
    out, status = engine.jp2_decode([data], 700, 1000)
    assert status == [0]
    got, want = out[0].cpu().numpy(), jc.expected(data)
    assert np.array_equal(got, want), _differs(got, want)
    if not layers:
        assert np.array_equal(got, page)


def test_damage_sample_equals_restatement(engine):
    """200 files of the damage sweep, one call per base (each base has one size): the status is the restatement's, the bytes of an
    accepted file are the restatement's (which the CPU sweep holds to Pillow's), and a refused slot keeps its fill."""
    sample = jc.sweep_sample(200, seed=2000)
    sizes = {name: jc.reference(data)[2][:2] for name, data in jc.damage_bases()}
    n_ok = 0
    for bname, (w, h) in sizes.items():
        group = [(name, data) for b, name, data in sample if b == bname]
        assert group
        out = torch.full((len(group), h, w, 3), 77, dtype=torch.uint8, device="cuda")
        out, status = engine.jp2_decode([d for _, d in group], h, w, out=out)
        got = out.cpu().numpy()
        for k, (name, data) in enumerate(group):
            st, _, info, rgb = jc.reference(data)
            if st == 0 and info[:2] != [w, h]:
                st = -4
            assert status[k] == st, (bname, name, status[k], st)
            if st == 0:
                assert np.array_equal(got[k], rgb), (bname, name, _differs(got[k], rgb))
                n_ok += 1
            else:
                assert (got[k] == 77).all(), (bname, name)
    assert n_ok >= 50


def test_sub_batches(engine):
    """jp2_sub_batch_mb = 1: 300 x 420 pages take 1 MB (grey) or 3 MB (RGB) of coefficient planes, so eleven pages mixed with refused
    ones split into many sub-batches, each opened by the page that did not fit the one before; the result is the single batch's."""
    h, w = 300, 420
    files = []
    for i in range(11):
        page = synth.synth_page(h, w, 40 + i, n_lines=5)[0]
        files.append(jc.write(page if i % 3 else np.ascontiguousarray(page[:, :, 0]), irreversible=False, **({"quality_layers": [10]} if i % 2 else {})))
    files.insert(4, b"not a file")
    files.insert(8, jc.write(jc.content("page", h, w, "RGB", 3), irreversible=True))
    want_status = [0, 0, 0, 0, -1, 0, 0, 0, -2, 0, 0, 0, 0]
    engine.set_option("jp2_sub_batch_mb", 1)
    try:
        out = torch.full((len(files), h, w, 3), 77, dtype=torch.uint8, device="cuda")
        out, status = engine.jp2_decode(files, h, w, out=out)
    finally:
        engine.set_option("jp2_sub_batch_mb", 4096)
    assert status == want_status, status
    got = out.cpu().numpy()
    for k, data in enumerate(files):
        if want_status[k] == 0:
            assert np.array_equal(got[k], jc.expected(data)), k
        else:
            assert (got[k] == 77).all(), k
