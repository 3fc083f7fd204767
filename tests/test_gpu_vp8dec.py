"""GPU: the device lossy-WebP decoder (csrc/vp8dec.hip, through lumina_ocr_webp_decode_lossy) vs Pillow's
Image.open(f).convert('RGB'), byte for byte: every intact file of tests/vp8_cases.py, the refused kinds, a mixed batch of lossless,
lossy, corrupt and wrong-size files, a seeded sample of 200 damaged files held to the plain-Python restatement (tests/vp8_reference.py) status for
status and byte for byte, and 70 small files in several sub-batches."""
import numpy as np
import pytest
import torch

import vp8_cases as vc
import webp_cases as wc
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu


def _by_size(cases):
    groups = {}
    for name, data in cases:
        rc, info = Engine.webp_probe_lossy(data)
        assert rc == 0 and info["lossy"] == 1 and info["partitions"] in (1, 2, 4, 8), (name, rc, info)
        groups.setdefault((info["height"], info["width"]), []).append((name, data))
    return groups


def _assert_equal(name, got, want):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ, first at %s: got %s want %s" % (name, len(d), got.size, d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])]))


def test_every_intact_case_equals_pillow(engine):
    """One call per size (the two 16383-pixel strips and the wide case run once each): every file is accepted and equals Pillow's decode."""
    cases = vc.intact_cases()
    n_ok = 0
    for (h, w), group in _by_size(cases).items():
        out, status = engine.webp_decode_lossy([d for _, d in group], h, w)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for k, (name, data) in enumerate(group):
            assert status[k] == 0, (name, status[k])
            _assert_equal(name, got[k], vc.pillow_rgb(data))
            n_ok += 1
    assert n_ok == len(cases)


def test_refused_cases_keep_their_pages(engine):
    cases = vc.refused_cases()
    out = torch.full((len(cases), 30, 40, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.webp_decode_lossy([d for _, d, _ in cases], 30, 40, out=out)
    torch.cuda.synchronize()
    assert status == [rc for _, _, rc in cases], status
    assert [Engine.webp_probe_lossy(d)[0] for _, d, _ in cases] == status
    assert bool((out == 77).all())


def test_just_beyond_the_coefficient_bound(engine):
    """Pillow reads these two files; a transform of theirs leaves 16 bits, so the device refuses them and leaves the pages alone."""
    cases = vc.bound_cases()
    out = torch.full((len(cases), 16, 16, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.webp_decode_lossy([d for _, d, _ in cases], 16, 16, out=out)
    torch.cuda.synchronize()
    assert status == [-1, -1] and bool((out == 77).all())
    assert all(vc.pillow_rgb(d) is not None and Engine.webp_probe_lossy(d)[0] == 0 for _, d, _ in cases)


def test_the_lossless_entries_still_refuse_lossy(engine):
    data = dict(vc.intact_cases())["pillow-48x48-RGB-m4-q80"]
    rc, info = Engine.webp_probe(data)
    assert rc == -2 and "lossy" in info["reason"]
    out = torch.full((1, 48, 48, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.webp_decode([data], 48, 48, out=out)
    torch.cuda.synchronize()
    assert status == [-2] and bool((out == 77).all())


def test_mixed_batch_of_both_kinds(engine):
    """One call: lossless and lossy files of 9 x 70 between a corrupt lossy one (-1), a corrupt lossless one (-1), a refused one (-2)
    and files of another size (-4).  The lossless pages equal lumina_ocr_webp_decode's bytes; refused pages keep the sentinel."""
    from PIL import Image
    ll = [dict(wc.writer_cases())[name] for name in ("predictor-bits9", "cross-bits2", "order-gpc")]   # 70 x 9
    pics = [vc._picture(70, 9, 50 + k, "mixed") for k in range(3)]
    lossy = [vc._save(Image.fromarray(p), quality=q) for p, q in zip(pics, (30, 75, 100))]
    (_, payload), = vc._chunks(lossy[0])
    bad_lossy = vc.riff([(b"VP8 ", payload[:-20])])   # the token partition cut short inside a regular container
    bad_ll = wc.flip(ll[0], 8 * (len(ll[0]) - 6) + 3)
    other = dict(vc.intact_cases())["pillow-48x48-RGB-m0-q50"]
    refused = vc.refused_cases()[0][1]
    files = [ll[0], lossy[0], bad_lossy, ll[1], refused, lossy[1], other, bad_ll, lossy[2], b"RIFF", ll[2]]
    want = [0, 0, -1, 0, -2, 0, -4, -1, 0, -1, 0]
    out = torch.full((len(files), 9, 70, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.webp_decode_lossy(files, 9, 70, out=out)
    torch.cuda.synchronize()
    assert status == want, status
    ref, ref_status = engine.webp_decode(files, 9, 70, out=torch.full_like(out, 77))
    torch.cuda.synchronize()
    for k, st in enumerate(want):
        if st == 0:
            _assert_equal(k, out[k].cpu().numpy(), vc.pillow_rgb(files[k]))
            if ref_status[k] == 0:
                assert torch.equal(out[k], ref[k]), k
        else:
            assert bool((out[k] == 77).all()), k
    assert [k for k, st in enumerate(ref_status) if st == 0] == [0, 3, 10]


def test_damaged_sample_equals_the_restatement(engine):
    """200 damaged files (seeded; flips and truncations of the two sweep files): the device's status is the restatement's file for file,
    and every accepted page equals the restatement's pixels, which tests/test_vp8_reference.py holds to Pillow's."""
    import vp8_reference as R
    sample = vc.sweep_sample(200, seed=7)
    ref = {name: R.decode(data) for name, _, data in sample}
    assert sum(1 for rc, _, _ in ref.values() if rc == 0) >= 120 and sum(1 for rc, _, _ in ref.values() if rc != 0) >= 15
    for base, data0 in vc.sweep_bases():
        part = [f for f in sample if f[0].startswith(base + "-")]
        h, w = vc.pillow_rgb(data0).shape[:2]
        out = torch.full((len(part), h, w, 3), 77, dtype=torch.uint8, device="cuda")
        out, status = engine.webp_decode_lossy([d for _, _, d in part], h, w, out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for k, (name, kind, data) in enumerate(part):
            rc, reason, px = ref[name]
            prc, info, _ = R.probe(data)
            if prc == 0 and (info["height"], info["width"]) != (h, w):
                rc = -4   # (a flip in the header's size bits: the batch contract refuses the file before it is decoded)
            assert status[k] == rc, (name, status[k], rc, reason)
            if rc == 0:
                _assert_equal(name, got[k], px)
            else:
                assert bool((got[k] == 77).all()), name


def test_seventy_files_in_sub_batches(engine):
    """70 files of 130 x 70 with webp_sub_batch_mb = 1: a file takes 54 KB of workspace, so the call runs in four sub-batches."""
    from PIL import Image
    files = [vc._save(Image.fromarray(vc._picture(130, 70, 900 + k, "mixed" if k % 3 else "noise")), quality=(10 + k) % 101, method=k % 7) for k in range(70)]
    engine.set_option("webp_sub_batch_mb", 1)
    try:
        out, status = engine.webp_decode_lossy(files, 70, 130)
        torch.cuda.synchronize()
    finally:
        engine.set_option("webp_sub_batch_mb", 2048)
    got = out.cpu().numpy()
    assert status == [0] * 70
    for k, data in enumerate(files):
        _assert_equal(k, got[k], vc.pillow_rgb(data))
