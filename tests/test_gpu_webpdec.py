"""GPU: the device lossless-WebP decoder (csrc/webpdec.hip, through lumina_ocr_webp_decode) vs Pillow's Image.open(f).convert('RGB'),
byte for byte: every intact file of tests/webp_cases.py (Pillow's encoder at every method / quality / mode and the test-side writer's
streams), a mixed batch with good, corrupt, refused and wrong-size files, and a seeded sample of 200 damaged files held to the plain-Python
restatement (tests/webp_reference.py) status for status and byte for byte."""
import numpy as np
import pytest
import torch

import webp_cases as wc
import webp_reference as wr
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu


def _by_size(cases):
    groups = {}
    for name, data in cases:
        _, info = Engine.webp_probe(data)
        groups.setdefault((info["height"], info["width"]), []).append((name, data))
    return groups


def _assert_equal(name, got, want):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ, first at %s: got %s want %s" % (name, len(d), got.size, d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])]))


def test_every_intact_case_equals_pillow(engine):
    """One call per size: every file is accepted and equals Pillow's decode byte for byte."""
    cases = wc.intact_cases()
    n_ok = 0
    for (h, w), group in _by_size(cases).items():
        out, status = engine.webp_decode([d for _, d in group], h, w)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for k, (name, data) in enumerate(group):
            assert status[k] == 0, (name, status[k])
            _assert_equal(name, got[k], wc.pillow_rgb(data))
            n_ok += 1
    assert n_ok == len(cases)


def test_mixed_batch_leaves_neighbours_alone(engine):
    """One call: good files of several kinds between a corrupt one (-1), the three refused kinds (-2) and one of another size (-4).
    Refused pages keep the sentinel the output was filled with."""
    by = _by_size(wc.intact_cases())
    good = by[(9, 70)][:6]
    refused = wc.refused_cases()
    other = by[(5, 13)][0][1]
    bad = wc.flip(good[0][1], 8 * (len(good[0][1]) - 6) + 3)   # inside the ARGB stream's last bytes
    assert wr.decode(bad)[0] == -1
    files = [good[0][1], bad, good[1][1], refused[0][1], good[2][1], refused[1][1], good[3][1], refused[2][1], other, good[4][1], b"RIFF", good[5][1]]
    want = [0, -1, 0, -2, 0, -2, 0, -2, -4, 0, -1, 0]
    out = torch.full((len(files), 9, 70, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.webp_decode(files, 9, 70, out=out)
    torch.cuda.synchronize()
    assert status == want, status
    for k, st in enumerate(want):
        if st == 0:
            _assert_equal(k, out[k].cpu().numpy(), wc.pillow_rgb(files[k]))
        else:
            assert bool((out[k] == 77).all()), k


def test_damaged_sample_equals_the_restatement(engine):
    """200 damaged files (seeded; flips and truncations of the two sweep files): the device's status is the restatement's, and every
    accepted page equals the restatement's pixels, which tests/test_webp_reference.py holds to Pillow's."""
    sample = wc.sweep_sample(200, seed=7)
    ref = [wr.decode(data) for _, _, data in sample]
    assert sum(1 for rc, _ in ref if rc == 0) >= 50
    groups = {}
    for k, (name, kind, data) in enumerate(sample):
        groups.setdefault(name.split("-flip")[0].split("-cut")[0], []).append(k)
    for base, ks in groups.items():
        h, w = wr.decode(dict(wc.sweep_bases())[base])[1].shape[:2]
        out = torch.full((len(ks), h, w, 3), 77, dtype=torch.uint8, device="cuda")
        out, status = engine.webp_decode([sample[k][2] for k in ks], h, w, out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for j, k in enumerate(ks):
            rc, px = ref[k]
            prc, info, _ = wr.probe(sample[k][2])
            if prc == 0 and (info["height"], info["width"]) != (h, w):
                rc = -4   # (a flip in the header's size bits: the batch contract refuses the file before it is decoded)
            assert status[j] == rc, (sample[k][0], status[j], rc)
            if rc == 0:
                _assert_equal(sample[k][0], got[j], px)
            else:
                assert bool((got[j] == 77).all()), sample[k][0]
