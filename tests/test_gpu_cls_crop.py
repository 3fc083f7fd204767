"""GPU: the orientation classifier's crops (lumina_ocr_cls_crop) and the oriented recognition crop (lumina_ocr_rec_crop_oriented)
against the CPU restatement of tests/cls_reference.py, byte for byte."""
import numpy as np
import pytest
import torch

from lumina_ocr import synth

import cls_reference as cr

pytestmark = pytest.mark.gpu


def _pages_and_quads():
    """Two synthetic pages; per page the rendered lines' boxes plus hand-made quads: vertical, skewed, wider than both caps,
    degenerate, corners off the page."""
    pages = np.stack([synth.synth_page(240, 520, s, n_lines=4)[0] for s in (11, 12)])
    hand = [[10, 0, 42, 0, 42, 64, 10, 64], [17, 20, 500, 31, 498, 60, 15, 49], [300, 10, 330, 12, 328, 110, 298, 108],
            [40, 40, 90, 40, 90, 60, 40, 60], [5, 5, 5, 5, 5, 5, 5, 5], [-8, 200, 60, 200, 60, 250, -8, 250], [0, 0, 7, 0, 7, 10, 0, 10]]
    quads, page_idx = [], []
    for p in range(2):
        for g in synth.synth_page(240, 520, 11 + p, n_lines=4)[1]:
            x0, y0, x1, y1 = g["box"]
            quads.append([x0 - 2, y0 - 2, x1 + 2, y0 - 2, x1 + 2, y1 + 2, x0 - 2, y1 + 2])
            page_idx.append(p)
        quads += hand
        page_idx += [p] * len(hand)
    return pages, np.array(quads, np.int32), np.array(page_idx, np.int32)


def test_cls_crop_is_bit_exact(engine):
    pages, quads, page_idx = _pages_and_quads()
    crops, widths = engine.cls_crop(torch.from_numpy(pages).cuda(), torch.from_numpy(quads).cuda(), torch.from_numpy(page_idx).cuda())
    crops, widths = crops.cpu().numpy(), widths.cpu().numpy()
    assert crops.shape == (len(quads), 48, 192, 3)
    caps = 0
    for i, (q, p) in enumerate(zip(quads, page_idx)):
        ref, wc = cr.crop(pages[p], q)
        assert widths[i] == wc and np.array_equal(crops[i], ref), (i, q.tolist())
        caps += wc == 192
    assert caps >= 4 and 0 in widths.tolist()          # lines at the 192 cap and the degenerate quad are in the set


def test_oriented_rec_crop(engine):
    """Flag 0: byte-identical to rec_crop; flag 1: exactly the 180-degree turn of that crop within its valid width."""
    pages, quads, page_idx = _pages_and_quads()
    pg, qd, pi = torch.from_numpy(pages).cuda(), torch.from_numpy(quads).cuda(), torch.from_numpy(page_idx).cuda()
    plain, w0 = engine.rec_crop(pg, qd, pi)
    zeros, wz = engine.rec_crop(pg, qd, pi, flip=torch.zeros(len(quads), dtype=torch.int32, device="cuda"))
    flip = (np.arange(len(quads)) % 2).astype(np.int32)
    turned, w1 = engine.rec_crop(pg, qd, pi, flip=torch.from_numpy(flip).cuda())
    plain, zeros, turned = plain.cpu().numpy(), zeros.cpu().numpy(), turned.cpu().numpy()
    w0, wz, w1 = w0.cpu().numpy(), wz.cpu().numpy(), w1.cpu().numpy()
    assert np.array_equal(zeros, plain) and np.array_equal(wz, w0) and np.array_equal(w1, w0)
    for i, f in enumerate(flip):
        want = cr.turn(plain[i], int(w0[i])) if f else plain[i]
        assert np.array_equal(turned[i], want), i
        ref, wc = cr.crop(pages[page_idx[i]], quads[i], 32, 320, flip=bool(f))
        assert wc == w0[i] and np.array_equal(turned[i], ref), i
