"""GPU: the progressive decode (lumina_ocr_jpeg_decode_progressive) on damaged copies of the 37 x 53 4:2:0 file: single-bit flips
and truncations, a few hundred cases from a fixed seed, each run through the restatement (tests/progressive_reference.py) on the CPU
first.  The contract is the baseline decoder's: status 0 => the pixels are Pillow's decode of that damaged file; anything else is left
to Pillow and the page is not written.  The sweep holds the undamaged file and flips in the JFIF density bytes, which must come back
with status 0, and prints how many cases were accepted, so that it cannot pass by refusing everything.  Where the restatement refuses a
file the device must refuse it with the same code (-1 corrupt, -2 outside the subset, -4 another size)."""
import numpy as np
import pytest
import torch

import progressive_cases as pc
import progressive_reference as pr
from jpeg_cases import pil_decode

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
W, H = 37, 53


def _pil(data):
    try:
        return pil_decode(data)
    except Exception:               # Pillow cannot decode it at all
        return None


def _restated_status(data):
    """The status the restatement gives, in the order the device decides: markers, then the size of the batch, then the entropy data."""
    try:
        fr = pr.parse(data)
    except pr.Refused as e:
        return e.code
    if (fr.width, fr.height) != (W, H):
        return -4
    return pr.status(data)


def test_status_zero_means_pillows_pixels(engine):
    corpus = pc.damage_corpus()
    ref_status = [_restated_status(d) for _, d in corpus]          # the restatement first: the definition the kernels restate
    accepted, wrong, written, disagree = 0, [], [], []
    for i in range(0, len(corpus), 64):
        items = corpus[i:i + 64]
        out = torch.full((len(items), H, W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        out, status = engine.jpeg_decode_progressive([d for _, d in items], H, W, out=out)
        torch.cuda.synchronize()
        pages = out.cpu().numpy()
        for k, (name, data) in enumerate(items):
            if status[k] == 0:
                accepted += 1
                want = _pil(data)
                if want is None or want.shape != pages[k].shape or not np.array_equal(pages[k], want):
                    wrong.append(name)
                if ref_status[i + k] not in (0, 1):                # (1: the flip made it a sequential file, the baseline decoder's)
                    disagree.append((name, status[k], ref_status[i + k]))
            else:
                if not (pages[k] == SENTINEL).all():
                    written.append((name, status[k]))
                if ref_status[i + k] == 0 and status[k] != -1:     # the device may refuse more only by its IDCT range check (-1)
                    disagree.append((name, status[k], ref_status[i + k]))
                if ref_status[i + k] not in (0, 1) and status[k] != ref_status[i + k]:     # the same refusal: -1, -2 or -4
                    disagree.append((name, status[k], ref_status[i + k]))
            if name == "clean" or name.startswith("density_"):
                assert status[k] == 0, (name, status[k])
    print("progressive damage sweep: %d of %d cases accepted (restatement: %d)" % (accepted, len(corpus), sum(s == 0 for s in ref_status)))
    assert not wrong, "%d accepted, but not Pillow's pixels: %s" % (len(wrong), wrong[:20])
    assert not written, "refused pages were written: %s" % written[:20]
    assert not disagree, "device and restatement disagree (name, device, restatement): %s" % disagree[:20]
    assert 5 <= accepted < len(corpus)


def test_clean_decode_after_the_sweep_is_still_exact(engine):
    data = pc.pillow_file(pc.BASE_420)
    out, status = engine.jpeg_decode_progressive([data, data], H, W)
    torch.cuda.synchronize()
    assert status == [0, 0] and np.array_equal(out[0].cpu().numpy(), pil_decode(data)) and torch.equal(out[0], out[1])
