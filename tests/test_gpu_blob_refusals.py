"""GPU: what the engine does with a weight blob it refuses (include/lumina_ocr.h: "a refused blob leaves the previously loaded model of
that kind intact and runnable, bit for bit"), for the detector, the CRNN, the orientation classifier and SVTR-Tiny.

Model A (seed 1) is loaded and its forward recorded; then one mutant of every refusal class, built from model B (seed 2) with B's
data throughout (tests/blob_cases.py gpu_mutants), is offered.  Each must raise EngineError naming the tensor, and afterwards the
forward must give A's bits and num_classes must be A's: a loader that had uploaded anything of B before it noticed would change them
(B's outputs differ from A's: asserted).  On a fresh engine the same blobs leave the model "not loaded".  Tensor order, unknown extra
tensors and the blob's address do not matter.  Small inputs: 2 crops, one 96 x 128 page."""
import functools

import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.engine import Engine, EngineError

import blob_cases as bc

pytestmark = pytest.mark.gpu

KINDS = ["det", "rec", "cls", "svtr"]
CLASSES = {1: 97, 2: 113}   # per seed: a load of B that got as far as the CTC head would change num_classes


@functools.lru_cache(maxsize=None)
def weights(kind, seed):
    if kind == "det":
        return arch.make_det_weights(seed, text_path=False)   # dense: every output depends on every seeded weight
    if kind == "rec":
        return arch.make_rec_weights(seed, num_classes=CLASSES[seed])
    if kind == "cls":
        return arch.make_cls_weights(seed)
    return arch.make_svtr_weights(seed, num_classes=CLASSES[seed], variant="tiny", dtype="bf16")


@functools.lru_cache(maxsize=None)
def inputs():
    rng = np.random.default_rng(97)
    crops = np.stack([synth.synth_crop(rng)[0] for _ in range(2)])
    cls_crops = np.zeros((2, arch.CLS_H, arch.CLS_W, 3), np.uint8)
    cls_crops[:, 8:40] = crops[:, :, :arch.CLS_W]
    return dict(page=synth.synth_page(96, 128, 5, n_lines=3)[0][None], crops=crops, widths=np.array([320, 150], np.int32), cls_crops=cls_crops,
                cls_widths=np.array([192, 77], np.int32))


def load(eng, kind, blob, **kw):
    getattr(eng, "load_" + kind)(blob, **kw)


def forward(eng, kind):
    """the model's outputs as integer arrays (a float comparison would call -0 and +0, or two NaNs' absence, equal)"""
    x = inputs()
    if kind == "det":
        out = [eng.det_forward(torch.from_numpy(x["page"]).cuda()).view(torch.int16)]
    elif kind == "cls":
        label, score, flip = eng.cls_forward(torch.from_numpy(x["cls_crops"]).cuda(), torch.from_numpy(x["cls_widths"]).cuda())
        out = [label, score.view(torch.int32), flip]
    else:
        fwd = eng.rec_forward if kind == "rec" else eng.svtr_forward
        idx, prob = fwd(torch.from_numpy(x["crops"]).cuda(), torch.from_numpy(x["widths"]).cuda())
        out = [idx, prob.view(torch.int32)]
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q) for p, q in zip(a, b))


def classes(eng, kind):
    return {"rec": eng.num_classes, "svtr": eng.svtr_num_classes}.get(kind)


def restore(request, eng, kind):
    """the session engine goes back to the suite's own weights (the classifier and SVTR have none: every test loads its own)"""
    if kind == "det":
        eng.load_det(request.getfixturevalue("det_weights"))
    elif kind == "rec":
        eng.load_rec(request.getfixturevalue("rec_weights"))


@pytest.mark.parametrize("kind", KINDS)
def test_refused_blob_leaves_previous_model_intact(request, engine, kind):
    a, b = arch.write_blob(weights(kind, 1)), arch.write_blob(weights(kind, 2))
    try:
        load(engine, kind, b)
        out_b = forward(engine, kind)
        load(engine, kind, a)
        ref, ncls = forward(engine, kind), classes(engine, kind)
        assert not same(ref, out_b), "models A and B must differ in their outputs, or this test shows nothing"
        assert ncls in (None, CLASSES[1])
        mutants = bc.gpu_mutants(kind, weights(kind, 2))
        want = {"missing", "dtype", "rank", "conv3x3-dims2", "short-bias", "duplicate", "truncated"}
        want |= {"torch-depthwise", "torch-squeeze-excite"} if kind in ("rec", "cls") else set()
        want |= {"short-bw-w_ih", "short-w_hh", "short-fw-w_hh"} if kind == "rec" else set()
        want |= {"bf16-ctc-bias"} if kind in ("rec", "svtr") else set()
        assert {m[0] for m in mutants} == want
        for label, names, blob in mutants:
            with pytest.raises(EngineError) as e:
                load(engine, kind, blob)
            assert any("(tensor %s)" % n in str(e.value) for n in names), (label, str(e.value))
            assert getattr(engine, kind + "_loaded"), label
            assert classes(engine, kind) == ncls, label
            assert same(forward(engine, kind), ref), label
    finally:
        restore(request, engine, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_refused_blob_on_a_fresh_engine_loads_nothing(kind):
    eng = Engine(0)
    try:
        for label, names, blob in bc.gpu_mutants(kind, weights(kind, 2)):
            with pytest.raises(EngineError) as e:
                load(eng, kind, blob)
            assert any("(tensor %s)" % n in str(e.value) for n in names), (label, str(e.value))
            assert not getattr(eng, kind + "_loaded") and not classes(eng, kind), label
            with pytest.raises(EngineError, match="not loaded"):
                forward(eng, kind)
    finally:
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_order_extras_and_address_do_not_matter(request, engine, kind):
    entries = bc.entries_of(weights(kind, 1))
    try:
        load(engine, kind, bc.full_blob(entries))
        ref = forward(engine, kind)
        load(engine, kind, arch.write_blob(weights(kind, 2)))   # (so that each of the loads below has something to change)
        load(engine, kind, bc.full_blob(entries[::-1]))
        assert same(forward(engine, kind), ref), "reverse order"
        load(engine, kind, arch.write_blob(weights(kind, 2)))
        extra = ("unknown.w", 1, (3, 5), np.arange(15, dtype=np.uint16).tobytes())
        load(engine, kind, bc.full_blob(entries[:7] + [extra] + entries[7:]))
        assert same(forward(engine, kind), ref), "extra tensor"
        # a blob at an odd address is loaded correctly (the choice stated in lumina_ocr.h)
        load(engine, kind, arch.write_blob(weights(kind, 2)))
        load(engine, kind, bc.full_blob(entries), _offset=1)
        assert same(forward(engine, kind), ref), "odd address"
        # trailing bytes are refused (the other choice stated there), and the model stays
        with pytest.raises(EngineError, match="trailing bytes"):
            load(engine, kind, bc.full_blob(entries) + b"\x00" * 16)
        assert same(forward(engine, kind), ref), "trailing bytes"
    finally:
        restore(request, engine, kind)
