"""GPU: which kernel the conv dispatch (engine.hip eng_run_conv / run_linear) launches for which layer, with what accounting, and every
output byte, against a recording taken before the dispatch was refactored (tests/golden/dispatch_recording.json).  A row is one timed
launch of option time_convs: layer, kernel instantiation, GFLOP and MB as lumina_ocr_conv_timing_detail prints them (the milliseconds are
dropped); sha256 is over the raw bytes of what the scenario computed."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "dispatch_recording.json"

# every option a scenario touches, at its default (engine.h)
DEFAULTS = dict(det_sub_batch=16, conv_big_min=1024, conv_ring=1, keep_taps=0, tail_group=16, fuse_head=1, fuse_short=1, fuse_mb=1,
                conv2d_variant=0, ring_orient=-1)


def _scenario(engine, options, run):
    """run() -> tensors, under `options` with the launches timed -> {"launches": rows, "sha256": of the tensors' bytes}."""
    engine.conv_timing_detail()   # (drops whatever an earlier test left in the list)
    try:
        for key, value in options.items():
            engine.set_option(key, value)
        engine.set_option("time_convs", 1)
        outs = run()
        torch.cuda.synchronize()
        rows = [[layer, kernel, "%.4f" % gflop, "%.4f" % mb] for layer, kernel, _, gflop, mb in engine.conv_timing_detail()]
    finally:
        engine.set_option("time_convs", 0)
        for key in options:
            engine.set_option(key, DEFAULTS[key])
    sha = hashlib.sha256()
    for t in outs:
        sha.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return {"launches": rows, "sha256": sha.hexdigest()}


def _cls_crops(crops):
    """48 x 192 classifier crops out of the recogniser's 32 x 320 ones (rows 8 .. 39, the first 192 columns)."""
    out = np.zeros((len(crops), arch.CLS_H, arch.CLS_W, 3), np.uint8)
    out[:, 8:40] = crops[:, :, :arch.CLS_W]
    return out


def record(engine, det_weights, rec_weights):
    """Every scenario, in a fixed order -> {scenario: {"launches", "sha256"}}."""
    rec = {}
    pages = torch.from_numpy(np.stack([synth.synth_page(90, 150, 31 + i, n_lines=3)[0] for i in range(3)])).cuda()   # padded 96 x 160
    engine.load_det(det_weights)
    det = lambda: [engine.det_forward(pages)]
    rec["det.default"] = _scenario(engine, {}, det)
    rec["det.big"] = _scenario(engine, dict(conv_big_min=1), det)
    rec["det.big.no_ring"] = _scenario(engine, dict(conv_big_min=1, conv_ring=0), det)
    rec["det.keep_taps"] = _scenario(engine, dict(keep_taps=1), det)
    rec["det.big.tail_group2.no_fuse_head"] = _scenario(engine, dict(conv_big_min=1, tail_group=2, fuse_head=0), det)
    rec["det.no_fuse_short"] = _scenario(engine, dict(fuse_short=0), det)
    rec["det.sub_batch2"] = _scenario(engine, dict(det_sub_batch=2), det)

    rng = np.random.default_rng(99)
    crops_np = np.stack([synth.synth_crop(rng)[0] for _ in range(5)])
    crops = torch.from_numpy(crops_np).cuda()
    widths = torch.tensor([320, 211, 77, 150, 33], dtype=torch.int32).cuda()
    cls_crops = torch.from_numpy(_cls_crops(crops_np)).cuda()
    cls_widths = torch.tensor([192, 150, 77, 31, 120], dtype=torch.int32).cuda()
    engine.load_rec(rec_weights)
    engine.load_cls(arch.make_cls_weights(2718))
    for fuse_mb in (1, 0):
        rec["rec.fuse_mb%d" % fuse_mb] = _scenario(engine, dict(fuse_mb=fuse_mb), lambda: list(engine.rec_forward(crops, widths)))
        rec["cls.fuse_mb%d" % fuse_mb] = _scenario(engine, dict(fuse_mb=fuse_mb), lambda: list(engine.cls_forward(cls_crops, cls_widths)))

    engine.load_svtr(arch.make_svtr_weights(variant="tiny", dtype="bf16", num_classes=500))
    rec["svtr.tiny.bf16"] = _scenario(engine, {}, lambda: list(engine.svtr_forward(crops[:3], widths[:3])))

    # the conv2d hook; after every call a default-option detector forward, which must find the handle as it was
    n, h, w, cin, cout = 1, 19, 37, 128, 128
    rng = np.random.default_rng(5)
    x = torch.from_numpy(arch.bf16_round(rng.standard_normal((n, h, w, cin), dtype=np.float32))).to(torch.bfloat16).cuda()
    wt = arch.bf16_round(rng.standard_normal((cout, 3, 3, cin), dtype=np.float32) * np.float32(np.sqrt(2.0 / (9 * cin))))
    bias = rng.standard_normal(cout, dtype=np.float32) * np.float32(0.1)
    res = torch.from_numpy(arch.bf16_round(rng.standard_normal((n, h, w, cout), dtype=np.float32))).to(torch.bfloat16).cuda()
    for variant, orient in ((0, -1), (1, -1), (2, 0), (2, 1)):
        name = "conv2d.variant%d" % variant + (".orient%d" % orient if variant == 2 else "")
        rec[name] = _scenario(engine, dict(conv2d_variant=variant, ring_orient=orient), lambda: [engine.conv2d(x, wt, bias, 3, 1, 1, res)])
        rec[name + ".then_det"] = _scenario(engine, {}, det)
    return rec


def test_dispatch_matches_the_recording(engine, dense_det_weights, rec_weights):
    want = json.loads(GOLDEN.read_text())
    got = record(engine, dense_det_weights, rec_weights)
    assert list(got) == list(want)
    for name in want:
        assert got[name]["launches"] == want[name]["launches"], name
        assert got[name]["sha256"] == want[name]["sha256"], name
    for name in got:
        if name.endswith(".then_det"):   # the hook left nothing behind in the handle
            assert got[name] == got["det.default"], name


def test_malformed_stem_tensor_fails_with_a_message(engine, det_weights, rec_weights):
    """A stem weight of another rank and a stem bias of another length are refused with the reason and the tensor's name (the recogniser
    and the detector used to read past them), by the check every loader runs before it touches the engine (csrc/blob_check.h): the
    models loaded before stay loaded."""
    from lumina_ocr.engine import EngineError
    bad_rec = dict(rec_weights)
    bad_rec["rec.conv1.w"] = rec_weights["rec.conv1.w"].reshape(rec_weights["rec.conv1.w"].shape[0], 27)
    engine.load_rec(rec_weights)
    with pytest.raises(EngineError, match=r"load_rec_weights: wrong rank \(tensor rec\.conv1\.w\)"):
        engine.load_rec(bad_rec)
    assert engine.rec_loaded
    bad_det = dict(det_weights)
    bad_det["stem.conv1.b"] = det_weights["stem.conv1.b"][:16]
    try:
        engine.load_det(det_weights)
        with pytest.raises(EngineError, match=r"load_det_weights: wrong dimension \(tensor stem\.conv1\.b\)"):
            engine.load_det(bad_det)
        assert engine.det_loaded
    finally:
        engine.load_det(det_weights)
