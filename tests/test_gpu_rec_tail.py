"""GPU: the recogniser tail's streaming GEMM (x-projections, conv2 + pool) and the twelve-wave LSTM against the paths they replace,
bit for bit, with each option off and on on one engine."""
import functools

import numpy as np
import pytest
import torch

from lumina_ocr import synth

pytestmark = pytest.mark.gpu

# N = 1: M = 80 rows, less than one 128-row GEMM tile and one ragged LSTM group; N = 33: a ragged second 32-sequence group and a
# ragged last GEMM tile (2640 = 20 * 128 + 80); N = 130: several full groups and tiles (10400 = 81 * 128 + 32)
SIZES = (1, 33, 130)
OLD = dict(fuse_xproj=0, fuse_conv2_pool=0, lstm_waves=3)
NEW = dict(fuse_xproj=1, fuse_conv2_pool=1, lstm_waves=12)
DEFAULTS = dict(NEW, seq_gemm_min=128)   # engine.h
TAPS = ("rec.feat", "lstm.l0", "lstm.l1")


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(2468)
    n = max(SIZES)
    crops = np.stack([synth.synth_crop(rng)[0] for _ in range(n)])
    widths = np.full(n, 320, np.int32)
    widths[1::4] = rng.integers(8, 320, len(widths[1::4]))
    return crops, widths


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)   # (np.array_equal on floats would call -0 and +0 equal)


def _forward(engine, n, opts, taps=TAPS):
    crops, widths = _inputs()
    for k, v in opts.items():
        engine.set_option(k, v)
    engine.set_option("seq_gemm_min", 1)   # these sizes are below the default threshold of 128 work-groups: take the new kernels anyway
    engine.set_option("keep_taps", 2)   # the fusions stay on; what still exists is tapped
    try:
        idx, prob = engine.rec_forward(torch.from_numpy(crops[:n]).cuda(), torch.from_numpy(widths[:n]).cuda())
        torch.cuda.synchronize()
        out = {t: _bits(engine.read_tap(t)) for t in taps}
    finally:
        engine.set_option("keep_taps", 0)
        for k, v in DEFAULTS.items():
            engine.set_option(k, v)
    out["idx"] = idx.cpu().numpy()
    out["prob"] = _bits(prob.cpu().numpy())
    return out


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("n", SIZES)
def test_tail_options_are_bit_identical(engine, rec_weights, n):
    """rec.feat, both LSTM layers' outputs and the final idx / prob: every option toggled alone, and all together, against all off."""
    engine.load_rec(rec_weights)
    ref = _forward(engine, n, OLD)
    assert ref["lstm.l1"].shape[-1] == 192 and len(np.unique(ref["idx"])) > 1   # (a live sequence, not a constant)
    for key in NEW:
        _same(ref, _forward(engine, n, dict(OLD, **{key: NEW[key]})), key)
    _same(ref, _forward(engine, n, NEW), "all")


def test_conv2_pool_member_order(engine, rec_weights):
    """conv2 + pool on weights whose conv2 outputs hold, inside one pool window, equal maxima (channels with zero weights: the four
    members are the same value, positive, negative, +0 and -0 = hswish of a value <= -3) next to the dense channels, where windows with
    members of both signs and windows whose maximum is shared by two members occur (counted on the unfused path's rec.conv2 tap).  rec.feat
    must carry the same bits, signs of zero included.  NOT covered: a window that holds +0 and -0 together.  -0 needs a pre-activation
    <= -3 and +0 one that is exactly 0 in the same channel, and the pixels that enter conv2 (rec.b10's output) cannot be set."""
    w = dict(rec_weights)
    cw, cb = w["rec.conv2.w"].copy(), w["rec.conv2.b"].copy()
    consts = {0: 0.5, 1: -1.0, 2: 0.0, 3: -5.0, 285: 0.75, 287: -4.0}   # (285, 287: the last, partly stored, tile)
    for c, b in consts.items():
        cw[c] = 0
        cb[c] = b
    w["rec.conv2.w"], w["rec.conv2.b"] = cw, cb
    engine.load_rec(w)
    try:
        n = 33
        ref = _forward(engine, n, dict(NEW, fuse_conv2_pool=0), taps=("rec.conv2", "rec.feat"))
        got = _forward(engine, n, NEW, taps=("rec.feat",))
        conv2 = ref["rec.conv2"].view(np.float32).reshape(n, 2, 80, 2, 288)   # [n][dy][t][dx][c]
        win = conv2.transpose(0, 2, 1, 3, 4).reshape(n, 80, 4, 288)
        feat = ref["rec.feat"].view(np.float32).reshape(n, 80, 288)
        assert np.array_equal(feat, win.max(axis=2))
        for c, b in consts.items():   # constant channels: four equal members, and the sign of a zero survives the chain
            assert (win[..., c] == win[:, :, :1, c]).all()
            assert np.signbit(feat[..., c]).all() == (b < 0) and (feat[..., c] == 0).all() == (b in (0.0, -5.0, -4.0))
        dense = np.delete(win, list(consts), axis=3)
        both = ((dense > 0).any(axis=2) & (dense < 0).any(axis=2)).sum()
        tied = ((dense == dense.max(axis=2, keepdims=True)).sum(axis=2) > 1).sum()
        assert both > 0 and tied > 0, (int(both), int(tied))
        assert np.array_equal(ref["rec.feat"], got["rec.feat"]), int((ref["rec.feat"] != got["rec.feat"]).sum())
        assert np.array_equal(ref["idx"], got["idx"]) and np.array_equal(ref["prob"], got["prob"])
    finally:
        engine.load_rec(rec_weights)


def test_streaming_gemm_waits_for_enough_row_tiles(engine, rec_weights):
    """Below seq_gemm_min work-groups of 128 rows the tile-parallel kernels stay (here 33 crops = 21 work-groups against the default 128);
    with the threshold lowered the same forward takes the streaming kernel.  Read from the timed launches' kernel names."""
    crops, widths = _inputs()
    engine.load_rec(rec_weights)
    kernels = {}
    try:
        for minimum in (128, 21, 22):
            engine.set_option("seq_gemm_min", minimum)
            engine.conv_timing_detail()
            engine.set_option("time_convs", 1)
            engine.rec_forward(torch.from_numpy(crops[:33]).cuda(), torch.from_numpy(widths[:33]).cuda())
            torch.cuda.synchronize()
            kernels[minimum] = {layer: kernel for layer, kernel, _, _, _ in engine.conv_timing_detail()}
    finally:
        engine.set_option("time_convs", 0)
        engine.set_option("seq_gemm_min", 128)
    for minimum in (128, 22):
        assert "rec.conv2" in kernels[minimum] and not any("seq_gemm" in k for k in kernels[minimum].values()), minimum
    assert kernels[21]["rec.conv2+pool"] == "seq_gemm_kernel<48,1>"
    assert kernels[21]["lstm.l0.xproj"] == "seq_gemm_kernel<288,0>" and kernels[21]["lstm.l1.xproj"] == "seq_gemm_kernel<192,0>"
