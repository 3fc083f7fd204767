"""GPU: every layer of the det, CRNN, orientation-classifier and SVTR nets graded on its OWN input (teacher forcing).

The engine keeps its layer boundaries readable (option keep_taps); each tap is bf16- (or, for an fp16 SVTR model, fp16-) exact.
For every tap the oracle layer (oracle/nets.py det_* / rec_* / lstm_layer / svtr_*) is run on the engine's own input tap, in the
same storage mode, and its result is graded against the engine's output tap: no error carries over from earlier layers, so the
bounds are those of the layer alone.  Ulps are the storage type's (conftest.close_stats); `maxulp` is the largest error in those
ulps (floored at |ref| = 2^-6, as close_stats does).

Tolerance classes (bounds in BOUNDS below, with the measured figures behind every non-exact one):

  EXACT (np.array_equal)
    det   stem.pool (from stem.conv3, keep_taps=1); fpn.fuse (nearest upsampling + concat of its own p5 .. p2 slices)
    CRNN  rec.feat (2x2 max pool of rec.conv2)
    cls   cls.feat (2x2 max pool of cls.conv2)
    all   the padded channels of every CRNN and classifier tap (rec.conv1 8 -> 16, rec.b3 20 -> 32, cls.conv2 200 -> 208 ...) are
          exactly 0.  Invariant: the loader zero-pads weights and biases, relu / hswish map 0 to 0, and the SE gate
          hsigmoid(0) = 0.5 only ever multiplies the zero padded channels of the depthwise output.  (det and SVTR tensors have
          no padded channels.)
  STEM1  det stem.conv1 from the u8 page: every value within 1 ulp (as end to end today), not array_equal — the 27-term fp32 sum is
         ordered differently from torch's, and 1 of 1.2 M values measured lands on the other side of a rounding boundary
  ONE    one rounding between the taps: within1 > 0.999 and within4 == 1.0 (as test_gpu_conv.py), max 2 ulps
    det   stem.conv2, stem.conv3, head.conv1, head.convt2 (keep_taps=1)
    CRNN  rec.conv1 (from the u8 crop, width-masked), rec.conv2
    cls   cls.conv1 (from the u8 crop, width-masked), cls.conv2
    LSTM  the first 8 steps of each layer's forward direction and the last 8 of its backward direction (gate order, gate arithmetic)
  PROB   det probability map from head.convt2 (keep_taps=1): one rounding after the device's fast_sigmoidf
  SVTR_SEQ  svtr.seq (row mean + linear + hswish): one-rounding tightness
  several internal roundings: a within4 floor and a max error in ulps, each tighter than that tap's end-to-end bound today
    DET_BLOCK   s{i}.b{j} (conv0, shortcut incl. the 2x2/s2 vd form fused into the block entry, conv1 + residual)
    STEM_SPAN   stem.pool from the u8 page with keep_taps=2 (fused stem.conv1+conv2, stem.conv3 with the pool in its epilogue)
    FPN         fpn.p5 .. fpn.p2 from c2 .. c5 (keep_taps=2 ring: the maps themselves; otherwise the slices of fpn.fuse)
    HEAD_TAIL   prob from head.conv1 with keep_taps=2 (fused DBHead tail incl. fast_sigmoidf)
    MBCONV      rec.b{i} (expand, depthwise, SE pool / FC / gate, project + residual: mbconv_kernel or conv + dwconv_kernel +
                se_pool_kernel, se_fc_kernel, the project conv applying the gate in its operand staging)
                cls.b{i}: the same code at scale 0.35, 24-row maps, 96 columns (3 squeeze-excite strips) and block 0 as a
                stride-2 block WITH squeeze-excite
    SVTR_EMBED  svtr.embed (im2col, two patch-embedding GEMMs with GELU, positional embedding)
    SVTR_MERGE  svtr.sub{s} (3x3 / (2,1) conv + LayerNorm epilogue); also graded with a small-variance input (LayerNorm eps)
    SVTR_BLOCK  svtr.b{i}, local (7x11 window) and global blocks alike
    LSTM        each whole layer (lstm.l0 from rec.feat, lstm.l1 from lstm.l0)

The device approximates where the oracle is exact: fast_erf (GELU), fast_sigmoidf / the LSTM's fast sigmoid and tanh, v_exp_f32 in
the attention soft-max.  The GELU and sigmoid layers are also graded against the oracle with the device's approximations emulated
(_device_approx): the gap between the two figures is the approximation's share of the error (recorded in the JSON dump, see _dump_stats).
"""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

from conftest import close_stats
from lumina_ocr import arch, synth

pytestmark = pytest.mark.gpu

STATS = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_stats():
    """Every graded tap's statistics, as JSON, to the file LUMINA_LAYER_STATS names (not written when it is unset)."""
    yield
    path = os.environ.get("LUMINA_LAYER_STATS")
    if not path:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(STATS, f, indent=1, sort_keys=True)
    except OSError:
        pass


# class -> (within1 floor or None, within4 floor, max error in ulps).  Measured on an MI355X over every case of this file (worst
# value over all cases and taps of the class; "w1" = share within 1 ulp, "w4" within 4, "max" = largest error in ulps):
BOUNDS = {
    "ONE": (0.999, 1.0, 2.0),           # measured: w1 1.0, max 1.0 ulp (stem.conv2/3, head.conv1/convt2, rec.conv1/conv2, LSTM 8-step windows)
                                        #   classifier: cls.conv1 w1 1.0, max 0.96 ulp; cls.conv2 w1 1.0, max 0.85 ulp
    "STEM1": (0.99999, 1.0, 1.0),       # stem.conv1 from the page: w1 1.0, max 0.06 ulp; bit-equal on all but 1 of 1.2 M values
    "PROB": (0.999, 1.0, 2.0),          # prob from head.convt2: w1 1.0, max 0.8 ulp; vs the oracle with fast_sigmoidf emulated: the same
                                        #   figures — the approximation's share of the error is below one bf16 rounding
    "DET_BLOCK": (None, 0.9995, 64.0),  # s{i}.b{j}: w4 0.99997, max 32.2 ulp (end to end today: w4 > 0.90)
    "STEM_SPAN": (None, 0.9995, 32.0),  # stem.pool from the page through the fused stem (keep_taps=2): w4 0.99999, max 12.1 ulp
    "FPN": (None, 0.999, 32.0),         # fpn.p5 .. p2 from c2 .. c5: w4 0.99985, max 13.9 ulp (end to end today: w4 > 0.85)
    "HEAD_TAIL": (None, 0.9999, 4.0),   # prob from head.conv1 (fused DBHead tail): w4 1.0, max 1.1 ulp; fast_sigmoidf share: none measurable
    "MBCONV": (None, 0.9999, 8.0),      # rec.b{i}: w1 1.0, w4 1.0, max 2.5 ulp (end to end today: w4 > 0.90)
                                        #   cls.b{i}: w1 0.999995, w4 1.0, max 2.1 ulp (cls.b9, N = 33); b0 .. b3 and b6 bit-equal to the
                                        #   oracle in all four cases, fused and unfused alike.  For scale: one depthwise tap dropped in the
                                        #   stride-2 blocks gives cls.b0 w4 0.04, max 7400 ulp; 2 of the 3 squeeze-excite strips summed gives
                                        #   cls.b0 w4 0.61, max 510 ulp
    "LSTM": (None, 0.999, 8.0),         # whole layer, teacher-forced: w4 1.0, max 1.7 ulp (end to end today: lstm.l1 w4 > 0.6)
    "SVTR_EMBED": (None, 0.999, 32.0),  # svtr.embed: bf16 max 0.9 ulp; f16 w4 0.99994, max 16 ulp (fast_erf emulated: max 7.1 ulp —
                                        #   half of the fp16 error is the GELU approximation's; in bf16 it does not show)
    "SVTR_MERGE": (None, 0.9995, 16.0), # svtr.sub{s} (conv + LayerNorm): w4 0.99998, max 7.5 ulp
    "SVTR_SEQ": (0.999, 1.0, 4.0),      # svtr.seq (row mean + linear + hswish): w1 1.0, max 1.0 ulp
    "SVTR_BLOCK": (None, 0.99, 128.0),  # svtr.b{i}: w1 0.937, w4 0.9918, max 70.5 ulp (end to end today: w4 > 0.7).  The attention
                                        #   kernel rounds the un-normalised soft-max weights exp(s - m) to the storage type for the P.V
                                        #   MFMA; the definition keeps them fp32.  fast_erf emulated: the same figures (GELU is not it)
}


def _stats(got, ref, dtype="bf16"):
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    st = close_stats(got, ref, dtype)
    ulp = np.maximum(np.abs(ref), 2.0 ** -6) * (2.0 ** -7 if dtype == "bf16" else 2.0 ** -10)
    st["maxulp"] = float((np.abs(got - ref) / ulp).max())
    st["equal"] = float((got == ref).mean())
    return st


class Grader:
    """Collects every tap's statistics first, then fails once with the list of every tap that missed its bound."""

    def __init__(self, key, dtype="bf16"):
        self.key, self.dtype, self.fails = key, dtype, []
        STATS[key] = self.st = {}

    def exact(self, name, got, ref):
        got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
        ok = got.shape == ref.shape and np.array_equal(got, ref)
        self.st[name] = dict(cls="EXACT", equal=bool(ok))
        if not ok:
            self.fails.append((name, "EXACT", _stats(got, ref, self.dtype) if got.shape == ref.shape else (got.shape, ref.shape)))

    def grade(self, name, got, ref, cls, w4=None, maxulp=None, **extra):
        st = _stats(got, ref, self.dtype)
        st.update(cls=cls, **extra)
        self.st[name] = st
        b1, b4, bu = BOUNDS[cls]
        b4 = b4 if w4 is None else w4
        bu = bu if maxulp is None else maxulp
        if (b1 is not None and not st["within1"] > b1) or st["within4"] < b4 or st["maxulp"] > bu:
            self.fails.append((name, cls, st))
        return st

    def done(self):
        assert not self.fails, "%s: %d tap(s) out of bounds:\n" % (self.key, len(self.fails)) + "\n".join(map(repr, self.fails))


@contextlib.contextmanager
def _device_approx():
    """The oracle with the device's GELU (Abramowitz & Stegun erf, common.h fast_erf) and sigmoid (exp2 + reciprocal) in fp32."""
    from oracle import nets
    orig = nets._act
    ln2e = np.float32(1.4426950408889634)

    def fast_erf(x):
        ax = x.abs()
        t = 1.0 / (1.0 + 0.3275911 * ax)
        poly = ((((1.061405429 * t - 1.453152027) * t + 1.421413741) * t - 0.284496736) * t + 0.254829592) * t
        return torch.copysign(1.0 - poly * torch.exp2(-ln2e * ax * ax), x)

    def act(x, a):
        if a == "gelu":
            return 0.5 * x * (1.0 + fast_erf(x * np.float32(0.70710678118654752)))
        if a == "sigmoid":
            return 1.0 / (1.0 + torch.exp2(-ln2e * x))
        return orig(x, a)

    nets._act = act
    try:
        yield
    finally:
        nets._act = orig


def _T(a):
    from oracle import nets
    return nets.nhwc_to_nchw(a)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# --------------------------------------------------------------------------------------------------------------------------- det
def _pages(b, h, w, seed):
    return np.stack([synth.synth_page(h, w, seed + i, n_lines=max(1, min(h, w) // 40))[0] for i in range(b)])


# kernel selection: "default" (engine defaults), "dma" (conv_big_min=1, conv_ring=0: LDS-DMA 16x32 tiles, fpn.p2 in two steps),
# "ring" (conv_big_min=1, conv_ring=1: persistent ring kernel, composed fpn.p2, head.conv1 over p5 .. p2 at their own resolution)
DET_CASES = [
    # b, h, w, keep_taps, selection
    (1, 32, 32, 1, "default"),        # smallest legal page: c5 is 1 x 1
    (1, 32, 32, 2, "ring"),
    (1, 32, 1024, 2, "ring"),         # strip page and its transpose
    (1, 1024, 32, 1, "dma"),
    (3, 250, 200, 1, "ring"),         # sides not multiples of 32: valid region != hp x wp; a batch of 3
    (3, 250, 200, 2, "dma"),
    (1, 447, 901, 2, "default"),
    (1, 447, 901, 1, "dma"),
]


def _det_taps(engine, keep):
    from lumina_ocr.engine import EngineError
    out = {}
    for name in ["stem.conv1", "stem.conv2", "stem.conv3", "stem.pool"] + ["s%d.b%d" % (i, j) for i in range(4) for j in range(2)] + \
                ["fpn.fuse", "fpn.p5", "fpn.p4", "fpn.p3", "fpn.p2", "head.conv1", "head.convt2"]:
        try:
            out[name] = engine.read_tap(name)
        except EngineError:
            pass
    return out


@pytest.mark.parametrize("case", DET_CASES, ids=lambda c: "b%d_%dx%d_keep%d_%s" % c)
def test_det_layers_teacher_forced(request, engine, any_det_weights, case):
    from oracle import nets
    b, h, w, keep, sel = case
    wd = any_det_weights
    pages = _pages(b, h, w, 21)
    engine.load_det(wd)
    engine.set_option("keep_taps", keep)
    engine.set_option("det_sub_batch", 8)
    if sel != "default":
        engine.set_option("conv_big_min", 1)
        engine.set_option("conv_ring", 1 if sel == "ring" else 0)
    try:
        prob = engine.det_forward(torch.from_numpy(pages).cuda())
        torch.cuda.synchronize()
        got = _det_taps(engine, keep)
        got["prob"] = prob.float().cpu().numpy()
    finally:
        engine.set_option("keep_taps", 0)
        engine.set_option("det_sub_batch", 16)
        engine.set_option("conv_big_min", 1024)
        engine.set_option("conv_ring", 1)
    compose = sel != "dma" and nets.compose_fpn_p2(wd) is not None      # (the engine composes fpn.p2 on the ring kernel only)
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    g = Grader(request.node.name)
    with torch.no_grad():
        x = nets.det_normalize(pages, hp, wp)
        if keep == 1:
            for name in ("stem.conv1", "stem.conv2", "stem.conv3"):
                assert name in got, name
            g.grade("stem.conv1", got["stem.conv1"], _nhwc(nets.det_stem_conv1(wd, x)), "STEM1")
            g.grade("stem.conv2", got["stem.conv2"], _nhwc(nets.det_stem_conv2(wd, _T(got["stem.conv1"]))), "ONE")
            g.grade("stem.conv3", got["stem.conv3"], _nhwc(nets.det_stem_conv3(wd, _T(got["stem.conv2"]))), "ONE")
            g.exact("stem.pool", got["stem.pool"], _nhwc(nets.det_stem_pool(_T(got["stem.conv3"]))))
        else:
            assert "stem.conv1" not in got and "stem.conv3" not in got and "head.convt2" not in got, sorted(got)
            s = nets.det_stem_pool(nets.det_stem_conv3(wd, nets.det_stem_conv2(wd, nets.det_stem_conv1(wd, x))))
            g.grade("stem.pool<-page", got["stem.pool"], _nhwc(s), "STEM_SPAN")
        prev = "stem.pool"
        for i in range(4):
            for j in range(2):
                name = "s%d.b%d" % (i, j)
                g.grade(name, got[name], _nhwc(nets.det_block(wd, _T(got[prev]), i, j)), "DET_BLOCK")
                prev = name
        ps = nets.det_fpn(wd, _T(got["s0.b1"]), _T(got["s1.b1"]), _T(got["s2.b1"]), _T(got["s3.b1"]), compose=compose)
        if "fpn.fuse" in got:
            fz = got["fpn.fuse"]
            mine = [fz[:, ::8, ::8, 0:64], fz[:, ::4, ::4, 64:128], fz[:, ::2, ::2, 128:192], fz[..., 192:256]]
            g.exact("fpn.fuse", fz, _nhwc(nets.det_fuse(*[_T(m) for m in mine])))
        else:
            assert keep == 2 and all(n in got for n in ("fpn.p5", "fpn.p4", "fpn.p3", "fpn.p2")), sorted(got)
            mine = [got[n] for n in ("fpn.p5", "fpn.p4", "fpn.p3", "fpn.p2")]
        for name, m, ref in zip(("fpn.p5", "fpn.p4", "fpn.p3", "fpn.p2"), mine, ps):
            g.grade(name, m, _nhwc(ref), "FPN")
        fuse = nets.det_fuse(*[_T(m) for m in mine])
        g.grade("head.conv1", got["head.conv1"], _nhwc(nets.det_head_conv1(wd, fuse)), "ONE")
        h1 = _T(got["head.conv1"])
        if keep == 1:
            g.grade("head.convt2", got["head.convt2"], _nhwc(nets.det_head_convt2(wd, h1)), "ONE")
            ref = nets.det_head_convt3(wd, _T(got["head.convt2"]))[:, 0].numpy()
            with _device_approx():
                ref_a = nets.det_head_convt3(wd, _T(got["head.convt2"]))[:, 0].numpy()
            g.grade("prob", got["prob"], ref, "PROB", vs_device_sigmoid=_stats(got["prob"], ref_a))
        else:
            ref = nets.det_head_convt3(wd, nets.det_head_convt2(wd, h1))[:, 0].numpy()
            with _device_approx():
                ref_a = nets.det_head_convt3(wd, nets.det_head_convt2(wd, h1))[:, 0].numpy()
            g.grade("prob<-head.conv1", got["prob"], ref, "HEAD_TAIL", vs_device_sigmoid=_stats(got["prob"], ref_a))
    g.done()


# -------------------------------------------------------------------------------------------------------------------------- CRNN
REC_WIDTHS = [1, 8, 18, 33, 77, 319, 320]


def _crops(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([synth.synth_crop(rng)[0] for _ in range(n)])


def _lstm_grade(g, name, got, ref, hidden=96):
    """Whole layer (drift class), then the first 8 forward steps and the last 8 backward steps at one-rounding tightness."""
    g.grade(name, got, ref, "LSTM")
    g.grade(name + ".fw[:8]", got[:, :8, :hidden], ref[:, :8, :hidden], "ONE")
    g.grade(name + ".bw[-8:]", got[:, -8:, hidden:], ref[:, -8:, hidden:], "ONE")


@pytest.mark.parametrize("n,fuse_mb", [(33, 1), (33, 0), (1, 1), (7, 1)], ids=lambda v: str(v))
def test_rec_layers_teacher_forced(request, engine, rec_weights, n, fuse_mb):
    """N = 33 leaves lstm_kernel (32 crops per work-group) a group of one; every width the stem masks by, incl. 1 and 319."""
    from oracle import nets
    wd = rec_weights
    crops = _crops(n, 555 + n)
    widths = np.array([REC_WIDTHS[(i + n) % len(REC_WIDTHS)] for i in range(n)], np.int32)
    engine.load_rec(wd)
    engine.set_option("keep_taps", 1)
    engine.set_option("fuse_mb", fuse_mb)
    try:
        engine.rec_forward(torch.from_numpy(crops).cuda(), torch.from_numpy(widths).cuda())
        torch.cuda.synchronize()
        names = ["rec.conv1"] + ["rec.b%d" % i for i in range(11)] + ["rec.conv2", "rec.feat", "lstm.l0", "lstm.l1"]
        got = {k: engine.read_tap(k) for k in names}
    finally:
        engine.set_option("keep_taps", 0)
        engine.set_option("fuse_mb", 1)
    g = Grader(request.node.name)
    chans = {"rec.conv1": arch.rec_stem_ch(), "rec.conv2": 288}
    for b in arch.rec_block_table():
        chans["rec.b%d" % b["idx"]] = b["cout"]
    with torch.no_grad():
        x = nets.rec_normalize(crops)
        for i, wv in enumerate(widths):
            x[i, :, :, int(wv):] = 0
        for name, c in chans.items():                      # padded channels: exactly zero
            if got[name].shape[-1] > c:
                g.exact(name + ".pad", got[name][..., c:], np.zeros_like(got[name][..., c:]))
        real = {k: got[k][..., :c] for k, c in chans.items()}
        g.grade("rec.conv1", real["rec.conv1"], _nhwc(nets.rec_conv1(wd, x)), "ONE")
        prev = "rec.conv1"
        for i in range(11):
            name = "rec.b%d" % i
            g.grade(name, real[name], _nhwc(nets.rec_block(wd, _T(real[prev]), i)), "MBCONV")
            prev = name
        g.grade("rec.conv2", real["rec.conv2"], _nhwc(nets.rec_conv2(wd, _T(real["rec.b10"]))), "ONE")
        feat = nets.rec_pool(_T(real["rec.conv2"]))                          # [N,288,1,80]
        g.exact("rec.feat", got["rec.feat"].reshape(n, 80, 288), feat.squeeze(2).permute(0, 2, 1).numpy())
        seq = torch.from_numpy(got["rec.feat"].reshape(n, 80, 288).copy())
        l0 = nets.lstm_layer(wd, seq, 0).numpy()
        _lstm_grade(g, "lstm.l0", got["lstm.l0"].reshape(n, 80, 192), l0)
        l1 = nets.lstm_layer(wd, torch.from_numpy(got["lstm.l0"].reshape(n, 80, 192).copy()), 1).numpy()
        _lstm_grade(g, "lstm.l1", got["lstm.l1"].reshape(n, 80, 192), l1)
    g.done()


# -------------------------------------------------------------------------------------------------- orientation classifier
CLS_TAPS = ["cls.conv1"] + ["cls.b%d" % i for i in range(11)] + ["cls.conv2", "cls.feat"]


def _cls_real_channels():
    chans = {"cls.conv1": arch.rec_stem_ch(arch.CLS_SCALE), "cls.conv2": arch.CLS_FEAT, "cls.feat": arch.CLS_FEAT}
    for b in arch.cls_block_table():
        chans["cls.b%d" % b["idx"]] = b["cout"]
    return chans


@pytest.fixture(scope="module")
def cls_weights():
    return arch.make_cls_weights(2718)


@pytest.mark.parametrize("n,fuse_mb", [(33, 1), (33, 0), (1, 1), (7, 1)], ids=lambda v: str(v))
def test_cls_layers_teacher_forced(request, engine, cls_weights, n, fuse_mb):
    """The shared MobileNetV3 code at the classifier's shapes: scale 0.35 (other padded channel counts), strides (2,2,1,2,1,1,1,1,2,1,1)
    (block 0 is stride 2 WITH squeeze-excite), 24-row maps, 96 columns (3 squeeze-excite strips), the 2 x 2 pool down to one row.
    N = 33 leaves a group of one wherever the code groups by 32; crop 0 is uniform noise, the others rendered text lines; the valid
    widths cycle through every edge of the stem's mask (1, 191, 192)."""
    import cls_reference as cr
    wd = cls_weights
    crops, widths = cr.layer_crops(n)
    engine.load_cls(wd)
    engine.set_option("keep_taps", 1)
    engine.set_option("fuse_mb", fuse_mb)
    try:
        engine.cls_forward(torch.from_numpy(crops).cuda(), torch.from_numpy(widths).cuda())
        torch.cuda.synchronize()
        got = {k: engine.read_tap(k) for k in CLS_TAPS}
    finally:
        engine.set_option("keep_taps", 0)
        engine.set_option("fuse_mb", 1)
    g = Grader(request.node.name)
    chans = _cls_real_channels()
    table = arch.cls_block_table()
    assert got["cls.conv1"].shape[:3] == (n, 24, 96) and got["cls.feat"].shape[:3] == (n, 1, 48)
    assert [got["cls.b%d" % b["idx"]].shape[1] for b in table] == [b["h"] for b in table]
    with torch.no_grad():
        for name, c in chans.items():                      # padded channels: exactly zero
            assert got[name].shape[-1] >= c, (name, got[name].shape)
            if got[name].shape[-1] > c:
                g.exact(name + ".pad", got[name][..., c:], np.zeros_like(got[name][..., c:]))
        real = {k: got[k][..., :c] for k, c in chans.items()}
        g.grade("cls.conv1", real["cls.conv1"], _nhwc(cr.cls_conv1(wd, cr.normalize(crops, widths))), "ONE")
        prev = "cls.conv1"
        for b in table:
            name = "cls.b%d" % b["idx"]
            g.grade(name, real[name], _nhwc(cr.cls_block(wd, _T(real[prev]), b)), "MBCONV", stride_h=b["stride_h"], se=bool(b["se"]))
            prev = name
        g.grade("cls.conv2", real["cls.conv2"], _nhwc(cr.cls_conv2(wd, _T(real["cls.b10"]))), "ONE")
        g.exact("cls.feat", real["cls.feat"], _nhwc(cr.cls_pool(_T(real["cls.conv2"]))))
    g.done()


def test_cls_fused_expand_depthwise_is_bit_identical(engine, cls_weights):
    """The classifier with fuse_mb 1 and 0 on the same 9 crops (ragged widths): every block output, the pooled features, the logits and
    label / score / flip are bit-identical, and the launch records show that the two runs really differ in kernels — mbconv_kernel<...>
    is listed with fuse_mb = 1 and absent with 0."""
    import cls_reference as cr
    crops, widths = cr.layer_crops(9, seed=77)
    names = ["cls.b%d" % i for i in range(11)] + ["cls.feat", "cls.logits"]
    engine.load_cls(cls_weights)
    engine.conv_timing_detail()                     # drop earlier records
    engine.set_option("keep_taps", 1)
    engine.set_option("time_convs", 1)
    outs, kernels = [], []
    try:
        for fuse in (1, 0):
            engine.set_option("fuse_mb", fuse)
            res = engine.cls_forward(torch.from_numpy(crops).cuda(), torch.from_numpy(widths).cuda())
            torch.cuda.synchronize()
            kernels.append([k for _, k, *_ in engine.conv_timing_detail()])
            outs.append(([engine.read_tap(k).copy() for k in names], [r.cpu().numpy() for r in res]))
    finally:
        engine.set_option("fuse_mb", 1)
        engine.set_option("keep_taps", 0)
        engine.set_option("time_convs", 0)
    fused = [k for k in kernels[0] if k.startswith("mbconv_kernel<")]
    assert fused and any(k.startswith("mbconv_kernel<3,2,") for k in fused), kernels[0]      # incl. a stride-2 block
    assert not any(k.startswith("mbconv_kernel<") for k in kernels[1]), kernels[1]
    for name, a, b in zip(names, outs[0][0], outs[1][0]):
        assert np.array_equal(a, b), name
    for name, a, b in zip(("label", "score", "flip"), outs[0][1], outs[1][1]):
        assert np.array_equal(a, b), name


# -------------------------------------------------------------------------------------------------------------------------- SVTR
@pytest.mark.parametrize("variant,dtype", [("tiny", "bf16"), ("tiny", "f16"), ("base", "bf16"), ("base", "f16")])
def test_svtr_layers_teacher_forced(request, engine, variant, dtype):
    """Ragged widths (incl. 33: most of the 7 x 11 windows of the first columns see zero tokens' neighbours), an odd N; the local
    blocks (window attention) and the global ones are graded alike."""
    from oracle import nets
    wd = arch.make_svtr_weights(variant=variant, dtype=dtype, num_classes=200)
    n = 3
    crops = _crops(n, 919)
    widths = np.array([211, 320, 33], np.int32)
    engine.load_svtr(wd)
    assert engine.svtr_dtype == dtype
    cfg = arch.svtr_config(wd)
    table = arch.svtr_block_table(cfg)
    names = ["svtr.embed", "svtr.sub0", "svtr.sub1", "svtr.seq"] + ["svtr.b%d" % b["idx"] for b in table]
    engine.set_option("keep_taps", 1)
    try:
        engine.svtr_forward(torch.from_numpy(crops).cuda(), torch.from_numpy(widths).cuda())
        torch.cuda.synchronize()
        got = {k: engine.read_tap(k, dtype) for k in names}
    finally:
        engine.set_option("keep_taps", 0)
    g = Grader(request.node.name, dtype)
    tok = lambda a: torch.from_numpy(a.reshape(n, -1, a.shape[-1]).copy())   # noqa: E731  ([N,h,w,C] tap -> tokens)
    with torch.no_grad():
        x = nets.rec_normalize(crops, dtype)
        for i, wv in enumerate(widths):
            x[i, :, :, int(wv):] = 0
        ref = nets.svtr_embed(wd, x, dtype).numpy()
        with _device_approx():
            ref_a = nets.svtr_embed(wd, x, dtype).numpy()
        g.grade("svtr.embed", tok(got["svtr.embed"]).numpy(), ref, "SVTR_EMBED", vs_device_gelu=_stats(tok(got["svtr.embed"]).numpy(), ref_a, dtype))
        prev = "svtr.embed"
        for b in table:
            if b["idx"] > 0 and b["stage"] != table[b["idx"] - 1]["stage"]:
                s = b["stage"] - 1
                g.grade("svtr.sub%d" % s, tok(got["svtr.sub%d" % s]).numpy(),
                        nets.svtr_merge(wd, tok(got[prev]), s, 2 * b["h"], b["w"], dtype).numpy(), "SVTR_MERGE")
                prev = "svtr.sub%d" % s
            name = "svtr.b%d" % b["idx"]
            inp = tok(got[prev])
            ref = nets.svtr_block(wd, inp, b["idx"], dtype).numpy()
            with _device_approx():
                ref_a = nets.svtr_block(wd, inp, b["idx"], dtype).numpy()
            g.grade(name, tok(got[name]).numpy(), ref, "SVTR_BLOCK", local=b["local"], vs_device_gelu=_stats(tok(got[name]).numpy(), ref_a, dtype))
            prev = name
        last = table[-1]
        g.grade("svtr.seq", tok(got["svtr.seq"]).numpy(), nets.svtr_last(wd, tok(got[prev]), last["h"], last["w"], dtype).numpy(), "SVTR_SEQ")
    g.done()


def test_svtr_merge_layernorm_at_small_variance(request, engine):
    """The merging convs' weights and biases scaled by 2^-8 (exact in bf16): the LayerNorm input's variance drops to ~1e-5, where
    the eps (1e-6, arch.SVTR_LN_EPS) moves rstd by several percent — at unit variance a wrong eps is invisible below one ulp."""
    from oracle import nets
    wd = dict(arch.make_svtr_weights(variant="tiny", dtype="bf16", num_classes=200))
    for s in range(2):
        for k in (".w", ".b"):
            wd["svtr.sub%d%s" % (s, k)] = wd["svtr.sub%d%s" % (s, k)] * np.float32(2.0 ** -8)
    n = 3
    crops = _crops(n, 313)
    widths = np.array([320, 97, 250], np.int32)
    engine.load_svtr(wd)
    table = arch.svtr_block_table(arch.svtr_config(wd))
    ends = [b["idx"] for b in table[:-1] if table[b["idx"] + 1]["stage"] != b["stage"]]       # last block of stages 0 and 1
    engine.set_option("keep_taps", 1)
    try:
        engine.svtr_forward(torch.from_numpy(crops).cuda(), torch.from_numpy(widths).cuda())
        torch.cuda.synchronize()
        got = {k: engine.read_tap(k) for k in ["svtr.sub0", "svtr.sub1"] + ["svtr.b%d" % i for i in ends]}
    finally:
        engine.set_option("keep_taps", 0)
    g = Grader(request.node.name)
    with torch.no_grad():
        for s, i in enumerate(ends):
            b = table[i]
            inp = torch.from_numpy(got["svtr.b%d" % i].reshape(n, -1, b["dim"]).copy())
            img = inp.reshape(n, b["h"], b["w"], b["dim"]).permute(0, 3, 1, 2)
            pre = nets.conv_bn_act(img, wd, "svtr.sub%d" % s, (2, 1), "none")
            assert float(pre.var(dim=1).mean()) < 1e-4                     # the eps matters at this variance
            ref = nets.svtr_merge(wd, inp, s, b["h"], b["w"]).numpy()
            g.grade("svtr.sub%d" % s, got["svtr.sub%d" % s].reshape(ref.shape), ref, "SVTR_MERGE")
    g.done()
