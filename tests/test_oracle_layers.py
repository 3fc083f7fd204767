"""CPU: the per-layer oracle entry points (oracle/nets.py det_* / rec_* / lstm_layer / svtr_*) compose to exactly the forwards they
were split out of.  `_legacy_*` below are the monolithic forward loops as they stood before the split (frozen here, built on the
unchanged helpers conv_bn_act / _convt2x2 / lstm_dir / _linear / _layernorm); every tap and every output must be bit-identical.
Then each layer function fed the previous tap must reproduce the next tap — the teacher-forced form the GPU layer tests
(test_gpu_layer_parity.py) use.  That check allows one storage-type ulp on a few values: torch's CPU convolution sums in another
order for a channels-last input (the concat det_forward builds is one), and the fp32 summation order is not part of the definition."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lumina_ocr import arch, synth
from oracle import nets


def _legacy_det(wd, pages_u8, mode="bf16", taps=None, compose=True):
    b, h, w, _ = pages_u8.shape
    hp, wp = (h + 31) // 32 * 32, (w + 31) // 32 * 32
    x = nets.det_normalize(pages_u8, hp, wp, mode)
    cba = nets.conv_bn_act

    def tap(name, t):
        taps[name] = t.permute(0, 2, 3, 1).contiguous().numpy()

    with torch.no_grad():
        x = cba(x, wd, "stem.conv1", 2, "relu", mode=mode); tap("stem.conv1", x)
        x = cba(x, wd, "stem.conv2", 1, "relu", mode=mode); tap("stem.conv2", x)
        x = cba(x, wd, "stem.conv3", 1, "relu", mode=mode); tap("stem.conv3", x)
        x = F.max_pool2d(x, 3, 2, 1); tap("stem.pool", x)
        feats = []
        for i in range(4):
            for j in range(2):
                p = f"s{i}.b{j}"
                stride = 2 if (i > 0 and j == 0) else 1
                y = cba(x, wd, p + ".conv0", stride, "relu", mode=mode)
                if j == 0:
                    sc = cba(x, wd, p + ".short", 1, "none", mode=mode) if i == 0 else cba(x, wd, p + ".short", 2, "none", mode=mode, pad=0)
                else:
                    sc = x
                x = cba(y, wd, p + ".conv1", 1, "relu", residual=sc, mode=mode)
                tap(p, x)
            feats.append(x)
        c2, c3, c4, c5 = feats
        up = lambda t, s: F.interpolate(t, scale_factor=s, mode="nearest")  # noqa: E731
        in5 = cba(c5, wd, "fpn.in5", 1, "none", mode=mode)
        out4 = cba(c4, wd, "fpn.in4", 1, "none", residual=up(in5, 2), mode=mode)
        out3 = cba(c3, wd, "fpn.in3", 1, "none", residual=up(out4, 2), mode=mode)
        p5 = cba(in5, wd, "fpn.p5", 1, "none", mode=mode); tap("fpn.p5", p5)
        p4 = cba(out4, wd, "fpn.p4", 1, "none", mode=mode); tap("fpn.p4", p4)
        p3 = cba(out3, wd, "fpn.p3", 1, "none", mode=mode); tap("fpn.p3", p3)
        wc = nets.compose_fpn_p2(wd) if compose else None
        if wc is not None:
            cat = torch.cat([c2, up(out3, 2)], dim=1)
            p2 = cba(cat, {"fpn.p2c.w": wc, "fpn.p2c.b": wd["fpn.p2.b"]}, "fpn.p2c", 1, "none", mode=mode)
        else:
            out2 = cba(c2, wd, "fpn.in2", 1, "none", residual=up(out3, 2), mode=mode)
            p2 = cba(out2, wd, "fpn.p2", 1, "none", mode=mode)
        tap("fpn.p2", p2)
        fuse = torch.cat([up(p5, 8), up(p4, 4), up(p3, 2), p2], dim=1); tap("fpn.fuse", fuse)
        y = cba(fuse, wd, "head.conv1", 1, "relu", mode=mode); tap("head.conv1", y)
        y = nets._convt2x2(y, wd, "head.convt2", "relu", mode); tap("head.convt2", y)
        y = nets._convt2x2(y, wd, "head.convt3", "sigmoid", mode)
    return y[:, 0].contiguous().numpy()


def _legacy_rec(wd, x, mode="bf16", taps=None):
    cba = nets.conv_bn_act

    def tap(name, t):
        taps[name] = t.permute(0, 2, 3, 1).contiguous().numpy()

    x = cba(x, wd, "rec.conv1", 2, "hswish", mode=mode); tap("rec.conv1", x)
    for b in arch.rec_block_table():
        p = f"rec.b{b['idx']}"
        y = cba(x, wd, p + ".expand", 1, b["act"], mode=mode)
        y = cba(y, wd, p + ".dw", (b["stride_h"], 1), b["act"], mode=mode, groups=b["exp"])
        if b["se"]:
            s = nets._rb(y.mean(dim=(2, 3), keepdim=True), mode)
            s = cba(s, wd, p + ".se1", 1, "relu", mode=mode)
            s = cba(s, wd, p + ".se2", 1, "hsigmoid", mode=mode)
            y = nets._rb(y * s, mode)
        x = cba(y, wd, p + ".project", 1, "none", residual=x if b["res"] else None, mode=mode)
        tap(p, x)
    x = cba(x, wd, "rec.conv2", 1, "hswish", mode=mode); tap("rec.conv2", x)
    feat = F.max_pool2d(x, 2, 2)
    seq = feat.squeeze(2).permute(0, 2, 1).contiguous()
    for layer in (0, 1):
        outs = []
        for d, rev in (("fw", False), ("bw", True)):
            p = f"lstm.l{layer}.{d}"
            outs.append(nets.lstm_dir(seq, torch.from_numpy(wd[p + ".w_ih"]), torch.from_numpy(wd[p + ".w_hh"]),
                                      torch.from_numpy(wd[p + ".b"]), rev, mode))
        seq = torch.cat(outs, dim=2)
        taps["lstm.l%d" % layer] = seq.numpy()
    return feat


def _legacy_svtr(wd, x, mode="bf16", taps=None):
    def tap(name, t):
        taps[name] = t.contiguous().numpy()

    cfg = arch.svtr_config(wd)
    x = nets.conv_bn_act(x, wd, "svtr.pe1", 2, "gelu", mode=mode)
    x = nets.conv_bn_act(x, wd, "svtr.pe2", 2, "gelu", mode=mode)
    n, c, h, w = x.shape
    t = x.permute(0, 2, 3, 1).reshape(n, h * w, c)
    t = nets._rb(t + nets._rb(torch.from_numpy(wd["svtr.pos.w"]), mode), mode); tap("svtr.embed", t)
    stage = 0
    for b in arch.svtr_block_table(cfg):
        if b["stage"] != stage:
            img = t.reshape(n, h, w, c).permute(0, 3, 1, 2)
            img = nets.conv_bn_act(img, wd, f"svtr.sub{stage}", (2, 1), "none", mode=mode)
            n, c, h, w = img.shape
            t = nets._layernorm(img.permute(0, 2, 3, 1).reshape(n, h * w, c), wd, f"svtr.sub{stage}.ln", mode); tap(f"svtr.sub{stage}", t)
            stage = b["stage"]
        p, heads = f"svtr.b{b['idx']}", b["heads"]
        hd = c // heads
        qkv = nets._linear(t, wd, p + ".qkv", mode=mode).reshape(n, h * w, 3, heads, hd).permute(2, 0, 3, 1, 4)
        sc = (qkv[0] @ qkv[1].transpose(-1, -2)) * np.float32(hd ** -0.5)
        if b["local"]:
            sc = sc.masked_fill(~nets._svtr_mask(h, w), float("-inf"))
        att = nets._rb((torch.softmax(sc, dim=-1) @ qkv[2]).permute(0, 2, 1, 3).reshape(n, h * w, c), mode)
        t = nets._layernorm(nets._linear(att, wd, p + ".proj", residual=t, mode=mode), wd, p + ".ln1", mode)
        m = nets._linear(t, wd, p + ".fc1", act="gelu", mode=mode)
        t = nets._layernorm(nets._linear(m, wd, p + ".fc2", residual=t, mode=mode), wd, p + ".ln2", mode); tap(p, t)
    pooled = nets._rb(t.reshape(n, h, w, c).mean(dim=1), mode)
    seq = nets._linear(pooled, wd, "svtr.last", act="hswish", mode=mode); tap("svtr.seq", seq)
    return seq


def _tf(got, want):
    """Teacher-forced output vs the tap: bit-identical but for summation order (<= 1 ulp, on < 0.1 % of the values)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    err = np.abs(got - want)
    assert (err <= np.maximum(np.abs(want), 2.0 ** -6) * 2.0 ** -7).all() and (err > 0).mean() < 1e-3
    return True


def _same_taps(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def det_w():
    return arch.make_det_weights(1234, text_path=False)


@pytest.fixture(scope="module")
def rec_w():
    return arch.make_rec_weights(4321)


def _crops(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([synth.synth_crop(rng)[0] for _ in range(n)])


@pytest.mark.parametrize("compose", [True, False])
def test_det_forward_composed_from_layers_is_bit_identical(det_w, compose):
    pages = np.stack([synth.synth_page(70, 90, 5 + i, n_lines=2)[0] for i in range(2)])
    t_old, t_new = {}, {}
    old = _legacy_det(det_w, pages, taps=t_old, compose=compose)
    new = nets.det_forward(det_w, pages, taps=t_new, compose=compose)
    assert np.array_equal(old, new)
    _same_taps(t_old, t_new)
    # teacher forcing: every layer function on the previous tap reproduces the next tap exactly
    T = {k: nets.nhwc_to_nchw(v) for k, v in t_new.items()}
    nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()  # noqa: E731
    with torch.no_grad():
        assert _tf(nhwc(nets.det_stem_conv2(det_w, T["stem.conv1"])), t_new["stem.conv2"])
        assert _tf(nhwc(nets.det_stem_conv3(det_w, T["stem.conv2"])), t_new["stem.conv3"])
        assert _tf(nhwc(nets.det_stem_pool(T["stem.conv3"])), t_new["stem.pool"])
        prev = "stem.pool"
        for i in range(4):
            for j in range(2):
                assert _tf(nhwc(nets.det_block(det_w, T[prev], i, j)), t_new[f"s{i}.b{j}"]), (i, j)
                prev = f"s{i}.b{j}"
        ps = nets.det_fpn(det_w, T["s0.b1"], T["s1.b1"], T["s2.b1"], T["s3.b1"], compose=compose)
        for name, p in zip(("fpn.p5", "fpn.p4", "fpn.p3", "fpn.p2"), ps):
            assert _tf(nhwc(p), t_new[name]), name
        assert _tf(nhwc(nets.det_fuse(T["fpn.p5"], T["fpn.p4"], T["fpn.p3"], T["fpn.p2"])), t_new["fpn.fuse"])
        assert _tf(nhwc(nets.det_head_conv1(det_w, T["fpn.fuse"])), t_new["head.conv1"])
        assert _tf(nhwc(nets.det_head_convt2(det_w, T["head.conv1"])), t_new["head.convt2"])
        assert _tf(nets.det_head_convt3(det_w, T["head.convt2"])[:, 0].numpy(), new)


def test_rec_forward_composed_from_layers_is_bit_identical(rec_w):
    crops = _crops(3, 11)
    x = nets.rec_normalize(crops)
    x[1, :, :, 77:] = 0
    t_old, t_new = {}, {}
    with torch.no_grad():
        f_old = _legacy_rec(rec_w, x, taps=t_old)
        f_new = nets.rec_backbone(rec_w, x, taps=t_new)
        assert np.array_equal(f_old.numpy(), f_new.numpy())
        ridx, rprob, logits, seq = nets.rec_head(rec_w, f_new)
        assert np.array_equal(seq, t_old["lstm.l1"])
        t_new["lstm.l0"] = nets.lstm_layer(rec_w, f_new.squeeze(2).permute(0, 2, 1).contiguous(), 0).numpy()
        t_new["lstm.l1"] = seq
        _same_taps(t_old, t_new)
        # the legacy head (CTC over the same sequence)
        lg = torch.from_numpy(seq) @ torch.from_numpy(rec_w["ctc.fc.w"]).t() + torch.from_numpy(rec_w["ctc.fc.b"])
        assert np.array_equal(lg.numpy(), logits)
        T = {k: nets.nhwc_to_nchw(v) for k, v in t_new.items() if v.ndim == 4}
        nhwc = lambda t: t.permute(0, 2, 3, 1).numpy()  # noqa: E731
        assert _tf(nhwc(nets.rec_conv1(rec_w, x)), t_new["rec.conv1"])
        prev = "rec.conv1"
        for i in range(11):
            assert _tf(nhwc(nets.rec_block(rec_w, T[prev], i)), t_new["rec.b%d" % i]), i
            prev = "rec.b%d" % i
        assert _tf(nhwc(nets.rec_conv2(rec_w, T["rec.b10"])), t_new["rec.conv2"])
        assert _tf(nets.rec_pool(T["rec.conv2"]).numpy(), f_new.numpy())
        assert _tf(nets.lstm_layer(rec_w, torch.from_numpy(t_new["lstm.l0"]), 1).numpy(), seq)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_svtr_forward_composed_from_layers_is_bit_identical(dtype):
    wd = arch.make_svtr_weights(variant="tiny", dtype=dtype, num_classes=100)
    crops = _crops(2, 12)
    x = nets.rec_normalize(crops, dtype)
    x[0, :, :, 150:] = 0
    t_old, t_new = {}, {}
    with torch.no_grad():
        s_old = _legacy_svtr(wd, x, dtype, t_old)
        s_new = nets.svtr_backbone(wd, x, dtype, t_new)
        assert np.array_equal(s_old.numpy(), s_new.numpy())
        _same_taps(t_old, t_new)
        T = {k: torch.from_numpy(v) for k, v in t_new.items()}
        cfg = arch.svtr_config(wd)
        prev = "svtr.embed"
        for b in arch.svtr_block_table(cfg):
            if b["idx"] > 0 and b["stage"] != arch.svtr_block_table(cfg)[b["idx"] - 1]["stage"]:
                s = b["stage"] - 1
                assert _tf(nets.svtr_merge(wd, T[prev], s, 2 * b["h"], b["w"], dtype).numpy(), t_new[f"svtr.sub{s}"])
                prev = f"svtr.sub{s}"
            assert _tf(nets.svtr_block(wd, T[prev], b["idx"], dtype).numpy(), t_new["svtr.b%d" % b["idx"]]), b["idx"]
            prev = "svtr.b%d" % b["idx"]
        last = arch.svtr_block_table(cfg)[-1]
        assert _tf(nets.svtr_last(wd, T[prev], last["h"], last["w"], dtype).numpy(), t_new["svtr.seq"])
