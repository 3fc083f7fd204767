"""Valid JPEG 2000 files that OpenJPEG's encoder never writes, built by tests/jp2_writer.py from seeded content.  The expected pixels
of an accepted file are always Pillow's (jp2_cases.expected); a pixel-preserving rewrite also names the file it was made from.

rewritten()   -> [Case]: every option of jp2_writer.rewrite on its own over a handful of Pillow files, then a few combinations.
synthesised() -> [Case]: codestreams from the Python tier-1 / tier-2 writer: blocks of 13 to 15 bit-planes, the pass-count escape,
                 zero bit-planes up to Mb 15, three-layer 4x4-block files with late inclusion and free byte splits, cut codewords.
refused()     -> [Case]: the variants that must give -2 (Mb 16, 33 layers).
accepted() = rewritten() + synthesised().  Everything is built once per session.

Case: .name, .data, .irreversible (takes the 9/7 entry points), .base (bytes whose Pillow pixels this file must keep, or None),
.family, .report (jp2_writer.synth's, or None), .deep (LL solved for a target and 15 planes deep), .full (no block stops early)."""
import numpy as np

import jp2_cases as jc
import jp2_irreversible_cases as ic
import jp2_reference as jr
import jp2_writer as jw


class Case:
    def __init__(self, name, data, family, irreversible=False, base=None, report=None, deep=False, full=True):
        self.name, self.data, self.family, self.irreversible, self.base = name, data, family, irreversible, base
        self.report, self.deep, self.full = report, deep, full

    def __repr__(self):
        return "Case(%s)" % self.name


PROVIDER_EDITS = dict(guard=1, tlm=True, parts=3, xlbox=True)   # the file of the provider test: tests/test_gpu_jp2_unusual.py


def bases():
    """{short name: (bytes, irreversible)}"""
    have, have97 = dict(jc.intact()), dict(ic.intact())
    return {
        "grey": (have["s63x65_L"], False),                  # LRCP, one layer, five levels: 6 packets
        "rpcl": (have["prog_RPCL"], False),                 # RGB, two layers, three levels: 24 packets
        "cprl": (have["prog_CPRL_L"], False),               # grey 65 x 63, two layers, 16 x 16 blocks
        "cb4": (have["cb4x4_RGB"], False),                  # RGB, 4 x 4 blocks: deep tag trees
        "raw": (have["no_jp2_RGB"], False),                 # a raw codestream
        "lv3": (jc.write(jc.content("page", 100, 130, "RGB", 77), irreversible=False, num_resolutions=4), False),   # three levels
        "rpcl97": (have97["prog_RPCL"], True),              # 9/7, RGB, two layers
    }


_BUILT = {}


def rewritten():
    if "rewritten" in _BUILT:
        return _BUILT["rewritten"]
    B = bases()
    out = []

    def add(name, base, keeps=True, **edits):
        data, irr = B[base]
        out.append(Case("%s_%s" % (base, name), jw.rewrite(data, **edits), "rewrite", irreversible=irr, base=data if keeps else None))

    # guard bits (5/3: Mb and so the pixels stay)
    for g in (0, 1, 3, 4, 5, 6, 7):
        add("guard%d" % g, "grey", guard=g)
    add("guard1", "rpcl", guard=1)
    add("guard3", "cb4", guard=3)
    # main header
    add("qcd_first", "rpcl", qcd_first=True)
    add("coms", "grey", coms=True)
    add("tlm", "rpcl", tlm=True)
    add("coc_qcc", "rpcl", coc_qcc=True)
    add("coc_qcc", "grey", coc_qcc=True)
    # tile-parts
    add("parts3_psot0_tn0", "grey", parts=3, psot0_last=True, tnsot=0)
    add("parts7_exact_tn7", "rpcl", parts=7)
    add("parts3_com_plt", "cprl", parts=3, part_com=True, plt=True)
    add("parts24_psot0_tn0", "rpcl", parts=24, psot0_last=True, tnsot=0)
    add("parts2_tn0_exact", "cb4", parts=2, tnsot=0)
    add("parts3_coms", "raw", parts=3, coms=True, psot0_last=True)
    # trailing empty layers: LRCP, RPCL, CPRL, and up to the 32 the decoder takes
    add("layers_plus3", "grey", extra_layers=3)
    add("layers_plus2", "rpcl", extra_layers=2)
    add("layers_to32", "cprl", extra_layers=30)
    add("layers_to32", "grey", extra_layers=31)
    # boxes
    add("xlbox", "grey", xlbox=True)
    add("len0", "rpcl", len0=True)
    add("extra_boxes", "cb4", extra_boxes=True)
    add("res", "grey", res=True)
    add("jpx", "lv3", jpx=True)
    # combinations
    add("provider", "rpcl", **PROVIDER_EDITS)
    add("all_markers", "rpcl", guard=1, qcd_first=True, coms=True, tlm=True, coc_qcc=True, parts=3, psot0_last=True, tnsot=0, part_com=True, plt=True,
        xlbox=True)
    add("mix_a", "cb4", guard=0, parts=5, extra_layers=2, extra_boxes=True, jpx=True, plt=True)
    add("mix_b", "lv3", guard=3, parts=4, plt=True, len0=True, res=True, tlm=True, tnsot=0)
    # 9/7: new guard bits change the step sizes, so only Pillow's decode of the new file says what the pixels are
    add("guard1", "rpcl97", keeps=False, guard=1)
    add("guard3", "rpcl97", keeps=False, guard=3)
    add("parts3_tlm_coms", "rpcl97", parts=3, tlm=True, coms=True, psot0_last=True, tnsot=0)
    add("layers_plus2_coc_qcc", "rpcl97", extra_layers=2, coc_qcc=True)
    _BUILT["rewritten"] = out
    return out


# ---------------------------------------------------------------------------------------------------------------- synthesised
DEEP_MAG = (1 << 14) - 1    # the detail bands of a deep file: 14 bit-planes


def deep_plane(W, H, seed):
    """one-level Mallat plane [H, W]: HL, LH and HH random in +-DEEP_MAG, LL solved so that the even / even output samples are a
    seeded target strictly inside 0..255.  Eight detail values next to LL[1, 1] are set to +-DEEP_MAG with the signs that add up, so
    that LL[1, 1] is certain to need 15 bit-planes.

    Rows and columns 6..13 of every detail band and 7..13 of LL are a quiet patch: zero but for a few values of 1 to 6 in magnitude.  Among large
    random values every coefficient is significant long before the last planes, whose significance and clean-up passes then take no
    decision, so that a decoder that dropped or misplaced one of the last passes would still give the same pixels; in the patch
    the passes down to the 43rd decide something (run-length mode included), and its output samples are not clamped."""
    rng = np.random.default_rng(seed)
    plane = rng.integers(-DEEP_MAG, DEEP_MAG + 1, (H, W)).astype(np.int64)
    (_, _, lys, lxs), (_, _, ays, axs), (_, _, bys, bxs), (_, _, cys, cxs) = jw.band_slices(W, H, 1)
    ll, hl, lh, hh = plane[lys, lxs], plane[ays, axs], plane[bys, bxs], plane[cys, cxs]
    hl[1, 0:2] = -DEEP_MAG
    lh[0:2, 1] = -DEEP_MAG
    hh[0:2, 0:2] = DEEP_MAG

    def quiet(n):
        q = np.zeros((n, n), np.int64)
        q[1, 1], q[1, 2] = 5, -2      # alone until the clean-up pass of plane 2; its neighbour follows in the significance pass of plane 1
        q[3, 1], q[3, 2] = 3, 1       # the same one plane lower
        q[5, 4] = -1                  # alone to the end: the last clean-up pass, in run-length mode where its stripe is whole
        return q
    for band in (hl, lh, hh):
        band[6:14, 6:14] = quiet(8)
    target = rng.integers(1, 255, (lys.stop, lxs.stop)).astype(np.uint8)
    jw.solve_ll(plane, 1, target)
    ll[7:14, 7:14] = quiet(7)     # (LL[i, j] is moved by the detail values at i - 1 .. i, j - 1 .. j: these have quiet ones only)
    out = jr.inverse_dwt(plane.astype(np.int32).copy(), W, H, 1)[::2, ::2] + 128
    assert out.min() >= 1 and out.max() <= 254
    return plane, out.astype(np.uint8)


def shallow_plane(W, H, levels, seed, ll=100, detail=12):
    rng = np.random.default_rng(seed)
    plane = rng.integers(-detail, detail + 1, (H, W)).astype(np.int64)
    _, _, ys, xs = jw.band_slices(W, H, levels)[0]
    plane[ys, xs] = rng.integers(-ll, ll + 1, (ys.stop, xs.stop))
    return plane


def _three_layer_plan(seed):
    """case (d): the inclusion class of a block (first layer 0, 1, 2 or never), the passes of each contribution, the shares of the
    bytes (an empty one in the middle among them) and the extra Lblock increments, all drawn per block"""
    rng = np.random.default_rng(seed)

    def plan(K, need):
        cls = int(rng.integers(0, 4))
        if cls == 3 or need == 0:
            return {"never": True}
        full = 3 * need - 2
        n = full if rng.integers(0, 3) else int(rng.integers(1, full + 1))
        layers = list(range(cls, 3))
        if len(layers) == 3 and rng.integers(0, 3) == 0:
            layers = [0, 2]                               # not included in the middle layer at all
        layers = layers[:n]                               # at least one pass per contribution
        cuts = sorted(rng.choice(np.arange(1, n), size=len(layers) - 1, replace=False).tolist()) if len(layers) > 1 else []
        passes = [b - a for a, b in zip([0] + cuts, cuts + [n])]
        weights = [int(rng.integers(1, 8)) for _ in layers]
        if len(layers) == 3:
            weights[1] = 0 if rng.integers(0, 2) else weights[1]   # passes but no byte in the middle layer
        return {"npasses": n, "split": list(zip(layers, passes, weights)), "extra": {layers[0]: int(rng.integers(0, 3)), layers[-1]: int(rng.integers(0, 2))}}
    return plan


def synthesised():
    if "synthesised" in _BUILT:
        return _BUILT["synthesised"]
    out = []

    def add(name, family, planes, levels, mb, deep=False, full=True, **kw):
        data, report = jw.synth(np.asarray(planes), levels, mb, **kw)
        out.append(Case(name, data, family, irreversible=kw.get("irreversible", False), report=report, deep=deep, full=full))

    p33, _ = deep_plane(33, 31, 1501)
    p64, _ = deep_plane(64, 40, 1502)
    # (a) all four sub-bands at Mb 15: 15 coded planes in LL, 14 in the detail bands
    add("a_deep_33x31", "a", [p33], 1, [15] * 4, deep=True)
    add("a_deep_64x40_cb64x32", "a", [p64], 1, [15] * 4, deep=True, cb=(64, 32))
    # (b) the same, stopped on both sides of the pass-count escape (37 passes and more take the 7-bit form)
    for n in (38, 37, 36, 20):
        add("b_deep_33x31_stop%d" % n, "b", [p33], 1, [15] * 4, deep=True, full=False, plan=lambda K, need, n=n: {"npasses": min(n, 3 * need - 2)})
    # (c) Mb 15 made of zero bit-planes: ordinary coefficients under raised exponents
    small = shallow_plane(33, 31, 1, 1503)
    add("c_zbp_mb15", "c", [small], 1, [15] * 4)
    # (d) 4 x 4 blocks in three layers
    add("d_three_layers_cb4", "d", [shallow_plane(33, 31, 1, 1504, detail=40)], 1, [9, 10, 10, 11], cb=(4, 4), layers=3, plan=_three_layer_plan(1505),
        explicit_empty=True, full=False)
    add("d_three_layers_cb4_rpcl", "d", [shallow_plane(33, 31, 1, 1506, detail=40)], 1, [9, 10, 10, 11], cb=(4, 4), layers=3, order=2,
        plan=_three_layer_plan(1507), full=False)
    # (e) every block's codeword cut to 0, 1 and 3 bytes, all passes announced
    cutp = shallow_plane(33, 31, 1, 1508, ll=200, detail=200)
    for n in (0, 1, 3):
        add("e_cut%d" % n, "e", [cutp], 1, [10] * 4, plan=lambda K, need, n=n: {"cut": n}, full=False)
    # (f) three components, 15 planes in component 0, with and without the reversible colour transform
    colour = [p33, shallow_plane(33, 31, 1, 1509, ll=20, detail=6), shallow_plane(33, 31, 1, 1510, ll=20, detail=6)]
    add("f_rgb_deep_rct", "f", colour, 1, [15] * 4, deep=True, mct=1)
    add("f_rgb_deep_plain", "f", colour, 1, [15] * 4, deep=True, mct=0)
    # (g) two levels at 63 x 65, the HH band of the first level 14 planes deep over its left half
    g = shallow_plane(63, 65, 2, 1511)
    _, _, ys, xs = jw.band_slices(63, 65, 2)[3]
    rng = np.random.default_rng(1512)
    g[ys, xs.start:xs.start + 8] = rng.integers(-DEEP_MAG, DEEP_MAG + 1, (ys.stop - ys.start, 8))
    add("g_two_levels_deep_hh", "g", [g], 2, [10, 11, 11, 15, 11, 11, 12], cb=(32, 32))
    # (h) 9/7 (expounded, mantissa 0, step 2^-6): most indices moderate, one of 15 planes in every block
    rng = np.random.default_rng(1513)
    h = rng.integers(-(1 << 11), (1 << 11) + 1, (31, 33)).astype(np.int64)
    for _, _, ys, xs in jw.band_slices(33, 31, 1):
        h[ys.start + 2, xs.start + 3] = (1 << 15) - 1
        h[ys.start + 5, xs.start + 1] = -(1 << 15) + 3
    add("h_deep_97", "h", [h], 1, [15] * 4, irreversible=True)
    _BUILT["synthesised"] = out
    return out


def accepted():
    return rewritten() + synthesised()


def refused():
    if "refused" in _BUILT:
        return _BUILT["refused"]
    B = bases()
    mb16, _ = jw.synth(np.asarray([shallow_plane(33, 31, 1, 1503)]), 1, [16] * 4)
    out = [Case("c_zbp_mb16", mb16, "refused"),
           Case("grey_layers_33", jw.rewrite(B["grey"][0], extra_layers=32), "refused"),
           Case("rpcl_layers_33", jw.rewrite(B["rpcl"][0], extra_layers=31), "refused"),
           Case("rpcl97_layers_33", jw.rewrite(B["rpcl97"][0], extra_layers=31), "refused", irreversible=True)]
    _BUILT["refused"] = out
    return out


def reference(case):
    """the restatement's (status, reason, info, rgb) of a case, computed once per distinct file of a session"""
    import jp2_irreversible_reference as ir
    return ir.reference(case.data) if case.irreversible else jc.reference(case.data)
