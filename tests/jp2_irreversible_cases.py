"""Seeded 9/7 (irreversible) JPEG 2000 files, written by Pillow (OpenJPEG) with irreversible=True.  The expected pixels of a file are
always Image.open(BytesIO(file)).convert('RGB') (jp2_cases.expected).

intact() -> [(name, bytes)]: files the irreversible entry points read (status 0).   refused() -> [(name, bytes, word of the reason)].
damage_bases() / full_sweep() / sweep_sample(): two 9/7 files and every damaged variant of them (jp2_cases.damage_sweep)."""
import numpy as np

import jp2_cases as jc


def intact():
    out = []

    def add(name, kind, h, w, mode, seed=1, **opts):
        out.append((name, jc.write(jc.content(kind, h, w, mode, seed), irreversible=True, **opts)))

    # sides (the smallest of each level count: no resolution from 1 upwards may have a side of one sample)
    add("s5x5_L_r3", "noise", 5, 5, "L", num_resolutions=3)
    add("s5x5_RGB_r3", "noise", 5, 5, "RGB", num_resolutions=3)
    add("s17x9_L_r4", "noise", 17, 9, "L", num_resolutions=4)
    add("s17x9_RGB_r4", "page", 17, 9, "RGB", num_resolutions=4)
    for h, w in ((63, 65), (64, 64), (65, 63), (129, 64), (100, 130)):
        add(f"s{h}x{w}_RGB", "page", h, w, "RGB", seed=h)
        add(f"s{h}x{w}_L", "page", h, w, "L", seed=w)
    # resolutions (6 = five decomposition levels, the writer's default and the most whose LL band stays within 15 bit-planes)
    for nr in (1, 2, 3, 4, 5, 6):
        add(f"res{nr}_RGB", "page", 100, 130, "RGB", seed=10 + nr, num_resolutions=nr)
        add(f"res{nr}_L_noise", "noise", 129, 64, "L", seed=20 + nr, num_resolutions=nr)
    # code-block sizes
    for cb in ((4, 4), (8, 64), (64, 8), (32, 32), (64, 64)):
        add(f"cb{cb[0]}x{cb[1]}_RGB", "page", 63, 65, "RGB", seed=30 + cb[0], codeblock_size=cb, num_resolutions=3)
        add(f"cb{cb[0]}x{cb[1]}_L", "noise", 65, 63, "L", seed=31 + cb[1], codeblock_size=cb, num_resolutions=3)
    # component transform
    for mct in (0, 1):
        add(f"mct{mct}", "noise", 64, 64, "RGB", seed=40, mct=mct)
        add(f"mct{mct}_page", "page", 100, 130, "RGB", seed=41, mct=mct)
    # progression orders, two layers
    for prog in ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL"):
        add(f"prog_{prog}", "page", 63, 65, "RGB", seed=50, progression=prog, quality_layers=[10, 2], num_resolutions=4)
        add(f"prog_{prog}_L", "noise", 65, 63, "L", seed=51, progression=prog, quality_layers=[10, 2], num_resolutions=3, codeblock_size=(16, 16))
    # layers: blocks that stop early
    for mode in ("RGB", "L"):
        add(f"layers_rate_{mode}", "page", 100, 130, mode, seed=60, quality_layers=[40, 20, 5])
        add(f"layers_rate_noise_{mode}", "noise", 64, 64, mode, seed=61, quality_layers=[40, 20, 5])
        add(f"layers_db_{mode}", "page", 100, 130, mode, seed=62, quality_mode="dB", quality_layers=[30, 40])
        add(f"layers_db_noise_{mode}", "noise", 63, 65, mode, seed=63, quality_mode="dB", quality_layers=[30, 40])
    # container and markers
    add("no_jp2_RGB", "page", 63, 65, "RGB", seed=70, no_jp2=True)
    add("no_jp2_L", "page", 65, 63, "L", seed=71, no_jp2=True)
    add("plt_RGB", "page", 63, 65, "RGB", seed=72, plt=True)
    add("plt_layers_L", "page", 65, 63, "L", seed=73, plt=True, quality_layers=[20, 4])
    # contents
    for kind in ("white", "flat0", "flat255", "noise"):
        add(f"c_{kind}_RGB", kind, 64, 64, "RGB", seed=80)
        add(f"c_{kind}_L", kind, 65, 63, "L", seed=81)
    page = jc.text_page()
    out.append(("text_page_RGB", jc.write(page, irreversible=True)))
    out.append(("text_page_L_layers", jc.write(page[:, :, 1].copy(), irreversible=True, quality_layers=[20, 5])))
    return out


def flipped_transform(data):
    """a 5/3 file with the transform byte of its COD set to 0 (9/7): the QCD keeps style 0"""
    p = data.index(b"\xff\x52")
    assert data[p + 13] == 1
    return data[:p + 13] + b"\x00" + data[p + 14:]


def refused():
    a = jc.content("page", 100, 130, "RGB", 3)
    return [
        ("res7", jc.write(a, irreversible=True, num_resolutions=7), "magnitude bit-planes"),
        ("flipped_transform", flipped_transform(jc.write(a, irreversible=False)), "derived or no quantisation"),
    ]


def damage_bases():
    return [
        ("rgb97_layers", jc.write(jc.content("page", 33, 40, "RGB", 90), irreversible=True, mct=1, quality_layers=[10, 2], num_resolutions=3)),
        ("grey97_layers", jc.write(jc.content("page", 48, 48, "L", 91), irreversible=True, quality_layers=[4], num_resolutions=4)),
    ]


_SWEEP = []


def full_sweep():
    """[(base name, case name, bytes)] over the two bases, built once"""
    if not _SWEEP:
        for bname, base in damage_bases():
            _SWEEP.extend((bname, name, data) for name, data in jc.damage_sweep(base))
    return _SWEEP


def sweep_sample(count, seed):
    """a seeded sample of the sweep, in sweep order"""
    sweep = full_sweep()
    pick = np.random.default_rng(seed).choice(len(sweep), size=count, replace=False)
    return [sweep[int(i)] for i in sorted(pick)]
