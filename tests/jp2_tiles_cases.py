"""Tiled JPEG 2000 files for the device decoder's tile / precinct / origin path, written by Pillow (OpenJPEG) from a seeded noise image
and a small rendered-text image; T8 and T9 are marker-level edits of them (tests/jp2_tiles_writer.py).  The expected pixels of a file
are always Pillow's own decode (jp2_cases.expected).

accepted() -> [Case(name, group, data, irreversible)]   refusals() -> [(name, data, status, word of the reason)]
damage_bases() / full_sweep(): the files of the damage test and the single-bit flips and truncations of them."""
import collections

import jp2_cases as jc
import jp2_tiles_writer as tw

Case = collections.namedtuple("Case", "name group data irreversible")

ORDERS = ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL")
_CACHE = {}


def _noise(h=201, w=150, mode="RGB", seed=7):
    return jc.content("noise", h, w, mode, seed)


def _text(h=201, w=150):
    return jc.text_page(h, w, seed=11)


def _cut_of(data):
    """-> cut_of(tile, body) for tw.two_parts_interleaved: the end of the middle packet of each tile, from the restatement's walk"""
    import jp2_tiles_reference as tr
    d = bytes(data)
    s, e, box = tr.jr.find_codestream(d)
    P = tr.parse_headers(d, s, e, box, [0] * 8)
    tr.tier2(d, P, tr.geometry(P))
    starts = {t: a for t, a, _ in P.parts}
    return lambda tile, body: P.packet_ends[tile][len(P.packet_ends[tile]) // 2] - starts[tile]


def t1_file():
    if "t1" not in _CACHE:
        _CACHE["t1"] = jc.write(_noise(), irreversible=False, tile_size=(64, 64))
    return _CACHE["t1"]


def accepted():
    if "accepted" in _CACHE:
        return _CACHE["accepted"]
    out = []

    def add(name, group, arr, irreversible=False, **opts):
        out.append(Case(name, group, jc.write(arr, irreversible=irreversible, **opts), irreversible))

    noise, text = _noise(), _text()
    # T1: 12 tiles, the edge tiles 22 wide and 9 high
    out.append(Case("T1_noise", "T1", t1_file(), False))
    add("T1_text", "T1", text, tile_size=(64, 64))
    # T2: odd corners on the lower resolutions
    add("T2_noise", "T2", noise, tile_size=(100, 70), num_resolutions=3)
    add("T2_text_L", "T2", text[:, :, 1].copy(), tile_size=(100, 70), num_resolutions=3)
    # T3: image and tile origins
    add("T3_offsets", "T3", noise, tile_size=(64, 64), offset=(10, 6), tile_offset=(4, 2))
    add("T3_offsets_text", "T3", text, tile_size=(64, 64), offset=(10, 6), tile_offset=(4, 2))
    add("T3_odd_origin", "T3", noise, tile_size=(256, 256), offset=(3, 5))   # one tile, an odd image origin alone
    add("T3_odd_origin_L", "T3", text[:, :, 0].copy(), tile_size=(256, 256), offset=(3, 5), num_resolutions=4)
    # (XTsiz = YTsiz = 2^32 - 1 is legal: a tile count formed as (X - XTO + XT - 1) / XT in 32 bits would wrap to 0)
    out.append(Case("T3_odd_origin_widest_tile", "T3", tw.set_siz(out[-2].data, XT=0xFFFFFFFF, YT=0xFFFFFFFF), False))
    # T4: precincts in every progression order, layered and not
    for prog in ORDERS:
        add(f"T4_{prog}", "T4", noise, precinct_size=(32, 32), codeblock_size=(16, 16), progression=prog)
        add(f"T4_{prog}_layers", "T4", text, precinct_size=(32, 32), codeblock_size=(16, 16), progression=prog, quality_layers=[40, 10, 2])
    # 64 x 64 code-blocks cut to 32 x 32 by their precinct.  (Pillow drops a precinct size that does not exceed the code-block size:
    # precinct_size=(64, 64) with codeblock_size=(64, 64) writes a COD without precinct sizes, a file of the first subset.  With
    # 128 x 128 the COD has them, and the blocks are cut on the resolution whose precincts are 64 x 64.)
    add("T4_cb64_in_p128", "T4", noise, precinct_size=(128, 128), codeblock_size=(64, 64))
    add("T4_cb64_in_p128_layers", "T4", text, precinct_size=(128, 128), codeblock_size=(64, 64), progression="CPRL", quality_layers=[40, 10, 2])
    # T5: tiles of one sample at an odd coordinate (a lone high-pass sample) in x, in y and in both
    add("T5_64x64", "T5", _noise(64, 64, "L", 8), tile_size=(63, 63), num_resolutions=2)
    add("T5_1x64", "T5", _noise(1, 64, "L", 9), tile_size=(63, 63), num_resolutions=2)
    add("T5_64x1", "T5", _noise(64, 1, "L", 10), tile_size=(63, 63), num_resolutions=2)
    add("T5_64x64_RGB", "T5", _noise(64, 64, "RGB", 12), tile_size=(63, 63), num_resolutions=2)
    # T6: tiles with precincts, RPCL, layered
    add("T6_RGB", "T6", text, tile_size=(128, 128), precinct_size=(64, 64), progression="RPCL", quality_layers=[40, 10, 2])
    add("T6_L", "T6", noise[:, :, 0].copy(), tile_size=(128, 128), precinct_size=(64, 64), progression="RPCL", quality_layers=[40, 10, 2])
    # T7: 9/7.  192 x 128 in 64 x 48 and 128 x 128 tiles: no tile-component has a line of one sample above its lowest resolution
    n97, t97 = _noise(128, 192, "RGB", 13), _text(128, 192)
    for ts in ((64, 48), (128, 128)):
        add(f"T7_{ts[0]}x{ts[1]}", "T7", t97, True, tile_size=ts, num_resolutions=4)
        add(f"T7_{ts[0]}x{ts[1]}_q5", "T7", n97, True, tile_size=ts, num_resolutions=4, quality_layers=[5])
    add("T7_precincts", "T7", t97, True, tile_size=(128, 128), precinct_size=(32, 32), codeblock_size=(16, 16), progression="PCRL", num_resolutions=4)
    add("T7_precincts_L", "T7", n97[:, :, 0].copy(), True, precinct_size=(64, 64), progression="RPCL", quality_layers=[20, 5])
    add("T7_offsets", "T7", t97, True, tile_size=(64, 64), offset=(10, 6), tile_offset=(4, 2), num_resolutions=3)
    # T8: the tile-parts of T1 rearranged
    t1 = t1_file()
    cut = _cut_of(t1)
    out.append(Case("T8_reversed", "T8", tw.reverse_tiles(t1), False))
    out.append(Case("T8_two_parts", "T8", tw.two_parts_interleaved(t1, cut), False))
    out.append(Case("T8_two_parts_psot0", "T8", tw.two_parts_interleaved(t1, cut, psot0_last=True), False))
    _CACHE["accepted"] = out
    return out


def one_tile_widest():
    """[(name, bytes)]: one-tile, origin-0 files with XTsiz = YTsiz = 2^32 - 1 and 2^32 - 16, which the older entries take too"""
    base = jc.write(_noise(40, 40, "RGB", 16), irreversible=False)
    return [("widest_tile", tw.set_siz(base, XT=0xFFFFFFFF, YT=0xFFFFFFFF)), ("wide_tile", tw.set_siz(base, XT=0xFFFFFFF0, YT=0xFFFFFFF0))]


def line_of_one_sample():
    """9/7, 130 wide in 64-wide tiles: the last tile is 2 wide, one sample on resolution 4 of 5"""
    return jc.write(_noise(64, 130, "L", 14), irreversible=True, tile_size=(64, 64), num_resolutions=5)


def refusals():
    t1 = t1_file()
    two = tw.two_parts_interleaved(t1, _cut_of(t1))
    prec = next(c.data for c in accepted() if c.name == "T4_LRCP")
    t3 = next(c.data for c in accepted() if c.name == "T3_offsets")
    return [
        ("tiles_4225", tw.set_siz(jc.write(_noise(65, 65, "L", 15), irreversible=False), XT=1, YT=1), -2, "4096 tiles"),
        ("tile_without_part", tw.drop_tile(t1, 5), -1, "without a tile-part"),
        ("tpsot_out_of_order", tw.swap_tpsot(two), -1, "out of order"),
        ("cod_in_tile_part", tw.cod_in_tile_part(t1), -2, "COD marker in a tile-part header"),
        ("ppx_zero", tw.zero_precinct(prec, 1), -1, "precinct of one sample"),
        ("first_tile_empty", tw.set_siz(t3, XO=70), -1, "first tile empty"),
        ("line_of_one_sample_97", line_of_one_sample(), -2, "line of one sample"),
    ]


def damage_bases():
    """[(name, bytes, thin)]: the first two are swept in full.  The third, T1's RGB form at the same size (the component loop of the
    tiled packet walk under damage), is three times the bytes and decodes three times as slowly in the restatement, so it is swept
    thinly; in full it alone took ten minutes."""
    return [
        ("t1_40x40_tiles16", jc.write(jc.content("page", 40, 40, "L", 93), irreversible=False, tile_size=(16, 16), num_resolutions=3), False),
        ("t4_precincts", jc.write(jc.content("page", 33, 40, "L", 94), irreversible=False, precinct_size=(16, 16), codeblock_size=(8, 8),
                                  progression="RPCL", quality_layers=[10, 2], num_resolutions=3), False),
        ("t1_rgb_40x40_tiles16", jc.write(jc.content("page", 40, 40, "RGB", 93), irreversible=False, tile_size=(16, 16)), True),
    ]


def damage_sweep(base, thin=False):
    """[(name, bytes)]: every single-bit flip and every truncation; thin: every bit up to the first SOD (the boxes, the main header and
    the first tile-part header), every 17th bit after it, truncation at every 8th byte"""
    out = []
    hdr = jc.data_start(base) * 8
    for bit in range(len(base) * 8):
        if thin and bit >= hdr and (bit - hdr) % 17:
            continue
        b = bytearray(base)
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((f"b{bit}", bytes(b)))
    for n in range(0, len(base), 8 if thin else 1):
        out.append((f"t{n}", base[:n]))
    return out


def full_sweep():
    if "sweep" not in _CACHE:
        _CACHE["sweep"] = [(bname, name, data) for bname, base, thin in damage_bases() for name, data in damage_sweep(base, thin)]
    return _CACHE["sweep"]
