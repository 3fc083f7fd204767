"""The JBIG2 pages the tests share, made by tests/jbig2_writer.py: intact pages with the source bitmap they must decode to, refused
pages with the status and reason they must get, and the damage sweep of two small streams.  Everything is seeded and computed once."""
import functools
import struct
from collections import namedtuple

import numpy as np

import jbig2_reference as jr
import jbig2_writer as jw

Case = namedtuple("Case", "name stream globals_data bits")          # bits: uint8 [H][W], 1 = black, the page the stream was made from
Refusal = namedtuple("Refusal", "name stream globals_data status reason")


def bitmap(w, h, seed, density=0.3, repeat=0.3):
    """a seeded bitmap with runs of equal rows (typical prediction has something to predict) and an empty first row now and then"""
    rng = np.random.default_rng(seed)
    bm = (rng.random((h, w)) < density).astype(np.uint8)
    # smear horizontally so that the contexts have something to learn
    bm[:, 1:] |= bm[:, :-1] & (rng.random((h, w - 1)) < 0.5) if w > 1 else 0
    for y in range(h):
        if rng.random() < repeat:
            bm[y] = bm[y - 1] if y else 0
    return bm


def compose(width, height, regions, default_pixel=0):
    """the page the regions make, from the source bitmaps (numpy, independent of the restatement's combine)"""
    bits = np.full((height, width), default_pixel, np.uint8)
    for r in regions:
        bm = np.asarray(r["bitmap"]).astype(np.uint8)
        x, y, op = r.get("x", 0), r.get("y", 0), r.get("op", jw.OR)
        h, w = min(bm.shape[0], height - y), min(bm.shape[1], width - x)
        dst, src = bits[y:y + h, x:x + w], bm[:h, :w]
        if op == jw.OR:
            dst |= src
        elif op == jw.AND:
            dst &= src
        elif op == jw.XOR:
            dst ^= src
        elif op == jw.XNOR:
            dst[...] = 1 - (dst ^ src)
        else:
            dst[...] = src
    return bits


def _one(name, w, h, seed, **region):
    bm = bitmap(w, h, seed)
    return Case(name, jw.page(w, h, [dict(bitmap=bm, **region)]), None, bm)


# AT pixels moved off their nominal places, per template: for T0 one at y = 0 and one far up among them
MOVED_AT = {0: [(-5, 0), (4, -1), (-2, -3), (1, -2)], 1: [(-4, 0)], 2: [(3, -2)], 3: [(-6, -1)]}

# the sizes of the issue (width x height): the word and wave edges, nothing larger
SIZES = [(1, 1), (1, 40), (40, 1), (31, 5), (32, 5), (33, 5), (63, 4), (64, 4), (65, 4), (70, 37), (129, 64), (64, 129), (8192, 3)]


@functools.lru_cache(maxsize=None)
def intact():
    out = []
    seed = 8800
    # every template x TPGDON on and off x nominal and moved AT pixels
    for tmpl in range(4):
        for tpgd in (False, True):
            for moved in (False, True):
                seed += 1
                out.append(_one(f"t{tmpl}_tpgd{int(tpgd)}_{'moved' if moved else 'nominal'}_70x37", 70, 37, seed, tmpl=tmpl, tpgd=tpgd,
                                at=MOVED_AT[tmpl] if moved else None))
    # AT at y = 0 with x = -1 and x = -128, and at y = -128 (a row of the plane long finished)
    out.append(_one("t0_at_y0_x-1", 129, 64, 8901, tmpl=0, at=[(-1, 0), (-3, -1), (2, -2), (-2, -2)]))
    out.append(_one("t0_at_y0_x-128", 129, 64, 8902, tmpl=0, tpgd=True, at=[(-128, 0), (-3, -1), (2, -2), (-2, -2)]))
    out.append(_one("t1_at_y0_x-128", 129, 64, 8903, tmpl=1, at=[(-128, 0)]))
    out.append(_one("t0_at_y-128", 64, 129, 8904, tmpl=0, at=[(3, -1), (-3, -1), (127, -128), (-128, -128)]))
    out.append(_one("t3_at_y-128", 64, 129, 8905, tmpl=3, tpgd=True, at=[(0, -128)]))
    # sizes
    for k, (w, h) in enumerate(SIZES):
        tmpl = k % 4
        out.append(_one(f"size_{w}x{h}_t{tmpl}", w, h, 9000 + k, tmpl=tmpl, tpgd=bool(k & 1)))
    out.append(_one("size_8192x3_t0_general", 8192, 3, 9050, tmpl=0, at=[(3, -1), (-3, -1), (2, -2), (-3, -2)]))
    # MMR
    for k, (w, h) in enumerate([(1, 1), (33, 5), (70, 37), (129, 64)]):
        out.append(_one(f"mmr_{w}x{h}", w, h, 9100 + k, mmr=True))
    # every operator on overlapping regions, both default pixels, regions sticking out of the page
    for dp in (0, 1):
        regions = [dict(bitmap=bitmap(50, 30, 9200 + dp), x=3, y=2, op=jw.REPLACE, tmpl=0)]
        for k, op in enumerate((jw.OR, jw.AND, jw.XOR, jw.XNOR, jw.REPLACE)):
            regions.append(dict(bitmap=bitmap(33 + 7 * k, 17 + k, 9210 + 10 * dp + k), x=5 + 9 * k, y=1 + 5 * k, op=op, tmpl=k % 4, tpgd=bool(k & 1)))
        regions.append(dict(bitmap=bitmap(40, 25, 9230 + dp), x=45, y=28, op=jw.XOR, mmr=True))          # sticks out right and below
        regions.append(dict(bitmap=bitmap(64, 9, 9240 + dp), x=69, y=0, op=jw.OR, tmpl=2))                # one column on the page
        out.append(Case(f"operators_default{dp}", jw.page(70, 37, regions, default_pixel=dp), None, compose(70, 37, regions, dp)))
    # a default operator that may not be overridden, kept by every region
    regions = [dict(bitmap=bitmap(20, 10, 9250), x=1, y=1, op=jw.XOR), dict(bitmap=bitmap(20, 10, 9251), x=8, y=4, op=jw.XOR, tmpl=3)]
    out.append(Case("no_override_kept", jw.page(33, 16, regions, default_op=jw.XOR, override=False), None, compose(33, 16, regions)))
    # striped pages with unknown height
    bm = bitmap(65, 40, 9300)
    stripes = [dict(bitmap=bm[0:16], y=0, tmpl=0, tpgd=True), dict(bitmap=bm[16:32], y=16, tmpl=1), dict(bitmap=bm[32:40], y=32, mmr=True)]
    out.append(Case("striped_unknown_height", jw.page(65, 40, stripes, stripes=[15, 31, 39], unknown_height=True, end_of_page=False), None, bm))
    out.append(Case("striped_known_height", jw.page(65, 40, stripes, stripes=[15, 31, 39]), None, bm))
    # a last stripe shorter than its region: the region is clipped at the page's bottom
    out.append(Case("striped_clipped", jw.page(65, 36, stripes, stripes=[15, 31, 35], unknown_height=True), None, bm[:36]))
    # globals: the page information and the first region split off
    regions = [dict(bitmap=bitmap(70, 20, 9400), tmpl=0), dict(bitmap=bitmap(70, 17, 9401), y=20, tmpl=2, tpgd=True)]
    g, rest = jw.split_globals(jw.page(70, 37, regions), 2)
    out.append(Case("globals_page_and_region", rest, g, compose(70, 37, regions)))
    g, rest = jw.split_globals(jw.page(70, 37, regions), 1)
    out.append(Case("globals_page_only", rest, g, compose(70, 37, regions)))
    # header field widths: segment number 300 with 2-byte references, the long referred-to count, a 4-byte page association; lossy
    # type 38; profiles and extension segments are skipped; bytes after the end of page are not read
    bm = bitmap(33, 9, 9500)
    r = [dict(bitmap=bm, tmpl=1)]
    out.append(Case("header_number_300_refs", jw.page(33, 9, r, first_number=300, refs=(7, 299)), None, bm))
    out.append(Case("header_number_70000_refs", jw.page(33, 9, r, first_number=70000, refs=(7, 65537, 3)), None, bm))
    out.append(Case("header_long_count", jw.page(33, 9, r, long_count=True, refs=(1, 2, 3, 4, 5, 6, 7, 8, 9)), None, bm))
    out.append(Case("header_page4", jw.page(33, 9, r, page4=True), None, bm))
    out.append(Case("type38", jw.page(33, 9, r, lossless=False), None, bm))
    s = jw.page(33, 9, r, end_of_page=False)
    out.append(Case("skipped_52_62_then_51", s + jw.segment(5, 52, b"\0\0\0\1" + b"\0" * 20) + jw.segment(6, 62, b"\x20\0\0\0hello", page=0)
                    + jw.segment(7, 51, b"", page=0) + b"\xde\xad", None, bm))
    return out


def _with_region_header(bm, **kw):
    return jw.segment(1, 39, jw.region_data(bm, **kw))


@functools.lru_cache(maxsize=None)
def refused():
    bm = bitmap(20, 6, 9600)
    info = jw.segment(0, 48, jw.page_info(20, 6))
    region = jw.segment(1, 39, jw.region_data(bm))
    eop = jw.segment(2, 49, b"")
    out = []
    add = lambda name, stream, status, reason, g=None: out.append(Refusal(name, stream, g, status, reason))
    # ---- -2: valid JBIG2 that is not read
    for typ, why in sorted(jr.OUTSIDE.items()):
        add(f"type_{typ}", info + jw.segment(1, typ, b"\0" * 12, page=0 if typ in (0, 16, 53) else 1) + eop, -2, why)
    add("symbol_dictionary_in_globals", info + region + eop, -2, "symbol dictionary", g=jw.segment(0, 0, b"\0" * 12, page=0))
    add("unknown_length", info + jw.segment(1, 38, jw.region_data(bm), length=0xFFFFFFFF) + eop, -2, "a segment of unknown length")
    add("exttemplate", info + _with_region_header(bm, generic_flags_extra=0x10) + eop, -2, "extended template (EXTTEMPLATE)")
    add("region_8193_wide", jw.segment(0, 48, jw.page_info(8192, 2)) + _with_region_header(bitmap(4, 2, 1), width=8193) + eop, -2, "region wider than 8192")
    add("page_8193_wide", jw.segment(0, 48, jw.page_info(8193, 2)) + eop, -2, "page wider than 8192")
    tiny = jw.region_data(np.ones((1, 1), np.uint8), tmpl=2)
    add("257_regions", info + b"".join(jw.segment(1 + k, 39, tiny) for k in range(257)) + eop, -2, "more than 256 regions on the page")
    add("page_association_2", info + jw.segment(1, 39, jw.region_data(bm), page=2) + eop, -2, "a segment of another page than page 1")
    add("second_page_information", info + region + info + eop, -2, "a second page information segment")
    # ---- -1: corrupt or irregular
    add("header_past_stream", info + region[:9], -1, "segment header past the stream")
    add("references_past_stream", info + jw.segment(300, 39, jw.region_data(bm), long_count=True, refs=(1,) * 40)[:30], -1, "segment header past the stream")
    add("length_past_stream", info + region[:-1], -1, "segment data past the stream")
    add("region_before_page", region + info + eop, -1, "a region before the page information")
    add("region_right_of_page", info + _with_region_header(bm, x=20) + eop, -1, "a region that does not meet the page")
    add("region_below_page", info + _with_region_header(bm, y=6) + eop, -1, "a region that does not meet the page")
    add("operator_overridden", jw.segment(0, 48, jw.page_info(20, 6, default_op=jw.OR, override=False)) + _with_region_header(bm, op=jw.XOR) + eop, -1,
        "a region operator other than the page's, which forbids overriding")
    add("reserved_page_flag", jw.segment(0, 48, jw.page_info(20, 6, flags_extra=0x80)) + region + eop, -1, "reserved page flag bits")
    add("reserved_region_flag", info + _with_region_header(bm, region_flags_extra=0x10) + eop, -1, "reserved region flag bits")
    add("operator_5", info + _with_region_header(bm, region_flags_extra=5) + eop, -1, "reserved region flag bits")
    add("reserved_generic_flag", info + _with_region_header(bm, generic_flags_extra=0x40) + eop, -1, "reserved generic region flag bits")
    for name, at in (("at_after_x0", [(0, 0)]), ("at_after_x5", [(5, 0)]), ("at_below", [(-1, 1)])):
        hdr = struct.pack(">IIIIBB", 20, 6, 0, 0, 0, 2 << 1) + struct.pack(">bb", *at[0])
        add(name, info + jw.segment(1, 39, hdr + jw.encode_generic(bm, 2)) + eop, -1, "an adaptive template pixel that is not before the current pixel")
    add("undefined_type_1", info + jw.segment(1, 1, b"") + eop, -1, "a segment type that T.88 does not define")
    add("undefined_type_63", info + jw.segment(1, 63, b"") + eop, -1, "a segment type that T.88 does not define")
    add("unknown_height_no_stripe", jw.segment(0, 48, jw.page_info(20, None, striped=True)) + region + eop, -1, "unknown page height without an end of stripe")
    add("no_page_information", jw.segment(0, 52, b"\0\0\0\0") + eop, -1, "no page information")
    add("empty_region", info + _with_region_header(bm, width=0) + eop, -1, "an empty region")
    add("short_page_information", jw.segment(0, 48, jw.page_info(20, 6)[:18]) + eop, -1, "page information of the wrong length")
    add("referred_count_5", info + region[:5] + bytes([5 << 5]) + region[6:] + eop, -1, "reserved referred-to segment count")
    return out


@functools.lru_cache(maxsize=None)
def sweep_bases():
    """name -> (stream, bits): the two small streams of the damage sweep, one arithmetic (typical prediction on), one MMR"""
    a, m = bitmap(16, 8, 9700), bitmap(16, 8, 9701)
    return {"arithmetic": (jw.page(16, 8, [dict(bitmap=a, tmpl=0, tpgd=True)]), a), "mmr": (jw.page(16, 8, [dict(bitmap=m, mmr=True)]), m)}


@functools.lru_cache(maxsize=None)
def damage_sweep():
    """[(base name, label, damaged stream)]: every single-bit flip and every truncation of the two bases"""
    out = []
    for name, (stream, _) in sweep_bases().items():
        for bit in range(len(stream) * 8):
            d = bytearray(stream)
            d[bit >> 3] ^= 0x80 >> (bit & 7)
            out.append((name, f"flip{bit}", bytes(d)))
        for n in range(len(stream)):
            out.append((name, f"cut{n}", stream[:n]))
    return out


@functools.lru_cache(maxsize=None)
def sweep_restatement():
    """[(status, info, bits or None)] of the restatement over damage_sweep(); bits only for pages of the bases' size"""
    out = []
    for name, _, d in damage_sweep():
        st, info, _ = jr.probe(d)
        bits = None
        if st == 0 and (info[0], info[1]) == (16, 8):
            st, bits = jr.page_bits(d)
        out.append((st, info, bits))
    return out


def sweep_sample(count=64, seed=8864):
    """indices into damage_sweep(): a seeded sample, half of it from each base"""
    rng = np.random.default_rng(seed)
    sweep = damage_sweep()
    idx = []
    for name in sweep_bases():
        own = [i for i, s in enumerate(sweep) if s[0] == name]
        idx += sorted(rng.choice(own, count // 2, replace=False).tolist())
    return idx
