"""Marker-level edits of tiled JPEG 2000 files (test side only): the codestream is split at its SOT markers and put together again with
the tile-parts in another order, cut in two at a packet boundary, or with single header bytes changed.  No packet is re-encoded."""


def _u16(v):
    return int(v).to_bytes(2, "big")


def _u32(v):
    return int(v).to_bytes(4, "big")


def _be(d, p, n):
    return int.from_bytes(d[p:p + n], "big")


def split(data):
    """-> (prefix, main_header, parts, suffix): prefix = everything before SOC (the boxes, or b''), main_header = SOC up to the first
    SOT, parts = [dict(tile, tp, tn, header (the marker segments between SOT and SOD), body)], suffix = EOC.  The codestream must be
    the last box and its box length is patched by join()."""
    s = data.index(b"\xff\x4f\xff\x51")
    p = s + 4
    p += _be(data, p, 2)
    while _be(data, p, 2) != 0xFF90:
        p += 2 + _be(data, p + 2, 2)
    main = data[s:p]
    parts = []
    while _be(data, p, 2) == 0xFF90:
        isot, psot, tp, tn = _be(data, p + 4, 2), _be(data, p + 6, 4), data[p + 10], data[p + 11]
        end = p + psot if psot else len(data) - 2
        q = p + 12
        while _be(data, q, 2) != 0xFF93:
            q += 2 + _be(data, q + 2, 2)
        parts.append(dict(tile=isot, tp=tp, tn=tn, header=data[p + 12:q], body=data[q + 2:end]))
        p = end
    assert data[p:] == b"\xff\xd9", "the codestream must end the file"
    return data[:s], main, parts, data[p:]


def join(prefix, main, parts, suffix, psot0_last=False):
    cs = bytearray(main)
    for i, t in enumerate(parts):
        ln = 12 + len(t["header"]) + 2 + len(t["body"])
        if psot0_last and i == len(parts) - 1:
            ln = 0
        cs += b"\xff\x90" + _u16(10) + _u16(t["tile"]) + _u32(ln) + bytes([t["tp"], t["tn"]]) + t["header"] + b"\xff\x93" + t["body"]
    cs += suffix
    if not prefix:
        return bytes(cs)
    # the last box is jp2c: a 4-byte length (or 0 = to the end of the file) followed by 'jp2c'
    assert prefix[-4:] == b"jp2c"
    head = bytearray(prefix)
    if _be(head, len(head) - 8, 4) != 0:
        head[-8:-4] = _u32(8 + len(cs))
    return bytes(head) + bytes(cs)


def reverse_tiles(data):
    prefix, main, parts, suffix = split(data)
    return join(prefix, main, parts[::-1], suffix)


def two_parts_interleaved(data, cut_of, psot0_last=False):
    """each tile's (only) tile-part cut in two at cut_of(tile index, body) (a packet boundary), then all first parts, then all second
    parts in reverse tile order"""
    prefix, main, parts, suffix = split(data)
    first, second = [], []
    for t in parts:
        assert t["tp"] == 0
        k = cut_of(t["tile"], t["body"])
        first.append(dict(t, tp=0, tn=2, body=t["body"][:k]))
        second.append(dict(t, tp=1, tn=2, header=b"", body=t["body"][k:]))
    return join(prefix, main, first + second[::-1], suffix, psot0_last=psot0_last)


def drop_tile(data, tile):
    prefix, main, parts, suffix = split(data)
    return join(prefix, main, [t for t in parts if t["tile"] != tile], suffix)


def swap_tpsot(data):
    """two_parts_interleaved with the TPsot of tile 0's parts exchanged"""
    prefix, main, parts, suffix = split(data)
    for t in parts:
        if t["tile"] == 0:
            t["tp"] = 1 - t["tp"]
    return join(prefix, main, parts, suffix)


def cod_in_tile_part(data):
    """the main header's COD repeated in the header of the first tile-part"""
    prefix, main, parts, suffix = split(data)
    p = main.index(b"\xff\x52")
    cod = main[p:p + 2 + _be(main, p + 2, 2)]
    parts[0] = dict(parts[0], header=cod + parts[0]["header"])
    return join(prefix, main, parts, suffix)


def zero_precinct(data, r=1):
    """PPx of resolution r set to 0 in a COD that carries precinct sizes"""
    p = data.index(b"\xff\x52")
    assert data[p + 4] & 1, "the COD must carry precinct sizes"
    b = bytearray(data)
    b[p + 14 + r] &= 0xF0
    return bytes(b)


def set_siz(data, **fields):
    """SIZ fields by name: X, Y, XO, YO, XT, YT, XTO, YTO"""
    off = dict(X=4, Y=8, XO=12, YO=16, XT=20, YT=24, XTO=28, YTO=32)
    p = data.index(b"\xff\x4f\xff\x51") + 4
    b = bytearray(data)
    for k, v in fields.items():
        b[p + off[k]:p + off[k] + 4] = _u32(v)
    return bytes(b)
