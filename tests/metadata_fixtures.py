"""Fixtures for the source-metadata tests (test_source_metadata.py,
test_gpu_source_metadata.py): ICC profiles built from bytes, a helper that
adds tags to a TIFF written by imaging.tiff_bytes / bigtiff_bytes, and a JP2
box walker.  Nothing here depends on a colour-management library."""
from __future__ import annotations

import struct
from fractions import Fraction

SHORT, LONG, RATIONAL, UNDEFINED, BYTE = 3, 4, 5, 7, 1
ICC, EXTRA, XRES, YRES, UNIT = 34675, 338, 282, 283, 296

RGB_MATRIX_TAGS = (b"rXYZ", b"gXYZ", b"bXYZ", b"rTRC", b"gTRC", b"bTRC")


def icc_profile(space=b"RGB ", cls=b"mntr", pcs=b"XYZ ", tags=None, magic=b"acsp", slack=0,
                size_field=None) -> bytes:
    """An ICC profile from bytes: the 128-byte header, the tag table, 20
    bytes of dummy data per tag, then `slack` bytes past the profile's own
    size field (size_field overrides that field)."""
    if tags is None:
        tags = RGB_MATRIX_TAGS if space == b"RGB " else (b"kTRC",)
    n = len(tags)
    data0 = 132 + 12 * n
    size = data0 + 20 * n
    hdr = bytearray(128)
    hdr[0:4] = struct.pack(">I", size if size_field is None else size_field)
    hdr[4:8] = b"test"
    hdr[8:12] = bytes([4, 0x30, 0, 0])
    hdr[12:16] = cls
    hdr[16:20] = space
    hdr[20:24] = pcs
    hdr[36:40] = magic
    table = struct.pack(">I", n) + b"".join(struct.pack(">4sII", t, data0 + 20 * i, 20) for i, t in enumerate(tags))
    body = b"".join(bytes([0x40 + i]) * 20 for i in range(n))
    return bytes(hdr) + table + body + bytes(range(1, slack + 1))


def rational(e: str, num: int, den: int) -> bytes:
    return struct.pack(e + "II", num, den)


def byte_order(tif: bytes) -> str:
    return "<" if tif[:2] == b"II" else ">"


def add_tags(tif: bytes, tags, drop=()) -> bytes:
    """`tif` (classic or BigTIFF, either byte order) with IFD entries added.

    `tags`: (tag, type, count, payload) with the payload already in the
    file's byte order -- stored inline when it fits, else appended to the
    file -- or (tag, type, count, None, offset) to point the entry at any
    offset (malformed-file fixtures).  Entries whose tag is in `drop` are
    left out.  The new IFD goes at the end of the file; the image data and
    the old entries' offsets stay where they are."""
    e = byte_order(tif)
    big = struct.unpack(e + "H", tif[2:4])[0] == 43
    ifd = struct.unpack(e + "Q", tif[8:16])[0] if big else struct.unpack(e + "I", tif[4:8])[0]
    cnt_fmt, esz, inl, off_fmt = ("Q", 20, 8, "Q") if big else ("H", 12, 4, "I")
    n = struct.unpack(e + cnt_fmt, tif[ifd:ifd + struct.calcsize(cnt_fmt)])[0]
    base = ifd + struct.calcsize(cnt_fmt)
    entries = [tif[base + i * esz: base + (i + 1) * esz] for i in range(n)]
    entries = [x for x in entries if struct.unpack(e + "H", x[:2])[0] not in drop]
    out = bytearray(tif)
    if len(out) % 2:
        out += b"\0"
    for t in tags:
        tag, typ, cnt, payload = t[:4]
        head = struct.pack(e + "HH" + off_fmt, tag, typ, cnt)
        if payload is None:
            val = struct.pack(e + off_fmt, t[4])
        elif len(payload) <= inl:
            val = (payload + b"\0" * inl)[:inl]
        else:
            val = struct.pack(e + off_fmt, len(out))
            out += payload
            if len(out) % 2:
                out += b"\0"
        entries.append(head + val)
    entries.sort(key=lambda x: struct.unpack(e + "H", x[:2])[0])
    new_ifd = len(out)
    out += struct.pack(e + cnt_fmt, len(entries)) + b"".join(entries) + struct.pack(e + off_fmt, 0)
    if big:
        out[8:16] = struct.pack(e + "Q", new_ifd)
    else:
        out[4:8] = struct.pack(e + "I", new_ifd)
    return bytes(out)


def tag_source(tif: bytes, icc: bytes | None = None, xres=None, yres=None, unit: int | None = None) -> bytes:
    """add_tags for the usual case: an ICC profile, X/YResolution as
    (num, den) and ResolutionUnit."""
    e = byte_order(tif)
    tags = []
    if icc is not None:
        tags.append((ICC, UNDEFINED, len(icc), icc))
    if xres is not None:
        tags.append((XRES, RATIONAL, 1, rational(e, *xres)))
    if yres is not None:
        tags.append((YRES, RATIONAL, 1, rational(e, *yres)))
    if unit is not None:
        tags.append((UNIT, SHORT, 1, struct.pack(e + "H", unit)))
    return add_tags(tif, tags)


def boxes(data: bytes, start=0, end=None):
    """[(type, payload)] of the boxes in data[start:end] (32-bit lengths; a
    length of 0 runs to the end)."""
    end = len(data) if end is None else end
    out = []
    p = start
    while p < end:
        n, typ = struct.unpack(">I4s", data[p:p + 8])
        if n == 0:
            n = end - p
        assert n >= 8 and p + n <= end, f"box {typ!r} at {p}: length {n}"
        out.append((typ, data[p + 8:p + n]))
        p += n
    return out


def jp2h_boxes(header: bytes):
    """The boxes inside jp2h of a file header (jp2hip.file_header output: the
    trailing jp2c box header stands for a box that runs past these bytes)."""
    top = []
    p = 0
    while p < len(header):
        n, typ = struct.unpack(">I4s", header[p:p + 8])
        if typ == b"jp2c":
            assert p + 8 == len(header)
            break
        top.append((typ, header[p + 8:p + n]))
        p += n
    assert [t for t, _ in top][:2] == [b"jP  ", b"ftyp"]
    (payload,) = [b for t, b in top if t == b"jp2h"]
    return boxes(payload)


def resc_fields(header: bytes):
    """(VRcN, VRcD, HRcN, HRcD, VRcE, HRcE) of the header's res box, or None."""
    res = [b for t, b in jp2h_boxes(header) if t == b"res "]
    if not res:
        return None
    (inner,) = boxes(res[0])
    assert inner[0] == b"resc" and len(inner[1]) == 10
    return struct.unpack(">HHHHbb", inner[1])


def points_per_metre(num: int, den: int, unit: int) -> Fraction:
    """The exact capture resolution a TIFF rational means (unit 2 inch, 3 cm)."""
    return Fraction(num * 10000, den * 254) if unit == 2 else Fraction(num * 100, den)
