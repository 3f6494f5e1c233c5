"""A plain NumPy / Python PNG decoder and a tiny encoder for the loader tests: slow, but every step is the PNG specification read aloud.

    encode(samples, bit_depth, colour_type, filters=..., palette=..., idat_split=..., interlace=0) -> bytes of a PNG file
    decode(data) -> dict(width, height, bit_depth, colour_type, palette, samples)     samples: integer array [H, W, channels]
    grey8(decoded) -> uint8 [H, W]      the 8-bit grey value cv2.imread(path, 0) gives

The encoder lets the test choose the filter type of every row and where the IDAT stream is cut into chunks.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(ctype: bytes, body: bytes) -> bytes:
    return struct.pack('>I', len(body)) + ctype + body + struct.pack('>I', zlib.crc32(ctype + body) & 0xffffffff)


def pack_rows(samples: np.ndarray, bit_depth: int) -> list:
    """[H, W, C] integer samples -> the H scanlines as lists of byte values (most significant bits first, 16 bits big-endian)."""
    rows = []
    for row in samples.reshape(samples.shape[0], -1):
        if bit_depth == 16:
            out = []
            for s in row:
                out += [int(s) >> 8, int(s) & 0xff]
        elif bit_depth == 8:
            out = [int(s) for s in row]
        else:
            per = 8 // bit_depth
            out = [0] * ((len(row) + per - 1) // per)
            for i, s in enumerate(row):
                out[i // per] |= int(s) << (8 - bit_depth - (i % per) * bit_depth)
        rows.append(out)
    return rows


def _paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def _predict(ft: int, left: int, up: int, upleft: int) -> int:
    return (0, left, up, (left + up) // 2, _paeth(left, up, upleft))[ft]


def filter_rows(rows: list, bpp: int, filters) -> bytes:
    out, prev = bytearray(), None
    for r, row in enumerate(rows):
        ft = filters[r % len(filters)]
        out.append(ft)
        for i, x in enumerate(row):
            left = row[i - bpp] if i >= bpp else 0
            up = prev[i] if prev is not None else 0
            upleft = prev[i - bpp] if (prev is not None and i >= bpp) else 0
            out.append((x - _predict(ft, left, up, upleft)) & 0xff)
        prev = row
    return bytes(out)


def encode(samples: np.ndarray, bit_depth: int, colour_type: int, filters=(0,), palette: bytes = None, idat_split: int = None,
           interlace: int = 0, level: int = 6) -> bytes:
    samples = np.asarray(samples)
    if samples.ndim == 2:
        samples = samples[..., None]
    h, w, c = samples.shape
    assert c == CHANNELS[colour_type]
    bpp = max(1, c * bit_depth // 8)
    stream = zlib.compress(filter_rows(pack_rows(samples, bit_depth), bpp, filters), level)
    out = SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, bit_depth, colour_type, 0, 0, interlace))
    if palette is not None:
        out += chunk(b'PLTE', palette)
    cut = len(stream) if not idat_split else idat_split
    for i in range(0, len(stream), cut):
        out += chunk(b'IDAT', stream[i:i + cut])
    return out + chunk(b'IEND', b'')


def decode(data: bytes) -> dict:
    assert data[:8] == SIGNATURE
    pos, idat, palette, ihdr = 8, b'', None, None
    while pos < len(data):
        length, ctype = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        assert zlib.crc32(ctype + body) & 0xffffffff == struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])[0]
        pos += 12 + length
        if ctype == b'IHDR':
            ihdr = struct.unpack('>IIBBBBB', body)
        elif ctype == b'PLTE':
            palette = body
        elif ctype == b'IDAT':
            idat += body
        elif ctype == b'IEND':
            break
    w, h, depth, colour, _, _, interlace = ihdr
    assert interlace == 0
    c = CHANNELS[colour]
    rb = (w * c * depth + 7) // 8
    bpp = max(1, c * depth // 8)
    raw = zlib.decompress(idat)
    assert len(raw) == h * (rb + 1)
    rows, prev = [], None
    for r in range(h):
        line = raw[r * (rb + 1):(r + 1) * (rb + 1)]
        ft, row = line[0], []
        assert ft <= 4
        for i in range(rb):
            left = row[i - bpp] if i >= bpp else 0
            up = prev[i] if prev is not None else 0
            upleft = prev[i - bpp] if (prev is not None and i >= bpp) else 0
            row.append((line[1 + i] + _predict(ft, left, up, upleft)) & 0xff)
        rows.append(row)
        prev = row
    samples = np.zeros((h, w * c), dtype=np.int64)
    for r, row in enumerate(rows):
        for i in range(w * c):
            if depth == 16:
                samples[r, i] = (row[2 * i] << 8) | row[2 * i + 1]
            elif depth == 8:
                samples[r, i] = row[i]
            else:
                per = 8 // depth
                samples[r, i] = (row[i // per] >> (8 - depth - (i % per) * depth)) & ((1 << depth) - 1)
    return dict(width=w, height=h, bit_depth=depth, colour_type=colour, palette=palette, samples=samples.reshape(h, w, c),
                raw=np.array(rows, dtype=np.uint8).reshape(h, rb))


def luma(r, g, b):
    """OpenCV's 8-bit BGR -> grey: 14-bit fixed point, rounded."""
    return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14


def grey8(dec: dict) -> np.ndarray:
    s, depth, colour = dec['samples'], dec['bit_depth'], dec['colour_type']
    if colour == 0:
        g = s[..., 0] >> 8 if depth == 16 else s[..., 0] * (255 // ((1 << depth) - 1))
    elif colour == 3:
        pal = np.frombuffer(dec['palette'], dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        rgb = pal[s[..., 0]]
        g = luma(rgb[..., 0], rgb[..., 1], rgb[..., 2])
    elif colour in (2, 6) and depth == 8:
        g = luma(s[..., 0], s[..., 1], s[..., 2])
    else:
        raise ValueError("no grey rule for colour type %d at %d bits" % (colour, depth))
    return g.astype(np.uint8)
