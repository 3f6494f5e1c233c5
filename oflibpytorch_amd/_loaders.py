"""Dataset files for Flow.from_kitti / Flow.from_sintel and load_kitti / load_sintel / load_sintel_mask (reference
flow_class.py:330-374, utils.py:810-875) -- without OpenCV or PIL.

Host: the PNG container is parsed here (chunks, CRCs, IHDR / PLTE / IDAT), the IDAT stream is inflated by `zlib`, the scanline filters
are undone by `ofl_png_unfilter` (plain C++ in libofl_hip.so), and the Sintel mask's 8-bit grey value is formed by `ofl_png_grey8`.
Device: `ofl_decode_kitti` / `ofl_decode_flo` turn the raw samples of the whole batch into flow planes, mask and flag words in one
launch (`_native.decode_kitti` / `decode_flo`).

Supported: non-interlaced PNGs; KITTI flow = colour type 2 (R G B) at 16 bits; masks = grey at 1 / 2 / 4 / 8 / 16 bits, palette,
8-bit R G B and R G B A.  Everything else raises ValueError saying what it is.
Extension: every `path` may be a list / tuple of paths of equally sized frames; they come back as one batch.
"""
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _native

PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
MAX_WORKERS = 16            # files of a batch decoded side by side (inflate and unfilter release the GIL); a fixed bound, not the core count
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
_MAX_SIDE = 1 << 24


class PngError(ValueError):
    """The bytes are not a PNG this decoder can read: malformed (`unsupported` False) or a feature it leaves out (True)."""

    def __init__(self, message: str, unsupported: bool = False):
        ValueError.__init__(self, message)
        self.unsupported = unsupported


class PngImage(object):
    """A decoded PNG: IHDR fields, the palette (bytes or None) and `raw`, the unfiltered scanlines uint8 [height, row_bytes] with the
    samples as the file stores them (16-bit ones big-endian)."""
    __slots__ = ('width', 'height', 'bit_depth', 'colour_type', 'palette', 'raw')

    @property
    def channels(self) -> int:
        return _CHANNELS[self.colour_type]


def parse_png(data: bytes):
    """Container level: (width, height, bit_depth, colour_type, palette or None, the concatenated IDAT bytes).  Every chunk's length
    and CRC are checked; IHDR must come first, IDAT chunks must be consecutive, IEND must end the file's chunks."""
    if len(data) < 8 or data[:8] != PNG_SIGNATURE:
        raise PngError("not a PNG file (signature)")
    pos, ihdr, palette, idat, idat_done, ended = 8, None, None, [], False, False
    while pos < len(data):
        if len(data) - pos < 12:
            raise PngError("truncated PNG chunk header")
        length, ctype = struct.unpack('>I4s', data[pos:pos + 8])
        if length > len(data) - pos - 12:
            raise PngError("PNG chunk %r runs past the end of the file" % ctype)
        body = data[pos + 8:pos + 8 + length]
        if zlib.crc32(body, zlib.crc32(ctype)) & 0xffffffff != struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])[0]:
            raise PngError("PNG chunk %r fails its CRC" % ctype)
        pos += 12 + length
        if ihdr is None and ctype != b'IHDR':
            raise PngError("PNG does not start with IHDR")
        if ctype == b'IHDR':
            if ihdr is not None or length != 13:
                raise PngError("bad PNG IHDR")
            ihdr = struct.unpack('>IIBBBBB', body)
        elif ctype == b'PLTE':
            if length == 0 or length % 3 != 0 or length > 768 or palette is not None or idat:
                raise PngError("bad PNG PLTE")
            palette = bytes(body)
        elif ctype == b'IDAT':
            if idat_done:
                raise PngError("PNG IDAT chunks are not consecutive")
            idat.append(body)
        elif ctype == b'IEND':
            ended = True
            break
        else:
            if not (ctype[0] & 0x20):
                raise PngError("unknown critical PNG chunk %r" % ctype, unsupported=True)
        if idat and ctype != b'IDAT':
            idat_done = True
    if ihdr is None or not ended or not idat:
        raise PngError("truncated PNG (IHDR, IDAT or IEND missing)")
    width, height, depth, colour, compression, filt, interlace = ihdr
    if colour not in _CHANNELS or depth not in _DEPTHS[colour] or compression != 0 or filt != 0 or interlace not in (0, 1):
        raise PngError("bad PNG IHDR (colour type %d, bit depth %d)" % (colour, depth))
    if width < 1 or height < 1:
        raise PngError("PNG of zero width or height")
    if width > _MAX_SIDE or height > _MAX_SIDE:
        raise PngError("PNG larger than 2^24 pixels a side", unsupported=True)
    if interlace != 0:
        raise PngError("Adam7-interlaced PNGs are not supported", unsupported=True)
    if colour == 3 and palette is None:
        raise PngError("palette PNG without PLTE")
    return width, height, depth, colour, palette, b''.join(idat)


def decode_png(data: bytes, out: np.ndarray = None, lib=None) -> PngImage:
    """bytes of a PNG file -> PngImage.  `out`: where the unfiltered bytes go (a contiguous uint8 array of height * row_bytes elements:
    a slice of a batch's staging buffer).  `lib`: a stand-alone build of ofl_png_host.cpp (tests)."""
    width, height, depth, colour, palette, idat = parse_png(data)
    row_bytes = (width * _CHANNELS[colour] * depth + 7) // 8
    expected = height * (row_bytes + 1)
    inflater = zlib.decompressobj()
    try:
        inflated = inflater.decompress(idat, expected + 1)          # (bounded: a stream that inflates to more is rejected, not held)
    except zlib.error as exc:
        raise PngError("PNG image data does not inflate: %s" % exc)
    if len(inflated) != expected or not inflater.eof:
        raise PngError("PNG image data inflates to %s%d bytes, the header promises %d"
                       % ("" if inflater.eof else "more than " if len(inflated) > expected else "a truncated stream of ", len(inflated), expected))
    rc, raw = _native.png_unfilter(inflated, width, height, depth, colour, out=out, lib=lib)
    if rc != 0:
        raise PngError("PNG scanlines cannot be unfiltered (status %d: %s)" % (rc, "a filter type above 4" if rc == -3 else "lengths"))
    img = PngImage()
    img.width, img.height, img.bit_depth, img.colour_type, img.palette = width, height, depth, colour, palette
    img.raw = raw.reshape(height, row_bytes)
    return img


def png_grey(img: PngImage, lib=None) -> np.ndarray:
    """uint8 [height, width]: the grey value cv2.imread(path, 0) yields (DESIGN.md 3.15 states the rule per colour type)."""
    rc, grey = _native.png_grey8(img.raw, img.width, img.height, img.bit_depth, img.colour_type, img.palette, lib=lib)
    if rc == -4:
        raise PngError("PNG masks of colour type %d at %d bits are not supported (grey at 1 / 2 / 4 / 8 / 16 bits, palette, 8-bit RGB "
                       "and RGBA are)" % (img.colour_type, img.bit_depth), unsupported=True)
    if rc != 0:
        raise PngError("PNG palette index beyond the palette" if rc == -3 else "PNG grey conversion failed (status %d)" % rc)
    return grey


# ------------------------------------------------------------------------------------------------
# the three file kinds: host side of one file
# ------------------------------------------------------------------------------------------------
_KITTI = "Error loading flow from KITTI data: "
_SINTEL = "Error loading flow from Sintel data: "


def _read(path: str) -> bytes:
    with open(path, 'rb') as f:
        return f.read()


def _kitti_header(path: str):
    """(file bytes, height, width) of a KITTI flow PNG, or the reference's ValueError (utils.py:821-825: `cv2.imread` gives None for
    what it cannot read, and anything but three channels has 'the wrong shape')."""
    if not isinstance(path, str):
        raise TypeError(_KITTI + "Path needs to be a string")
    try:
        data = _read(path)
        width, height, depth, colour, _, _ = parse_png(data)
    except PngError as exc:
        if exc.unsupported:
            raise ValueError(_KITTI + "Flow data could not be loaded: %s" % exc)
        raise ValueError(_KITTI + "Flow data could not be loaded")
    except OSError:
        raise ValueError(_KITTI + "Flow data could not be loaded")
    if colour in (0, 4, 6):                                  # cv2.IMREAD_UNCHANGED: H-W, or H-W-4 with alpha
        raise ValueError(_KITTI + "Loaded flow data has the wrong shape")
    if colour != 2 or depth != 16:
        raise ValueError(_KITTI + "Flow data could not be loaded: only 16-bit RGB PNGs are supported, this one has colour type %d at "
                         "%d bits" % (colour, depth))
    return data, height, width


def _kitti_decode(data: bytes, out: np.ndarray):
    try:
        decode_png(data, out=out)
    except PngError:
        raise ValueError(_KITTI + "Flow data could not be loaded")


def _flo_payload(path: str):
    """(payload bytes as a uint8 array, height, width) of a .flo file (utils.py:842-854); the length is checked against the header."""
    if not isinstance(path, str):
        raise TypeError(_SINTEL + "Path needs to be a string")
    data = _read(path)
    if data[:4] != b'PIEH':
        raise ValueError(_SINTEL + "Path not a valid .flo file")
    if len(data) < 12:
        raise ValueError(_SINTEL + "Path not a valid .flo file")
    w, h = struct.unpack('<ii', data[4:12])
    if w < 1 or w > 99999:
        raise ValueError(_SINTEL + "Invalid width read from file ('{}')".format(w))
    if h < 1 or h > 99999:
        raise ValueError(_SINTEL + "Invalid height read from file ('{}')".format(h))
    if len(data) != 12 + 8 * h * w:
        raise ValueError(_SINTEL + "File holds {} bytes of flow data, its header ({} x {}) promises {}".format(len(data) - 12, w, h, 8 * h * w))
    return np.frombuffer(data, dtype=np.uint8, offset=12), h, w


def _mask_grey(path: str) -> np.ndarray:
    """uint8 [H, W] grey plane of a Sintel invalid-pixel PNG (utils.py:869-873)."""
    if not isinstance(path, str):
        raise TypeError(_SINTEL + "Path needs to be a string")
    try:
        return png_grey(decode_png(_read(path)))
    except PngError as exc:
        if exc.unsupported:
            raise ValueError(_SINTEL + "Invalid mask could not be loaded from path: %s" % exc)
        raise ValueError(_SINTEL + "Invalid mask could not be loaded from path")
    except OSError:
        raise ValueError(_SINTEL + "Invalid mask could not be loaded from path")


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------
def _paths(path, what: str):
    """(list of paths, was it a single one).  A str is the reference's call; a list / tuple of them is the batch extension."""
    if isinstance(path, (list, tuple)):
        if len(path) == 0:
            raise ValueError(what + "The list of paths is empty")
        return list(path), False
    return [path], True


def _map(fn, items):
    """fn over the items, side by side for more than one.  A caller whose fn reaches `png_unfilter` / `png_grey8` loads the library
    first, on its own thread (`_native.load_library()` may rebuild a stale one): the workers only ever find it loaded."""
    if len(items) == 1:
        return [fn(items[0])]
    with ThreadPoolExecutor(max_workers=min(MAX_WORKERS, len(items))) as pool:
        return list(pool.map(fn, items))


def _same_size(sizes, what: str):
    if any(s != sizes[0] for s in sizes):
        raise ValueError(what + "The frames of a batch need to be of equal size, found " + ", ".join(sorted(set("%d x %d" % (s[1], s[0]) for s in sizes))))
    return sizes[0]


def kitti(path, want_mask: bool = True):
    """KITTI file(s) -> (vecs fp32 [N,2,H,W], mask bool [N,H,W] or None, flag words int32 [N], single) on the HIP device."""
    paths, single = _paths(path, _KITTI)
    heads = _map(_kitti_header, paths)
    h, w = _same_size([(hd[1], hd[2]) for hd in heads], _KITTI)
    _native.device()                                                   # (no device: NativeUnavailable before any decoding)
    _native.load_library()                                             # (on this thread, before the pool: see _map)
    stage = torch.empty((len(paths), 6 * h * w), dtype=torch.uint8)   # all frames' raw samples: ONE upload
    rows = stage.numpy()
    _map(lambda i: _kitti_decode(heads[i][0], rows[i]), list(range(len(paths))))
    return _native.decode_kitti(stage, h, w, want_mask) + (single,)


def sintel(path, inv_path=None):
    """.flo file(s) and optionally their invalid-pixel PNG(s) -> (vecs, mask or None, flag words, single, mask error or None).
    A mask of another size than the flow is reported, not raised: the reference's constructor looks at the vectors first."""
    paths, single = _paths(path, _SINTEL)
    loads = _map(_flo_payload, paths)
    h, w = _same_size([(ld[1], ld[2]) for ld in loads], _SINTEL)
    grey, mask_error = None, None
    if inv_path is not None:
        inv_paths, inv_single = _paths(inv_path, _SINTEL)
        if inv_single != single or len(inv_paths) != len(paths):
            raise ValueError(_SINTEL + "Flow paths and invalid mask paths need to be given in equal numbers")
        _native.load_library()                                         # (on this thread, before the pool: see _map)
        greys = _map(_mask_grey, inv_paths)
        if any(g.shape != (h, w) for g in greys):
            mask_error = "Error setting flow mask: Input shape does not match the desired shape"
        else:
            grey = torch.from_numpy(np.stack(greys))
    _native.device()
    stage = torch.empty((len(paths), h, w, 2), dtype=torch.float32)
    rows = stage.view(torch.uint8).numpy().reshape(len(paths), -1)
    for i, ld in enumerate(loads):
        rows[i] = ld[0]
    return _native.decode_flo(stage, grey) + (single, mask_error)


def sintel_mask(path):
    """Invalid-pixel PNG(s) -> bool [H,W] ([N,H,W] for a list) CPU tensor, True where the grey value is zero (utils.py:874)."""
    paths, single = _paths(path, _SINTEL)
    _native.load_library()                                             # (on this thread, before the pool: see _map)
    greys = _map(_mask_grey, paths)
    _same_size([g.shape for g in greys], _SINTEL)
    mask = torch.from_numpy(np.stack(greys)) == 0
    return mask[0] if single else mask
