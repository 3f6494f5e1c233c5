"""CPU tier of the dataset loaders: the host PNG decoder (container parsing in oflibpytorch_amd/_loaders.py, scanline
unfilter and grey rule in csrc/ofl_png_host.cpp) against the plain NumPy decoder of tests/png_oracle.py, its rejections, the
reference's fixtures, the errors the public API raises before any device work, and the stand-alone sanitizer program."""
import ctypes
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, 'tests', 'golden', 'loaders')
HOST_SRC = os.path.join(ROOT, 'oflibpytorch_amd', 'csrc', 'ofl_png_host.cpp')
INCLUDE = os.path.join(ROOT, 'include')

# every colour type / bit depth pair PNG defines; the grey rule covers the first eleven
KINDS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (3, 1), (3, 2), (3, 4), (3, 8), (2, 8), (6, 8), (2, 16), (4, 8), (4, 16), (6, 16)]
GREY_KINDS = KINDS[:11]
WIDTHS, HEIGHTS = (1, 2, 3, 5, 8, 33), (1, 4)


def _host_compiler():
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """ofl_png_host.cpp compiled ON ITS OWN by the host compiler (no hipcc, no HIP header)."""
    out = str(tmp_path_factory.mktemp("pnghost") / "libofl_png_host.so")
    subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-fPIC', '-shared', '-I', INCLUDE, '-o', out, HOST_SRC],
                   check=True)
    lib = ctypes.CDLL(out)
    p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.ofl_png_unfilter.argtypes = [p, i64, i32, i32, i32, i32, p, i64]
    lib.ofl_png_grey8.argtypes = [p, i64, i32, i32, i32, i32, p, i32, p, i64]
    return lib


@pytest.fixture(scope="module", params=["standalone", "library"])
def lib(request, host_lib):
    """Both builds of the same source: the stand-alone one and the copy inside libofl_hip.so (loading it touches no GPU)."""
    if request.param == "standalone":
        return host_lib
    from oflibpytorch_amd import _native
    return _native.load_library()


def _image(w, h, colour, depth, seed):
    rng = np.random.RandomState(seed)
    c = po.CHANNELS[colour]
    top = (1 << depth) - 1
    s = rng.randint(0, top + 1, size=(h, w, c)).astype(np.int64)
    s[rng.rand(h, w) < 0.3] = 0                     # pixels that are exactly zero: the mask rule's other side
    s.reshape(-1)[::7] = top
    palette = None
    if colour == 3:
        pal = rng.randint(0, 256, size=(top + 1, 3)).astype(np.uint8)
        pal[0] = 0                                  # index 0 black, index 1 so dark that its grey value rounds to zero
        if top >= 1:
            pal[1] = (0, 0, 1)
        palette = pal.tobytes()
    return s, palette


@pytest.mark.parametrize("colour,depth", KINDS)
def test_host_decoder_matches_the_oracle(lib, colour, depth):
    """Every filter type on consecutive rows (all 5 rotations of the order), every width and height, one and several IDAT chunks."""
    from oflibpytorch_amd import _loaders
    for w in WIDTHS:
        for h in HEIGHTS:
            s, palette = _image(w, h, colour, depth, seed=w * 10 + h)
            for rot in range(5):
                filters = [(rot + k) % 5 for k in range(5)]
                data = po.encode(s, depth, colour, filters=filters, palette=palette, idat_split=(7 if rot % 2 else None), level=rot)
                ref = po.decode(data)
                assert np.array_equal(ref['samples'], s)                      # (the oracle reads back what the encoder was given)
                img = _loaders.decode_png(data, lib=lib)
                assert (img.width, img.height, img.bit_depth, img.colour_type) == (w, h, depth, colour)
                assert img.raw.dtype == np.uint8 and np.array_equal(img.raw, ref['raw']), (w, h, filters)
                if (colour, depth) in GREY_KINDS:
                    assert np.array_equal(_loaders.png_grey(img, lib=lib), po.grey8(ref)), (w, h)
                else:
                    with pytest.raises(ValueError, match="not supported"):
                        _loaders.png_grey(img, lib=lib)


def test_grey_rule_values(lib):
    """The rule itself, on values worked out by hand: 16-bit grey keeps the high byte, low depths scale to 255, colours take
    OpenCV's rounded 14-bit weights -- (0, 0, 1), (0, 0, 4) and (1, 0, 0) round to grey 0, (0, 1, 0) and (0, 0, 5) to 1."""
    from oflibpytorch_amd import _loaders

    def grey(samples, depth, colour, palette=None):
        return _loaders.png_grey(_loaders.decode_png(po.encode(np.array(samples), depth, colour, palette=palette), lib=lib), lib=lib)

    assert grey([[0, 1, 255, 256, 0xffff]], 16, 0).tolist() == [[0, 0, 0, 1, 255]]
    assert grey([[0, 1]], 1, 0).tolist() == [[0, 255]]
    assert grey([[0, 1, 2, 3]], 2, 0).tolist() == [[0, 85, 170, 255]]
    assert grey([[0, 1, 15]], 4, 0).tolist() == [[0, 17, 255]]
    rgb = [[(0, 0, 0), (0, 0, 1), (0, 0, 4), (1, 0, 0), (0, 1, 0), (0, 0, 5), (255, 255, 255), (255, 0, 0)]]
    assert grey(rgb, 8, 2).tolist() == [[0, 0, 0, 0, 1, 1, 255, 76]]
    rgba = [[p + (a,) for p, a in zip(rgb[0], (0, 255, 0, 255, 0, 255, 0, 255))]]
    assert grey(rgba, 8, 6).tolist() == [[0, 0, 0, 0, 1, 1, 255, 76]]                       # alpha is ignored
    pal = bytes([0, 0, 0, 0, 0, 1, 0, 1, 0, 255, 255, 255])
    assert grey([[0, 1, 2, 3]], 2, 3, palette=pal).tolist() == [[0, 0, 1, 255]]


def _kitti_like(w=5, h=4):
    s, _ = _image(w, h, 2, 16, seed=3)
    return s, po.encode(s, 16, 2, filters=[4, 1, 3, 2])


def _rewrite_chunk(data, ctype, fn):
    """Apply fn(body) to the first chunk of that type and repair the CRC (unless fn returns a whole chunk)."""
    pos = 8
    while pos < len(data):
        length, ct = struct.unpack('>I4s', data[pos:pos + 8])
        if ct == ctype:
            return data[:pos] + po.chunk(ctype, fn(data[pos + 8:pos + 8 + length])) + data[pos + 12 + length:]
        pos += 12 + length
    raise AssertionError(ctype)


def test_rejections(lib):
    from oflibpytorch_amd import _loaders
    s, good = _kitti_like()
    assert np.array_equal(_loaders.decode_png(good, lib=lib).raw, po.decode(good)['raw'])
    refiltered = lambda fn: _rewrite_chunk(good, b'IDAT', lambda body: zlib.compress(fn(bytearray(zlib.decompress(body)))))

    def bad_filter(raw):
        raw[31] = 5                                   # the second row's filter byte (rows of 1 + 5 * 6 bytes)
        return bytes(raw)

    bad = {
        "truncated file": good[:-20],
        "truncated inside IDAT": good[:60],
        "truncated stream": _rewrite_chunk(good, b'IDAT', lambda body: body[:len(body) // 2]),
        "short image data": refiltered(lambda raw: bytes(raw[:-1])),
        "long image data": refiltered(lambda raw: bytes(raw) + b'\0'),
        "bad filter byte": refiltered(bad_filter),
        "wrong CRC": good[:40] + bytes([good[40] ^ 1]) + good[41:],
        "wrong chunk length": good[:33] + struct.pack('>I', struct.unpack('>I', good[33:37])[0] + 1) + good[37:],
        "huge chunk length": good[:33] + b'\x7f\xff\xff\xff' + good[37:],
        "interlace": po.encode(s, 16, 2, interlace=1),
        "zero width": _rewrite_chunk(good, b'IHDR', lambda b: struct.pack('>II', 0, 4) + b[8:]),
        "zero height": _rewrite_chunk(good, b'IHDR', lambda b: struct.pack('>II', 5, 0) + b[8:]),
        "wider header": _rewrite_chunk(good, b'IHDR', lambda b: struct.pack('>II', 6, 4) + b[8:]),
        "bit depth 3": _rewrite_chunk(good, b'IHDR', lambda b: b[:8] + b'\x03' + b[9:]),
        "no signature": b'\0' + good[1:],
        "no IEND": good[:-12],
        "empty": b'',
    }
    for what, data in bad.items():
        with pytest.raises(ValueError):
            _loaders.decode_png(data, lib=lib)
            pytest.fail("accepted: " + what)
    with pytest.raises(ValueError, match="interlace"):
        _loaders.decode_png(bad["interlace"], lib=lib)
    # the C entry points themselves: lengths are the caller's, and a mismatch is a status, not a read
    one = np.zeros(8, dtype=np.uint8)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.ofl_png_unfilter(None, 8, 1, 1, 8, 0, vp(one), 1) == -1
    assert lib.ofl_png_unfilter(vp(one), 2, 1, 1, 8, 0, vp(one), 2) == -2 and lib.ofl_png_unfilter(vp(one), 1, 1, 1, 8, 0, vp(one), 1) == -2
    assert lib.ofl_png_unfilter(vp(one), 2, 1, 1, 8, 0, vp(one), 1) == 0
    assert lib.ofl_png_unfilter(vp(one), 2, 1, 1, 8, 1, vp(one), 1) == -3 and lib.ofl_png_unfilter(vp(one), 2, 1, 1, 16, 3, vp(one), 1) == -3
    assert lib.ofl_png_unfilter(vp(one), 2, 1, 0, 8, 0, vp(one), 1) == -2 and lib.ofl_png_unfilter(vp(one), 2, 1 << 25, 1, 8, 0, vp(one), 1) == -2
    assert lib.ofl_png_grey8(vp(one), 2, 1, 1, 8, 4, None, 0, vp(one), 1) == -4 and lib.ofl_png_grey8(vp(one), 6, 1, 1, 16, 2, None, 0, vp(one), 1) == -4
    assert lib.ofl_png_grey8(vp(one), 1, 1, 1, 8, 3, None, 0, vp(one), 1) == -1 and lib.ofl_png_grey8(vp(one), 1, 1, 1, 8, 0, None, 0, vp(one), 2) == -2


def test_reference_fixtures_on_the_host():
    """The six files of the reference's tests: headers, and the values test_flow_class.py:205-238 asserts, at the host level."""
    from oflibpytorch_amd import _loaders
    want = np.arange(10)[:, None] * np.arange(20)[None, :]
    img = _loaders.decode_png(open(os.path.join(FIX, 'kitti.png'), 'rb').read())
    assert (img.width, img.height, img.bit_depth, img.colour_type) == (20, 10, 16, 2)
    s = img.raw.reshape(10, 20, 3, 2).astype(np.int64)
    s = s[..., 0] * 256 + s[..., 1]
    assert np.array_equal((s[..., 0] - 2 ** 15) / 64, want) and np.all((s[..., 1] - 2 ** 15) / 64 == 0)
    assert np.all(s[:, 0, 2] > 0) and np.all(s[:, 10, 2] == 0)
    for name, shape in (('sintel_invalid.png', (10, 20)), ('sintel_invalid_wrong.png', (12, 20))):
        m = _loaders.sintel_mask(os.path.join(FIX, name))
        assert m.dtype.is_floating_point is False and tuple(m.shape) == shape and str(m.dtype) == 'torch.bool'
        assert bool(m[:, 0].all()) and not bool(m[:, 10].any())
    payload, h, w = _loaders._flo_payload(os.path.join(FIX, 'sintel.flo'))
    flo = payload.view('<f4').reshape(h, w, 2)
    assert (h, w) == (10, 20) and np.array_equal(flo[..., 0], want)


def test_fixtures_agree_with_an_image_library():
    """Where PIL happens to be installed: the mask's grey plane and the KITTI samples as it reads them."""
    Image = pytest.importorskip("PIL.Image")
    from oflibpytorch_amd import _loaders
    for name in ('sintel_invalid.png', 'sintel_invalid_wrong.png'):
        path = os.path.join(FIX, name)
        grey = np.array(Image.open(path).convert('L'))
        assert np.array_equal(_loaders.png_grey(_loaders.decode_png(open(path, 'rb').read())), grey)
        assert np.array_equal(_loaders.sintel_mask(path).numpy(), ~grey.astype(bool))
    for w in (1, 5, 33):                              # generated grey masks of every depth: the expansion to 8 bits
        for depth in (1, 2, 4, 8):
            s, _ = _image(w, 4, 0, depth, seed=w)
            data = po.encode(s, depth, 0, filters=[0, 1, 2, 3, 4])
            import io
            grey = np.array(Image.open(io.BytesIO(data)).convert('L'))
            assert np.array_equal(_loaders.png_grey(_loaders.decode_png(data)), grey), (w, depth)
    img = _loaders.decode_png(open(os.path.join(FIX, 'kitti.png'), 'rb').read())
    pil = Image.open(os.path.join(FIX, 'kitti.png'))
    if pil.mode == 'RGB':                             # (PIL cuts 16-bit RGB down to the high bytes)
        assert np.array_equal(img.raw.reshape(10, 20, 3, 2)[..., 0], np.array(pil))


def test_api_errors_need_no_device():
    """The error cases of test_flow_class.py:205-238 that the reference raises before it builds a flow (plus the batch extension's
    own), with its types and messages.  All of them are decided on the host."""
    import oflibpytorch_amd as ofl
    fx = lambda name: os.path.join(FIX, name)
    with pytest.raises(TypeError, match="Error loading flow from KITTI data: Load_valid needs to be boolean"):
        ofl.Flow.from_kitti(fx('kitti.png'), load_valid='test')
    with pytest.raises(ValueError, match="Error loading flow from KITTI data: Flow data could not be loaded"):
        ofl.Flow.from_kitti('test')
    with pytest.raises(ValueError, match="Error loading flow from KITTI data: Loaded flow data has the wrong shape"):
        ofl.Flow.from_kitti(fx('kitti_wrong.png'))
    with pytest.raises(ValueError, match="Error loading flow from KITTI data: Flow data could not be loaded"):
        ofl.load_kitti(fx('sintel.flo'))
    with pytest.raises(ValueError, match="Error loading flow from Sintel data: Path not a valid .flo file"):
        ofl.Flow.from_sintel(fx('sintel_wrong.flo'))
    with pytest.raises(ValueError, match="Error loading flow from Sintel data: Invalid mask could not be loaded from path"):
        ofl.Flow.from_sintel(fx('sintel.flo'), 'test.png')
    with pytest.raises(ValueError, match="Error loading flow from Sintel data: Invalid mask could not be loaded from path"):
        ofl.load_sintel_mask(fx('sintel.flo'))
    with pytest.raises(TypeError, match="Error loading flow from Sintel data: Path needs to be a string"):
        ofl.load_sintel(3)
    with pytest.raises(TypeError, match="Error loading flow from Sintel data: Path needs to be a string"):
        ofl.load_sintel_mask(3)
    with pytest.raises(ValueError, match="equal size"):
        ofl.load_sintel_mask([fx('sintel_invalid.png'), fx('sintel_invalid_wrong.png')])


def test_flo_length_is_checked_against_the_header(tmp_path):
    import oflibpytorch_amd as ofl
    good = open(os.path.join(FIX, 'sintel.flo'), 'rb').read()
    for what, data in (("short", good[:-4]), ("long", good + b'\0' * 8), ("header only", good[:12]), ("zero width", good[:4] + b'\0' * 4 + good[8:]),
                       ("negative height", good[:8] + struct.pack('<i', -10) + good[12:]), ("tag only", good[:4])):
        path = str(tmp_path / (what.replace(' ', '_') + '.flo'))
        with open(path, 'wb') as f:
            f.write(data)
        with pytest.raises(ValueError, match="Error loading flow from Sintel data"):
            ofl.load_sintel(path)
            pytest.fail("accepted: " + what)


def test_sanitizer_program(tmp_path):
    """tools/png_unfilter_check.cpp + the decoder under AddressSanitizer and UBSan, as a process of its own: the fixtures' inflated
    bytes, then single-byte mutations and truncations of them.  Exit status 0 and not a word on stderr."""
    cxx = _host_compiler()
    exe = str(tmp_path / "png_unfilter_check")
    cmd = [cxx, '-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', INCLUDE,
           os.path.join(ROOT, 'tools', 'png_unfilter_check.cpp'), HOST_SRC, '-o', exe]
    # the sanitizer runtimes linked INTO the program where the compiler can (gcc's flags; clang does so by default)
    build = subprocess.run(cmd + ['-static-libasan', '-static-libubsan'], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    from oflibpytorch_amd import _loaders
    jobs = [open(os.path.join(FIX, name), 'rb').read() for name in ('kitti.png', 'sintel_invalid.png', 'kitti_wrong.png')]
    s, palette = _image(9, 3, 3, 2, seed=1)
    jobs.append(po.encode(s, 2, 3, filters=[4, 3, 1], palette=palette))                   # sub-byte samples, a palette
    s, _ = _image(5, 4, 6, 8, seed=2)
    jobs.append(po.encode(s, 8, 6, filters=[3, 4, 2, 1]))
    for i, data in enumerate(jobs):
        w, h, depth, colour, _, idat = _loaders.parse_png(data)
        path = str(tmp_path / ("inflated_%d.bin" % i))
        with open(path, 'wb') as f:
            f.write(zlib.decompress(idat))
        run = subprocess.run([exe, path, str(w), str(h), str(depth), str(colour)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stderr == '', (i, run.returncode, run.stderr[-2000:])
        assert 'png_unfilter_check: ok' in run.stdout


def test_library_is_loaded_once_and_never_by_a_pool_worker(monkeypatch):
    """A process whose first call into the package is a list load: the library is loaded (and, were it stale, rebuilt) on the calling
    thread before the pool starts, and `load_library` itself lets one thread at a time through -- 16 simultaneous first calls dlopen once."""
    import threading
    from oflibpytorch_amd import _loaders, _native
    real_load, real_cdll, seen, opened = _native.load_library, ctypes.CDLL, [], []

    def recording_load(path=None):
        seen.append((threading.current_thread() is threading.main_thread(), _native._lib is None))
        return real_load(path)

    def counting_cdll(*a, **kw):
        opened.append(threading.current_thread().name)
        return real_cdll(*a, **kw)

    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "load_library", recording_load)
    monkeypatch.setattr(_native.ctypes, "CDLL", counting_cdll)
    paths = [os.path.join(FIX, 'sintel_invalid.png')] * 16
    masks = _loaders.sintel_mask(paths)
    assert tuple(masks.shape) == (16, 10, 20)
    assert len(opened) == 1 and seen[0] == (True, True)                   # loaded by the first call, which the calling thread made
    assert any(not main for main, _ in seen)                              # (the workers did run, and did ask for the library)
    assert all(main for main, unloaded in seen if unloaded)               # ... but none of them ever found it missing
    # the lock on its own: 16 threads ask an unloaded module at once
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "load_library", real_load)
    del opened[:]
    gate, libs = threading.Barrier(16), []

    def ask():
        gate.wait()
        libs.append(_native.load_library())

    threads = [threading.Thread(target=ask) for _ in range(16)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(opened) == 1 and len(libs) == 16 and all(lib is libs[0] for lib in libs)
