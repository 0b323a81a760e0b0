"""frt_read_hdr (csrc/host/hdr.cpp): the Radiance RGBE reader behind
frt::Scene::set_env_map and frt_render --env-map.  The files are written here
(tests/env_specs.py) and decoded independently with m * 2^(e - 136); the
reader's floats must be bit-exact.  Malformed files fail with the codes
include/frt.h documents."""
import ctypes

import numpy as np
import pytest

import env_specs as ES
import first_raytracer_amd as frt

FRT_E_INVALID, FRT_E_UNSUPPORTED, FRT_E_IO = -1, -4, -5


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def read_rc(path):
    nx, ny = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = frt.lib().frt_read_hdr(path.encode(), ctypes.byref(nx), ctypes.byref(ny), None)
    if rc != 0:
        return rc
    out = np.zeros((ny.value, nx.value, 3), np.float32)
    return frt.lib().frt_read_hdr(path.encode(), ctypes.byref(nx), ctypes.byref(ny), out.ctypes.data)


def rle_image():
    a = ES.rgbe_random(16, 4, seed=2)
    a[:, 3:11, 0] = 77          # runs in the red channel
    a[1, :, 3] = 129            # a whole-scanline run of exponents
    a[2, 5:9, :] = (1, 2, 3, 128)
    return a


def test_flat_small(tmp_path):
    a = ES.rgbe_random(5, 3, seed=1, zero_exp_at=[(2, 1)])   # width < 8: flat scanlines
    got = frt.read_hdr(write(tmp_path, "flat.hdr", ES.hdr_bytes(a)))
    want = ES.rgbe_decode(a)
    assert got.shape == (3, 5, 3) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[1, 2] == 0).all()                              # e == 0 -> 0 whatever the mantissa
    assert a[1, 2, :3].any()


def test_rle(tmp_path):
    a = rle_image()
    data = ES.hdr_bytes(a, rle=True)
    body = ES.rle_channel(a[0, :, 0])
    kinds = set()
    i = 0
    while i < len(body):                                       # the scanline has both packet kinds
        if body[i] > 128:
            kinds.add("run"); i += 2
        else:
            kinds.add("literal"); i += 1 + body[i]
    assert kinds == {"run", "literal"}
    got = frt.read_hdr(write(tmp_path, "rle.hdr", data))
    assert np.array_equal(got.view(np.uint32), ES.rgbe_decode(a).view(np.uint32))
    # the same texels stored flat (no scanline marker) decode to the same floats
    flat = frt.read_hdr(write(tmp_path, "rle_flat.hdr", ES.hdr_bytes(a)))
    assert np.array_equal(flat.view(np.uint32), got.view(np.uint32))


def test_header_comments_and_rgbe_magic(tmp_path):
    a = ES.rgbe_random(9, 2, seed=4)
    extra = (b"# written by a test", b"EXPOSURE=1.0", b"SOFTWARE=none")
    got = frt.read_hdr(write(tmp_path, "c.hdr", ES.hdr_bytes(a, rle=True, header_extra=extra, magic=b"#?RGBE")))
    assert np.array_equal(got.view(np.uint32), ES.rgbe_decode(a).view(np.uint32))


def test_sizes_only(tmp_path):
    a = ES.rgbe_random(5, 3, seed=1)
    p = write(tmp_path, "s.hdr", ES.hdr_bytes(a)[:-7])         # sizes come from the header alone
    nx, ny = ctypes.c_int32(0), ctypes.c_int32(0)
    assert frt.lib().frt_read_hdr(p.encode(), ctypes.byref(nx), ctypes.byref(ny), None) == 0
    assert (nx.value, ny.value) == (5, 3)


def test_malformed(tmp_path):
    flat = ES.hdr_bytes(ES.rgbe_random(5, 3, seed=1))
    rle = ES.hdr_bytes(rle_image(), rle=True)
    assert read_rc(str(tmp_path / "missing.hdr")) == FRT_E_IO
    assert read_rc(write(tmp_path, "t1.hdr", flat[:-7])) == FRT_E_IO            # truncated texels
    assert read_rc(write(tmp_path, "t2.hdr", rle[:-3])) == FRT_E_IO             # truncated RLE packet
    assert read_rc(write(tmp_path, "t3.hdr", flat[:20])) == FRT_E_IO            # truncated header
    assert read_rc(write(tmp_path, "m.hdr", b"P6\n" + flat[11:])) == FRT_E_INVALID   # bad magic
    a = ES.rgbe_random(5, 3, seed=1)
    assert read_rc(write(tmp_path, "y.hdr", ES.hdr_bytes(a, size_line=b"+Y 3 +X 5"))) == FRT_E_UNSUPPORTED
    assert read_rc(write(tmp_path, "x.hdr", ES.hdr_bytes(a, size_line=b"-Y 3 -X 5"))) == FRT_E_UNSUPPORTED
    assert read_rc(write(tmp_path, "z.hdr", ES.hdr_bytes(a, size_line=b"-Y 0 +X 5"))) == FRT_E_INVALID
    assert read_rc(write(tmp_path, "g.hdr", ES.hdr_bytes(a, size_line=b"5 by 3"))) == FRT_E_INVALID
    # an RLE run overrunning the scanline: 16 wide, a run of 20
    head = ES.hdr_bytes(ES.rgbe_random(16, 1, seed=1), rle=True).split(b"+X 16\n")[0] + b"+X 16\n"
    over = head + bytes([2, 2, 0, 16, 128 + 20, 9]) + bytes(64)
    assert read_rc(write(tmp_path, "o.hdr", over)) == FRT_E_INVALID
    lit = head + bytes([2, 2, 0, 16, 12]) + bytes(12) + bytes([9]) + bytes(64)   # literal of 9 with 4 left
    assert read_rc(write(tmp_path, "l.hdr", lit)) == FRT_E_INVALID
    wrong = head + bytes([2, 2, 0, 17]) + bytes(64)                               # scanline length != width
    assert read_rc(write(tmp_path, "w.hdr", wrong)) == FRT_E_INVALID
    with pytest.raises(frt.FrtError, match="frt_read_hdr"):
        frt.read_hdr(str(tmp_path / "o.hdr"))
