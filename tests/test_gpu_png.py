"""Colour frames encoded on the device (csrc/device/encode.hip k_frame_rows, k_png_pack,
k_png_finish behind ops.device.png_encode and render.write_png(encode="device")): the file
must decode, with every checksum right, to the pixels of render.colormap."""
import struct
import zlib

import numpy as np
import pytest
import torch

from tclb_amd.io import render
from tclb_amd.ops import device as D

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


def _decode(b):
    """(pixels (h, w, 4), IDAT bytes) of an 8-bit RGBA PNG with filter types 0 and 1"""
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    p, idat, types = 8, b"", []
    while p < len(b):
        n = struct.unpack(">I", b[p:p + 4])[0]
        t, d = b[p + 4:p + 8], b[p + 8:p + 8 + n]
        assert zlib.crc32(t + d) == struct.unpack(">I", b[p + 8 + n:p + 12 + n])[0], t
        types.append(t)
        if t == b"IHDR":
            w, h = struct.unpack(">II", d[:8])
            assert d[8:] == bytes([8, 6, 0, 0, 0])
        if t == b"IDAT":
            idat += d
        p += 12 + n
    assert types[0] == b"IHDR" and types[-1] == b"IEND"
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)      # checks the Adler-32
    assert (rows[:, 0] <= 1).all()
    px = rows[:, 1:].reshape(h, w, 4).copy()
    sub = rows[:, 0] == 1
    px[sub] = np.cumsum(px[sub], axis=1, dtype=np.uint8)
    return px, len(idat)


def _on_boundary(t):
    """an fp32 l with fl(l * 111) == t exactly"""
    c = np.float32(t) / np.float32(111)
    for v in (c, np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-2))):
        if np.float32(v) * np.float32(111) == np.float32(t):
            return float(v)
    raise AssertionError(t)


def _pattern(kind, nx, ny):
    if kind == "const":
        return torch.full((ny, nx), 0.05, dtype=torch.float64), torch.ones((ny, nx), dtype=torch.float64)
    g = torch.Generator().manual_seed(nx * 1000 + ny)
    if kind == "random":
        return torch.rand((ny, nx), generator=g, dtype=torch.float64) * 2.4 - 1.2, \
            torch.rand((ny, nx), generator=g, dtype=torch.float64)
    l = torch.linspace(-1.2, 1.2, nx, dtype=torch.float64).repeat(ny, 1) + 1e-3 * torch.arange(ny)[:, None]
    w = torch.ones((ny, nx), dtype=torch.float64)
    edges = [_on_boundary(t) for t in (-111, -11, -1, 0, 1, 11, 111)]
    m = min(nx * ny, len(edges))
    l.view(-1)[nx * ny - m:] = torch.tensor(edges[:m], dtype=torch.float64)
    if kind == "bad":
        idx = torch.arange(0, nx * ny, 5)
        l.view(-1)[idx] = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=torch.float64)[idx % 3]
        w[:, ::3] = 0.0
    return l, w


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", ["const", "random", "ramp", "bad"])
@pytest.mark.parametrize("nx,ny", [(1, 1), (63, 3), (64, 2), (65, 5), (130, 4), (321, 7)])
def test_png_encode_matches_colormap(nx, ny, kind, dtype):
    l, w = _pattern(kind, nx, ny)
    lw = torch.stack([l, w]).to(dtype).cuda()
    pix = torch.empty((ny, nx, 4), dtype=torch.uint8, device="cuda")
    data = D.png_encode(lw, pixels=pix)
    assert data.dtype == torch.uint8 and data.is_cuda
    want = render.colormap(lw[0], lw[1]).cpu().numpy()[::-1]
    got, nidat = _decode(data.cpu().numpy().tobytes())
    assert got.shape == (ny, nx, 4)
    assert np.array_equal(got, want)
    assert np.array_equal(pix.cpu().numpy(), want)
    if kind == "const" and (nx, ny) == (321, 7):
        # every row is a literal pixel and six matches: a few dozen bytes against 1285
        assert nidat < ny * (1 + 4 * nx) / 8


def test_png_encode_refuses_bad_arguments():
    with pytest.raises(ValueError):
        D.png_encode(torch.zeros((2, 4, 4)))                                  # not on the device
    with pytest.raises(ValueError):
        D.png_encode(torch.zeros((3, 4, 4), device="cuda"))                   # not a colour pair
    with pytest.raises(ValueError):
        D.png_encode(torch.zeros((2, 4, 0), device="cuda"))                   # empty
    L = D.lib()
    a, b = D.ctypes.c_longlong(0), D.ctypes.c_longlong(0)
    assert L.tclb_enc_png_bytes(1 << 15, 1 << 14, D.ctypes.byref(a), D.ctypes.byref(b)) != 0    # 2^31 bytes
    assert L.tclb_enc_png_bytes(0, 5, D.ctypes.byref(a), D.ctypes.byref(b)) != 0


def test_write_png_host_and_device_agree(tmp_path, monkeypatch):
    from tclb_amd.lattice import Lattice
    nx, ny = 96, 20
    lat = Lattice("d2q9", (nx, ny, 1), device=torch.device("cuda"))
    lat.set_flags(np.full((lat.NZ, lat.NY, nx), lat.model.node_type("MRT").value, dtype=np.uint32))
    lat.set_setting("Viscosity", 0.1)
    lat.set_setting("GravitationX", 1e-4)
    lat.init()
    for x in range(10, 14):
        for y in range(2, 6):
            lat.draw_wall(x, y, kind="Solid")
    lat.iterate(20)
    calls = []
    encode = D.png_encode
    monkeypatch.setattr(D, "png_encode", lambda *a, **k: calls.append(1) or encode(*a, **k))
    ph, pd = str(tmp_path / "h.png"), str(tmp_path / "d.png")
    ih = render.write_png(lat, ph, encode="host")
    assert not calls
    idev = render.write_png(lat, pd, encode="device")
    assert len(calls) == 1
    assert np.array_equal(ih, idev)
    assert tuple(ih[ny - 1 - 3, 11]) == (0, 255, 0, 255) and ih[ny - 1 - 10, 30, 0] > 0
    assert np.array_equal(_decode(open(ph, "rb").read())[0], ih)
    assert np.array_equal(_decode(open(pd, "rb").read())[0], ih)
    monkeypatch.setenv("TCLB_PNG_ENCODE", "host")
    assert np.array_equal(render.write_png(lat, pd, encode="device"), ih)
    assert len(calls) == 1
    assert np.array_equal(_decode(open(pd, "rb").read())[0], ih)
    monkeypatch.delenv("TCLB_PNG_ENCODE")
    with pytest.raises(ValueError):
        render.write_png(Lattice("d2q9", (8, 8, 1), device=torch.device("cpu")), pd, encode="device")
