"""Device encoding of VTK payloads (csrc/device/encode.hip): ops.device.b64encode against
base64.b64encode, Lattice.flag_groups against the numpy expression of
Solver.output_fields, and write_vtk(encode="device") against encode="host" byte for byte."""
import base64
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

import gather_cases as G
from tclb_amd import handlers  # noqa: F401
from tclb_amd.io.vtk import CHUNK_MIN, read_vti
from tclb_amd.ops import device as D
from tclb_amd.solver import Solver

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
TRIP = 256 * 4 * 12           # bytes one work-group of k_b64 covers per loop trip (encode.hip)
SIZES = [0, 1, 2, 3, 4, 11, 12, 13, 23, 24, 25, 767, 768, 769, TRIP - 1, TRIP, TRIP + 1, 1000003]


def _dev(data: bytes):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


@pytest.mark.parametrize("n", SIZES)
def test_b64encode(n):
    data = np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8).tobytes()
    got = D.b64encode(_dev(data))
    assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == base64.b64encode(data)


def test_b64encode_every_symbol_in_every_position():
    """the alphabet rotated by 0-3 characters: each symbol in each position of a group"""
    text = b"".join(ALPHABET[r:] + ALPHABET[:r] for r in range(4))
    data = base64.b64decode(text)
    assert len(data) == 192
    # as float64: any dtype is encoded as its bytes
    src = _dev(data).view(torch.float64)
    assert D.b64encode(src).cpu().numpy().tobytes() == text


def test_b64encode_refuses_misaligned_pointer():
    buf = _dev(bytes(64))
    with pytest.raises(D.DeviceRuntimeError):
        D.b64encode(buf[1:])
    with pytest.raises(D.DeviceRuntimeError):
        D.b64encode(buf[:24], out=torch.empty(64, dtype=torch.uint8, device="cuda")[1:])
    torch.cuda.synchronize()


def test_b64encode_into_slice():
    data = np.random.default_rng(0).integers(0, 256, 1000, dtype=np.uint8).tobytes()
    want = base64.b64encode(data)
    big = torch.full((4096,), 0x7E, dtype=torch.uint8, device="cuda")
    got = D.b64encode(_dev(data), out=big[64:])
    assert got.data_ptr() == big.data_ptr() + 64 and got.numel() == len(want)
    host = big.cpu().numpy().tobytes()
    assert host[64:64 + len(want)] == want
    assert host[:64] == b"~" * 64 and host[64 + len(want):] == b"~" * (4096 - 64 - len(want))


def _groups(model):
    return [(g, model.group_masks[g], model.group_shift.get(g, 0)) for g in sorted(model.group_masks)
            if g not in ("ALL", "NONE")]


# d2q9q9_cm_cht: the catalog's 32-bit flags
FLAG_CASES = [(m, i) for m in ("d3q27", "d2q9", "d2q9q9_cm_cht") for i in range(len(G.WINDOWS_3D))]


@pytest.mark.parametrize("name,wi", FLAG_CASES)
def test_flag_groups(name, wi):
    lat = G.case(name, "cuda")
    assert lat.lib.kind == "hip" and lat.model.flag_bits == (32 if name == "d2q9q9_cm_cht" else 16)
    win = G.windows_of(name)[wi]
    groups = _groups(lat.model)
    flags = lat.get_flags(win)
    assert flags.any()
    got = lat.flag_groups([(m, s) for _, m, s in groups], win)
    assert len(got) == len(groups)
    for (g, m, s), a in zip(groups, got):
        assert a.dtype == torch.uint8 and a.is_contiguous()
        assert np.array_equal(a.cpu().numpy(), ((flags & m) >> s).astype(np.uint8)), g
    with pytest.raises(ValueError):
        lat.flag_groups([(1, 0)], (90, 0, 0, 10, 1, 1))


def test_flag_groups_int32_strided():
    """the 32-bit kernel with every bit in use (the d2q9q9_cm_cht case above has 32-bit flags
    but sets few of the high ones): a window (rows of 7: not a multiple of four;
    7 * 5 * 3 = 105: a ragged last dword) of a padded int32 array, masks above bit 16, more
    pairs than one launch takes"""
    full = np.random.default_rng(0).integers(0, 2 ** 32, (6, 9, 16), dtype=np.uint32)
    win = full[2:5, 1:6, 3:10]
    pairs = [(0xFF << s, s) for s in range(0, 25, 2)] + [(0xFFFFFFFF, 24), (0x80000000, 31), (0x00F0F000, 12),
                                                         (0xFFFFFFFF, 0), (0x7FFF0000, 17)]
    assert len(pairs) > D.FLAG_GROUPS_MAX
    dev = torch.from_numpy(full.view(np.int32)).cuda()[2:5, 1:6, 3:10]
    got = D.flag_groups(dev, pairs)
    for (m, s), a in zip(pairs, got):
        assert np.array_equal(a.cpu().numpy(), ((win & np.uint32(m)) >> np.uint32(s)).astype(np.uint8)), (m, s)


CHANNEL = """<?xml version="1.0"?>
<CLBConfig version="2.0" output="{out}/" permissive="true">
  <Geometry nx="{nx}" ny="{ny}" nz="{nz}">
    <MRT><Box/></MRT>
    <WVelocity name="Inlet"><Inlet/></WVelocity>
    <EPressure name="Outlet"><Outlet/></EPressure>
    <Wall mask="ALL"><Channel/></Wall>
  </Geometry>
  <Model>
    <Param name="VelocityX" value="0.02"/>
    <Param name="Viscosity" value="0.05"/>
    <Param name="Velocity" value="0.02"/>
    <Param name="nu" value="0.05"/>
  </Model>
  <Solve Iterations="20"/>
</CLBConfig>"""


@pytest.fixture(scope="module", params=[("d2q9", G.SHAPES[2]), ("d3q27", G.SHAPES[3])], ids=["d2q9", "d3q27"])
def solver(request, tmp_path_factory):
    model, (nx, ny, nz) = request.param
    tmp = tmp_path_factory.mktemp(model)
    s = Solver(model, ET.fromstring(CHANNEL.format(out=tmp, nx=nx, ny=ny, nz=nz)), conffile=str(tmp / "case.xml"),
               device="cuda")
    s.run()
    assert s.lattice.lib.kind == "hip" and s.iter == 20
    return s


@pytest.mark.parametrize("region", [None, (60, 1, 0, 10, 4, 1)], ids=["whole", "across-x64"])
def test_device_file_is_byte_identical(solver, region):
    s = solver
    what = ["all", "flag"]
    s.write_vtk("host", what, region, encode="host")
    # the smallest chunk (12 raw bytes): every field spans several chunks, and the 8-, 2- and
    # 1-byte fields of the 40-node region end in a ragged one
    s.write_vtk("dev", what, region, encode="device", chunk=CHUNK_MIN)
    host, dev = (open(s.out_iter_file(n, ".vti"), "rb").read() for n in ("host", "dev"))
    assert dev == host
    assert open(s.out_iter_file("dev", ".pvti")).read() == \
        open(s.out_iter_file("host", ".pvti")).read().replace("_host_", "_dev_")
    lreg, fields = s.output_fields(what, region)
    back = read_vti(s.out_iter_file("dev", ".vti"))
    assert [n for n, _, _ in fields] == list(back)
    for n, a, _ in fields:
        assert back[n].dtype == a.dtype and np.array_equal(back[n], a), n
    assert np.abs(back["U"]).max() > 0
