"""VTK ImageData output (.vti per rank + .pvti index on rank 0).

Same layout as the reference writer (reference: src/vtkOutput.cpp:54-200,
src/vtkLattice.cpp:9-54): CellData, inline base64 binary with a separately encoded
UInt32 byte-count header, one piece per rank, flag groups written as UInt8 fields
(value >> shift), quantities scaled back to SI units."""
from __future__ import annotations

import base64
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_VTK_T = {np.dtype(np.float64): "Float64", np.dtype(np.float32): "Float32", np.dtype(np.uint8): "UInt8",
          np.dtype(np.uint16): "UInt16", np.dtype(np.uint32): "UInt32", np.dtype(np.int32): "Int32"}


def _b64(a: np.ndarray) -> str:
    data = np.ascontiguousarray(a).tobytes()
    return (base64.b64encode(np.uint32(len(data)).tobytes()) + base64.b64encode(data)).decode()


def extent(reg) -> str:
    x0, y0, z0, nx, ny, nz = reg
    return f"{x0} {x0 + nx} {y0} {y0 + ny} {z0} {z0 + nz}"


def _vti_head(reg, spacing, origin) -> str:
    return ('<?xml version="1.0"?>\n<VTKFile type="ImageData" version="0.1" byte_order="LittleEndian">\n'
            f'<ImageData WholeExtent="{extent(reg)}" Origin="{origin[0]:g} {origin[1]:g} {origin[2]:g}" '
            f'Spacing="{spacing:g} {spacing:g} {spacing:g}">\n'
            f'<Piece Extent="{extent(reg)}">\n<CellData Scalars="rho" Vectors="velocity">\n')


def _array_open(t: str, name: str, nc: int) -> str:
    return f'<DataArray type="{t}" Name="{name}" format="binary" encoding="base64" NumberOfComponents="{nc}">\n'


_ARRAY_CLOSE = "\n</DataArray>\n"
_VTI_TAIL = "</CellData>\n</Piece>\n</ImageData>\n</VTKFile>\n"


def write_vti(path: str, total_reg, reg, fields: List[Tuple[str, np.ndarray, int]], spacing: float = 1.0,
              origin=(0.0, 0.0, 0.0), interleaved: bool = False):
    """fields: (name, array (nz,ny,nx) or (ncomp,nz,ny,nx), ncomp); interleaved: vectors
    come as (nz,ny,nx,ncomp), the layout of the file (Solver.output_fields), and are
    encoded without a copy"""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(_vti_head(reg, spacing, origin))
        for name, arr, nc in fields:
            a = np.asarray(arr)
            if nc > 1 and not interleaved:
                a = np.moveaxis(a, 0, -1)  # (nz,ny,nx,nc) interleaved components
            f.write(_array_open(_VTK_T[a.dtype], name, nc))
            f.write(_b64(a))
            f.write(_ARRAY_CLOSE)
        f.write(_VTI_TAIL)


def vtk_type(a) -> str:
    """the DataArray type name of a numpy array or a torch tensor"""
    if isinstance(a, np.ndarray):
        return _VTK_T[a.dtype]
    return _VTK_T[np.dtype(str(a.dtype).replace("torch.", ""))]


CHUNK_MIN = 16                   # one 12-byte group: the smallest text that concatenates
CHUNK_DEFAULT = 16 << 20       # measured best of 16, 64, 256 MiB (profiles/README.md, r08a)


def chunk_bytes(chunk: Optional[int] = None) -> int:
    """bytes of text per pipeline chunk of write_vti_device: the environment's
    TCLB_VTK_CHUNK, else `chunk`, else CHUNK_DEFAULT; rounded down to whole 16-character
    groups (12 raw bytes), so that the chunks' texts concatenate exactly"""
    c = int(os.environ.get("TCLB_VTK_CHUNK") or chunk or CHUNK_DEFAULT)
    return max(CHUNK_MIN, c // 16 * 16)


class EncodeSlots:
    """the staging memory of write_vti_device: two device and two pinned host slots of
    `size` bytes of text, a side stream for the copies and the events that order them;
    made once (Solver keeps one) and reused by every write"""

    def __init__(self, device, size: int):
        import torch
        self.device, self.size = torch.device(device), int(size)
        self.dev = [torch.empty(self.size, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.host = [torch.empty(self.size, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self.view = [memoryview(h.numpy()) for h in self.host]
        self.copy_stream = torch.cuda.Stream(self.device)
        self.encoded = [torch.cuda.Event() for _ in range(2)]
        self.copied = [torch.cuda.Event() for _ in range(2)]


def write_vti_device(path: str, total_reg, reg, fields, spacing: float = 1.0, origin=(0.0, 0.0, 0.0),
                     chunk: Optional[int] = None, slots: Optional[EncodeSlots] = None):
    """write_vti for fields that lie on the device: (name, contiguous device tensor in the
    layout of the file — scalars (nz,ny,nx), vectors (nz,ny,nx,ncomp) — , ncomp).  The
    file is byte for byte the one write_vti writes from the same values.  Each payload is
    the byte count (encoded here) and the data encoded on the device (ops.device.b64encode)
    in chunks of chunk_bytes(chunk) characters: chunk k is encoded into device slot k % 2 on
    the current stream and copied into pinned slot k % 2 on the slots' side stream, ordered
    by events, while the host writes chunk k - 1 from its pinned slot.  slots: an
    EncodeSlots at least one chunk long, default a new one; the one used is returned."""
    import torch
    from ..ops import device as D
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    text = chunk_bytes(chunk)
    raw = text // 16 * 12
    jobs = []                                  # (field index, first byte, bytes) in file order
    flat = []
    for k, (name, t, nc) in enumerate(fields):
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"write_vti_device: field {name} is not a contiguous device tensor")
        flat.append(t.view(-1).view(torch.uint8))
        n = flat[-1].numel()
        jobs += [(k, o, min(raw, n - o)) for o in range(0, n, raw)] or [(k, 0, 0)]
    if slots is None or slots.size < text:     # one chunk long: only a larger chunk replaces them
        slots = EncodeSlots(fields[0][1].device if fields else "cuda", text)
    # the fields were produced on the device's current stream (Lattice.gather and flag_groups
    # launch on Lattice._stream(), which is that stream), so encoding there needs no event
    main = torch.cuda.current_stream(slots.device)

    def issue(j):
        k, o, n = jobs[j]
        s = j % 2
        if n == 0:
            return
        main.wait_event(slots.copied[s])       # the slot's previous text has left the device
        m = D.b64encode(flat[k][o:o + n], out=slots.dev[s], stream=main.cuda_stream).numel()
        slots.encoded[s].record(main)
        slots.copy_stream.wait_event(slots.encoded[s])
        with torch.cuda.stream(slots.copy_stream):
            slots.host[s][:m].copy_(slots.dev[s][:m], non_blocking=True)
        slots.copied[s].record(slots.copy_stream)

    with open(path, "wb") as f:
        f.write(_vti_head(reg, spacing, origin).encode())
        if jobs:
            issue(0)
        for j, (k, o, n) in enumerate(jobs):
            if j + 1 < len(jobs):
                issue(j + 1)                   # encodes and copies while this chunk is written
            if o == 0:
                name, t, nc = fields[k]
                f.write(_array_open(vtk_type(t), name, nc).encode())
                f.write(base64.b64encode(np.uint32(flat[k].numel()).tobytes()))
            if n:
                slots.copied[j % 2].synchronize()
                f.write(slots.view[j % 2][:4 * ((n + 2) // 3)])
            if o + n == flat[k].numel():
                f.write(_ARRAY_CLOSE.encode())
        f.write(_VTI_TAIL.encode())
    return slots


def write_pvti(path: str, total_reg, pieces: Sequence[Tuple[tuple, str]], fields: List[Tuple[str, str, int]],
               spacing: float = 1.0, origin=(0.0, 0.0, 0.0)):
    with open(path, "w") as f:
        f.write('<?xml version="1.0"?>\n<VTKFile type="PImageData" version="0.1" byte_order="LittleEndian">\n')
        f.write(f'<PImageData WholeExtent="{extent(total_reg)}" Origin="{origin[0]:g} {origin[1]:g} {origin[2]:g}" '
                f'Spacing="{spacing:g} {spacing:g} {spacing:g}">\n')
        for reg, src in pieces:
            f.write(f'<Piece Extent="{extent(reg)}" Source="{src}"/>\n')
        f.write('<PCellData Scalars="rho" Vectors="velocity">\n')
        for name, t, nc in fields:
            f.write(f'<PDataArray type="{t}" Name="{name}" NumberOfComponents="{nc}"/>\n')
        f.write("</PCellData>\n</PImageData>\n</VTKFile>\n")


def read_vti(path: str) -> Dict[str, np.ndarray]:
    """Minimal reader for our own .vti files (tests / compare tool)."""
    import xml.etree.ElementTree as ET
    root = ET.parse(path).getroot()
    piece = root.find("ImageData/Piece")
    e = [int(v) for v in piece.get("Extent").split()]
    nx, ny, nz = e[1] - e[0], e[3] - e[2], e[5] - e[4]
    out = {}
    inv = {v: k for k, v in _VTK_T.items()}
    for da in piece.find("CellData"):
        t = inv[da.get("type")]
        nc = int(da.get("NumberOfComponents", "1"))
        txt = da.text.strip()
        hdr = base64.b64decode(txt[:8])
        n = int(np.frombuffer(hdr, dtype=np.uint32)[0])
        data = base64.b64decode(txt[8:])[:n]
        a = np.frombuffer(data, dtype=t)
        a = a.reshape(nz, ny, nx, nc) if nc > 1 else a.reshape(nz, ny, nx)
        out[da.get("Name")] = a
    return out


def read_pvti(path: str) -> Dict[str, np.ndarray]:
    """assemble the pieces of a .pvti index into whole-extent arrays (tests, comparisons
    of runs on different rank counts)"""
    import xml.etree.ElementTree as ET
    root = ET.parse(path).getroot()
    img = root.find("PImageData")
    w = [int(v) for v in img.get("WholeExtent").split()]
    out: Dict[str, np.ndarray] = {}
    base = os.path.dirname(path)
    for piece in img.findall("Piece"):
        e = [int(v) for v in piece.get("Extent").split()]
        data = read_vti(os.path.join(base, piece.get("Source")))
        for name, a in data.items():
            if name not in out:
                shape = (w[5] - w[4], w[3] - w[2], w[1] - w[0]) + a.shape[3:]
                out[name] = np.zeros(shape, dtype=a.dtype)
            out[name][e[4] - w[4]:e[5] - w[4], e[2] - w[2]:e[3] - w[2], e[0] - w[0]:e[1] - w[0]] = a
    return out
