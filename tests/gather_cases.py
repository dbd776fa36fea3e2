"""Shared set-up of the Lattice.gather tests (CPU: test_gather.py, GPU: test_gpu_gather.py):
the windows, the lattices (built once per model and device) and the comparison of a
gather against the crop of Lattice.quantity."""
import functools

import torch

import model_cases

SHAPES = {2: (96, 7, 1), 3: (96, 6, 5)}
# (x0, y0, z0, nx, ny, nz), local interior coordinates: the whole interior, one node, a box
# across the 64-lane boundary of a row, a box on the far x and z faces, one full row
WINDOWS_3D = [None, (1, 1, 1, 1, 1, 1), (60, 0, 0, 10, 6, 5), (65, 2, 4, 31, 3, 1), (0, 5, 0, 96, 1, 1)]
WINDOWS_2D = [None if w is None else (w[0], w[1], 0, w[3], w[4], 1) for w in WINDOWS_3D]


def shape_of(name):
    from tclb_amd.models import registry
    return SHAPES[registry.get(name).dims]


def windows_of(name):
    from tclb_amd.models import registry
    return WINDOWS_2D if registry.get(name).dims == 2 else WINDOWS_3D


@functools.lru_cache(maxsize=None)
def case(name, device="cpu", precision="double"):
    """the lattice after 2 steps of the generic perturbed case; never stepped again"""
    return model_cases.run(name, device, steps=2, precision=precision, shape=shape_of(name))


def plain_names(lat):
    return [q.name for q in lat.model.quantities if not q.adjoint]


def scale_of(k):
    """a different unit scale per entry of a call"""
    return 1.5 if k % 2 == 0 else 0.25


@functools.lru_cache(maxsize=None)
def reference(name, device="cpu", precision="double"):
    """{quantity: (Lattice.quantity(name, scale) over the whole interior, atol)} with the
    catalog's quantity tolerance (tests/test_catalog.py): atol = 1e-10 max|q| + 1e-12 max|f|"""
    lat = case(name, device, precision)
    fmax = lat.fields_interior().abs().max().item() + 1e-300
    out = {}
    for k, n in enumerate(plain_names(lat)):
        q = lat.quantity(n, scale_of(k))
        out[n] = (q, 1e-10 * (q.abs().max().item() + 1e-300) + 1e-12 * fmax)
    return out


RTOL = 1e-10


def crop(a, win, shape):
    x0, y0, z0, wx, wy, wz = win or (0, 0, 0) + tuple(shape)
    return a[..., z0:z0 + wz, y0:y0 + wy, x0:x0 + wx]


def planar(a, interleave):
    """a gather result as (ncomp, nz, ny, nx)"""
    if a.dim() == 3:
        return a[None]
    return a.permute(3, 0, 1, 2) if interleave else a


def check_against_quantity(lat, ref, win, interleave, dtype=None, other=None):
    """gather of every plain quantity over `win` (two different scales in the call) against
    the crop of the reference; dtype=float32 on an fp64 lattice: against .to(float32) of
    the fp64 reference with one fp32 ulp (relative 2^-23) more.  other: a second result
    dict (e.g. the CPU gather) compared under the same tolerance."""
    names = plain_names(lat)
    got = lat.gather(names, win, scales=[scale_of(k) for k in range(len(names))], interleave=interleave,
                     dtype=dtype)
    assert set(got) == set(names)
    for n in names:
        q, atol = ref[n]
        want = crop(q, win, lat.shape)
        a = planar(got[n], interleave)
        vec = lat.model.quantities[[x.name for x in lat.model.quantities].index(n)].vector
        assert got[n].dtype == (dtype or lat.rdtype) and a.shape == want.shape, (n, a.shape, want.shape)
        assert got[n].dim() == (4 if vec else 3)
        rtol = RTOL
        if dtype == torch.float32 and lat.rdtype == torch.float64:
            want = want.to(torch.float32)
            rtol = RTOL + 2.0 ** -23
        assert torch.allclose(a, want.to(a.device), atol=atol, rtol=rtol), (n, win, (a - want.to(a.device)).abs().max().item())
        if other is not None:
            b = planar(other[n], interleave).to(a.device)
            assert torch.allclose(a, b, atol=atol, rtol=rtol), (n, win, "vs other", (a - b).abs().max().item())
    return got
