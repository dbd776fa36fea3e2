"""Lattice.gather on the HIP executor (k_gather, executor_hip.hpp): the windows of
test_gather.py against Lattice.quantity cropped on the same device and against the CPU
gather, for the plain d3q27 / d2q9 nodes, a stencil quantity (d3q27_pf_velocity), a heavy
get_quantity (d3q27q27_cm_cht: more than 256 registers) and the shifted-storage pop
(d3q27 mixed-shift); and the memory bound of a one-plane output."""
import pytest
import torch

import gather_cases as G

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]

CONFIGS = [("d3q27", "double"), ("d3q27", "mixed-shift"), ("d2q9", "double"), ("d3q27_pf_velocity", "double"),
           ("d3q27q27_cm_cht", "double")]
CASES = [(m, p, i) for m, p in CONFIGS for i in range(len(G.WINDOWS_3D))]


@pytest.mark.parametrize("name,precision,wi", CASES)
def test_gather_on_gpu(name, precision, wi):
    lat = G.case(name, "cuda", precision)
    cpu = G.case(name, "cpu", precision)
    assert lat.lib.kind == "hip" and cpu.lib.kind == "cpu"
    win = G.windows_of(name)[wi]
    names = G.plain_names(lat)
    scales = [G.scale_of(k) for k in range(len(names))]
    ref = G.reference(name, "cuda", precision)
    for il in (False, True):
        other = cpu.gather(names, win, scales=scales, interleave=il)
        G.check_against_quantity(lat, ref, win, il, other=other)
    other = cpu.gather(names, win, scales=scales, interleave=True, dtype=torch.float32)
    G.check_against_quantity(lat, ref, win, True, dtype=torch.float32, other=other)


def test_flags_region_on_gpu():
    import numpy as np
    lat = G.case("d3q27", "cuda")
    assert lat.lib.kind == "hip"
    win = (65, 2, 4, 31, 3, 1)
    assert np.array_equal(lat.get_flags(win), G.crop(lat.get_flags(), win, lat.shape))


def test_one_plane_output_memory_bound():
    """a one-plane gather of every quantity allocates less than one full-lattice scalar:
    the plane's whole output (7 fp64 values per node of 128 x 64) is 7/64 of a
    128 x 64 x 64 scalar, where a quantity pass over the whole slab holds at least three"""
    import model_cases
    shape = (128, 64, 64)
    lat = model_cases.run("d3q27", "cuda", steps=1, shape=shape)
    assert lat.lib.kind == "hip"
    names = G.plain_names(lat)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    got = lat.gather(names, (0, 0, 31, 128, 64, 1), interleave=True)
    fl = lat.get_flags((0, 0, 31, 128, 64, 1))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < 128 * 64 * 64 * 8, rise
    assert fl.shape == (1, 64, 128)
    want = lat.quantity("U")[:, 31:32]
    atol = 1e-10 * lat.quantity("U").abs().max().item() + 1e-12 * lat.fields_interior().abs().max().item()
    assert torch.allclose(got["U"].permute(3, 0, 1, 2), want, atol=atol, rtol=G.RTOL)
