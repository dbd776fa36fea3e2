"""TCLB_GEOMETRY = auto | host | device: where a Geometry is painted (Geometry.on_device)."""
import xml.etree.ElementTree as ET

import pytest
import torch

from tclb_amd.geometry.geometry import Geometry
from tclb_amd.lattice import Lattice
from tclb_amd.models import registry

XML = '<Geometry nx="16" ny="8"><MRT><Box/></MRT><Wall mask="ALL"><Sphere dx="2" nx="6" dy="1" ny="6"/></Wall></Geometry>'


@pytest.mark.parametrize("where, error", [("device", "needs a lattice on a GPU"), ("bogus", "none of auto, host, device"),
                                          (None, None), ("auto", None), ("host", None)])
def test_switch_on_a_cpu_lattice(where, error, monkeypatch):
    if where is None:
        monkeypatch.delenv("TCLB_GEOMETRY", raising=False)
    else:
        monkeypatch.setenv("TCLB_GEOMETRY", where)
    g = Geometry(registry.get("d2q9"), (16, 8, 1), 0, 8, 1, 1)
    g.lattice = Lattice("d2q9", (16, 8, 1), device=torch.device("cpu"))
    if error:
        with pytest.raises(ValueError, match=error):
            g.load(ET.fromstring(XML))
        return
    g.load(ET.fromstring(XML))
    assert g.device_paints == 0 and g.device_flags() is None
    assert (g.flags == g.model.node_type("Wall").value).sum() > 10
