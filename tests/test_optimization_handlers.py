"""Reference grammar of <Threshold Levels=>, <ThresholdNow> and the <FDTest> h sweep with
its CSV (tclb_amd/handlers/optimization.py; reference src/Handlers/acThreshold.cpp:5-52,
acThresholdNow.cpp:5-44, acFDTest.cpp:5-146) on the topology-optimisation model d2q9_adj.
Expected values are recomputed here from the reference's formulas."""
import math
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from tclb_amd import handlers  # noqa: F401
from tclb_amd.handlers.base import Callback, HandlerError, register
from tclb_amd.handlers.optimization import PAR_GET, _get_all, _set_all
from tclb_amd.solver import Solver

# the case of tests/test_optimization.py
CASE = """<?xml version="1.0"?>
<CLBConfig version="2.0" output="output/">
  <Geometry nx="24" ny="10">
    <MRT><Box/></MRT>
    <WVelocity><Box nx="1"/></WVelocity>
    <EPressure><Box dx="-1"/></EPressure>
    <Inlet><Box dx="2" nx="1"/></Inlet>
    <Outlet><Box dx="-3" nx="1"/></Outlet>
    <DesignSpace name="des"><Box dx="8" nx="6" dy="2" ny="6"/></DesignSpace>
    <Wall mask="ALL"><Channel/></Wall>
  </Geometry>
  <Model>
    <Param name="Velocity" value="0.01"/>
    <Param name="nu" value="0.1"/>
    <Param name="PorocityTheta" value="-2"/>
    <Param name="Porocity" value="0.4" zone="des"/>
    <Param name="PressureLossInObj" value="-1"/>
    <Param name="MaterialPenaltyInObj" value="-0.0001"/>
  </Model>
  {design}
  {body}
</CLBConfig>"""

NPAR = 36
RAMP = (np.arange(NPAR) + 0.5) / NPAR          # strictly inside (0, 1), no value on a level


@register("TestRamp")
class Ramp(Callback):
    """the design parameters become a ramp, so that threshold levels separate them"""

    def do_it(self):
        _set_all(self.solver, RAMP)
        return 0


@register("TestRecord")
class Record(Callback):
    def do_it(self):
        s = self.solver
        if not hasattr(s, "record"):
            s.record = []
        s.record.append((s.lattice.get_setting("Threshold"), _get_all(s, PAR_GET)))
        return 0


def run(tmp_path, design, body):
    os.chdir(tmp_path)
    root = ET.fromstring(CASE.format(design=design, body=body))
    s = Solver("d2q9_adj", root, conffile=str(tmp_path / "case.xml"), device="cpu")
    s.run()
    return s


# -------------------------------------------------------------------------- Threshold
def test_threshold_levels_sweep(tmp_path):
    s = run(tmp_path, "<InternalTopology/>", '<TestRamp/><Threshold Levels="3"><TestRecord/></Threshold>')
    assert [th for th, _ in s.record] == [0.0, 0.5, 1.0]
    for th, x in s.record:
        assert x.shape == (NPAR,)
        assert np.array_equal(x, (RAMP > th).astype(np.float64)), th      # from the start, exactly 0.0 / 1.0
    assert s.record[0][1].sum() == NPAR and s.record[1][1].sum() == NPAR // 2
    assert not s.record[2][1].any()                                       # nothing exceeds level 1
    assert s.lattice.get_setting("Threshold") == 1.0


@pytest.mark.parametrize("body", ['<Threshold Levels="1"><TestRecord/></Threshold>',
                                  '<Threshold Levels="0"/>'])
def test_threshold_levels_below_two(tmp_path, body):
    with pytest.raises(HandlerError):
        run(tmp_path, "<InternalTopology/>", body)


@pytest.mark.parametrize("tag", ['Threshold Levels="3"', "ThresholdNow"])
def test_threshold_without_parameters(tmp_path, tag):
    with pytest.raises(HandlerError):
        run(tmp_path, "", f"<{tag}/>")


def test_threshold_without_levels_as_before(tmp_path):
    """bare <Threshold>: once, to the bounds, children not run, setting untouched"""
    s = run(tmp_path, "<InternalTopology/>", '<Param name="Threshold" value="0.3"/><TestRamp/>'
            '<Threshold Level="0.5"><TestRecord/></Threshold><TestRecord/>')
    (th, x), = s.record
    assert th == 0.3
    assert np.array_equal(x, (RAMP > 0.5).astype(np.float64))
    s = run(tmp_path, "<InternalTopology/>", '<Param name="Threshold" value="0.3"/><TestRamp/><Threshold/><TestRecord/>')
    (th, x), = s.record
    assert th == 0.3 and np.array_equal(x, (RAMP > 0.3).astype(np.float64))


@pytest.mark.parametrize("attr,level", [("", 0.5), (' Level="0.3"', 0.3)])
def test_threshold_now(tmp_path, attr, level):
    s = run(tmp_path, "<InternalTopology/>", f'<Param name="Threshold" value="0.9"/><TestRamp/><ThresholdNow{attr}/>'
            '<TestRecord/>')
    (th, x), = s.record
    assert th == level
    assert np.array_equal(x, (RAMP > level).astype(np.float64))
    assert 0 < x.sum() < NPAR


# ----------------------------------------------------------------------------- FDTest
ADJOINT = '<Adjoint type="unsteady"><Solve Iterations="20"/></Adjoint>'


def read_csv(path):
    lines = open(path).read().splitlines()
    return lines[0], [[float(v) for v in ln.split(", ")] for ln in lines[1:]]


def central(val, o):
    """reference acFDTest.cpp:129-139 on val[m + o], m = -o..o; highest order first"""
    v = lambda m: val[o + m]   # noqa: E731
    out = []
    if o >= 3:
        out.append((v(3) + 9 * (-v(2) + 5 * (v(1) - v(-1)) + v(-2)) - v(-3)) / 60)
    if o >= 2:
        out.append((-v(2) + 8 * (v(1) - v(-1)) + v(-2)) / 12)
    out.append((v(1) - v(-1)) / 2)
    return out


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sweep")
    cwd = os.getcwd()
    try:
        s = run(tmp, "<InternalTopology/>",
                f'<FDTest parameters="3:4" order="4" hmin="2e-6" hmax="2e-4" levels="3">{ADJOINT}</FDTest>')
    finally:
        os.chdir(cwd)
    return s, tmp


def test_fdtest_sweep_csv(sweep):
    s, tmp = sweep
    assert s.outpath == "output/case"
    head, rows = read_csv(tmp / "output" / "case_FD_test.csv")
    assert head == ("Parameter, Value, Gradient, H, RightObj2, RightObj1, Objective, LeftObj1, LeftObj2, "
                    "CentralDiff2, CentralDiff1")
    assert len(rows) == 6 and all(len(r) == 11 for r in rows)
    assert [r[0] for r in rows] == [3, 3, 3, 4, 4, 4]
    lmin, lmax = math.log(2e-6), math.log(2e-4)
    for i, r in enumerate(rows):
        h = 0.5 * math.exp(lmin + ((lmax - lmin) * (i % 3)) / 2)         # dx = (1 - 0)/2 for InternalTopology
        assert abs(r[3] - h) <= 1e-15 * h, (i, r[3], h)
        assert abs(h - 10.0 ** (i % 3 - 6)) <= 1e-12 * h
        assert r[1] == 1.0 - 0.4                                          # w = 1 - Porocity at the start
        assert r[6] == rows[0][6]                                         # one objective at the start point
        d2, d1 = central(r[4:9], 2)
        print(f"row {i}: h {r[3]:.3g} gradient {r[2]:.16g} CentralDiff2 {r[9]:.16g} recomputed {d2 / r[3]:.16g} "
              f"CentralDiff1 {r[10]:.16g} recomputed {d1 / r[3]:.16g}")
        assert abs(r[9] - d2 / r[3]) <= 1e-12 * abs(r[9]), (i, r[9], d2 / r[3])
        assert abs(r[10] - d1 / r[3]) <= 1e-12 * abs(r[10]), (i, r[10], d1 / r[3])
        assert r[9] != 0 and len({r[4], r[5], r[7], r[8]}) == 4
        if i % 3 == 1:       # h = 1e-5: the step and tolerance of test_optimization.test_fdtest_topology
            assert abs(r[2] - r[9]) <= 1e-5 * abs(r[9]) + 1e-12, (i, r[2], r[9])


def test_fdtest_sweep_rows(sweep):
    s, tmp = sweep
    _, rows = read_csv(tmp / "output" / "case_FD_test.csv")
    assert len(s.fdtest) == 6
    for (k, adj, fd), r in zip(s.fdtest, rows):          # one per file row, in file order, highest order
        assert k == r[0] and abs(adj - r[2]) <= 1e-15 * abs(adj) and abs(fd - r[9]) <= 1e-15 * abs(fd)
    w = s.lattice.fields_interior()[s.model.field_index("w")].numpy()
    assert np.array_equal(w[0, 2:8, 8:14], np.full((6, 6), 1.0 - 0.4))   # start point restored


def test_fdtest_single_h_as_before_plus_csv(tmp_path):
    s = run(tmp_path, "<InternalTopology/>", f'<FDTest parameters="3:5" h="1e-5">{ADJOINT}</FDTest>')
    assert len(s.fdtest) == 3
    for i, adj, fd in s.fdtest:
        assert abs(adj - fd) <= 1e-5 * abs(fd) + 1e-12, (i, adj, fd)
        assert abs(fd) > 0
    head, rows = read_csv(tmp_path / "output" / "case_FD_test.csv")
    assert head == "Parameter, Value, Gradient, H, RightObj1, Objective, LeftObj1, CentralDiff1"
    assert [r[0] for r in rows] == [3, 4, 5] and all(r[3] == 1e-5 for r in rows)      # h is not scaled by dx
    for (i, adj, fd), r in zip(s.fdtest, rows):
        assert abs(adj - r[2]) <= 1e-15 * abs(adj)
        assert abs(fd - r[7]) <= 1e-12 * abs(fd)         # 0.5 (J+ - J-)/h against ((J+ - J-)/2)/h


@pytest.mark.parametrize("attrs", ['hmin="0"', 'hmax="-1"', 'levels="1"', 'levels="3" parameters="30:36"',
                                   'levels="3" parameters="5:3"'])
def test_fdtest_sweep_errors(tmp_path, attrs):
    with pytest.raises(HandlerError):
        run(tmp_path, "<InternalTopology/>", f'<FDTest {attrs}>{ADJOINT}</FDTest>')
