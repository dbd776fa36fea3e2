"""Reference grammar of the control callbacks <PID>, <Keep> and the <Failcheck> region
(tclb_amd/handlers/core.py; reference src/Handlers/cbPID.cpp:5-131, cbKeep.cpp:5-73,
cbFailcheck.cpp:5-40) on a small d2q9 channel.

Every expected value is recomputed here from the reference's formulas and the globals
the run itself produced: a probe callback stacked behind the handler under test records,
at each firing, the globals and the table of zonal settings.  The replays use the same
double arithmetic in the same order as the handlers, so they must agree to rounding
(1e-12 relative).

The check functions take the device, so that tests/test_gpu_control_handlers.py runs the
same cases on the HIP executor."""
import os
import xml.etree.ElementTree as ET

import pytest

from tclb_amd import handlers  # noqa: F401
from tclb_amd.handlers.base import Callback, HandlerError, register
from tclb_amd.solver import ITER_NORM, Solver

CASE = """<?xml version="1.0"?>
<CLBConfig version="2.0" output="output/">
  <Geometry nx="32" ny="10">
    <MRT><Box/></MRT>
    <WVelocity name="inlet"><Box nx="1"/></WVelocity>
    <EPressure name="outlet"><Box dx="-1"/></EPressure>
    <Inlet><Box dx="2" nx="1"/></Inlet>
    <Outlet><Box dx="-3" nx="1"/></Outlet>
    <Wall mask="ALL"><Channel/></Wall>
  </Geometry>
  <Model>
    <Param name="VelocityX" value="0.01"/>
    <Param name="VelocityX" value="0.02" zone="inlet"/>
    <Param name="Viscosity" value="0.1"/>
  </Model>
  {body}
</CLBConfig>"""

REL = 1e-12


@register("TestProbe")
class Probe(Callback):
    """records iteration, iteration type, globals and the zonal settings table; it does
    not ask for globals itself, so what it sees is what the handlers before it forced"""

    def do_it(self):
        s = self.solver
        lat = s.lattice
        if not hasattr(s, "probe"):
            s.probe = []
        s.probe.append({"iter": s.iter, "iter_type": s.iter_type, "globals": dict(lat.globals),
                        "zvals": lat.zvals.copy()})
        return 0


@register("TestPlantNaN")
class PlantNaN(Callback):
    """one density of the node (x, y) becomes NaN"""

    def do_it(self):
        lat = self.solver.lattice
        x, y = int(self.node.get("x")), int(self.node.get("y"))
        lat.snaps[lat.cur][0, lat.gz, lat.gy + y, x] = float("nan")
        return 0


def run(tmp_path, body, device="cpu"):
    os.chdir(tmp_path)
    root = ET.fromstring(CASE.format(body=body))
    s = Solver("d2q9", root, conffile=str(tmp_path / "case.xml"), device=device)
    s.run()
    return s


def zval(s, rec, name, zone):
    lat = s.lattice
    return float(rec["zvals"][lat.zsettings.index(name), lat.zone_names[zone]])


def close(a, b):
    return abs(a - b) <= REL * max(abs(a), abs(b))


# ------------------------------------------------------------------------------- PID
def pid_replay(gs, sval, target, dt, itime=1.0, dtime=1.0, scale=1.0):
    """reference cbPID::DoIt (cbPID.cpp:103-120) over the recorded globals"""
    integral, old_err, out = 0.0, 0.0, []
    for g in gs:
        err = target - g
        integral = integral + (old_err + err) * dt / 2.0
        derivative = (err - old_err) / dt
        control = err + integral / itime + derivative * dtime
        old_err = err
        out.append(sval + control * scale)
    return out


def check_pid(tmp_path, device, times, zone=True):
    attrs = {"": {}, "explicit": {"IntegrationTime": 50.0, "DerivativeTime": 2.0, "scale": 0.1}}[times]
    xml_attrs = "".join(f' {k}="{v:g}"' for k, v in attrs.items()) + (' zone="inlet"' if zone else "")
    s = run(tmp_path, '<Solve Iterations="20">'
            f'<PID integral="OutletFlux" target="0.01" control="VelocityX" Iterations="5"{xml_attrs}/>'
            '<TestProbe Iterations="5"/></Solve><TestProbe/>', device)
    fired, after = s.probe[:-1], s.probe[-1]
    assert [r["iter"] for r in fired] == [5, 10, 15, 20]
    gs = [r["globals"]["OutletFlux"] for r in fired]
    assert len(set(gs)) == 4 and all(g != 0 for g in gs)          # fresh globals at every firing
    sval = 0.02 if zone else 0.01                                   # the named zone, or zone 0
    want = pid_replay(gs, sval, 0.01, 5.0, attrs.get("IntegrationTime", 1.0), attrs.get("DerivativeTime", 1.0),
                      attrs.get("scale", 1.0))
    zones = sorted(s.lattice.zone_names)
    assert {"DefaultZone", "inlet", "outlet"} <= set(zones)
    for r, w in zip(fired, want):
        assert w != sval
        for z in zones:
            if zone and z != "inlet":
                assert zval(s, r, "VelocityX", z) == 0.01, (r["iter"], z)
            else:
                assert close(zval(s, r, "VelocityX", z), w), (r["iter"], z, zval(s, r, "VelocityX", z), w)
        assert r["iter_type"] != ITER_NORM
    assert after["iter"] == 20 and after["iter_type"] == ITER_NORM    # restored behind the Solve
    assert s.iter_type == ITER_NORM


@pytest.mark.parametrize("times", ["", "explicit"])
def test_pid_reference_grammar_replay(tmp_path, times):
    check_pid(tmp_path, "cpu", times)


def test_pid_without_zone_writes_every_zone(tmp_path):
    check_pid(tmp_path, "cpu", "explicit", zone=False)


@pytest.mark.parametrize("attrs", ['integral="OutletFlux" control="VelocityX"',                    # no target
                                   'integral="NoSuchGlobal" target="0.01" control="VelocityX"',
                                   'integral="OutletFlux" target="0.01" control="Viscosity"',      # not zonal
                                   'integral="OutletFlux" target="0.01"',                          # no control
                                   'integral="OutletFlux" target="0.01" control="VelocityX" zone="nozone"'])
def test_pid_errors(tmp_path, attrs):
    with pytest.raises(HandlerError):
        run(tmp_path, f'<Solve Iterations="5"><PID {attrs} Iterations="5"/></Solve>')


def test_pid_old_grammar_law_and_restore(tmp_path):
    s = run(tmp_path, '<Solve Iterations="10"><PID OutletFlux="0.01" control="VelocityX" zone="inlet" P="0.5" '
            'Iterations="5"/><TestProbe Iterations="5"/></Solve><TestProbe/>')
    for r in s.probe[:2]:
        assert close(zval(s, r, "VelocityX", "inlet"), 0.5 * (0.01 - r["globals"]["OutletFlux"]))
        assert zval(s, r, "VelocityX", "outlet") == 0.01
    assert s.probe[-1]["iter_type"] == ITER_NORM and s.iter_type == ITER_NORM


# ------------------------------------------------------------------------------- Keep
def keep_weight(kind, thr, g, force):
    """reference cbKeep::DoIt (cbKeep.cpp:49-62)"""
    v = (thr - g) * force
    if kind == "Above":
        return v if v > 0 else 0.0
    if kind == "Below":
        return v if v < 0 else 0.0
    return v


def check_keep(tmp_path, device, kind, thr):
    s = run(tmp_path, f'<Solve Iterations="10"><Keep What="PressureLoss" {kind}="{thr:g}" Force="3" Iterations="5"/>'
            '<TestProbe Iterations="5"/></Solve><TestProbe/>', device)
    fired = s.probe[:-1]
    assert [r["iter"] for r in fired] == [5, 10]
    gs = [r["globals"]["PressureLoss"] for r in fired]
    assert gs[0] != gs[1] and all(g != 0 and abs(g) < 1e3 for g in gs)      # fresh, and well inside +-1e6
    for r, g in zip(fired, gs):
        w = keep_weight(kind, thr, g, 3.0)
        assert (w == 0.0) == ((kind, thr > 0) in (("Above", False), ("Below", True)))
        for z in s.lattice.zone_names:
            assert close(zval(s, r, "PressureLossInObj", z), w) if w else zval(s, r, "PressureLossInObj", z) == 0.0
    assert s.probe[-1]["iter_type"] == ITER_NORM and s.iter_type == ITER_NORM


@pytest.mark.parametrize("thr", [1e6, -1e6])
@pytest.mark.parametrize("kind", ["Above", "Below", "Equal"])
def test_keep_reference_grammar(tmp_path, kind, thr):
    check_keep(tmp_path, "cpu", kind, thr)


@pytest.mark.parametrize("attrs", ['Above="1"',                                   # no What
                                   'What="PressureLoss"',                         # no comparison
                                   'What="NoSuchGlobal" Above="1"',
                                   'What="Objective" Above="1"'])                 # no ObjectiveInObj setting
def test_keep_errors(tmp_path, attrs):
    with pytest.raises(HandlerError):
        run(tmp_path, f'<Solve Iterations="5"><Keep {attrs} Iterations="5"/></Solve>')


def test_keep_checks_above_before_below(tmp_path):
    """with more than one comparison the reference takes Above, then Below, then Equal"""
    s = run(tmp_path, '<Solve Iterations="5"><Keep What="PressureLoss" Equal="7" Below="1e6" Above="1e6" '
            'Iterations="5"/><TestProbe Iterations="5"/></Solve>')
    r, = s.probe
    w = keep_weight("Above", 1e6, r["globals"]["PressureLoss"], 1.0)
    assert w > 0 and close(zval(s, r, "PressureLossInObj", "inlet"), w)


def test_keep_old_spelling(tmp_path):
    """<Keep PressureLossAbove=> keeps its arithmetic, now with the globals of each firing"""
    s = run(tmp_path, '<Solve Iterations="10"><Keep PressureLossAbove="1e6" Force="3" Iterations="5"/>'
            '<TestProbe Iterations="5"/></Solve>')
    assert len(s.probe) == 2
    for r in s.probe:
        g = r["globals"]["PressureLoss"]
        assert g != 0 and close(zval(s, r, "PressureLossInObj", "outlet"), 3.0 * (1e6 - g))
    assert s.probe[0]["globals"]["PressureLoss"] != s.probe[1]["globals"]["PressureLoss"]
    assert s.iter_type == ITER_NORM


# -------------------------------------------------------------------------- Failcheck
# a NaN planted at x = 16 reaches x = 12..20 at most in 4 iterations (one node per step)
FAILCHECK_BODY = ('<TestPlantNaN x="16" y="5"/><Solve Iterations="4">'
                  '<Failcheck Iterations="1" {region}><TestProbe/></Failcheck></Solve>')


def check_failcheck(tmp_path, device, region, stops):
    s = run(tmp_path, FAILCHECK_BODY.format(region=region), device)
    if stops:
        assert s.iter == 1
        assert [r["iter"] for r in s.probe] == [1]          # the Failcheck's children ran, once
    else:
        assert s.iter == 4 and not hasattr(s, "probe")


def test_failcheck_region_away_from_nan_runs_on(tmp_path):
    check_failcheck(tmp_path, "cpu", 'nx="8"', stops=False)


def test_failcheck_region_negative_offset_away_from_nan(tmp_path):
    check_failcheck(tmp_path, "cpu", 'dx="-8" dy="2" ny="-2"', stops=False)     # x 24..31, y 2..7


def test_failcheck_region_with_nan_stops(tmp_path):
    check_failcheck(tmp_path, "cpu", 'dx="12" nx="8"', stops=True)


def test_failcheck_without_region_stops(tmp_path):
    check_failcheck(tmp_path, "cpu", "", stops=True)


def test_failcheck_empty_region_is_an_error(tmp_path):
    with pytest.raises(HandlerError):
        run(tmp_path, '<Solve Iterations="2"><Failcheck Iterations="1" dx="40" nx="4"/></Solve>')


DIST_CASE = CASE.format(body="""<RunPython>
y = 7 - lattice.slab.offset[1]
if 0 &lt;= y &lt; lattice.shape[1]:
    lattice.snaps[lattice.cur][0, lattice.gz, lattice.gy + y, 16] = float("nan")
</RunPython>
  <Log Iterations="1"/>
  <Solve Iterations="4"><Failcheck Iterations="1" {region}><DumpSettings name="Last"/></Failcheck></Solve>""")


def test_failcheck_region_two_ranks(tmp_path):
    """2 gloo ranks split y = 0..4 | 5..9.  The NaN sits at y = 7 on rank 1 and reaches
    y = 3..9 at most in 4 iterations: a region y = 0..2 (all on rank 0) runs to the end; a
    region y = 6..8 (all on rank 1, nothing of it on rank 0) stops every rank at once"""
    from test_dist_xml import _run
    for tag, region, iters in (("clean", 'ny="3"', 4), ("hit", 'dy="6" ny="3"', 1)):
        d = tmp_path / tag
        d.mkdir()
        (d / "case.xml").write_text(DIST_CASE.format(region=region))
        _run(d, "d2q9", "case.xml", 2)
        rows = open(d / "output" / "case_Log_P00_00000000.csv").read().splitlines()
        assert len(rows) == 1 + iters, (tag, rows)
        assert (d / "output" / "case_Last_P00_00000001.csv").exists() == (iters == 1)


def test_schema_lists_reference_attributes():
    """the XSD's handler elements carry the attributes of the reference grammar"""
    from tclb_amd.tools import docgen
    hs = docgen.handler_elements()
    want = {"PID": {"integral", "target", "control", "zone", "IntegrationTime", "DerivativeTime", "scale"},
            "Keep": {"What", "Above", "Below", "Equal", "Force"},
            "Failcheck": {"dx", "dy", "dz", "nx", "ny", "nz"},
            "Threshold": {"Levels", "Level"}, "ThresholdNow": {"Level"},
            "FDTest": {"order", "parameters", "h", "hmin", "hmax", "levels"}}
    for tag, attrs in want.items():
        assert attrs <= set(hs[tag]), (tag, attrs - set(hs[tag]))
