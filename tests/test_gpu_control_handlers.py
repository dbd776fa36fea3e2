"""The control callbacks of tests/test_control_handlers.py on the HIP executor: the same
32x10 d2q9 channel, the same replays from the run's own globals (1e-12 relative, no
CPU-vs-GPU tolerance), and the Failcheck region on the quantity tensor of the device."""
import pytest

import test_control_handlers as cases

pytestmark = pytest.mark.gpu


def test_pid_reference_grammar_replay_gpu(tmp_path):
    cases.check_pid(tmp_path, "cuda", "explicit")


def test_keep_reference_grammar_gpu(tmp_path):
    cases.check_keep(tmp_path, "cuda", "Above", 1e6)


def test_failcheck_region_away_from_nan_runs_on_gpu(tmp_path):
    cases.check_failcheck(tmp_path, "cuda", 'nx="8"', stops=False)


def test_failcheck_region_with_nan_stops_gpu(tmp_path):
    cases.check_failcheck(tmp_path, "cuda", 'dx="12" nx="8"', stops=True)
