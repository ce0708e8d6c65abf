"""The fused step's schedule, call by call (cvhip/engine.py ClearStep._programs / _segments).

tests/step_traces.json is the output of tools/step_trace.py: for each configuration (the default schedules of every
mode, the forced data-parallel steps, and each kept schedule switch) the number of calls of every program of
`eng.graphs[n]` and a sha256 of its call list — name, lane and normalised arguments, pointer aliasing included — and
the step's segment layout.  Each test rebuilds one configuration's programs (nothing is launched) and compares; a
program that differs is printed call by call (`tools/step_trace.py --full` prints every list, to diff two commits).
bench.py addresses a call as program[index] and Program._event reuses its events by call position at capture time,
so the order and number of calls is part of the engine's contract; a schedule change on purpose regenerates the file
with the tool."""

import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("step_trace", os.path.join(ROOT, "tools", "step_trace.py"))
step_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(step_trace)

TRACE_FILE = os.path.join(ROOT, "tests", "step_traces.json")
CONFIGS = step_trace.configs()
SINGLE = [k for k, c in CONFIGS.items() if not c[4].get("dp")]
DP = [k for k, c in CONFIGS.items() if c[4].get("dp")]


@pytest.fixture(scope="module")
def recorded():
    with open(TRACE_FILE) as f:
        return json.load(f)


def _check(full, want):
    got = step_trace.digest(full)
    for key in step_trace.KEYS:
        assert got["programs"][key] == want["programs"][key], (key, full["programs"][key])
    assert got["segments"] == want["segments"]


def test_recorded_file_covers_the_configurations(recorded):
    assert list(recorded) == list(CONFIGS)
    with open(TRACE_FILE) as f:
        assert f.read() == step_trace.dumps(recorded)  # (the tool's own layout: one line per configuration)


@pytest.mark.parametrize("name", SINGLE)
def test_step_programs_match_the_recorded_trace(name, recorded):
    _check(step_trace.trace(name), recorded[name])


@pytest.mark.parametrize("name", DP)
def test_forced_dp_step_programs_match_the_recorded_trace(name, recorded):
    """The data-parallel programs, as tests/graph_coll_worker.py sets them up: a world-1 RCCL group in a child
    process with CVHIP_FORCE_DP=1 (one child per mode, under its own time limit)."""
    _check(step_trace.trace_dp_child(name, timeout=120), recorded[name])
