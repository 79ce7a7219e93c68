"""The refusals of the four run entry points (rbl_ensemble_run, _run_jointed, _run_observed, _run_driven) against the table in
tests/golden/ensemble_run_refusals.json, which tools/record_run_refusals.py wrote with the library of the commit before the four
became one request path: every case's status, message -- the name that leads it included -- and what the call left in
rbl_run_out, byte for byte.  Single faults are those of the four *_cpu.py files' refusal tests; pairs of faults from two layers pin
the order.  The cases live in the recorder, which this file replays.

The CPU cases are decided on a context without an ensemble and touch no device.  The cases that need R run on the GPU."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_run_refusals", os.path.join(ROOT, "tools", "record_run_refusals.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec


def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "ensemble_run_refusals.json")))


def _same(rows, golden):
    assert [r[:2] for r in rows] == [g[:2] for g in golden], "the recorder's cases are not the recorded ones: record again on the parent"
    for row, g in zip(rows, golden):
        assert row == g, "\n  now:      %r\n  recorded: %r" % (row, g)


def test_the_table_holds_every_entry_point_and_the_pairs_that_pin_the_order():
    g = _golden()
    assert len(g["cpu"]) >= 200 and len(g["gpu"]) >= 15
    assert {r[0] for r in g["cpu"]} == {"run", "run_jointed", "run_observed", "run_driven"}
    assert all(r[2] != 0 for r in g["cpu"] + g["gpu"])
    said = {(r[0], r[1]): r[3] for r in g["cpu"]}
    pair = '{"change": {"o.n_steps": 0, "obs.size": 8}}'
    assert said[("run_observed", pair)].startswith("ensemble_run_observed: obs.size")
    empty = '{"change": {"d.cos_amp": null, "d.lockin": 0, "d.n_phases": 0, "d.start_sets": 0, "o.n_steps": 0}, "observed": true}'
    assert said[("run_driven", empty)].startswith("ensemble_run: n_steps must be >= 1")


def test_every_refusal_decided_without_an_ensemble_is_the_recorded_one():
    rec = _recorder()
    _same(rec.replay_cpu(*rec.load(ROOT)), _golden()["cpu"])


@pytest.mark.gpu
def test_every_refusal_that_needs_the_replica_count_is_the_recorded_one_and_the_ensemble_still_steps():
    rec = _recorder()
    _same(rec.replay_gpu(*rec.load(ROOT)), _golden()["gpu"])
