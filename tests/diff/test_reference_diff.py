"""Differential tests against the reference implementation (SURVEY §4 "Differential").

The same pipeline ran once on the reference (in its own process, with shims for its two missing
tiny dependencies; what it published is stored under ``tests/golden/reference_diff_*.json``) and
runs once on rocket_amd; everything a user can observe must agree: the full (capsule, event)
trace, the loss / lr published each iteration, metric values, final weights and the checkpoint directory layout.  The one intended
difference is the reference's quirk Q1: its default Checkpointer makes
``destroy`` raise after training; rocket_amd completes the destroy sequence.

With ``ROCKET_REFERENCE_DIR`` pointing at a reference checkout the reference side is run live
instead of read from the stored results (``_driver.py reference ...`` is also how they are made).
"""

import json
import os
import subprocess
import sys

REF = os.environ.get("ROCKET_REFERENCE_DIR")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(os.path.dirname(HERE), "golden")


def _run(which, scenario, tmp_path):
    work = tmp_path / which
    work.mkdir()
    out = tmp_path / f"{which}.json"
    env = dict(os.environ, PYTHONPATH=REPO, ACCELERATE_USE_CPU="1")
    cmd = [sys.executable, os.path.join(HERE, "_driver.py"), which, scenario, str(out), str(work)]
    if which == "reference":
        cmd.append(REF)
    r = subprocess.run(cmd, cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.load(open(out))


def _reference(scenario, tmp_path):
    if REF and os.path.isdir(os.path.join(REF, "rocket", "core")):
        return _run("reference", scenario, tmp_path)
    with open(os.path.join(GOLDEN, f"reference_diff_{scenario}.json")) as fh:
        return json.load(fh)


def _close(a, b, tol=1e-6):
    if a is None or b is None:
        return a is b
    if isinstance(a, list):
        return len(a) == len(b) and all(_close(u, v, tol) for u, v in zip(a, b))
    return abs(a - b) <= tol * max(1.0, abs(a))


def test_train_pipeline_matches_reference(tmp_path):
    """GA=2 over 6 batches x 2 epochs, StepLR, Checkpointer(save_every=4)."""
    ref, amd = _reference("train", tmp_path), _run("rocket_amd", "train", tmp_path)
    assert ref["error"] and "Illegal destroy request" in ref["error"]  # Q1, fixed here
    assert amd["error"] is None
    n = len(ref["trace"])
    assert amd["trace"][:n] == ref["trace"]
    assert [e for e in amd["trace"][n:]] == [[c, "destroy"] for c in
                                            ("Module", "Scheduler", "Optimizer", "Loss", "Dataset")]
    assert _close(ref["seen"], amd["seen"]), (ref["seen"], amd["seen"])
    assert _close(ref["params"], amd["params"])
    assert ref["ckpts"] == amd["ckpts"] and sorted(ref["ckpts"]) == ["003", "007", "011"]


def test_eval_looper_and_meter_match_reference(tmp_path):
    """Train looper + eval looper (grad disabled, run_every=2) with a Meter over keys [1, 2]."""
    ref, amd = _reference("eval", tmp_path), _run("rocket_amd", "eval", tmp_path)
    assert ref["error"] is None and amd["error"] is None
    assert amd["trace"] == ref["trace"]
    assert amd["metrics"] == ref["metrics"] and len(ref["metrics"]) == 2
    assert _close(ref["seen"], amd["seen"])
    assert _close(ref["params"], amd["params"])
