"""The scan lanes' bookkeeping (a-nice-rag_amd/csrc/scan_lanes.hpp: which lane and list set a single query takes, which
back-pressure event covers the set's reuse, which event is recorded behind the query) against a fake device -- no GPU.
`dense_single_enqueue` and `hybrid_lane_enqueue` (api.hip) run exactly this header with HIP streams and events; a slip in
its arithmetic would overwrite a list set under a merge that has not read it yet, which the GPU stress tests
(tests/test_gpu_pipeline_stress.py) would only see by losing a race.  The model (tests/native/scan_lanes_model.cpp) is a
stand-alone program built with g++ under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "scan_lanes_model.cpp")
INC = os.path.join(REPO, "a-nice-rag_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build_and_run(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=undefined,address",
           "-fno-sanitize-recover=undefined", "-I", INC, *extra, SRC, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_lane_tickets_keep_their_invariant(tmp_path):
    """1, 2 and 4 lanes, more than 10 * kPipeSlots queries each, with and without a drain in the middle: set ownership,
    no early wait, every reuse covered by an event already recorded, the event schedule."""
    r = _build_and_run(tmp_path, "scan_lanes_model")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "(a) 0 (b) 0 (c) 0 (d) 0 failures" in r.stdout, r.stdout[-3000:]


def test_the_model_catches_an_event_named_too_early(tmp_path):
    """The same model over the same formula with m one too small must fail property (c), and only that one: the test
    above is not vacuous."""
    r = _build_and_run(tmp_path, "scan_lanes_broken", ["-DBREAK_LANES"])
    assert "FAIL (c)" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 4, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
