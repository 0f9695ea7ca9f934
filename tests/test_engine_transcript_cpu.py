"""CPU: the launch sequence of ``viscy_amd.engine_unext2.Engine`` — every ops call of two consecutive steps with the dtype and
shape of each tensor argument, the flat-buffer slot of each parameter / gradient view, every scalar, and the points at which the
gradient buckets are yielded — equals the transcript recorded one commit before the engine's layers were paired
(tests/golden/engine_transcript.json, tools/gen_golden_engine_transcript.py), launch by launch."""

import json
import os

import pytest

from tests import engine_transcript as T
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "engine_transcript.json")) as f:
        return T.unpack(json.load(f))


def test_every_case_is_in_the_golden(golden):
    assert list(golden) == list(T.CASES)


@pytest.mark.parametrize("tag", list(T.CASES))
def test_engine_transcript_equals_the_recorded_one(golden, tag):
    got, want = T.run_case(tag), golden[tag]
    for i, (w, g) in enumerate(zip(want["steps"], got["steps"])):
        diff = T.first_difference(w, g)
        assert diff is None, f"{tag}, step {i}, {diff}"
    assert len(got["steps"]) == len(want["steps"]) == 2
    assert got["za_need"] == want["za_need"]
    # the second step is served by the arena: one `zeros` per pass, sized by the first
    assert sum(s.startswith("zeros(") for s in got["steps"][1]) <= 2 < sum(s.startswith("zeros(") for s in got["steps"][0])


def test_recorder_restores_the_ops_module():
    from tests import ref_ops

    before = dict(vars(ref_ops))
    eng, step = T.build("unext2_atto_infer")
    with T.Recorder(ref_ops, eng) as rec:
        assert ref_ops.gemm is not before["gemm"] and eng.ops is ref_ops
        step(rec)
    assert dict(vars(ref_ops)) == before and rec.log[-1] == "saved(None)"
