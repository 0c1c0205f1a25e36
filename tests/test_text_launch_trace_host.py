"""The launch trace of a step (no GPU): every medmoe_* launch of one train_step (for some cases also an eval_step) with all its arguments -
pointers as buffer name + offset - for the modes of the text tower (frozen / full / LoRA, padded / packed, the dropouts, the depths at which
the summed hidden states change), as tools/text_launch_trace.py records it against a stub library, equals the trace whose SHA-256 stands in
tests/golden/text_launch_digests.json.  A change to the engine that is meant to keep the launches (a refactor of the block loops) passes
unchanged.  A change that alters them ON PURPOSE re-records: `python tools/text_launch_trace.py --dump CASE` before and after, diff the two
and check that the difference is the intended one, then `python tools/text_launch_trace.py --record`."""
import hashlib
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("text_launch_trace", os.path.join(ROOT, "tools", "text_launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
with open(TOOL.GOLDEN) as _f:
    WANT = json.load(_f)


def test_every_case_is_recorded():
    assert list(WANT) == list(TOOL.CASES)


@pytest.mark.parametrize("case", list(TOOL.CASES))
def test_launch_trace_is_the_recorded_one(case):
    got = TOOL.digest(case)
    assert got == WANT[case], f"python tools/text_launch_trace.py --dump {case}  (at both commits, then diff) shows the launch"


def test_two_fresh_engines_give_one_trace():
    """The buffer names are resolved while the buffers are alive: no address of a freed tensor can stand for a temporary's."""
    case = "lora-packed-lora-drop+eval"
    a, b = TOOL.trace(case), TOOL.trace(case)
    assert a == b and hashlib.sha256("\n".join(a).encode()).hexdigest() == WANT[case]["sha256"]
