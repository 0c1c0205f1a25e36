"""The bf16 gradient exchange (MedMoEConfig.grad_comm_dtype = "bf16") at engine level, each case in a child process of its own
(the process group has to exist before anything touches the GPU): a one-rank "nccl" group over the real RCCL backend
(tools/rccl_world1_bf16.py) and two gloo ranks sharing the one GPU (tools/two_rank_bf16.py).  A child that fails stops the cases after it:
nothing more is started on a GPU that a child may have left in a bad state."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_failed = []


def _child(tool, port, ok_line, *argv, **env):
    if _failed:
        pytest.fail(f"not started: {_failed[0]} failed before it")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **env)
    env.pop("MEDMOE_GRAD_COMM", None)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *argv], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _failed.append(tool)
        raise
    if r.returncode != 0 or ok_line not in r.stdout:
        _failed.append(tool)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert ok_line in r.stdout, r.stdout[-2000:]
    return r.stdout


def test_one_rank_rccl_group_adam_reads_the_bf16_sum_and_fp32_stays_the_default():
    """bf16: in front of every arena's adam_step g16 == bf16(g32) bit for bit and the step equals the fp32-gradient kernel's on g16.float();
    fp32: no pack, no bf16 buffer, the step agrees with a non-distributed engine."""
    out = _child("rccl_world1_bf16.py", 29547, "rccl world-1 bf16 path OK")
    assert "bf16 exchange:" in out and "fp32 exchange:" in out


def test_one_rank_rccl_group_swin_engine_step_through_the_hydra_key():
    """model.grad_comm_dtype=bf16 with vision.arch=swin_t: the MoE arena's reduce under the tower's backward and the tower arena's reduce
    both travel as bf16 (flags set in front of both adam_steps), and the parameters stay finite."""
    out = _child("rccl_world1_bf16.py", 29549, "rccl world-1 bf16 path OK", "swin")
    assert "swin step with the bf16 exchange" in out


@pytest.mark.parametrize("case,port", [("", 29551), ("text", 29553), ("accum", 29555)], ids=["image", "text", "accum"])
def test_two_ranks_reduce_bf16_averages_and_keep_identical_replicas(case, port):
    """Every rank's g16 is bf16(g32_rank0 / 2) + bf16(g32_rank1 / 2) in bf16 arithmetic (bit for bit), the clip norms are bit-identical, the
    replicas end two steps with identical masters.  text: the text arena too.  accum: two micro-batches, nothing packed or reduced on the
    first, the reduced gradient is the bf16 average of the accumulated sums."""
    _child("two_rank_bf16.py", port, "two-rank bf16 exchange OK", TWO_RANK_BF16_CASE=case)
