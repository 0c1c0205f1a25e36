"""The `model.grounding` block through the Hydra entry point's path (src/train.py::train) on the GPU: the experiment
pretraining_medmoe_cfg2_grounding on data=unimed_boxes, shrunk to the tiny model, reports val/pg_acc, val/cnr_mean and val/ground_iou@0.5, and
every validation key a run without the block logs keeps its value bit for bit."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
SMALL = ["model.model.vision.config_name=tiny", "data.synthetic_size=32", "data.synthetic_vocab=97", "data.batch_size=8", "data.max_len=16",
         "data.num_workers=0", "extras.print_config=false", "test=true", "trainer.max_epochs=1", "+trainer.limit_train_batches=2",
         "+trainer.limit_val_batches=2", "trainer.deterministic=true"]
KEYS = ("pg_acc", "cnr_mean", "ground_iou@0.5")


def _run(overrides, tmp):
    os.environ.setdefault("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    import src.train as T
    cfg = compose(CONFIGS, "train.yaml", overrides + SMALL + [f"callbacks.model_checkpoint.dirpath={tmp}/ckpt"], output_dir=str(tmp))
    return T.train(cfg)


def test_the_grounding_experiment_logs_its_keys_and_leaves_the_others_alone(tmp_path):
    with_, objects = _run(["experiment=pretraining_medmoe_cfg2_grounding", "data=unimed_boxes", "data.boxes.size=48", "model.grounding.size=48"],
                          tmp_path / "with")
    without, _ = _run(["experiment=pretraining_medmoe_cfg2"], tmp_path / "without")
    lit = objects["model"]
    assert lit._grounding == {"mode": "attention", "thetas": (0.5,), "size": (48, 48), "span_key": "span", "box_key": "box"}
    for stage in ("val", "test"):
        for k in KEYS:
            assert f"{stage}/{k}" in with_ and f"{stage}/{k}" not in without, (stage, k, sorted(with_))
            assert math.isfinite(float(with_[f"{stage}/{k}"])), (k, with_)
        assert 0.0 <= with_[f"{stage}/pg_acc"] <= 1.0 and with_[f"{stage}/cnr_mean"] >= 0.0 and 0.0 <= with_[f"{stage}/ground_iou@0.5"] <= 1.0
    # two validation batches of 8, every sample with a box
    assert int(lit._gbank.ints[0]) == 16 and int(lit._gbank.ints[1]) == 16 and len(lit._gbank) == 2
    shared = [k for k in without if k.startswith(("val/", "test/", "train/"))]
    assert "val/loss" in shared and "train/loss" in shared
    for k in shared:
        a, b = with_[k], without[k]
        assert (torch.equal(torch.as_tensor(a), torch.as_tensor(b))), (k, a, b)
    assert sorted(k for k in with_ if k not in without) == sorted(f"{s}/{k}" for s in ("val", "test") for k in KEYS)
