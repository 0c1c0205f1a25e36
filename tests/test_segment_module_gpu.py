"""MedMoESegmenterLightningModule through the Hydra entry point's path (src/train.py::train) on the GPU: the fine-tuning experiment
runs one epoch on data=unimed_seg and reports val/loss, val/dice_mean, val/iou_mean and val/dice/<class>; a checkpoint round trip restores
the head and its Adam moments; a pretraining checkpoint loads with the head at zero."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")
SMALL = ["model.model.vision.config_name=tiny", "data.synthetic_size=32", "data.synthetic_vocab=97", "data.batch_size=8", "data.max_len=16",
         "data.num_workers=0", "extras.print_config=false", "data.masks.size=48", "data.masks.num_classes=2", "model.segmenter.num_classes=2",
         "model.segmenter.class_names=[lung,heart]"]


def _compose(overrides, out_dir):
    os.environ.setdefault("PROJECT_ROOT", ROOT)
    from medmoe_amd.hydra_lite import compose
    return compose(CONFIGS, "train.yaml", overrides, output_dir=str(out_dir))


@pytest.fixture(scope="module")
def finetune_run(tmp_path_factory):
    """experiment=segment_finetune_medmoe_cfg2 at unit-test scale: one epoch of two training batches, validation, checkpoint, test."""
    tmp = tmp_path_factory.mktemp("segment")
    import src.train as T
    cfg = _compose(["experiment=segment_finetune_medmoe_cfg2", "test=true", "trainer.max_epochs=1", "+trainer.limit_train_batches=2",
                    "+trainer.limit_val_batches=2", f"callbacks.model_checkpoint.dirpath={tmp}/ckpt"] + SMALL, tmp)
    metrics, objects = T.train(cfg)
    return tmp, metrics, objects


def test_the_finetune_experiment_runs_and_reports_its_metrics(finetune_run):
    tmp, metrics, objects = finetune_run
    lit, trainer = objects["model"], objects["trainer"]
    assert type(lit).__name__ == "MedMoESegmenterLightningModule" and lit.train_tower and trainer.global_step == 2
    for k in ("train/loss", "val/loss", "val/dice_mean", "val/iou_mean", "val/dice/lung", "val/dice/heart", "val/iou/lung", "test/dice_mean",
              "test/iou_mean"):
        assert k in metrics, (k, sorted(metrics))
    for k in ("train/loss", "val/loss", "val/dice_mean", "val/iou_mean"):
        assert math.isfinite(float(metrics[k])), (k, metrics)
    assert 0.0 <= metrics["val/dice_mean"] <= 1.0 and 0.0 <= metrics["val/iou_mean"] <= metrics["val/dice_mean"]
    assert lit.head.store.step_count == 2 and lit.model.engine.params.step_count == 2 and bool(lit.head.weight.abs().max() > 0)


def test_checkpoint_round_trip_restores_the_head_and_its_moments(finetune_run):
    tmp, _, objects = finetune_run
    lit = objects["model"]
    ckpt = torch.load(os.path.join(str(tmp), "ckpt", "last.ckpt"), map_location="cpu", weights_only=True)
    sd = ckpt["state_dict"]
    assert "seg_head.weight" in sd and "seg_head.bias" in sd and "model.image_encoder.moe.router.0.weight" in sd
    assert set(ckpt["fused_adam"]) == {"image", "seg_head"} and ckpt["fused_adam"]["seg_head"]["step"] == 2
    from medmoe_amd.hydra_lite import instantiate
    fresh = instantiate(_compose(["experiment=segment_finetune_medmoe_cfg2"] + SMALL, tmp).model)
    assert not fresh.head.weight.any() and not fresh.head.store.has_adam_state()
    fresh.load_state_dict(sd)
    fresh.on_load_checkpoint(ckpt)
    assert torch.equal(fresh.head.weight, lit.head.weight) and torch.equal(fresh.head.bias, lit.head.bias)
    assert torch.equal(fresh.head.weight.cpu(), sd["seg_head.weight"])
    for a, b in zip(fresh.head.store.adam_state(), lit.head.store.adam_state()):
        assert torch.equal(a, b) and bool(a.abs().max() > 0)
    assert fresh.head.store.step_count == 2 and fresh.model.engine.params.step_count == 2
    assert torch.equal(fresh.model.engine.params.p32, lit.model.engine.params.p32)


def test_a_pretraining_checkpoint_loads_with_the_head_at_zero(tmp_path):
    from medmoe_amd.hydra_lite import instantiate
    pre = instantiate(_compose(["experiment=pretraining_medmoe", "model.fused_step=true"] + SMALL[:7], tmp_path).model)
    with torch.no_grad():
        pre.model.weights.mul_(1.01)                                 # away from the seeded initial values a fresh module starts from
    path = os.path.join(str(tmp_path), "pretrained.ckpt")
    torch.save({"state_dict": pre.state_dict()}, path)
    lit = instantiate(_compose(["experiment=segment_probe_medmoe_cfg2", f"model.segmenter.pretrained_ckpt={path}", "model.segmenter.w_dice=0.0"]
                               + SMALL, tmp_path).model)
    assert not lit.train_tower and torch.equal(lit.model.engine.params.p32, pre.model.engine.params.p32)
    assert not lit.head.weight.any() and not lit.head.bias.any()
    # the first BCE of a zero head is ln 2 whatever the features are
    dev, size = lit.model.engine.device, lit.model.cfg.img_size
    batch = {"image": torch.randn(8, 3, size, size, device=dev), "mask": (torch.rand(8, 2, 40, 40, device=dev) < 0.3).to(torch.int8)}
    out = lit.fused_training_step(batch)
    assert abs(float(out["loss"]) - math.log(2.0)) < 1e-6
    assert tuple(lit.predict(batch, (40, 40)).shape) == (8, 2, 40, 40)
