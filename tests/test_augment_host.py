"""On-device training augmentation, host side (no GPU): the `transformations` block as an AugmentConfig, its refusals, the centre
crop's offsets, the datamodule's dispatch and counter against a stub library that computes nothing, the trainer's train flag, the Hydra
group file, the header - and the convention of the GPU tests' float64 reference against torch's affine_grid + grid_sample on the CPU."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "configs")

GLORIA = {"norm": "imagenet", "imsize": 256, "random_crop": {"crop_size": 224}, "random_horizontal_flip": 0.5,
          "random_affine": {"degrees": 20, "translate": [0.1, 0.1], "scale": [0.95, 1.05]},
          "color_jitter": {"bightness": [0.8, 1.2], "contrast": [0.8, 1.2]}}
# the block of the reference's chexpert.yaml: everything off, a stray `crop_size` next to `random_crop: false`
ALL_FALSE = {"norm": "half", "imsize": 256, "random_crop": False, "crop_size": 224, "random_horizontal_flip": False,
             "random_affine": False, "color_jitter": False}


def _edit(block, dotted, value):
    """a deep copy of `block` with one key replaced"""
    import copy
    out = copy.deepcopy(block)
    node, keys = out, dotted.split(".")
    for k in keys[:-1]:
        node = node[k]
    node[keys[-1]] = value
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# the configuration
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_from_hydra_reads_the_reference_block_shapes():
    from medmoe_amd.data import IMAGENET_MEAN, IMAGENET_STD, AugmentConfig
    from medmoe_amd.hydra_lite import _wrap
    for block in (GLORIA, _wrap(GLORIA)):
        c = AugmentConfig.from_hydra(block)
        assert (c.imsize, c.crop_size, c.out_size, c.norm, c.flip_p, c.seed) == (256, 224, 224, "imagenet", 0.5, 0)
        assert c.degrees == (-20.0, 20.0) and c.translate == (0.1, 0.1) and c.scale == (0.95, 1.05)
        assert c.brightness == (0.8, 1.2) and c.contrast == (0.8, 1.2)           # the reference's `bightness`
        assert c.mean_std() == (IMAGENET_MEAN, IMAGENET_STD)
    off = AugmentConfig.from_hydra(ALL_FALSE)
    assert off == AugmentConfig(imsize=256, norm="half") and off.out_size == 256 and off.mean_std() == ((0.5,) * 3, (0.5,) * 3)
    c = AugmentConfig.from_hydra(_edit(GLORIA, "color_jitter", {"brightness": [0.7, 1.1]}))
    assert c.brightness == (0.7, 1.1) and c.contrast == (1.0, 1.0)               # the plain spelling; an absent operation is off
    c = AugmentConfig.from_hydra(_edit(_edit(GLORIA, "random_affine", {"degrees": [-5, 30]}), "seed", 7))
    assert c.degrees == (-5.0, 30.0) and c.translate == (0.0, 0.0) and c.scale == (1.0, 1.0) and c.seed == 7
    for norm, want in (("slake", (0.2469, 0.2292)), ("pmcoa", (0.1307, 0.3081)), (False, (0.0, 1.0)), (None, (0.0, 1.0))):
        m, s = AugmentConfig.from_hydra(_edit(ALL_FALSE, "norm", norm)).mean_std()
        assert m == (want[0],) * 3 and s == (want[1],) * 3
    absent = dict(ALL_FALSE)
    del absent["norm"]
    assert AugmentConfig.from_hydra(absent).norm == "imagenet"


@pytest.mark.parametrize("dotted, value", [
    ("imsize", 0), ("imsize", 224.5), ("norm", "cifar"), ("random_crop.crop_size", 257), ("random_crop.crop_size", 0),
    ("random_horizontal_flip", 1.5), ("random_horizontal_flip", True), ("random_affine.degrees", -3), ("random_affine.degrees", [10, -10]),
    ("random_affine.translate", [0.1, 1.5]), ("random_affine.translate", [0.1]), ("random_affine.scale", [0.0, 1.0]),
    ("random_affine.scale", [1.2, 0.9]), ("color_jitter.bightness", [-0.1, 1.0]), ("color_jitter.contrast", [1.2, 0.8]), ("seed", 1.5)])
def test_validate_names_the_hydra_key(dotted, value):
    from medmoe_amd.data import AugmentConfig
    key = dotted.replace("bightness", "b(r)?ightness")
    with pytest.raises(ValueError, match=r"data\.transformations\." + key.replace(".", r"\.")):
        AugmentConfig.from_hydra(_edit(GLORIA, dotted, value))


def test_missing_keys_are_named():
    from medmoe_amd.data import AugmentConfig
    no_size = dict(GLORIA)
    del no_size["imsize"]
    with pytest.raises(ValueError, match=r"data\.transformations\.imsize"):
        AugmentConfig.from_hydra(no_size)
    with pytest.raises(ValueError, match=r"data\.transformations\.random_crop\.crop_size"):
        AugmentConfig.from_hydra(_edit(GLORIA, "random_crop", {"size": 224}))
    with pytest.raises(ValueError, match=r"data\.transformations"):
        AugmentConfig.from_hydra(None)


def test_centre_crop_offsets_and_the_flip_threshold():
    from medmoe_amd.data import center_crop_offset, flip_thresh
    # int(round((S - C) / 2)) with Python's round: an odd difference goes to the even neighbour
    assert [center_crop_offset(S, 224) for S in (224, 225, 226, 227, 229, 256)] == [0, 0, 1, 2, 2, 16]
    assert [center_crop_offset(64, C) for C in (56, 57, 59)] == [4, 4, 2]
    assert flip_thresh(0.0) == 0 and flip_thresh(0.5) == 1 << 31 and flip_thresh(1.0) == 0xFFFFFFFF
    with pytest.raises(ValueError):
        flip_thresh(1.01)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the datamodule and the trainer against a stub library
# ------------------------------------------------------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("medmoe_"):
            raise AttributeError(name)

        def f(*a):
            self.calls.append((name, a))
            return 0
        return f


@pytest.fixture
def stub(monkeypatch):
    from medmoe_amd import _lib, data, ops
    lib = _StubLib()
    monkeypatch.setattr(_lib, "_LIB", lib)
    monkeypatch.setattr(ops, "load_library", lambda: lib)
    monkeypatch.setattr(data, "load_library", lambda: lib)
    monkeypatch.setattr(ops, "_require_gpu", lambda t, name: None)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(ops, "_stream_handle", lambda: 0)
    monkeypatch.setattr(ops, "_FN", {})
    return lib


def _batch(n=4):
    g = torch.Generator().manual_seed(0)
    return {"image": [torch.randint(0, 256, (20 + i, 30 - i, 3), generator=g, dtype=torch.uint8) for i in range(n)],
            "caption": [torch.arange(1, 7)] * n, "label": torch.zeros(n, dtype=torch.long)}


SMALL = _edit(_edit(GLORIA, "imsize", 64), "random_crop.crop_size", 56)


def test_no_block_is_to_device_batch_and_issues_no_augment_call(stub, monkeypatch):
    from src.data.unimed_datamodule import UnimedDataModule
    dm = UnimedDataModule(batch_size=4, synthetic_size=8)
    assert dm.augment is None and dm.state_dict() == {"augment_step": 0}
    seen = []
    real = UnimedDataModule.to_device_batch
    monkeypatch.setattr(UnimedDataModule, "to_device_batch", staticmethod(lambda b, d, s=224: seen.append(s) or real(b, d, s)))
    out = dm.device_batch(_batch(), "cpu", 64, True)
    assert seen == [64] and tuple(out["image"].shape) == (4, 3, 64, 64)
    assert [n for n, _ in stub.calls] == ["medmoe_preprocess_bicubic"]
    assert dm.augment_step == 0


def test_a_block_runs_resize_params_apply_and_counts_training_batches(stub):
    from src.data.unimed_datamodule import UnimedDataModule
    dm = UnimedDataModule(transformations=_edit(SMALL, "seed", 11), batch_size=8, synthetic_size=8)
    dm.trainer = types.SimpleNamespace(world_size=2, global_rank=1)
    dm.setup("fit")                                                               # 8 over 2 devices
    steps = []
    for train in (True, True, False, True):
        del stub.calls[:]
        out = dm.device_batch(_batch(), "cpu", 56, train)
        assert tuple(out["image"].shape) == (4, 3, 56, 56) and out["image"].dtype == torch.bfloat16
        assert [n for n, _ in stub.calls] == ["medmoe_preprocess_bicubic", "medmoe_augment_params", "medmoe_augment_apply"]
        resize, params, apply = (a for _, a in stub.calls)
        assert resize[4].value is None and resize[5].value                        # the resize alone: no normalised tensor, the uint8 image
        B, sample0, seed, step, S, C, tr, thresh = params[1:9]
        assert (B, sample0, seed, S, C, tr, thresh) == (4, 4, 11, 64, 56, int(train), 1 << 31)      # sample0 = rank * per-device batch
        assert params[9:19] == (-20.0, 20.0, 0.1, 0.1, 0.95, 1.05, 0.8, 1.2, 0.8, 1.2)
        assert apply[3:7] == (4, 64, 64, 56)
        steps.append(step)
    assert steps == [0, 1, 2, 2] and dm.state_dict() == {"augment_step": 3}
    other = UnimedDataModule(transformations=SMALL, batch_size=8, synthetic_size=8)
    other.load_state_dict(dm.state_dict())
    assert other.augment_step == 3


def test_size_mismatch_names_the_key_and_the_model_size(stub):
    from src.data.unimed_datamodule import UnimedDataModule
    dm = UnimedDataModule(transformations=SMALL, batch_size=4, synthetic_size=8)
    with pytest.raises(ValueError, match=r"data\.transformations\.random_crop\.crop_size = 56.*image size is 224"):
        dm.device_batch(_batch(), "cpu", 224, True)
    flat = UnimedDataModule(transformations=_edit(ALL_FALSE, "imsize", 64), batch_size=4, synthetic_size=8)
    with pytest.raises(ValueError, match=r"data\.transformations\.imsize = 64.*image size is 56"):
        flat.device_batch(_batch(), "cpu", 56, False)
    assert not stub.calls and dm.augment_step == 0
    with pytest.raises(ValueError, match=r"data\.transformations\.random_affine\.scale"):      # a bad block is refused at construction
        UnimedDataModule(transformations=_edit(SMALL, "random_affine.scale", [0, 1]), batch_size=4, synthetic_size=8)


def test_wrappers_refuse_bad_tensors(stub):
    from medmoe_amd.data import AugmentConfig, augment_apply, augment_params
    cfg = AugmentConfig(imsize=16, crop_size=8).validate()
    u8, params = torch.zeros(2, 16, 16, 3, dtype=torch.uint8), torch.zeros(2, 16)
    assert tuple(augment_apply(u8, params, cfg).shape) == (2, 3, 8, 8)
    for bad in (lambda: augment_apply(u8.float(), params, cfg), lambda: augment_apply(u8[:, :, :, :2], params, cfg),
                lambda: augment_apply(u8, params[:1], cfg), lambda: augment_apply(u8, params.double(), cfg),
                lambda: augment_apply(u8, params, cfg, out=torch.zeros(2, 3, 8, 8))):
        with pytest.raises(TypeError, match="augment_apply"):
            bad()
    with pytest.raises(ValueError, match="augment_apply"):
        augment_apply(u8[:, :6].contiguous(), params, cfg)                        # a 6-row source cannot hold an 8 x 8 crop
    for bad in (lambda: augment_params(cfg, 0, 0, 0, True, "cpu"), lambda: augment_params(cfg, 2, -1, 0, True, "cpu")):
        with pytest.raises(ValueError, match="augment_params"):
            bad()
    assert [n for n, _ in stub.calls] == ["medmoe_augment_apply"]


def test_trainer_hands_the_train_flag_to_device_batch():
    from medmoe_amd.trainer import Trainer
    t = Trainer.__new__(Trainer)
    module = torch.nn.Linear(1, 1)
    module.model = types.SimpleNamespace(cfg=types.SimpleNamespace(img_size=56))

    class New:
        def __init__(self):
            self.seen = []

        def to_device_batch(self, batch, dev, size):
            raise AssertionError("device_batch takes precedence")

        def device_batch(self, batch, dev, size, train):
            self.seen.append((size, train))
            return "new"

    class Old:
        def to_device_batch(self, batch, dev, size):
            return ("old", size)
    dm = New()
    assert t._to_device(dm, module, {"image": [1]}, True) == "new" and t._to_device(dm, module, {"image": [1]}, False) == "new"
    assert dm.seen == [(56, True), (56, False)]
    assert t._to_device(Old(), module, {"image": [1]}, True) == ("old", 56)
    tensors = {"image": torch.zeros(1)}
    assert t._to_device(dm, module, tensors, True) is tensors                     # a batch of tensors passes through


# ------------------------------------------------------------------------------------------------------------------------------------------
# Hydra, the header, the reference's convention
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_group_file_composes_and_builds_the_datamodule(monkeypatch):
    monkeypatch.setenv("PROJECT_ROOT", ROOT)
    from medmoe_amd.data import AugmentConfig
    from medmoe_amd.hydra_lite import compose, instantiate
    cfg = compose(CONFIGS, "train.yaml", ["data=unimed_aug"])
    base = compose(CONFIGS, "train.yaml", [])
    assert "transformations" not in base.data
    assert {k: v for k, v in cfg.data.items() if k != "transformations"} == dict(base.data)
    c = AugmentConfig.from_hydra(cfg.data.transformations)
    assert c == AugmentConfig(imsize=256, norm="imagenet", crop_size=224, flip_p=0.5, degrees=(-20.0, 20.0), translate=(0.1, 0.1),
                              scale=(0.95, 1.05), brightness=(0.8, 1.2), contrast=(0.8, 1.2), seed=0)
    dm = instantiate(cfg.data)
    assert dm.augment == c and dm.augment.out_size == 224
    for root, _, files in os.walk(os.path.join(CONFIGS, "experiment")):          # no existing experiment refers to it
        for f in files:
            assert "unimed_aug" not in open(os.path.join(root, f)).read(), f


def test_header_declares_both_symbols_and_the_site_is_free():
    hdr = open(os.path.join(ROOT, "include", "medmoe_hip.h")).read()
    from medmoe_amd import ops
    for name in ("medmoe_augment_params", "medmoe_augment_apply"):
        m = re.search(r"^int %s\((.*)\);" % name, hdr, re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(ops._SIGS[name[len("medmoe_"):]]) + 1, name          # + the stream
    phil = open(os.path.join(ROOT, "medmoe_amd", "csrc", "philox.h")).read()
    assert re.search(r"#define DROPOUT_SITE_AUGMENT 0x20000000u", phil) and ops.DROPOUT_SITE_AUGMENT == 0x20000000
    # clear of the layer sites 4 l + {0..3}, of the drop-path sites and of the embedding site
    assert 4 * 4096 < ops.DROPOUT_SITE_AUGMENT < ops.DROPOUT_SITE_VIT_DROP_PATH < ops.DROPOUT_SITE_EMBED


@pytest.mark.parametrize("C", [32, 40])
def test_the_reference_convention_is_torchs_affine_grid(C):
    """what tests/test_augment_gpu.py holds the kernel to, against affine_grid + grid_sample(nearest, zeros, align_corners=False)"""
    from test_augment_gpu import grid_sample_check
    assert max(grid_sample_check(C)) <= 0.02
