"""Mirror of reference src/data/unimed_datamodule.py:16-140 (`UnimedDataModule`): same constructor arguments and loader
methods.  Lightning and webdataset are optional in this image: with `webdataset` importable and shard paths given, the
loaders read `jpg`/`txt`/`cls` tuples as the reference does (:44-46); otherwise they fall back to the seeded
SyntheticUnimed set.  `to_device_batch` turns a collated batch into what the MI355X model takes: images preprocessed on the
GPU (medmoe_amd.data), captions as id / mask tensors.  `device_batch` is the same with the `transformations` block applied: the
reference builds its torchvision pipeline from that block (src/utils/utils.py:16-68); here it becomes an AugmentConfig and the
augmentation runs on the GPU behind the resize (medmoe_amd.data.preprocess_augmented)."""
from typing import Any, Dict, Optional

import torch
from torch.utils.data import DataLoader

from src.data.components.unimed import SyntheticUnimed, collate_fn

try:                                                     # pragma: no cover - not installed in this image
    from lightning import LightningDataModule as _Base
except Exception:                                        # noqa: BLE001
    _Base = object

try:                                                     # pragma: no cover
    import webdataset as wds
except Exception:                                        # noqa: BLE001
    wds = None


class UnimedDataModule(_Base):
    def __init__(self, data_dir: str = "data/", transformations: Any = None, batch_size: int = 64, num_workers: int = 0,
                 pin_memory: bool = False, train_data_paths: Optional[str] = None, val_data_paths: Optional[str] = None,
                 synthetic_size: int = 4096, max_len: int = 77, synthetic_vocab: int = 28996, synthetic_classes: int = 5,
                 masks: Any = None, boxes: Any = None) -> None:
        super().__init__()
        if boxes is not None and transformations is not None:
            raise NotImplementedError("data.boxes with data.transformations: the augmentation moves the image and not its boxes - augmented "
                                      "grounding is a named follow-up (DESIGN 3u)")
        if masks is not None and transformations is not None:
            raise NotImplementedError("data.masks with data.transformations: the augmentation moves the image and not its mask - augmented "
                                      "segmentation is a named follow-up (DESIGN 3t)")
        self.data_dir, self.transformations = data_dir, transformations
        # the block is read (and refused, naming its key) here, not at the first batch; augment_step counts the TRAINING batches handed
        # to device_batch and is the `step` of the augmentation's random stream, carried by state_dict()
        self.augment, self.augment_step = None, 0
        if transformations is not None:
            from medmoe_amd.data import AugmentConfig
            self.augment = AugmentConfig.from_hydra(transformations)
        self.batch_size, self.num_workers, self.pin_memory = batch_size, num_workers, pin_memory
        self.batch_size_per_device = batch_size
        self.collate_fn = collate_fn

        def make(paths, seed):
            if wds is not None and paths:                # unimed_datamodule.py:44-46
                return wds.WebDataset(paths, resampled=True, shardshuffle=True, nodesplitter=wds.split_by_node) \
                    .decode("pil").to_tuple("jpg", "txt", "cls")
            return SyntheticUnimed(synthetic_size, max_len=max_len, vocab=synthetic_vocab, n_classes=synthetic_classes, seed=seed, masks=masks, boxes=boxes)

        self.data_train = make(train_data_paths, 12345)
        self.data_val = make(val_data_paths, 54321)
        self.data_test = make(val_data_paths, 54321)

    def setup(self, stage: Optional[str] = None, world_size: int = 1) -> None:
        """unimed_datamodule.py:63-79: the global batch is split evenly over the devices."""
        trainer = getattr(self, "trainer", None)
        ws = trainer.world_size if trainer is not None else world_size
        if self.batch_size % ws != 0:
            raise RuntimeError(f"Batch size ({self.batch_size}) is not divisible by the number of devices ({ws}).")
        self.batch_size_per_device = self.batch_size // ws

    def _loader(self, ds) -> DataLoader:
        """Under data parallelism every rank reads its own 1/W of a map-style set (rank-strided indices, no shuffle: the shards of the
        reference are split by `wds.split_by_node`, unimed_datamodule.py:44-46, which the WebDataset branch above keeps)."""
        trainer = getattr(self, "trainer", None)
        ws = getattr(trainer, "world_size", 1) if trainer is not None else 1
        sampler = None
        if ws > 1 and hasattr(ds, "__len__") and hasattr(ds, "__getitem__"):
            from torch.utils.data.distributed import DistributedSampler
            sampler = DistributedSampler(ds, num_replicas=ws, rank=trainer.global_rank, shuffle=False, drop_last=False)
        return DataLoader(dataset=ds, batch_size=self.batch_size_per_device, num_workers=self.num_workers,
                          pin_memory=self.pin_memory, shuffle=False, sampler=sampler, collate_fn=self.collate_fn)

    def train_dataloader(self) -> DataLoader:
        return self._loader(self.data_train)

    def val_dataloader(self) -> DataLoader:
        return self._loader(self.data_val)

    def test_dataloader(self) -> DataLoader:
        return self._loader(self.data_test)

    @staticmethod
    def to_device_batch(batch: Dict[str, Any], device, size: int = 224) -> Dict[str, Any]:
        """Collated host batch -> the dict MedMoE.forward / Engine.train_step take (images resized + normalised on the GPU)."""
        from medmoe_amd.data import preprocess_images
        imgs = [torch.as_tensor(im).to(device, non_blocking=True).contiguous() for im in batch["image"]]
        image = preprocess_images(imgs, size=size)
        return UnimedDataModule._with_captions(image, batch, device)

    @staticmethod
    def _with_captions(image, batch: Dict[str, Any], device) -> Dict[str, Any]:
        ids = torch.stack([torch.as_tensor(c) for c in batch["caption"]]).to(device)
        mask = (ids != 0).long()
        out = {"image": image, "ids": ids, "attn_mask": mask, "token_type": torch.zeros_like(ids), "label": batch["label"].to(device),
               "caption": {"ids": ids, "attn_mask": mask}}
        if "mask" in batch:                                  # segmentation masks (data.masks) travel as they are
            out["mask"] = batch["mask"].to(device)
        for key in ("box", "span"):                          # grounding annotations (data.boxes): host tables, validated on the host
            if key in batch:
                out[key] = batch[key]
        return out

    def device_batch(self, batch: Dict[str, Any], device, size: int = 224, train: bool = True) -> Dict[str, Any]:
        """to_device_batch with the `transformations` block applied.  No block: to_device_batch itself (the same launches, the same bits).
        Otherwise the images are resized to `imsize`, augmented (train) or centre-cropped (validation, test) and normalised on the GPU;
        the parameters of a sample are a function of (transformations.seed, augment_step, global sample index), and augment_step moves
        once per TRAINING batch, so the micro-batches of an accumulation window draw different parameters and a restored run repeats."""
        if self.augment is None:
            return self.to_device_batch(batch, device, size)
        cfg = self.augment
        if cfg.out_size != size:
            key = "data.transformations.random_crop.crop_size" if cfg.crop_size is not None else "data.transformations.imsize"
            raise ValueError(f"{key} = {cfg.out_size} is the size of the augmented images, but the model's image size is {size}: "
                             "the two must be equal")
        from medmoe_amd.data import preprocess_augmented
        imgs = [torch.as_tensor(im).to(device, non_blocking=True).contiguous() for im in batch["image"]]
        trainer = getattr(self, "trainer", None)
        rank = getattr(trainer, "global_rank", 0) if trainer is not None else 0
        image = preprocess_augmented(imgs, cfg, self.augment_step, sample0=rank * self.batch_size_per_device, train=train)
        if train:
            self.augment_step += 1
        return self._with_captions(image, batch, device)

    def state_dict(self) -> Dict[str, Any]:
        return {"augment_step": self.augment_step}

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        self.augment_step = int(state_dict.get("augment_step", 0))
