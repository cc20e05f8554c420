"""Input pipeline: sharded uint8 batches -> pinned host -> async H2D on a HIP
copy stream -> GPU normalise kernel -> model input.

Replaces the reference's ``DataLoader(..., num_workers=10, sampler=
DistributedSampler, pin_memory=True)`` + ``.cuda(non_blocking=True)`` +
CPU ``ToTensor/Normalize`` (``imagenet.py:119-120, 280-283, 346-359``):

* workers only decode + resize to uint8 (4x fewer bytes than the reference's
  fp32 tensors through shared memory, pinning and PCIe: 38.5 MB instead of
  154 MB per 256-image 224^2 batch);
* the next batch's H2D copy runs on a dedicated copy stream while the
  current step computes; the compute stream waits on an event, never on the
  host;
* normalisation (``(x/255 - mean)/std``), the NHWC channel padding for the
  stem and optional random crop / horizontal flip are one HIP kernel; so is
  RandomResizedCrop (``rrc=``: boxes drawn on the device by ``data/augment.py``,
  crop + antialiased resize + normalise + flip fused, ``ops.misc.rrc_normalize_u8``);
* RandAugment (``randaug=``, ``data/randaug.py``) is a uint8 -> uint8 stage of HIP kernels in front of those, on
  the batch as stored;
* workers are persistent (the reference re-forks 10 workers every epoch).
"""

from __future__ import annotations

from typing import Iterator, Optional, Sequence, Tuple

import torch

from ..parallel.sampler import ShardSampler
from .imagenet import collate_u8

MEAN = (0.5, 0.5, 0.5)   # imagenet.py:283
STD = (0.5, 0.5, 0.5)


class InputTransform:
    """uint8 [B,H,W,3] (on the compute device) -> model input."""

    def __init__(self, backend: str, size: Tuple[int, int], mean=MEAN, std=STD, cpad: int = 8,
                 flip: bool = False, dtype=torch.float32, resize: bool = False, rrc=None,
                 center_frac: Optional[float] = None, seed: int = 0, rank: int = 0, randaug=None):
        self.backend, self.size = backend, tuple(size)
        self.mean, self.std, self.cpad = tuple(mean), tuple(std), cpad
        self.flip = flip
        self.dtype = dtype
        # resize: an image of another size is bilinearly resampled to `size` (records stored smaller than the
        # model input, --record-resize) instead of randomly cropped
        self.resize = resize
        # rrc = (scale, ratio): RandomResizedCrop (data/augment.py) -- a random box per sample, resampled to
        # `size` with the antialiased filter; it takes precedence over `resize` and the same-scale crop.
        # center_frac: the centred box of that fraction of each side instead, through the same antialiased path
        # (validation: no randomness, no flip).
        if rrc is not None:
            from .augment import check_ranges
            rrc = (tuple(float(v) for v in rrc[0]), tuple(float(v) for v in rrc[1]))
            check_ranges(*rrc)
        if center_frac is not None and not (0.0 < center_frac <= 1.0):
            raise ValueError(f"centre crop fraction {center_frac}: need 0 < frac <= 1")
        self.rrc, self.center_frac = rrc, center_frac
        # the random boxes and their flip mask come from a generator of the transform's own, on the compute
        # device, reseeded from (seed, rank, epoch): a resumed run repeats the epoch's boxes
        self.seed, self.rank, self.epoch = int(seed), int(rank), 0
        self._gen = None
        self._center = {}
        # randaug: a data.randaug.RandAugment stage the uint8 batch passes through first, as stored and ahead of any
        # crop (the train transform only); None: every path below is as it was
        self.randaug = randaug

    def _epoch_seed(self) -> int:
        return (self.seed * 0x9E3779B1 + self.rank * 0x85EBCA6B + self.epoch * 0xC2B2AE35 + 1) % (2 ** 63 - 1)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)
        if self._gen is not None:
            self._gen.manual_seed(self._epoch_seed())

    def _generator(self, device) -> torch.Generator:
        if self._gen is None or self._gen.device != torch.device(device):
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed(self._epoch_seed())
        return self._gen

    def _boxed(self, u8: torch.Tensor, boxes, flip) -> torch.Tensor:
        """The box path: RandomResizedCrop (rrc) or the centre box (center_frac), antialiased resample to `size`."""
        from .augment import center_box, sample_boxes
        B, H, W, _ = u8.shape
        oh, ow = self.size
        dev = u8.device
        if boxes is None:
            if self.rrc is not None:
                boxes = sample_boxes(B, H, W, self.rrc[0], self.rrc[1], self._generator(dev), dev)
            else:
                key = (dev, B, H, W)
                if key not in self._center:
                    self._center = {key: torch.tensor([center_box(H, W, self.center_frac)] * B,
                                                      dtype=torch.int32).to(dev)}
                boxes = self._center[key]
        if flip is None and self.flip and self.rrc is not None:
            flip = (torch.rand(B, generator=self._generator(dev), device=dev) < 0.5).to(torch.uint8)
        if self.backend in ("hip", "hip_f32"):
            from ..ops.misc import rrc_normalize_u8
            return rrc_normalize_u8(u8, (oh, ow), self.cpad, self.mean, self.std, boxes, flip,
                                    dtype=torch.float32 if self.backend == "hip_f32" else torch.bfloat16)
        # torch: crop each sample, interpolate(antialias=True), batched over samples with equal box shapes
        x = u8.permute(0, 3, 1, 2)
        out = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=dev)
        bl = boxes.tolist()
        groups = {}
        for i, (t, l, h, w) in enumerate(bl):
            groups.setdefault((h, w), []).append(i)
        for (h, w), idx in groups.items():
            crops = torch.stack([x[i, :, bl[i][0]:bl[i][0] + h, bl[i][1]:bl[i][1] + w] for i in idx]).float()
            out[idx] = torch.nn.functional.interpolate(crops, size=(oh, ow), mode="bilinear", antialias=True,
                                                       align_corners=False)
        m = torch.tensor(self.mean, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
        s = torch.tensor(self.std, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
        out = (out / 255.0 - m) / s
        if flip is not None:
            out = torch.where(flip.view(-1, 1, 1, 1).bool(), out.flip(3), out)
        return out.to(self.dtype).contiguous()

    def __call__(self, u8: torch.Tensor, boxes: Optional[torch.Tensor] = None,
                 flip: Optional[torch.Tensor] = None, ra_params: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``boxes`` (int32 [B, 4] = top, left, h, w) / ``flip`` (uint8 [B]): explicit draws for the box path
        instead of the transform's own (comparing backends on identical draws); ``ra_params`` (int32 [B, L, 8])
        likewise for the RandAugment stage."""
        if self.randaug is not None:
            u8 = self.randaug(u8, ra_params)
        elif ra_params is not None:
            raise ValueError("explicit ra_params need randaug=")
        if self.rrc is not None or self.center_frac is not None:
            return self._boxed(u8, boxes, flip)
        if boxes is not None or flip is not None:
            raise ValueError("explicit boxes / flip need rrc= or center_frac=")
        B, H, W, _ = u8.shape
        oh, ow = self.size
        if self.backend in ("hip", "hip_f32"):
            from ..ops.misc import normalize_u8
            if self.backend == "hip_f32":  # fp32 NHWC for the fp32 kernel path
                from ..ops.f32 import normalize_u8_f32 as normalize_u8
            crop = flip = None
            if self.flip:
                flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device=u8.device)
            if self.resize and (H, W) != (oh, ow):
                if self.backend == "hip_f32":
                    raise NotImplementedError("--record-resize: the bf16 input path only")
                from ..ops.misc import resize_normalize_u8
                return resize_normalize_u8(u8, (oh, ow), self.cpad, self.mean, self.std, flip)
            if (H, W) != (oh, ow):
                cy = torch.randint(0, H - oh + 1, (B,), dtype=torch.int32, device=u8.device)
                cx = torch.randint(0, W - ow + 1, (B,), dtype=torch.int32, device=u8.device)
                crop = torch.stack([cy, cx], 1).contiguous()
            return normalize_u8(u8, (oh, ow), self.cpad, self.mean, self.std, crop, flip)
        if self.resize and (H, W) != (oh, ow):
            x = torch.nn.functional.interpolate(u8.permute(0, 3, 1, 2).float(), size=(oh, ow), mode="bilinear",
                                                align_corners=False).to(self.dtype).div_(255.0)
        else:
            x = u8[:, :oh, :ow].permute(0, 3, 1, 2).to(self.dtype).div_(255.0)
        m = torch.tensor(self.mean, dtype=self.dtype, device=u8.device).view(1, 3, 1, 1)
        s = torch.tensor(self.std, dtype=self.dtype, device=u8.device).view(1, 3, 1, 1)
        x = (x - m) / s
        if self.flip:
            f = torch.rand(B, device=u8.device) < 0.5
            x[f] = x[f].flip(3)
        return x.contiguous()


class _IndexBatches(torch.utils.data.Sampler):
    def __init__(self, sampler: ShardSampler, batch_size: int, drop_last: bool):
        self.s, self.b, self.d = sampler, batch_size, drop_last

    def __iter__(self):
        for idx in self.s.batches(self.b, self.d):
            yield idx.tolist()

    def __len__(self):
        return self.s.num_batches(self.b, self.d)


class DeviceLoader:
    """Iterates (model_input, labels) for one epoch of one rank's shard."""

    def __init__(self, dataset, sampler: ShardSampler, batch_size: int, transform: InputTransform,
                 device: torch.device, workers: int = 8, drop_last: bool = False,
                 prefetch_factor: int = 4):
        self.dataset, self.sampler, self.batch = dataset, sampler, batch_size
        self.transform, self.device = transform, torch.device(device)
        pin = self.device.type == "cuda"
        kw = dict(num_workers=workers, pin_memory=pin, collate_fn=collate_u8)
        if workers > 0:
            kw.update(persistent_workers=True, prefetch_factor=prefetch_factor)
        self.dl = torch.utils.data.DataLoader(dataset, batch_sampler=_IndexBatches(sampler, batch_size, drop_last),
                                              **kw)
        self.copy_stream = torch.cuda.Stream(self.device) if pin else None

    def __len__(self):
        return len(self.dl)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        it = iter(self.dl)
        if self.copy_stream is None:
            for u8, y in it:
                yield self.transform(u8.to(self.device)), y.to(self.device)
            return
        nxt = self._stage(it)
        while nxt is not None:
            u8, y, ev = nxt
            nxt = self._stage(it)                      # next H2D overlaps this step
            torch.cuda.current_stream(self.device).wait_event(ev)
            u8.record_stream(torch.cuda.current_stream(self.device))
            y.record_stream(torch.cuda.current_stream(self.device))
            yield self.transform(u8), y

    def _stage(self, it):
        try:
            u8, y = next(it)
        except StopIteration:
            return None
        with torch.cuda.stream(self.copy_stream):
            u8d = u8.to(self.device, non_blocking=True)
            yd = y.to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        return u8d, yd, ev


class SyntheticLoader:
    """Synthetic batches through the same GPU transform."""

    def __init__(self, source, steps: int, transform: InputTransform):
        self.source, self.steps, self.transform = source, steps, transform

    def __len__(self):
        return self.steps

    def __iter__(self):
        for u8, y in self.source.batches(self.steps):
            yield self.transform(u8), y
