"""Random Erasing on the GPU (--random-erase): ``ops.misc.erase_boxes`` (csrc/kernels/erase.hip erase_boxes_kernel)
against ``data.erase.erase_torch``, past 2^31 bytes, the three backends of ``BatchEraser`` on identical draws, and
three trainer steps on both kernel paths.

``const`` mode is compared bit for bit; so is every element outside the boxes (the input is random, pad channels too),
and the pad channels inside a box are zero. ``pixel`` mode is compared with ``r``, the noise formed in float64 from the
Philox words (``data.erase.noise_words``, themselves checked against plain Python integers in test_erase_cpu.py):
``|out - r| <= 2^-16`` for fp32, ``<= 2^-8 |r| + 2^-16`` for bf16. The bound: ``u`` and ``v`` are exact in fp32, the
radius is at most 5.77, the rounded ``2 pi v`` is off by under 6e-7 and the precise ``logf`` / ``sinf`` / ``cosf`` are
good to a few ulp -- about 5e-6 absolute in total, so 2^-16 leaves a factor of three; bf16 adds its half ulp. The
largest error seen is printed (profiles/erase.md records it).

Shapes: 5 x 7 x 4 bf16 samples are 280 bytes, so odd samples start at an odd 8-byte pixel and the 16-byte pairs shift;
33 x 71 the same at a size of several blocks' worth of rows; Cp 8 and fp32 take the one-pixel-per-store paths. Every
box of three rows or more is spread over several blocks (rows interleaved over the grid's second dimension)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(3, 5, 7, 4), (3, 5, 7, 8), (4, 16, 16, 4), (3, 33, 70, 4), (3, 33, 71, 4)]
E = (0, 0, 0, 0)


def _cases(H, W):
    """Two boxes per sample."""
    return [(E, E),                                   # empty
            ((0, 0, 0, 5), (0, 0, 5, 0)),             # empty: h = 0, w = 0
            ((2, 3, 1, 1), E),                        # one pixel, at an odd column
            ((1, 1, 3, 2), E),                        # starts at an odd column
            ((1, 2, 2, 3), E),                        # ends at an odd column
            ((0, 2, 2, 3), (H - 2, 1, 2, 3)),         # touches the top; the bottom
            ((1, 0, 3, 2), E),                        # the left
            (E, (1, W - 2, 3, 2)),                    # the right (the box is the second of the sample)
            ((0, W - 1, H, 1), E),                    # the last column, every row
            ((0, 0, H, W), E),                        # the whole image
            ((0, 0, 2, 3), (3, 4, 2, 3)),             # two disjoint boxes
            ((1, 1, 3, 3), (2, 3, 3, 4))]             # two overlapping boxes


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _inside(boxes, H, W):
    """bool [B, H, W] on the CPU: the pixels inside any box."""
    rows, cols = torch.arange(H).view(1, 1, H, 1), torch.arange(W).view(1, 1, 1, W)
    t, l, h, w = (boxes[..., i].long().view(boxes.shape[0], -1, 1, 1) for i in range(4))
    return ((rows >= t) & (rows < t + h) & (cols >= l) & (cols < l + w) & (h > 0) & (w > 0)).any(1)


def _noise(keys, H, W):
    """r: float64 [B, H, W, 3] on the CPU."""
    from imagent_amd.data.erase import noise_words, normals_from_words
    return normals_from_words(noise_words(keys.cpu(), H, W))


def _check(out, x, boxes, keys, mode, value):
    """out, x: NHWC on the CPU. -> the largest pixel-mode error"""
    from imagent_amd.data.erase import erase_torch
    B, H, W, Cp = x.shape
    ins = _inside(boxes, H, W)
    keep = ~ins.unsqueeze(-1).expand_as(x)
    assert torch.equal(_bits(out)[keep], _bits(x)[keep]), "outside the boxes"
    assert not _bits(out)[..., 3:][ins].any(), "pad channels inside the boxes"
    if mode == "const":
        want = erase_torch(x[..., :3].permute(0, 3, 1, 2), boxes, None, "const", value).permute(0, 2, 3, 1)
        assert torch.equal(_bits(out[..., :3].contiguous()), _bits(want.contiguous()))
        return 0.0
    r = _noise(keys, H, W)[ins]
    err = (out[..., :3][ins].double() - r).abs()
    bound = torch.full_like(r, 2.0 ** -16)
    if x.dtype == torch.bfloat16:
        bound += 2.0 ** -8 * r.abs()
    assert (err <= bound).all(), f"{(err - bound).max().item():.3e} over the bound"
    return err.max().item() if err.numel() else 0.0


@pytest.mark.parametrize("mode", ["const", "pixel"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_erase_boxes_matches_definition(shape, dtype, mode):
    from imagent_amd.ops.misc import erase_boxes
    B, H, W, Cp = shape
    g = torch.Generator().manual_seed(B * 1000 + H * W + Cp)
    x = torch.randn(shape, generator=g).to(dtype)  # pad channels too: the kernel has to clear them inside a box
    keys = torch.randint(-2 ** 31, 2 ** 31, (B, 2), generator=g).to(torch.int32)
    cases = _cases(H, W)
    n = len(cases)
    worst = 0.0
    for launch in range(n):  # sample i takes case launch + i: every case meets every sample
        boxes = torch.tensor([cases[(launch + i) % n] for i in range(B)], dtype=torch.int32)
        d = x.to(DEV)
        out = erase_boxes(d, boxes.to(DEV), keys.to(DEV), mode, -0.7)
        assert out.data_ptr() == d.data_ptr()  # in place
        worst = max(worst, _check(out.cpu(), x, boxes, keys, mode, -0.7))
        again = erase_boxes(x.to(DEV), boxes.to(DEV), keys.to(DEV), mode, -0.7)
        assert torch.equal(_bits(again), _bits(out)), "two calls on the same draws"
    if mode == "pixel":
        print(f"{shape} {dtype}: largest |out - r| {worst:.3e}")


def test_arguments():
    from imagent_amd.ops.misc import erase_boxes
    x = torch.zeros((2, 4, 4, 4), device=DEV, dtype=torch.bfloat16)
    boxes = torch.zeros((2, 1, 4), dtype=torch.int32, device=DEV)
    keys = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    for xx, bb, kk, mode in ((x[..., :3], boxes, keys, "const"), (x.half(), boxes, keys, "const"),
                             (x, boxes[:1], keys, "const"), (x, boxes[:, 0], keys, "const"),
                             (x, boxes, None, "pixel"), (x, boxes, keys[:1], "pixel"), (x, boxes, keys, "noise")):
        with pytest.raises(ValueError):
            erase_boxes(xx, bb, kk, mode, 0.0)
    assert erase_boxes(x[:0], boxes[:0], None).shape == (0, 4, 4, 4)
    # a box that leaves the image is clipped to it, not written out of bounds
    x = torch.randn((3, 4, 4, 4), device=DEV).to(torch.bfloat16)
    keep = x.clone()
    wild = torch.tensor([[[0, 0, 0, 0]], [[-2, -3, 4, 5], ], [[0, 0, 0, 0]]], dtype=torch.int32, device=DEV)
    erase_boxes(x, wild, None, "const", 1.0)
    assert torch.equal(x[0], keep[0]) and torch.equal(x[2], keep[2])
    assert (x[1, :2, :2, :3] == 1.0).all() and torch.equal(x[1, 2:], keep[1, 2:])
    assert torch.equal(x[1, :, 2:], keep[1, :, 2:])
    far = torch.tensor([[[2, 2, 2 ** 31 - 1, 2 ** 31 - 1]], [[5, 0, 2, 2]], [[0, 4, 1, 1]]], dtype=torch.int32,
                       device=DEV)
    x = keep.clone()
    erase_boxes(x, far, None, "const", 1.0)
    assert (x[0, 2:, 2:, :3] == 1.0).all() and torch.equal(x[0, :2], keep[0, :2]) and torch.equal(x[1:], keep[1:])


def test_past_2gb():
    """One launch on bf16 [2731, 224, 224, 8] (2.19 GB) with boxes in the first and the last sample only; the last
    sample starts past 2^31 bytes and its second box ends at the tensor's last element. Those two samples equal the
    same boxes applied to them alone, and every sample in between is untouched."""
    from imagent_amd.ops.misc import erase_boxes
    B, H, W, Cp = 2731, 224, 224, 8
    g = torch.Generator(device=DEV).manual_seed(7)
    blk = torch.randn((H, W, Cp), device=DEV, generator=g).to(torch.bfloat16)
    x = torch.empty((B, H, W, Cp), device=DEV, dtype=torch.bfloat16)
    x[:] = blk
    assert (B - 1) * H * W * Cp * 2 > 2 ** 31
    boxes = torch.zeros((B, 2, 4), dtype=torch.int32, device=DEV)
    boxes[0] = torch.tensor([[10, 11, 100, 101], [0, 0, 0, 0]], dtype=torch.int32)
    boxes[-1] = torch.tensor([[50, 3, 120, 77], [100, 50, 124, 174]], dtype=torch.int32)
    keys = torch.randint(-2 ** 31, 2 ** 31, (B, 2), device=DEV, generator=g).to(torch.int32)
    ends = [0, B - 1]
    for mode in ("const", "pixel"):
        erase_boxes(x, boxes, keys, mode, 1.5)
        small = torch.stack([blk, blk])
        erase_boxes(small, boxes[ends].contiguous(), keys[ends].contiguous(), mode, 1.5)
        assert torch.equal(_bits(x[0]), _bits(small[0])) and torch.equal(_bits(x[-1]), _bits(small[1])), mode
        assert not torch.equal(x[0], blk) and not torch.equal(x[-1], blk)
        assert not x[0, 10:110, 11:112, 3:].any() and not x[-1, 100:, 50:, 3:].any()
        for lo in range(1, B - 1, 512):  # every sample in between, in slabs
            hi = min(lo + 512, B - 1)
            assert torch.equal(_bits(x[lo:hi]), _bits(blk.expand(hi - lo, H, W, Cp))), (mode, lo)


def test_backends_agree():
    from imagent_amd.data.erase import BatchEraser
    B, H, W, Cp = 6, 12, 10, 4
    g = torch.Generator().manual_seed(3)
    xc = torch.randn((B, 3, H, W), generator=g)
    boxes = torch.tensor([[E, E], [(2, 3, 5, 4), E], [E, (0, 1, 12, 3)], [(0, 0, 12, 10), E],
                          [(1, 1, 4, 4), (3, 3, 5, 5)], [(11, 9, 1, 1), (0, 0, 1, 1)]], dtype=torch.int32)
    keys = torch.randint(-2 ** 31, 2 ** 31, (B, 2), generator=g).to(torch.int32)
    params = (boxes.to(DEV), keys.to(DEV))
    ins = _inside(boxes, H, W)
    r = _noise(keys, H, W)[ins]
    for mode in ("const", "pixel"):
        for backend, dtype in (("hip", torch.bfloat16), ("hip_f32", torch.float32)):
            x = xc.to(dtype)
            xn = torch.zeros((B, H, W, Cp), dtype=dtype)
            xn[..., :3] = x.permute(0, 2, 3, 1)
            oh = BatchEraser(backend, 1.0, count=2, mode=mode, value=0.25)(xn.to(DEV), params).cpu()
            ot = BatchEraser("torch", 1.0, count=2, mode=mode, value=0.25)(x.to(DEV), params).cpu()
            assert ot.dtype == oh.dtype == dtype and not oh[..., 3:].any()
            _check(oh, xn, boxes, keys, mode, 0.25)
            if mode == "const":
                assert torch.equal(_bits(oh[..., :3].contiguous()), _bits(ot.permute(0, 2, 3, 1).contiguous()))
            else:
                keep = ~ins.unsqueeze(-1).expand(B, H, W, 3)
                on = ot.permute(0, 2, 3, 1)
                assert torch.equal(on[keep], xn[..., :3][keep])
                bound = 2.0 ** -16 + (2.0 ** -8 * r.abs() if dtype == torch.bfloat16 else 0.0)
                assert ((on[ins].double() - r).abs() <= bound).all()
                assert ((oh[..., :3][ins].double() - r).abs() <= bound).all()
    # own draws: two stages at the same epoch give identical draws and outputs, on the device
    outs = []
    for _ in range(2):
        e = BatchEraser("hip", 0.5, count=3, mode="pixel", seed=11, rank=1)
        e.set_epoch(4)
        d = e.draw(B, H, W, DEV)
        e.set_epoch(4)
        outs.append((d, e(torch.zeros((B, H, W, Cp), device=DEV, dtype=torch.bfloat16))))
    (d0, x0), (d1, x1) = outs
    assert all(torch.equal(a, b) for a, b in zip(d0, d1)) and all(t.is_cuda for t in d0)
    assert torch.equal(_bits(x0), _bits(x1))
    assert torch.equal(x0.cpu().ne(0).any(-1), _inside(d0[0].cpu(), H, W))  # the call drew what draw() drew


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_trainer_three_steps(tmp_path, monkeypatch, dtype):
    """(100 classes: the fp32 kernel path takes class counts that are a multiple of 4.)"""
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    args = ["--arch", "resnet18", "--image-size", "64", "--data", "synthetic", "--synthetic-train-size", "64",
            "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "100", "--quiet-banner", "--tb-dir", "",
            "--kernels", "hip", "--launcher", "single", "--random-erase", "1", "--erase-mode", "pixel", "--erase-count",
            "2", "--mixup", "0.2", "--cutmix", "1.0", "--max-steps", "3", "--dtype", dtype, "--log-interval", "0"]
    tr = Trainer(build_parser().parse_args(args))
    try:
        assert tr.eraser is not None and tr.eraser.backend == ("hip" if dtype == "bf16" else "hip_f32")
        seen, erased = [], []
        loss_fn, stage = tr.step.loss, type(tr.eraser).__call__
        monkeypatch.setattr(tr.step, "loss", lambda logits, y: (seen.append(type(y)), loss_fn(logits, y))[1])
        monkeypatch.setattr(type(tr.eraser), "__call__", lambda s, x, params=None: (
            erased.append((tuple(x.shape), x.dtype)), stage(s, x, params))[1])
        train, val = tr._loaders(0)
        loss, t1, t5, _ = tr.train_epoch(0, train)
        assert math.isfinite(loss) and loss > 0, loss
        assert tr.metrics.buf[3].item() == 24 and tr.last_train_images == 24
        assert seen == [tuple] * 3 and len(erased) == 3
        assert erased[0][0][0] == 8 and erased[0][0][1:3] == (64, 64)
        assert erased[0][1] == (torch.bfloat16 if dtype == "bf16" else torch.float32)
        del seen[:]
        vloss, v1, v5, _ = tr.validate(val)   # validation neither erases nor mixes
        assert seen == [torch.Tensor] * 2 and math.isfinite(vloss) and len(erased) == 3
    finally:
        tr.close()
