"""RandomResizedCrop fused into the input normalise on the GPU (--random-resized-crop, csrc/kernels/misc.hip
rrc_normalize_kernel). Yardstick: the resampling definition in float64 on the host (tests/test_rrc_cpu.py holds it to
``F.interpolate(antialias=True)``), then ToTensor / Normalize with MEAN / STD as tests/test_resize_gpu.py.

One launch mixes seven boxes of a 97 x 131 source (neither a multiple of 4): the full image, a box touching (0, 0),
one touching the bottom-right corner, an up-scale (20 x 31), an anisotropic one (16 x 120: 0.43 vertical, 3 horizontal
onto 37 x 40), one row (1 x 50) and scale exactly 2 (74 x 80 onto 37 x 40) -- one sample more than the six the
shapes were first planned with, so that no box shares a sample. Outputs 37 x 40 and 64 x 80 (the 8-row band does
not divide 37), channel padding 4 and 8, bf16 and fp32, a mixed flip mask and none. A 192 x 192 box of a 200 x 200
source onto 32 x 32 (scale 6) takes the many-tap loops, a 200 x 200 box onto 8 x 160 (scale 25 vertically: its band
does not fit the LDS rows) the generic per-pixel gather.

bf16 bound: 2^-7 of the largest reference value + 1e-3, the bound of tests/test_resize_gpu.py. fp32 bound: 1e-4
(at most 13 taps per axis at scale 6, weights good to ~1e-6, values <= 255, then / 255 and / std 0.25: ~2e-5, x 5).
No test feeds the GPU a box outside its image."""

import functools

import numpy as np
import pytest
import torch

from test_rrc_cpu import MEAN, RATIO, SCALE, STD, yardstick

pytestmark = pytest.mark.gpu

SRC = (97, 131)
BOXES = [(0, 0, 97, 131), (0, 0, 50, 60), (52, 61, 45, 70), (30, 40, 20, 31), (40, 5, 16, 120), (96, 50, 1, 50),
         (10, 20, 74, 80)]
FLIP = [0, 1, 1, 0, 1, 1, 0]
B = len(BOXES)


@functools.lru_cache(maxsize=None)
def _images(shape=SRC, n=B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n,) + shape + (3,), dtype=torch.uint8, generator=g)


@functools.lru_cache(maxsize=None)
def _reference(size, flipped, boxes=tuple(BOXES), shape=SRC, seed=0):
    """float64 [B, H, W, 3], computed once per case and shared (read-only)."""
    ref = yardstick(_images(shape, len(boxes), seed), boxes, size, FLIP[:len(boxes)] if flipped else None)
    ref.setflags(write=False)
    return ref


def _check(y, ref, cpad, dtype):
    assert y.shape == ref.shape[:3] + (cpad,) and y.dtype == dtype
    err = np.abs(y[..., :3].double().cpu().numpy() - ref).max()
    bound = 1e-4 if dtype == torch.float32 else 2 ** -7 * np.abs(ref).max() + 1e-3
    print(f"rrc {tuple(ref.shape)} cpad {cpad} {dtype}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)
    assert (y[..., 3:] == 0).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("size,cpad", [((37, 40), 4), ((37, 40), 8), ((64, 80), 4), ((64, 80), 8), ((37, 42), 4),
                                       ((37, 40), 3)])
def test_mixed_boxes_match_the_definition(size, cpad, dtype):
    from imagent_amd.ops.misc import rrc_normalize_u8
    u8 = _images().cuda()
    boxes = torch.tensor(BOXES, dtype=torch.int32, device="cuda")
    flip = torch.tensor(FLIP, dtype=torch.uint8, device="cuda")
    for fl in (None, flip):
        y = rrc_normalize_u8(u8, size, cpad, MEAN, STD, boxes, fl, dtype=dtype)
        _check(y, _reference(size, fl is not None), cpad, dtype)
    # host boxes are validated, copied and give the same result
    yh = rrc_normalize_u8(u8, size, cpad, MEAN, STD, torch.tensor(BOXES, dtype=torch.int32), flip, dtype=dtype)
    assert torch.equal(yh, y)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("box,size", [((4, 4, 192, 192), (32, 32)), ((0, 0, 200, 200), (8, 160))],
                         ids=["scale6", "generic_gather"])
def test_large_scales(box, size, dtype):
    from imagent_amd.ops.misc import rrc_normalize_u8
    boxes = (box, (3, 5, 150, 97))
    u8 = _images((200, 200), 2, 7).cuda()
    flip = torch.tensor(FLIP[:2], dtype=torch.uint8, device="cuda")
    bx = torch.tensor(boxes, dtype=torch.int32, device="cuda")
    for fl in (None, flip):
        y = rrc_normalize_u8(u8, size, 4, MEAN, STD, bx, fl, dtype=dtype)
        _check(y, _reference(size, fl is not None, boxes, (200, 200), 7), 4, dtype)


@pytest.mark.parametrize("cpad", [4, 8])
def test_box_of_the_output_size_is_the_plain_crop(cpad):
    """n == m: the weights are exactly 1 and 0, bit for bit normalize_u8 with that crop, flip included."""
    from imagent_amd.ops.f32 import normalize_u8_f32
    from imagent_amd.ops.misc import normalize_u8, rrc_normalize_u8
    u8 = _images().cuda()
    crop = torch.tensor([[0, 0], [60, 91], [13, 7], [1, 90], [59, 0], [30, 44], [60, 1]], dtype=torch.int32,
                        device="cuda")
    boxes = torch.cat([crop, torch.tensor([[37, 40]] * B, dtype=torch.int32, device="cuda")], 1).contiguous()
    flip = torch.tensor(FLIP, dtype=torch.uint8, device="cuda")
    for fl in (None, flip):
        a = rrc_normalize_u8(u8, (37, 40), cpad, MEAN, STD, boxes, fl)
        assert torch.equal(a, normalize_u8(u8, (37, 40), cpad, MEAN, STD, crop, fl))
        a32 = rrc_normalize_u8(u8, (37, 40), cpad, MEAN, STD, boxes, fl, dtype=torch.float32)
        assert (a32 - normalize_u8_f32(u8, (37, 40), cpad, MEAN, STD, crop, fl)).abs().max().item() <= 1e-6


def test_upscaled_box_is_the_bilinear_resize_of_the_crop():
    """Both scales <= 1: plain bilinear, resize_normalize_u8 of the cropped tensor."""
    from imagent_amd.ops.misc import resize_normalize_u8, rrc_normalize_u8
    u8 = _images().cuda()
    t, l, h, w = 30, 40, 20, 31
    boxes = torch.tensor([[t, l, h, w]] * B, dtype=torch.int32, device="cuda")
    flip = torch.tensor(FLIP, dtype=torch.uint8, device="cuda")
    a = rrc_normalize_u8(u8, (64, 80), 4, MEAN, STD, boxes, flip).float()
    b = resize_normalize_u8(u8[:, t:t + h, l:l + w].contiguous(), (64, 80), 4, MEAN, STD, flip).float()
    assert (a - b).abs().max().item() <= 2 ** -7 * b.abs().max().item() + 1e-3


def test_backends_agree_on_the_same_draws():
    from imagent_amd.data.augment import sample_boxes
    from imagent_amd.data.loader import InputTransform
    u8 = _images()
    boxes = sample_boxes(B, SRC[0], SRC[1], SCALE, RATIO, torch.Generator().manual_seed(5), "cpu")
    flip = torch.tensor(FLIP, dtype=torch.uint8)
    kw = dict(rrc=(SCALE, RATIO), mean=MEAN, std=STD, flip=True)
    ref = InputTransform("torch", (37, 40), **kw)(u8, boxes=boxes, flip=flip).permute(0, 2, 3, 1)
    hip = InputTransform("hip", (37, 40), cpad=4, **kw)(u8.cuda(), boxes=boxes.cuda(), flip=flip.cuda())
    assert hip.dtype == torch.bfloat16 and hip.shape == (B, 37, 40, 4)
    assert (hip[..., :3].float().cpu() - ref).abs().max().item() <= 2 ** -7 * ref.abs().max().item() + 1e-3
    f32 = InputTransform("hip_f32", (37, 40), cpad=4, **kw)(u8.cuda(), boxes=boxes.cuda(), flip=flip.cuda())
    assert f32.dtype == torch.float32
    assert (f32[..., :3].cpu() - ref).abs().max().item() <= 1e-4
    # the validation transform: the centre box, no randomness, no flip
    vref = InputTransform("torch", (32, 32), center_frac=0.875, mean=MEAN, std=STD)(u8).permute(0, 2, 3, 1)
    for backend, bound in (("hip", 2 ** -7 * vref.abs().max().item() + 1e-3), ("hip_f32", 1e-4)):
        va = InputTransform(backend, (32, 32), cpad=4, center_frac=0.875, mean=MEAN, std=STD)
        v = va(u8.cuda())
        assert torch.equal(v, va(u8.cuda()))
        assert (v[..., :3].float().cpu() - vref).abs().max().item() <= bound


def test_own_draws_on_the_device_repeat_per_epoch():
    from imagent_amd.data.loader import InputTransform
    u8 = _images().cuda()
    tr = InputTransform("hip", (37, 40), cpad=4, rrc=(SCALE, RATIO), flip=True, seed=3)
    a, b = tr(u8), tr(u8)
    assert a.shape == (B, 37, 40, 4) and torch.isfinite(a.float()).all()
    assert not torch.equal(a, b)
    tr.set_epoch(0)
    assert torch.equal(a, tr(u8))
    tr.set_epoch(1)
    assert not torch.equal(a, tr(u8))


def test_past_2gb():
    """A > 2 GB uint8 tensor (3600 images of 448 x 448): cat([x, x]) with duplicated boxes gives bit-identical halves
    that equal the small launch. Boxes from 45 x 45 up to the whole image onto 32 x 32: the separable path and (past
    scale ~12) the generic gather."""
    from imagent_amd.data.augment import sample_boxes
    from imagent_amd.ops.misc import rrc_normalize_u8
    n = 1800
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randint(0, 256, (n, 448, 448, 3), dtype=torch.uint8, device="cuda", generator=g)
    x2 = torch.cat([x, x])
    assert x2.numel() > 2 ** 31
    boxes = sample_boxes(n, 448, 448, (0.01, 1.0), RATIO, g, "cuda")
    boxes[0] = torch.tensor([0, 0, 448, 448], dtype=torch.int32)
    flip = (torch.arange(n, device="cuda") % 2).to(torch.uint8)
    y = rrc_normalize_u8(x, (32, 32), 4, MEAN, STD, boxes, flip)
    y2 = rrc_normalize_u8(x2, (32, 32), 4, MEAN, STD, torch.cat([boxes, boxes]), torch.cat([flip, flip]))
    assert torch.equal(y2[:n], y2[n:]), "the two halves differ"
    assert torch.equal(y2[:n], y), "the large launch differs from the small one"
    assert torch.isfinite(y.float()).all() and y.float().abs().max().item() > 0.5
