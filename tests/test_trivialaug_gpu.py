"""TrivialAugmentWide on the GPU (--trivialaugment): ``ops.misc.randaug_u8`` (csrc/kernels/randaug.hip) against
``randaug_torch`` bit for bit at the stage's wide ranges -- shears to 0.99, rotations to 135 degrees, blends from
F = 3 to F = 509, Posterize down to two bits -- which RandAugment's tests (magnitude 9 of its narrower ranges) never
reach, and one drawn batch through ``InputTransform`` with RandomResizedCrop on both backends."""

import functools

import pytest
import torch

from imagent_amd.data import randaug as RA
from imagent_amd.data import trivialaug as TA

pytestmark = pytest.mark.gpu

DEV = "cuda"
BINS = (0, 1, 15, 29, 30)


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """Every op x BINS x both signs, one image each: (u8, params, {fill: reference}), computed once."""
    rows = [[op] + TA.ta_op_args(op, b, neg, H, W) for op in range(RA.NUM_OPS) for b in BINS for neg in (False, True)]
    params = torch.tensor(rows, dtype=torch.int32).view(-1, 1, 8)
    g = torch.Generator().manual_seed(H * 1000 + W)
    u8 = torch.randint(0, 256, (len(rows), H, W, 3), dtype=torch.uint8, generator=g)
    narrow = torch.arange(len(rows)) % 3 == 0  # a third of the images, and AutoContrast's own, span a narrow range:
    narrow |= params[:, 0, 0] == RA.AUTOCONTRAST  # it has work to do
    u8[narrow] = (u8[narrow].float() * 0.6 + 40).to(torch.uint8)
    return u8, params, {fill: RA.randaug_torch(u8, params, fill) for fill in (0, 128)}


@pytest.mark.parametrize("fill", [0, 128])
@pytest.mark.parametrize("H,W", [(33, 71), (64, 64)])
def test_every_op_at_the_wide_ranges(H, W, fill):
    from imagent_amd.ops.misc import randaug_u8
    u8, params, want = _case(H, W)
    assert params.shape[0] == 14 * 5 * 2
    got = randaug_u8(u8.to(DEV), params.to(DEV), fill).cpu()
    for i in range(params.shape[0]):
        op = int(params[i, 0, 0])
        assert torch.equal(got[i], want[fill][i]), (RA.OP_NAMES[op], BINS[(i // 2) % 5], "neg" if i % 2 else "pos")
    # the wide ends are no identity: the test has something to compare
    changed = [not torch.equal(want[fill][i], u8[i]) for i in range(params.shape[0])]
    for op in range(1, RA.NUM_OPS):
        assert changed[op * 10 + 8] and changed[op * 10 + 9], RA.OP_NAMES[op]  # bin 30, both signs
    # and the stage object gives the same on explicit draws
    assert torch.equal(TA.TrivialAugmentWide("hip", fill=fill)(u8.to(DEV), params.to(DEV)).cpu(), got)


def test_drawn_batch_through_the_input_transform():
    """64 drawn images: the stage's two backends agree bit for bit on the stage's own draws, and the crop that
    follows agrees within tests/test_rrc_gpu.py's tolerance (bf16: 2^-7 of the largest reference value + 1e-3;
    fp32: 1e-4)."""
    from imagent_amd.data.augment import sample_boxes
    from imagent_amd.data.loader import InputTransform
    B, H, W = 64, 45, 52
    g = torch.Generator().manual_seed(8)
    u8 = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)
    stage = TA.TrivialAugmentWide("hip", seed=6)
    stage.set_epoch(2)
    params = stage.draw(B, H, W, DEV)
    assert params.is_cuda and params.shape == (B, 1, 8) and len(params[:, 0, 0].unique()) >= 12
    stage.set_epoch(2)
    own = stage(u8.to(DEV))  # the call draws what draw() drew
    want = RA.randaug_torch(u8, params.cpu(), 128)
    assert torch.equal(own.cpu(), want)
    assert torch.equal(TA.TrivialAugmentWide("torch")(u8.to(DEV), params).cpu(), want)
    scale, ratio = (0.08, 1.0), (0.75, 1.3333)
    boxes = sample_boxes(B, H, W, scale, ratio, torch.Generator().manual_seed(5), "cpu")
    flip = (torch.arange(B) % 3 == 0).to(torch.uint8)
    kw = dict(rrc=(scale, ratio), flip=True)
    ref = InputTransform("torch", (32, 32), randaug=TA.TrivialAugmentWide("torch"), **kw)(
        u8, boxes=boxes, flip=flip, ra_params=params.cpu()).permute(0, 2, 3, 1)
    for backend, dtype, bound in (("hip", torch.bfloat16, 2 ** -7 * ref.abs().max().item() + 1e-3),
                                  ("hip_f32", torch.float32, 1e-4)):
        t = InputTransform(backend, (32, 32), cpad=4, randaug=TA.TrivialAugmentWide(backend), **kw)
        out = t(u8.to(DEV), boxes=boxes.to(DEV), flip=flip.to(DEV), ra_params=params)
        assert out.dtype == dtype and out.shape == (B, 32, 32, 4) and not out[..., 3:].any()
        assert (out[..., :3].float().cpu() - ref).abs().max().item() <= bound, backend
        # and it is the transform without the stage on the stage's reference output, exactly
        plain = InputTransform(backend, (32, 32), cpad=4, **kw)(want.to(DEV), boxes=boxes.to(DEV), flip=flip.to(DEV))
        assert torch.equal(out, plain)
