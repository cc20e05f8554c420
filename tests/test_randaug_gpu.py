"""RandAugment's HIP kernels (csrc/kernels/randaug.hip through ops.misc.randaug_u8) against the definition in torch
integer ops (data.randaug.randaug_torch, itself held to a per-pixel loop by tests/test_randaug_cpu.py): bit for
bit, every op alone with both signs, mixed batches of several layers, offsets past 2^31 bytes, and the stage inside
the input transform and the trainer."""

import functools
import math

import pytest
import torch

from imagent_amd.data import randaug as RA

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(3, 37, 41),   # 4,551 bytes per image, odd: every image starts at another alignment
          (2, 64, 64), (2, 130, 67), (2, 3, 5), (1, 1, 1)]
KINDS = ["random", "constant", "constant_channel", "two_valued", "ramp"]


def all_rows(m, H, W):
    """Every op, both signs where it has one."""
    rows = []
    for op in range(14):
        rows.append([op] + RA.op_args(op, m, False, H, W))
        if 1 <= op <= 9:
            rows.append([op] + RA.op_args(op, m, True, H, W))
    return rows


def make_input(kind, B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + B * 100 + H * 10 + W)
    u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    if kind == "constant":
        u8 = torch.full((B, H, W, 3), 93, dtype=torch.uint8)
    elif kind == "constant_channel":
        u8[..., 1] = 200
    elif kind == "two_valued":
        u8 = torch.where(u8 < 90, torch.full_like(u8, 50), torch.full_like(u8, 150))
    elif kind == "ramp":  # every value 0 .. 255 over the image's bytes, wrapping
        u8 = (torch.arange(B * H * W * 3) % 256).to(torch.uint8).view(B, H, W, 3)
    if kind == "random":
        u8.view(-1)[0] = 255  # (Solarize's >= at the top of the range)
    return u8


@functools.lru_cache(maxsize=None)
def single_op_case(shape, kind):
    """(images on the device, [(row, reference)]): the torch reference of every op row, computed once on the CPU."""
    B, H, W = shape
    u8 = make_input(kind, B, H, W)
    refs = []
    for m in (9, 30):
        for r in all_rows(m, H, W):
            if m == 30 and r[0] in (0, 12, 13):
                continue  # no magnitude: the same row as at 9
            params = torch.tensor([[r]] * B, dtype=torch.int32)
            refs.append((tuple(r), RA.randaug_torch(u8, params, 128)))
    return u8.to(DEV), refs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_op_alone(shape, kind):
    from imagent_amd.ops.misc import randaug_u8
    u8, refs = single_op_case(shape, kind)
    B = shape[0]
    keep = u8.clone()
    for r, want in refs:
        params = torch.tensor([[list(r)]] * B, dtype=torch.int32, device=DEV)
        got = randaug_u8(u8, params, 128)
        assert got.dtype == torch.uint8 and got.shape == u8.shape and got.data_ptr() != u8.data_ptr()
        bad = (got.cpu() != want).nonzero()
        assert bad.numel() == 0, (RA.OP_NAMES[r[0]], r, bad[:4].tolist(), got.cpu()[tuple(bad[0])].item(),
                                  want[tuple(bad[0])].item())
    assert torch.equal(u8, keep)  # the input is never written


def test_each_image_takes_its_own_op():
    """One launch, every op row on another image: the op is a per-block choice."""
    from imagent_amd.ops.misc import randaug_u8
    H, W = 37, 41
    rows = all_rows(9, H, W) + all_rows(30, H, W)
    B = len(rows)
    u8 = make_input("random", B, H, W, seed=1)
    params = torch.tensor(rows, dtype=torch.int32).view(B, 1, 8)
    want = RA.randaug_torch(u8, params, 0)
    got = randaug_u8(u8.to(DEV), params.to(DEV), 0).cpu()
    for b in range(B):
        assert torch.equal(got[b], want[b]), (b, RA.OP_NAMES[rows[b][0]], rows[b])


@functools.lru_cache(maxsize=None)
def mixed_case():
    B, L, H, W = 29, 3, 45, 52
    u8 = make_input("random", B, H, W, seed=2)
    params = RA.sample_params(B, L, 9, H, W, torch.Generator().manual_seed(11), "cpu")
    # statistics ops following each other: the second must see the first's output (also behind a gather)
    r = lambda op, neg=False: [op] + RA.op_args(op, 9, neg, H, W)  # noqa: E731
    params[0] = torch.tensor([r(8), r(13), r(12)], dtype=torch.int32)
    params[1] = torch.tensor([r(13), r(8, True), r(8)], dtype=torch.int32)
    params[2] = torch.tensor([r(5), r(12), r(13)], dtype=torch.int32)
    params[3] = torch.tensor([r(12), r(12), r(9)], dtype=torch.int32)
    return u8, params, RA.randaug_torch(u8, params, 128)


def test_mixed_batch_of_three_layers():
    from imagent_amd.ops.misc import randaug_u8
    u8, params, want = mixed_case()
    assert len(params[..., 0].unique()) >= 12  # the draws cover the table
    d = u8.to(DEV)
    keep = d.clone()
    got = randaug_u8(d, params.to(DEV), 128)
    again = randaug_u8(d, params.to(DEV), 128)
    for b in range(u8.shape[0]):
        assert torch.equal(got[b].cpu(), want[b]), (b, [RA.OP_NAMES[o] for o in params[b, :, 0].tolist()])
    assert torch.equal(got, again)   # two calls give equal results
    assert torch.equal(d, keep)      # and leave the input as it was
    # the stage object: the same through RandAugment("hip") with explicit draws, and one and two layers of them
    assert torch.equal(RA.RandAugment("hip", 3, 9)(d, params.to(DEV)), got)
    for L in (1, 2):
        sub = params[:, :L].contiguous()
        assert torch.equal(randaug_u8(d, sub.to(DEV), 128).cpu(), RA.randaug_torch(u8, sub, 128)), L


def test_arguments():
    from imagent_amd.ops.misc import randaug_u8
    u8 = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device=DEV)
    ok = torch.zeros((2, 1, 8), dtype=torch.int32, device=DEV)
    for imgs, params, fill in ((u8.float(), ok, 0), (u8[..., :2], ok, 0), (u8, ok[:1], 0), (u8, ok[..., :4], 0),
                               (u8, ok, 256), (u8, ok, -1)):
        with pytest.raises(ValueError):
            randaug_u8(imgs, params, fill)
    assert randaug_u8(u8[:0], ok[:0], 0).shape == (0, 4, 4, 3)


def test_past_2gb():
    """A 16-image 448 x 448 batch repeated 224 times (2.16 GB; params repeated the same way, an affine, a table and a
    statistics op among each image's layers): every repeat equals the 16-image launch, chunk by chunk."""
    from imagent_amd.ops.misc import randaug_u8
    H = W = 448
    g = torch.Generator(device=DEV).manual_seed(5)
    base = torch.randint(0, 256, (16, H, W, 3), generator=g, device=DEV, dtype=torch.uint8)
    r = lambda op, neg=False: [op] + RA.op_args(op, 9, neg, H, W)  # noqa: E731
    layers = [[r(5), r(11), r(13)], [r(8), r(1, True), r(10)], [r(6), r(12), r(3)], [r(9), r(4, True), r(8, True)]]
    p16 = torch.tensor([layers[i % 4] for i in range(16)], dtype=torch.int32, device=DEV)
    p16[8:, :, :] = p16[8:].flip(1)  # and in the other order
    small = randaug_u8(base, p16, 128)
    assert not torch.equal(small, base)
    big_in = base.repeat(224, 1, 1, 1)
    assert big_in.numel() > 2 ** 31
    big = randaug_u8(big_in, p16.repeat(224, 1, 1), 128)
    del big_in
    for i in range(224):
        assert torch.equal(big[16 * i:16 * i + 16], small), i


def test_inside_the_input_transform():
    """InputTransform("hip", rrc=..., randaug=...) on explicit boxes, flips and params is the transform without the
    stage applied to randaug_torch(u8): exactly."""
    from imagent_amd.data.loader import InputTransform
    B, H, W = 6, 45, 52
    u8, params, _ = mixed_case()
    u8, params = u8[:B].contiguous(), params[:B].contiguous()
    boxes = torch.tensor([[0, 0, 45, 52], [3, 5, 30, 40], [10, 2, 20, 20], [0, 12, 45, 30], [7, 7, 8, 9],
                          [20, 20, 25, 32]], dtype=torch.int32, device=DEV)
    flip = torch.tensor([0, 1, 0, 1, 1, 0], dtype=torch.uint8, device=DEV)
    rrc = ((0.08, 1.0), (0.75, 1.3333))
    for backend in ("hip", "hip_f32"):
        with_stage = InputTransform(backend, (32, 32), cpad=4, flip=True, rrc=rrc,
                                    randaug=RA.RandAugment(backend, 3, 9, fill=128))
        without = InputTransform(backend, (32, 32), cpad=4, flip=True, rrc=rrc)
        got = with_stage(u8.to(DEV), boxes, flip, ra_params=params.to(DEV))
        want = without(RA.randaug_torch(u8, params, 128).to(DEV), boxes, flip)
        assert got.dtype == want.dtype and torch.equal(got, want), backend
    # and the plain (no box) path
    got = InputTransform("hip", (45, 52), cpad=4, randaug=RA.RandAugment("hip", 3, 9))(u8.to(DEV),
                                                                                    ra_params=params.to(DEV))
    assert torch.equal(got, InputTransform("hip", (45, 52), cpad=4)(RA.randaug_torch(u8, params, 128).to(DEV)))


def test_trainer_three_steps(tmp_path, monkeypatch):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    args = ["--arch", "resnet18", "--image-size", "64", "--data", "synthetic", "--synthetic-train-size", "64",
            "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "100", "--quiet-banner", "--tb-dir", "",
            "--kernels", "hip", "--launcher", "single", "--randaugment", "9", "--random-resized-crop", "--flip",
            "--mixup", "0.2", "--max-steps", "3", "--log-interval", "0"]
    tr = Trainer(build_parser().parse_args(args))
    try:
        assert tr.randaug is not None and tr.randaug.backend == "hip" and tr.transform_val.randaug is None
        calls = []
        stage = tr.randaug.__call__
        monkeypatch.setattr(type(tr.randaug), "__call__", lambda self, u8, params=None: (calls.append(u8.shape),
                                                                                         stage(u8, params))[1])
        train, val = tr._loaders(0)
        loss, t1, t5, _ = tr.train_epoch(0, train)
        assert math.isfinite(loss) and loss > 0, loss
        assert tr.last_train_images == 24 and len(calls) == 3
        vloss, v1, v5, _ = tr.validate(val)   # validation never augments
        assert math.isfinite(vloss) and len(calls) == 3
    finally:
        tr.close()
