"""RandomResizedCrop without a GPU: the box sampler (data/augment.py) against a scalar loop of the published rule,
the resampling definition that the HIP kernel, the torch backend and the GPU tests share (README "Input",
csrc/kernels/misc.hip rrc_normalize_kernel) against ``F.interpolate(antialias=True)``, the torch backend of
``InputTransform``, the host-side box validation and the command line."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

MEAN, STD = (0.5, 0.45, 0.4), (0.5, 0.25, 0.3)
SCALE, RATIO = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)


# ------------------------------------------------------------------ the resampling definition, float64
def axis_weights(n, m):
    """[m, n] weights of one axis: a box of n source pixels onto m outputs (taps clamped to the box)."""
    s = n / m
    sup = max(s, 1.0)
    wm = np.zeros((m, n))
    for i in range(m):
        c = (i + 0.5) * s
        lo, hi = max(0, int(c - sup + 0.5)), min(n, int(c + sup + 0.5))
        w = np.array([max(0.0, 1.0 - abs((j - c + 0.5) / sup)) for j in range(lo, hi)])
        wm[i, lo:hi] = w / w.sum()
    return wm


def yardstick(u8, boxes, size, flip=None, mean=MEAN, std=STD):
    """uint8 [B, Hs, Ws, 3] -> float64 [B, H, W, 3]: the box resampled with the outer product of the two axes'
    weights, then (v / 255 - mean) / std, flip mirrors the output columns."""
    H, W = size
    out = np.zeros((u8.shape[0], H, W, 3))
    a = u8.numpy().astype(np.float64)
    for b, (t, l, h, w) in enumerate(np.asarray(boxes).tolist()):
        crop = a[b, t:t + h, l:l + w]
        v = np.einsum("ij,jkc->ikc", axis_weights(h, H), np.einsum("kl,jlc->jkc", axis_weights(w, W), crop))
        v = (v / 255.0 - np.array(mean)) / np.array(std)
        out[b] = v[:, ::-1] if (flip is not None and int(flip[b])) else v
    return out


@pytest.mark.parametrize("src,box,size", [((97, 131), (5, 9, 80, 117), (32, 40)), ((64, 64), (3, 5, 7, 50), (32, 32)),
                                          ((48, 40), (0, 0, 48, 40), (48, 40))])
def test_definition_matches_antialiased_interpolate(src, box, size):
    torch.manual_seed(0)
    u8 = torch.randint(0, 256, (1,) + src + (3,), dtype=torch.uint8)
    t, l, h, w = box
    ref = F.interpolate(u8[:, t:t + h, l:l + w].permute(0, 3, 1, 2).float(), size=size, mode="bilinear",
                        antialias=True, align_corners=False).permute(0, 2, 3, 1).double().numpy()
    got = yardstick(u8, [box], size, mean=(0.0,) * 3, std=(1.0 / 255.0,) * 3)  # grey levels
    err = np.abs(got - ref).max()
    print("definition vs interpolate(antialias=True), grey levels:", err)
    assert err <= 5e-3, err
    if (h, w) == size:  # the identity: weights exactly 1 and 0
        assert np.array_equal(got[0], u8[0].double().numpy())


# ------------------------------------------------------------------ the box sampler
def scalar_boxes(ua, ul, up, Hs, Ws, scale, ratio):
    out = []
    for b in range(len(ua)):
        box = None
        for t in range(len(ua[b])):
            area = Hs * Ws * (scale[0] + (scale[1] - scale[0]) * ua[b][t])
            aspect = math.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * ul[b][t])
            w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if 0 < w <= Ws and 0 < h <= Hs:
                top = min(max(int(math.floor(up[b][0] * (Hs - h + 1))), 0), Hs - h)
                left = min(max(int(math.floor(up[b][1] * (Ws - w + 1))), 0), Ws - w)
                box = (top, left, h, w)
                break
        if box is None:
            in_ratio = Ws / Hs
            if in_ratio < ratio[0]:
                w, h = Ws, min(Hs, int(round(Ws / ratio[0])))
            elif in_ratio > ratio[1]:
                h, w = Hs, min(Ws, int(round(Hs * ratio[1])))
            else:
                w, h = Ws, Hs
            box = ((Hs - h) // 2, (Ws - w) // 2, h, w)
        out.append(box)
    return out


@pytest.mark.parametrize("Hs,Ws", [(448, 448), (97, 131), (32, 32), (40, 400)])
def test_boxes_from_uniforms_equals_scalar_loop(Hs, Ws):
    from imagent_amd.data.augment import TRIES, boxes_from_uniforms
    g = torch.Generator().manual_seed(Hs * 1000 + Ws)
    B = 512
    ua, ul, up = torch.rand(B, TRIES, generator=g), torch.rand(B, TRIES, generator=g), torch.rand(B, 2, generator=g)
    got = boxes_from_uniforms(ua, ul, up, Hs, Ws, SCALE, RATIO)
    assert got.dtype == torch.int32 and got.shape == (B, 4)
    ref = scalar_boxes(ua.double().tolist(), ul.double().tolist(), up.double().tolist(), Hs, Ws, SCALE, RATIO)
    assert got.tolist() == [list(r) for r in ref]
    fell_back = sum(1 for r in ref if r == ((Hs - r[2]) // 2, (Ws - r[3]) // 2, r[2], r[3]) and
                    (r[3] == Ws or r[2] == Hs))
    if (Hs, Ws) == (40, 400):  # most samples find no fitting try: the centre crop at the clamped aspect
        assert fell_back > B // 2, fell_back
        assert (40 // 2 - 20, (400 - 53) // 2, 40, 53) in ref


def test_sample_boxes_inside_and_reproducible():
    from imagent_amd.data.augment import sample_boxes
    from imagent_amd.data.loader import InputTransform
    for Hs, Ws in [(448, 448), (97, 131), (40, 400)]:
        g = torch.Generator().manual_seed(3)
        bx = sample_boxes(1000, Hs, Ws, SCALE, RATIO, g, "cpu")
        t, l, h, w = bx.long().unbind(1)
        assert (t >= 0).all() and (l >= 0).all() and (h >= 1).all() and (w >= 1).all()
        assert (t + h <= Hs).all() and (l + w <= Ws).all()
        assert torch.equal(bx, sample_boxes(1000, Hs, Ws, SCALE, RATIO, torch.Generator().manual_seed(3), "cpu"))
    assert len(set(map(tuple, bx.tolist()))) > 100
    # the transform's own generator: (seed, rank, epoch) decide the draws
    u8 = torch.randint(0, 256, (4, 40, 48, 3), dtype=torch.uint8)

    def run(epoch, seed=0, rank=0):
        tr = InputTransform("torch", (16, 16), rrc=(SCALE, RATIO), flip=True, seed=seed, rank=rank)
        tr.set_epoch(epoch)
        return tr(u8)

    assert torch.equal(run(0), run(0))
    assert not torch.equal(run(0), run(1))
    assert not torch.equal(run(0), run(0, seed=1))
    assert not torch.equal(run(0), run(0, rank=1))
    tr = InputTransform("torch", (16, 16), rrc=(SCALE, RATIO))
    a = tr(u8)
    assert not torch.equal(a, tr(u8))  # a second batch of the epoch draws new boxes
    tr.set_epoch(0)
    assert torch.equal(a, tr(u8))      # the epoch starts over


def test_center_box():
    from imagent_amd.data.augment import center_box
    assert center_box(256, 256, 0.875) == (16, 16, 224, 224)
    assert center_box(97, 131, 0.875) == ((97 - 85) // 2, (131 - 115) // 2, 85, 115)
    assert center_box(97, 131, 1.0) == (0, 0, 97, 131)
    with pytest.raises(ValueError):
        center_box(10, 10, 0.0)


# ------------------------------------------------------------------ the torch backend, host validation
def test_torch_backend_matches_the_definition():
    from imagent_amd.data.loader import InputTransform
    torch.manual_seed(1)
    u8 = torch.randint(0, 256, (5, 97, 131, 3), dtype=torch.uint8)
    boxes = torch.tensor([[0, 0, 97, 131], [5, 9, 80, 117], [77, 100, 20, 31], [3, 4, 20, 31], [10, 20, 37, 40]],
                         dtype=torch.int32)
    flip = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8)
    tr = InputTransform("torch", (37, 40), rrc=(SCALE, RATIO), mean=MEAN, std=STD)
    for fl in (None, flip):
        y = tr(u8, boxes=boxes, flip=fl)
        assert y.shape == (5, 3, 37, 40) and y.dtype == torch.float32
        ref = yardstick(u8, boxes, (37, 40), fl)
        # 5e-3 grey levels (the definition vs interpolate) through / 255 / std
        assert np.abs(y.permute(0, 2, 3, 1).double().numpy() - ref).max() <= 5e-3 / 255.0 / min(STD) + 1e-6
    # its own draws: the requested size, inside the image by construction
    assert tr(u8).shape == (5, 3, 37, 40)
    # the validation transform: the centre box, no randomness
    va = InputTransform("torch", (32, 32), center_frac=0.875, mean=MEAN, std=STD, flip=True)
    from imagent_amd.data.augment import center_box
    v = va(u8)
    assert torch.equal(v, va(u8))
    ref = yardstick(u8, [center_box(97, 131, 0.875)] * 5, (32, 32))
    assert np.abs(v.permute(0, 2, 3, 1).double().numpy() - ref).max() <= 5e-3 / 255.0 / min(STD) + 1e-6


def test_rrc_takes_precedence_and_old_paths_stay():
    from imagent_amd.data.loader import InputTransform
    u8 = torch.randint(0, 256, (2, 24, 24, 3), dtype=torch.uint8)
    full = torch.tensor([[0, 0, 24, 24]] * 2, dtype=torch.int32)
    a = InputTransform("torch", (12, 12), rrc=(SCALE, RATIO), resize=True)(u8, boxes=full)
    ref = yardstick(u8, full, (12, 12), mean=(0.5,) * 3, std=(0.5,) * 3)
    assert np.abs(a.permute(0, 2, 3, 1).double().numpy() - ref).max() < 1e-4
    plain = InputTransform("torch", (24, 24))
    assert plain.rrc is None and plain.center_frac is None
    assert torch.equal(plain(u8), (u8.permute(0, 3, 1, 2).float() / 255.0 - 0.5) / 0.5)
    with pytest.raises(ValueError):
        plain(u8, boxes=full)
    with pytest.raises(ValueError):
        InputTransform("torch", (12, 12), rrc=((0.5, 0.2), RATIO))


@pytest.mark.parametrize("box", [(-1, 0, 10, 10), (0, 0, 41, 10), (35, 0, 10, 10), (0, 45, 10, 10), (0, 0, 0, 10)])
def test_host_boxes_outside_the_image_raise(box):
    from imagent_amd.ops.misc import rrc_normalize_u8
    u8 = torch.zeros((1, 40, 48, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="outside"):
        rrc_normalize_u8(u8, (16, 16), 4, MEAN, STD, torch.tensor([box], dtype=torch.int32))
    with pytest.raises(ValueError, match="boxes"):
        rrc_normalize_u8(u8, (16, 16), 4, MEAN, STD, torch.zeros((2, 4), dtype=torch.int32))


# ------------------------------------------------------------------ command line, trainer
COMMON = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
          "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--quiet-banner", "--tb-dir", "",
          "--device", "cpu", "--kernels", "torch", "--launcher", "single"]


def test_cli_flags():
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    p = build_parser()
    a = p.parse_args(COMMON)
    assert a.random_resized_crop is False and a.rrc_scale == [0.08, 1.0] and a.rrc_ratio == [0.75, 1.3333]
    assert a.val_center_crop == 1.0 and a.source_size is None
    a = p.parse_args(COMMON + ["--random-resized-crop", "--rrc-scale", "0.25", "1", "--rrc-ratio", "0.5", "2",
                               "--val-center-crop", "0.875", "--source-size", "64"])
    assert a.random_resized_crop and a.rrc_scale == [0.25, 1.0] and a.rrc_ratio == [0.5, 2.0]
    assert a.val_center_crop == 0.875 and a.source_size == 64
    for bad in (["--rrc-scale", "0.5", "0.2"], ["--rrc-scale", "0", "1"], ["--rrc-scale", "0.5", "1.5"],
                ["--rrc-ratio", "2", "0.5"], ["--val-center-crop", "1.5"], ["--source-size", "0"]):
        with pytest.raises(SystemExit):
            Trainer(p.parse_args(COMMON + ["--random-resized-crop"] + bad))


def test_trainer_transforms(tmp_path, monkeypatch):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    tr = Trainer(build_parser().parse_args(COMMON + ["--random-resized-crop", "--flip", "--val-center-crop", "0.875"]))
    try:
        assert tr.transform_train.rrc == ((0.08, 1.0), (0.75, 1.3333)) and tr.transform_train.flip
        assert tr.transform_val.rrc is None and tr.transform_val.center_frac == 0.875 and not tr.transform_val.flip

        def first(epoch):
            train, val = tr._loaders(epoch)
            return next(iter(train))[0].clone(), next(iter(val))[0].clone()

        t0, v0 = first(0)
        t0b, v0b = first(0)
        t1, v1 = first(1)
        assert t0.shape == (8, 3, 32, 32)
        assert torch.equal(t0, t0b) and torch.equal(v0, v0b)  # an epoch repeats its boxes (resume)
        assert not torch.equal(t0, t1)                        # a random train transform
        assert torch.equal(v0, v1)                            # a deterministic val transform
    finally:
        tr.close()
    # without the flags: the existing transforms
    tr = Trainer(build_parser().parse_args(COMMON))
    try:
        assert tr.transform_train.rrc is None and tr.transform_val.center_frac is None
    finally:
        tr.close()
