"""RandAugment (data/randaug.py) without a GPU: the level table, the draws, the torch backend against a plain
per-pixel Python loop written here from the stated integer rules, geometric properties that need no oracle, the
degenerate inputs of the statistics ops, the command line and a short CPU run."""

import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from imagent_amd.data import randaug as RA  # noqa: E402


def P(*rows):
    """params [1, L, 8] from rows (op, a0, ...), zero-padded."""
    return torch.tensor([[list(r) + [0] * (8 - len(r)) for r in rows]], dtype=torch.int32)


def row(op, m, neg, H, W):
    return [op] + RA.op_args(op, m, neg, H, W)


# ------------------------------------------------------------------ the level table, worked out by hand at m = 9
def test_level_table_at_magnitude_9():
    H = W = 224
    u_op = torch.tensor([(op + 0.5) / 14 for op in range(14)] * 2)
    u_sign = torch.tensor([0.75] * 14 + [0.25] * 14)  # positive, then negative
    p = RA.params_from_uniforms(u_op, u_sign, 9, H, W)
    assert p.dtype == torch.int32 and tuple(p.shape) == (28, 8)
    pos, neg = p[:14].tolist(), p[14:].tolist()
    assert [r[0] for r in pos] == list(range(14)) and [r[0] for r in neg] == list(range(14))
    one = 65536
    s = 5898  # round(65536 * 0.09) = round(5898.24)
    assert pos[1][1:] == [one, s, 0, 0, one, 0, 0] and neg[1][1:] == [one, -s, 0, 0, one, 0, 0]      # ShearX 0.09
    assert pos[2][1:] == [one, 0, 0, s, one, 0, 0] and neg[2][1:] == [one, 0, 0, -s, one, 0, 0]      # ShearY
    t = 30  # round(150 / 331 * 0.3 * 224) = round(30.45)
    assert pos[3][1:] == [one, 0, -2 * t * one, 0, one, 0, 0] and neg[3][1:] == [one, 0, 2 * t * one, 0, one, 0, 0]
    assert pos[4][1:] == [one, 0, 0, 0, one, -2 * t * one, 0] and neg[4][1:] == [one, 0, 0, 0, one, 2 * t * one, 0]
    c, sn = 64729, 10252  # round(65536 cos 9 deg) = round(64729.14), round(65536 sin 9 deg) = round(10252.09)
    assert pos[5][1:] == [c, -sn, 0, sn, c, 0, 0] and neg[5][1:] == [c, sn, 0, -sn, c, 0, 0]         # Rotate 9 deg
    for op in (6, 7, 8, 9):  # F = round(256 * 1.27) = round(325.12), round(256 * 0.73) = round(186.88)
        assert pos[op][1] == 325 and neg[op][1] == 187
    assert pos[10][1] == 0xFE == neg[10][1]  # 8 - round(1.2) = 7 bits
    assert pos[11][1] == 179 == neg[11][1]   # ceil(178.5)
    for op in (0, 12, 13):
        assert pos[op][1:] == [0] * 7
    # the ends of the scale
    assert RA.op_args(RA.POSTERIZE, 30, False, H, W)[0] == 0xF0 and RA.op_args(RA.POSTERIZE, 0, False, H, W)[0] == 0xFF
    assert RA.op_args(RA.SOLARIZE, 30, False, H, W)[0] == 0 and RA.op_args(RA.SOLARIZE, 0, False, H, W)[0] == 255
    assert RA.op_args(RA.BRIGHTNESS, 30, False, H, W)[0] == 486 and RA.op_args(RA.BRIGHTNESS, 30, True, H, W)[0] == 26
    # the op choice: min(13, floor(14 u))
    edge = RA.params_from_uniforms(torch.tensor([0.0, 1 / 14 - 1e-4, 1 / 14 + 1e-4, 0.99999, 1.0]), torch.ones(5), 9, H, W)
    assert edge[:, 0].tolist() == [0, 0, 1, 13, 13]


def test_check_randaug():
    RA.check_randaug(1, 0)
    RA.check_randaug(4, 30)
    for n, m in ((0, 9), (5, 9), (2, -1), (2, 31), (2.5, 9), (2, 9.5)):
        with pytest.raises(ValueError):
            RA.check_randaug(n, m)
    with pytest.raises(ValueError):
        RA.RandAugment("torch", 2, 9, fill=256)
    with pytest.raises(ValueError):
        RA.RandAugment("triton", 2, 9)


def test_draws_ranges_and_reseeding():
    g = torch.Generator().manual_seed(3)
    p = RA.sample_params(512, 3, 9, 64, 48, g, "cpu")
    assert tuple(p.shape) == (512, 3, 8) and p.dtype == torch.int32
    ops = p[..., 0]
    assert ops.min() == 0 and ops.max() == 13 and len(ops.unique()) == 14
    f = p[..., 1][ops == RA.BRIGHTNESS]
    assert set(f.tolist()) == {325, 187}          # both signs occur
    s = p[..., 2][ops == RA.SHEAR_X]
    assert set(s.tolist()) == {5898, -5898}
    a = RA.RandAugment("torch", 2, 9, seed=5, rank=1)
    a.set_epoch(3)
    d1, d2 = a.draw(16, 32, 32, "cpu"), a.draw(16, 32, 32, "cpu")
    assert not torch.equal(d1, d2)                # successive batches differ
    b = RA.RandAugment("torch", 2, 9, seed=5, rank=1)
    b.set_epoch(3)
    assert torch.equal(b.draw(16, 32, 32, "cpu"), d1) and torch.equal(b.draw(16, 32, 32, "cpu"), d2)
    b.set_epoch(4)
    assert not torch.equal(b.draw(16, 32, 32, "cpu"), d1)
    b.set_epoch(3)                                # a resumed epoch repeats its draws
    assert torch.equal(b.draw(16, 32, 32, "cpu"), d1)
    assert not torch.equal(RA.RandAugment("torch", 2, 9, seed=5, rank=0).draw(16, 32, 32, "cpu"), d1)
    # unrelated to the crop boxes' and the mixer's streams
    from imagent_amd.data.loader import InputTransform
    from imagent_amd.data.mix import BatchMixer
    seeds = {a._epoch_seed(), InputTransform("torch", (8, 8), seed=5, rank=1)._epoch_seed(),
             BatchMixer("torch", 0.2, seed=5, rank=1)._epoch_seed()}
    assert len(seeds) == 3


# ------------------------------------------------------------------ the independent oracle: a per-pixel loop
def loop_layer(img, H, W, r, fill):
    """img: list [H][W][3] of ints; r: (op, a0 .. a6). Written from the rules of the issue, not from randaug.py."""
    op, a = r[0], r[1:]
    n = H * W

    def clamp(v):
        return max(0, min(255, v))

    def blend(v, d, F):
        return clamp((F * v + (256 - F) * d + 128) >> 8)

    def gray(px):
        return (77 * px[0] + 150 * px[1] + 29 * px[2] + 128) >> 8

    out = [[list(img[y][x]) for x in range(W)] for y in range(H)]
    if 1 <= op <= 5:
        for y in range(H):
            for x in range(W):
                X, Y = 2 * x - (W - 1), 2 * y - (H - 1)
                sx = (a[0] * X + a[1] * Y + a[2] + (W << 16)) >> 17
                sy = (a[3] * X + a[4] * Y + a[5] + (H << 16)) >> 17
                out[y][x] = list(img[sy][sx]) if (0 <= sx < W and 0 <= sy < H) else [fill] * 3
    elif op == 6:
        for y in range(H):
            for x in range(W):
                out[y][x] = [blend(v, 0, a[0]) for v in img[y][x]]
    elif op == 7:
        for y in range(H):
            for x in range(W):
                out[y][x] = [blend(v, gray(img[y][x]), a[0]) for v in img[y][x]]
    elif op == 8:
        d = (sum(gray(img[y][x]) for y in range(H) for x in range(W)) + n // 2) // n
        for y in range(H):
            for x in range(W):
                out[y][x] = [blend(v, d, a[0]) for v in img[y][x]]
    elif op == 9:
        for y in range(H):
            for x in range(W):
                for c in range(3):
                    v = img[y][x][c]
                    d = v
                    if 0 < y < H - 1 and 0 < x < W - 1:
                        d = (sum(img[y + dy][x + dx][c] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) + 4 * v + 6) // 13
                    out[y][x][c] = blend(v, d, a[0])
    elif op == 10:
        for y in range(H):
            for x in range(W):
                out[y][x] = [v & a[0] for v in img[y][x]]
    elif op == 11:
        for y in range(H):
            for x in range(W):
                out[y][x] = [255 - v if v >= a[0] else v for v in img[y][x]]
    elif op == 12:
        for c in range(3):
            vals = [img[y][x][c] for y in range(H) for x in range(W)]
            lo, hi = min(vals), max(vals)
            if lo == hi:
                continue
            for y in range(H):
                for x in range(W):
                    out[y][x][c] = ((img[y][x][c] - lo) * 255 + (hi - lo) // 2) // (hi - lo)
    elif op == 13:
        for c in range(3):
            h = [0] * 256
            for y in range(H):
                for x in range(W):
                    h[img[y][x][c]] += 1
            last = [v for v in h if v][-1]
            step = (n - last) // 255
            if step == 0:
                continue
            lut, acc = [], 0
            for i in range(256):
                lut.append(min(255, (acc + step // 2) // step))
                acc += h[i]
            assert lut[0] == 0
            for y in range(H):
                for x in range(W):
                    out[y][x][c] = lut[img[y][x][c]]
    return out


def loop_randaug(u8, params, fill):
    B, H, W, _ = u8.shape
    res = []
    for b in range(B):
        img = u8[b].tolist()
        for r in params[b].tolist():
            img = loop_layer(img, H, W, r, fill)
        res.append(img)
    return torch.tensor(res, dtype=torch.uint8).view(B, H, W, 3)


def all_rows(m, H, W):
    """Every op, both signs where it has one."""
    rows = []
    for op in range(14):
        rows.append(row(op, m, False, H, W))
        if 1 <= op <= 9:
            rows.append(row(op, m, True, H, W))
    return rows


@pytest.mark.parametrize("H,W", [(7, 9), (3, 3), (1, 5), (2, 8)])
def test_torch_backend_equals_the_pixel_loop(H, W):
    g = torch.Generator().manual_seed(H * 31 + W)
    for m in (9, 30):
        rows = all_rows(m, H, W)
        B = len(rows)
        u8 = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        u8[:, 0, 0, 0] = 255  # (Solarize's >= at the top of the range)
        params = torch.tensor(rows, dtype=torch.int32).view(B, 1, 8)
        got = RA.randaug_torch(u8, params, 128)
        want = loop_randaug(u8, params, 128)
        for b in range(B):
            assert torch.equal(got[b], want[b]), (m, RA.OP_NAMES[rows[b][0]], rows[b])
    # layers in order, each seeing the one before (statistics included): Equalize after Contrast after Rotate
    u8 = torch.randint(0, 256, (4, H, W, 3), generator=g, dtype=torch.uint8)
    params = torch.tensor([[row(5, 20, False, H, W), row(8, 20, True, H, W), row(13, 20, False, H, W)],
                           [row(13, 9, False, H, W), row(12, 9, False, H, W), row(8, 9, False, H, W)],
                           [row(9, 30, False, H, W), row(1, 30, True, H, W), row(12, 0, False, H, W)],
                           [row(3, 30, False, H, W), row(4, 30, True, H, W), row(7, 30, True, H, W)]], dtype=torch.int32)
    assert torch.equal(RA.randaug_torch(u8, params, 7), loop_randaug(u8, params, 7))


# ------------------------------------------------------------------ geometric properties that need no oracle
def test_quarter_turn_is_rot90():
    g = torch.Generator().manual_seed(1)
    for n in (1, 2, 5, 8):
        u8 = torch.randint(0, 256, (2, n, n, 3), generator=g, dtype=torch.uint8)
        quarter = [5] + RA.affine_args(0.0, -1.0, 0.0, 1.0, 0.0, 0.0)  # cos 90 = 0, sin 90 = 1
        got = RA.randaug_torch(u8, torch.tensor([[quarter]] * 2, dtype=torch.int32), 99)
        assert torch.equal(got, torch.rot90(u8, 1, (1, 2))), n  # counter-clockwise as displayed


def test_translate_is_a_shift_with_a_fill_border():
    g = torch.Generator().manual_seed(2)
    H, W = 6, 11
    u8 = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)
    for t in (0, 1, 4, -3, 11, -20):
        want = torch.full_like(u8, 55)
        if abs(t) < W:  # the content moves by +t
            want[:, :, max(t, 0):W + min(t, 0)] = u8[:, :, max(-t, 0):W - max(t, 0)]
        got = RA.randaug_torch(u8, P([3] + RA.affine_args(1, 0, -2 * t, 0, 1, 0)), 55)
        assert torch.equal(got, want), t
    for t in (0, 2, -5, 6):
        want = torch.full_like(u8, 55)
        if abs(t) < H:
            want[:, max(t, 0):H + min(t, 0)] = u8[:, max(-t, 0):H - max(t, 0)]
        got = RA.randaug_torch(u8, P([4] + RA.affine_args(1, 0, 0, 0, 1, -2 * t)), 55)
        assert torch.equal(got, want), t
    # the table's translation at m = 30 in a 224-wide image: round(150 / 331 * 224) = 102 pixels
    assert RA.op_args(3, 30, False, 64, 224)[2] == -2 * 102 * 65536


def test_magnitude_zero_and_identity_matrix_change_nothing():
    g = torch.Generator().manual_seed(4)
    for H, W in ((5, 7), (4, 4), (1, 3)):
        u8 = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)
        for op in range(1, 10):
            for neg in (False, True):
                assert torch.equal(RA.randaug_torch(u8, P(row(op, 0, neg, H, W)), 0), u8), (op, neg)
            if op <= 5:
                assert torch.equal(RA.randaug_torch(u8, P([op] + RA.affine_args(1, 0, 0, 0, 1, 0)), 0), u8)
        assert torch.equal(RA.randaug_torch(u8, P([0]), 0), u8)
        assert torch.equal(RA.randaug_torch(u8, P([10, 0xFF]), 0), u8)  # Posterize at 8 bits
        assert torch.equal(RA.randaug_torch(u8, P([77, 1, 2, 3]), 0), u8)  # an op id outside the table


def test_solarize_at_magnitude_zero_inverts_255():
    """Threshold 255 with >=: a pixel of 255 becomes 0, as in PIL and torchvision."""
    u8 = torch.tensor([[[[255, 254, 0]]]], dtype=torch.uint8)
    assert RA.randaug_torch(u8, P(row(11, 0, False, 1, 1)), 0).flatten().tolist() == [0, 254, 0]


# ------------------------------------------------------------------ degenerate inputs of the statistics ops
def test_constant_images_and_channels():
    const = torch.full((1, 6, 5, 3), 93, dtype=torch.uint8)
    g = torch.Generator().manual_seed(6)
    one = torch.randint(0, 256, (1, 20, 20, 3), generator=g, dtype=torch.uint8)
    one[..., 1] = 200  # one constant channel
    for op in (12, 13):
        assert torch.equal(RA.randaug_torch(const, P([op]), 0), const)  # lo == hi, step == 0
        got = RA.randaug_torch(one, P([op]), 0)
        assert torch.equal(got[..., 1], one[..., 1])
        assert torch.equal(got, loop_randaug(one, P([op]), 0)) and not torch.equal(got, one)
    # fewer than 255 pixels besides the top bin: step == 0, Equalize leaves the image
    small = one[:, :6, :5].contiguous()
    assert torch.equal(RA.randaug_torch(small, P([13]), 0), small)


def test_two_valued_image_by_hand():
    # 20 x 30 = 600 pixels: 200 of value 50, 400 of value 150 (every channel)
    u8 = torch.full((1, 20, 30, 3), 150, dtype=torch.uint8)
    u8[:, :, :10] = 50
    # AutoContrast: lo 50, hi 150: 50 -> 0, 150 -> (100 * 255 + 50) / 100 = 255
    ac = RA.randaug_torch(u8, P([12]), 0)
    assert torch.equal(ac[:, :, :10], torch.zeros_like(ac[:, :, :10])) and bool((ac[:, :, 10:] == 255).all())
    # Equalize: last = 400, step = (600 - 400) / 255 = 0: unchanged
    assert torch.equal(RA.randaug_torch(u8, P([13]), 0), u8)
    # with 400 of 50 and 200 of 150: step = 400 / 255 = 1; lut[50] = 0 / 1 = 0, lut[150] = min(255, 400) = 255
    v8 = torch.full((1, 20, 30, 3), 50, dtype=torch.uint8)
    v8[:, :, :10] = 150
    eq = RA.randaug_torch(v8, P([13]), 0)
    assert bool((eq[:, :, :10] == 255).all()) and bool((eq[:, :, 10:] == 0).all())
    # Contrast: gray = (256 v + 128) >> 8 = v; mean = (200 * 50 + 400 * 150 + 300) / 600 = 70300 / 600 = 117
    assert (200 * 50 + 400 * 150 + 300) // 600 == 117
    ct = RA.randaug_torch(u8, P([8, 325]), 0)  # (325 v - 69 * 117 + 128) >> 8
    assert ct[0, 0, 0].tolist() == [(325 * 50 - 69 * 117 + 128) >> 8] * 3 == [32] * 3
    assert ct[0, 0, 29].tolist() == [(325 * 150 - 69 * 117 + 128) >> 8] * 3 == [159] * 3


def test_full_range_ramp_by_hand():
    # 256 x 255 image, every value 0 .. 255 in 255 pixels: n = 65280, last = 255, step = 255:
    # lut[i] = min(255, (255 i + 127) / 255) = i -- Equalize is the identity, and so is AutoContrast (lo 0, hi 255)
    ramp = torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1).expand(1, 256, 255, 3).contiguous()
    assert torch.equal(RA.randaug_torch(ramp, P([13]), 0), ramp)
    assert torch.equal(RA.randaug_torch(ramp, P([12]), 0), ramp)
    # half the range, 0 .. 127 in 510 pixels each: n = 65280, last = 510, step = 254:
    # lut[i] = (510 i + 127) / 254; AutoContrast: (255 i + 63) / 127
    half = (torch.arange(256) // 2).to(torch.uint8).view(1, 256, 1, 1).expand(1, 256, 255, 3).contiguous()
    eq = RA.randaug_torch(half, P([13]), 0)[0, :, 0, 0].tolist()
    assert eq == [min(255, (510 * (i // 2) + 127) // 254) for i in range(256)] and eq[255] == 255 and eq[2] == 2
    ac = RA.randaug_torch(half, P([12]), 0)[0, :, 0, 0].tolist()
    assert ac == [(255 * (i // 2) + 63) // 127 for i in range(256)] and ac[255] == 255 and ac[2] == 2


# ------------------------------------------------------------------ command line, trainer, transform
COMMON = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
          "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--quiet-banner", "--tb-dir", "",
          "--device", "cpu", "--kernels", "torch", "--launcher", "single"]


def test_cli_flags():
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    p = build_parser()
    a = p.parse_args(COMMON)
    assert a.randaugment is None and a.randaug_ops == 2 and a.randaug_fill == 128
    a = p.parse_args(COMMON + ["--randaugment", "9", "--randaug-ops", "3", "--randaug-fill", "0"])
    assert a.randaugment == 9 and a.randaug_ops == 3 and a.randaug_fill == 0
    for bad, flag in ((["--randaugment", "31"], "--randaugment"), (["--randaugment", "-1"], "--randaugment"),
                      (["--randaugment", "9", "--randaug-ops", "0"], "--randaug-ops"),
                      (["--randaugment", "9", "--randaug-ops", "5"], "--randaug-ops"),
                      (["--randaugment", "9", "--randaug-fill", "256"], "--randaug-fill"),
                      (["--randaugment", "9", "--hip-graph"], "--hip-graph")):
        with pytest.raises(SystemExit) as e:
            Trainer(p.parse_args(COMMON + bad))
        assert flag in str(e.value), (bad, e.value)


def test_trainer_builds_the_stage(tmp_path, monkeypatch, capsys):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    tr = Trainer(build_parser().parse_args(COMMON + ["--randaugment", "9", "--seed", "5"]))
    try:
        ra = tr.randaug
        assert ra is not None and (ra.backend, ra.num_ops, ra.magnitude, ra.fill, ra.seed, ra.rank) == \
            ("torch", 2, 9, 128, 5, 0)
        assert tr.transform_train.randaug is ra and tr.transform_val.randaug is None  # validation never augments
        assert "Augmentation: RandAugment 2 ops at magnitude 9" in capsys.readouterr().out
        tr._loaders(2)
        assert ra.epoch == 2
    finally:
        tr.close()
    tr = Trainer(build_parser().parse_args(COMMON))  # without the flag: no stage
    try:
        assert tr.randaug is None and tr.transform_train.randaug is None
    finally:
        tr.close()


def test_transform_without_the_stage_is_the_transform_as_before():
    from imagent_amd.data.loader import InputTransform
    g = torch.Generator().manual_seed(8)
    u8 = torch.randint(0, 256, (4, 16, 16, 3), generator=g, dtype=torch.uint8)
    plain = InputTransform("torch", (16, 16))
    assert plain.randaug is None
    ref = ((u8.permute(0, 3, 1, 2).float() / 255.0) - 0.5) / 0.5
    assert torch.equal(plain(u8), ref) and torch.equal(InputTransform("torch", (16, 16), randaug=None)(u8), ref)
    with pytest.raises(ValueError):
        plain(u8, ra_params=P([0]).expand(4, 1, 8))
    # with the stage: the same transform applied to randaug_torch(u8), on explicit draws and on the stage's own
    stage = RA.RandAugment("torch", 2, 9, fill=128, seed=3)
    t = InputTransform("torch", (16, 16), randaug=stage)
    params = RA.sample_params(4, 2, 9, 16, 16, torch.Generator().manual_seed(9), "cpu")
    assert torch.equal(t(u8, ra_params=params), plain(RA.randaug_torch(u8, params, 128)))
    own = RA.RandAugment("torch", 2, 9, fill=128, seed=3).draw(4, 16, 16, "cpu")
    assert torch.equal(t(u8), plain(RA.randaug_torch(u8, own, 128)))
    assert u8.dtype == torch.uint8 and t(u8).shape == (4, 3, 16, 16)


def test_short_cpu_run(tmp_path):
    """Started the way tests/test_engine_cpu.py starts its runs."""
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    args = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
            "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--log-interval", "1",
            "--quiet-banner", "--tb-dir", "", "--epochs", "1", "--device", "cpu", "--kernels", "torch",
            "--randaugment", "9", "--max-steps", "2"]
    r = subprocess.run([sys.executable, "-m", "imagent_amd.cli"] + args, cwd=tmp_path, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    out = r.stdout
    assert "Augmentation: RandAugment 2 ops at magnitude 9" in out and "Epoch 1 Summary: " in out
    tl, vl = re.search(r"Train loss: (\S+) ; Test loss: (\S+)", out).groups()
    assert math.isfinite(float(tl)) and float(tl) > 0 and math.isfinite(float(vl)), out[-2000:]
