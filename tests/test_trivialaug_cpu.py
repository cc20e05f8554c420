"""TrivialAugmentWide without a GPU (--trivialaugment, data/trivialaug.py): the device table against the Python argument
function, hand-worked arguments at the ends of the wide ranges, the draws' coverage and epoch seeding, the command
line, and ``randaug_torch`` on the stage's rows."""

import math

import pytest
import torch

from imagent_amd.data import randaug as RA
from imagent_amd.data import trivialaug as TA

AFFINE = (RA.SHEAR_X, RA.SHEAR_Y, RA.TRANSLATE_X, RA.TRANSLATE_Y, RA.ROTATE)
COLOUR = (RA.BRIGHTNESS, RA.COLOR, RA.CONTRAST, RA.SHARPNESS)


@pytest.mark.parametrize("H,W", [(224, 224), (33, 71), (448, 300)])
def test_table_equals_the_argument_function(H, W):
    t = TA._table(H, W, "cpu")
    assert t.shape == (31, 14, 2, 7) and t.dtype == torch.int32
    for b in range(31):
        for op in range(14):
            for neg in (0, 1):
                assert t[b, op, neg].tolist() == TA.ta_op_args(op, b, bool(neg), H, W), (b, op, neg)
    # and the draws index it: uniforms at each cell's centre give that cell's row
    op = torch.arange(14).view(1, 14, 1).expand(31, 14, 2)
    b = torch.arange(31).view(31, 1, 1).expand(31, 14, 2)
    neg = torch.arange(2).view(1, 1, 2).expand(31, 14, 2)
    p = TA.params_from_uniforms((op + 0.5) / 14, (b + 0.5) / 31, 0.75 - 0.5 * neg, H, W)
    assert p.shape == (31, 14, 2, 8) and p.dtype == torch.int32
    assert torch.equal(p[..., 0], op.to(torch.int32)) and torch.equal(p[..., 1:], t)


def test_hand_worked_arguments():
    one = RA.ONE
    ident = [one, 0, 0, 0, one, 0, 0]
    for op in AFFINE:  # bin 0 of every affine op is the identity matrix, with either sign
        for neg in (False, True):
            assert TA.ta_op_args(op, 0, neg, 224, 300) == ident, op
    for op in COLOUR:
        assert TA.ta_op_args(op, 0, False, 8, 8)[0] == 256
        assert TA.ta_op_args(op, 30, False, 8, 8)[0] == 509 and TA.ta_op_args(op, 30, True, 8, 8)[0] == 3
        assert TA.ta_op_args(op, 15, False, 8, 8)[0] == 383 and TA.ta_op_args(op, 15, True, 8, 8)[0] == 129
    assert TA.ta_op_args(RA.SHEAR_X, 30, False, 8, 8) == [one, 64881, 0, 0, one, 0, 0]
    assert TA.ta_op_args(RA.SHEAR_Y, 30, True, 8, 8) == [one, 0, 0, -64881, one, 0, 0]
    # 32 pixels of a 224-pixel image, scaled to the stored size
    assert TA.ta_op_args(RA.TRANSLATE_X, 30, False, 100, 224)[2] == -2 * 32 * one
    assert TA.ta_op_args(RA.TRANSLATE_X, 30, True, 100, 448)[2] == 2 * 64 * one
    assert TA.ta_op_args(RA.TRANSLATE_Y, 15, False, 448, 100) == [one, 0, 0, 0, one, -2 * 32 * one, 0]
    assert TA.ta_op_args(RA.TRANSLATE_Y, 1, False, 224, 100)[5] == -2 * 1 * one  # round(32 / 30) = 1
    c = round(one * math.cos(math.radians(135.0)))
    s = round(one * math.sin(math.radians(135.0)))
    assert TA.ta_op_args(RA.ROTATE, 30, False, 8, 8) == [c, -s, 0, s, c, 0, 0] and c < 0 < s
    assert TA.ta_op_args(RA.ROTATE, 30, True, 8, 8) == [c, s, 0, -s, c, 0, 0]
    # Posterize: bits 8 .. 2
    bits = [8 - round(b / 5) for b in range(31)]
    assert bits[0] == 8 and bits[2] == 8 and bits[3] == 7 and bits[30] == 2 and sorted(set(bits)) == list(range(2, 9))
    for b in range(31):
        assert TA.ta_op_args(RA.POSTERIZE, b, False, 8, 8)[0] == (0xFF << (8 - bits[b])) & 0xFF
    assert [TA.ta_op_args(RA.POSTERIZE, b, False, 8, 8)[0] for b in (0, 5, 10, 15, 20, 25, 30)] == \
        [0xFF, 0xFE, 0xFC, 0xF8, 0xF0, 0xE0, 0xC0]
    assert [TA.ta_op_args(RA.SOLARIZE, b, False, 8, 8)[0] for b in (0, 1, 15, 30)] == [255, 247, 128, 0]
    for op in (RA.IDENTITY, RA.AUTOCONTRAST, RA.EQUALIZE):
        assert TA.ta_op_args(op, 17, True, 8, 8) == [0] * 7
    for bad in (-1, 31, 2.5):
        with pytest.raises(ValueError):
            TA.ta_op_args(RA.ROTATE, bad, False, 8, 8)
    with pytest.raises(ValueError):
        TA.ta_op_args(14, 3, False, 8, 8)


def _bins_of(params, H, W):
    """Per drawn row the bins whose table entry (either sign) it equals; -1 for an op without a magnitude."""
    t = TA._table(H, W, "cpu")
    out = []
    for row in params.view(-1, 8).tolist():
        op = row[0]
        if op in (RA.IDENTITY, RA.AUTOCONTRAST, RA.EQUALIZE):
            out.append(-1)
            continue
        hit = [b for b in range(31) if row[1:] in (t[b, op, 0].tolist(), t[b, op, 1].tolist())]
        out.append(hit)
    return out


def test_draws_cover_the_ops_and_the_bins():
    g = torch.Generator().manual_seed(3)
    H = W = 448
    u = torch.rand((10000, 1, 3), generator=g)
    p = TA.params_from_uniforms(u[..., 0], u[..., 1], u[..., 2], H, W)
    assert p.shape == (10000, 1, 8)
    ops = p[:, 0, 0]
    counts = torch.bincount(ops.long(), minlength=14)
    assert (counts > 10000 / 14 * 0.8).all() and ops.min() == 0 and ops.max() == 13
    b = torch.floor(u[..., 1].double() * 31).long().view(-1)
    assert torch.bincount(b, minlength=31).min() > 10000 / 31 * 0.7 and b.min() == 0 and b.max() == 30
    # the rows are those of the drawn bins: rotations tell all 31 bins apart (both signs at bin 0 are the identity)
    rot = (ops == RA.ROTATE).nonzero().view(-1)
    seen = set()
    for i in rot.tolist():
        hit = _bins_of(p[i], H, W)[0]
        assert hit == [int(b[i])]
        seen.add(hit[0])
    assert seen == set(range(31))
    # both signs occur
    sh = p[ops == RA.SHEAR_X][:, 0, 2]
    assert (sh > 0).any() and (sh < 0).any()
    # sample_params: one rand launch of [B, 1, 3]
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    u = torch.rand((64, 1, 3), generator=g2)
    assert torch.equal(TA.sample_params(64, 33, 71, g1),
                       TA.params_from_uniforms(u[..., 0], u[..., 1], u[..., 2], 33, 71))
    # the ends of the uniforms stay inside the table
    ends = torch.tensor([0.0, 1.0 - 2.0 ** -24, 1.0])
    p = TA.params_from_uniforms(ends, ends, ends, 8, 8)
    assert p[:, 0].tolist() == [0, 13, 13]


def test_draws_repeat_per_epoch():
    from imagent_amd.data.erase import BatchEraser
    from imagent_amd.data.mix import BatchMixer

    def draws(seed, rank, epoch):
        s = TA.TrivialAugmentWide("torch", seed=seed, rank=rank)
        s.set_epoch(epoch)
        return s.draw(32, 40, 40, "cpu"), s.draw(32, 40, 40, "cpu")

    a, b = draws(1, 0, 3), draws(1, 0, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], a[1])
    for other in (draws(1, 0, 4), draws(1, 1, 3), draws(2, 0, 3)):
        assert not torch.equal(a[0], other[0])
    seeds = {TA.TrivialAugmentWide("torch", seed=3, rank=2)._epoch_seed(),
             RA.RandAugment("torch", seed=3, rank=2)._epoch_seed(),
             BatchMixer("torch", 0.2, seed=3, rank=2)._epoch_seed(),
             BatchEraser("torch", 0.5, seed=3, rank=2)._epoch_seed()}
    assert len(seeds) == 4
    s = TA.TrivialAugmentWide("torch", fill=7)
    assert s.num_ops == 1 and s.fill == 7
    for bad in (dict(backend="cuda"), dict(backend="torch", fill=256), dict(backend="torch", fill=-1)):
        with pytest.raises(ValueError):
            TA.TrivialAugmentWide(**bad)


def test_identity_and_bin_0_leave_the_image_unchanged():
    g = torch.Generator().manual_seed(1)
    H, W = 21, 35
    # (no pixel of 255: Solarize at bin 0 flips it)
    u8 = torch.randint(0, 255, (14 * 2 + 5, H, W, 3), dtype=torch.uint8, generator=g)
    rows = [[op] + TA.ta_op_args(op, 0, neg, H, W) for op in range(14) for neg in (False, True)]
    rows += [[RA.IDENTITY] + TA.ta_op_args(RA.IDENTITY, b, False, H, W) for b in (1, 7, 15, 29, 30)]
    params = torch.tensor(rows, dtype=torch.int32).view(-1, 1, 8)
    out = RA.randaug_torch(u8, params, 128)
    for i, row in enumerate(rows):
        if row[0] in (RA.AUTOCONTRAST, RA.EQUALIZE):  # (no magnitude: they change a random image at any bin)
            assert not torch.equal(out[i], u8[i])
        else:
            assert torch.equal(out[i], u8[i]), RA.OP_NAMES[row[0]]
    # the stage object on explicit and on its own draws
    st = TA.TrivialAugmentWide("torch", seed=2)
    assert torch.equal(st(u8, params), out)
    st.set_epoch(1)
    d = st.draw(u8.shape[0], H, W, "cpu")
    st.set_epoch(1)
    assert torch.equal(st(u8), RA.randaug_torch(u8, d, 128))
    # the wide ends do what they say: a 135-degree rotation brings the fill into the corners, Brightness at F = 3
    # leaves almost nothing, Posterize at bin 30 keeps two bits
    wide = torch.tensor([[RA.ROTATE] + TA.ta_op_args(RA.ROTATE, 30, False, H, W),
                         [RA.BRIGHTNESS] + TA.ta_op_args(RA.BRIGHTNESS, 30, True, H, W),
                         [RA.POSTERIZE] + TA.ta_op_args(RA.POSTERIZE, 30, False, H, W)],
                        dtype=torch.int32).view(3, 1, 8)
    o = RA.randaug_torch(u8[:3], wide, 77)
    assert (o[0, 0, 0] == 77).all() and (o[0, -1, -1] == 77).all()
    assert torch.equal(o[0, H // 2, W // 2], u8[0, H // 2, W // 2])
    assert o[1].max() <= 3 and torch.equal(o[2], u8[2] & 0xC0)


COMMON = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
          "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--quiet-banner", "--tb-dir", "",
          "--device", "cpu", "--kernels", "torch", "--launcher", "single"]


def test_cli_flag_and_trainer(tmp_path, monkeypatch, capsys):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    p = build_parser()
    assert p.parse_args(COMMON).trivialaugment is False
    for bad, word in ((["--trivialaugment", "--randaugment", "9"], "--randaugment"),
                      (["--trivialaugment", "--hip-graph"], "--hip-graph"),
                      (["--trivialaugment", "--randaug-fill", "300"], "--randaug-fill")):
        with pytest.raises(SystemExit) as e:
            Trainer(p.parse_args(COMMON + bad))
        assert word in str(e.value), (bad, e.value)
    args = COMMON + ["--trivialaugment", "--randaug-fill", "0", "--random-resized-crop", "--flip", "--random-erase",
                     "0.1", "--mixup", "0.2", "--cutmix", "1.0", "--label-smoothing", "0.1", "--model-ema", "0.999",
                     "--seed", "4", "--max-steps", "2", "--log-interval", "0"]
    tr = Trainer(p.parse_args(args))  # the torchvision reference recipe as one command line
    try:
        assert isinstance(tr.randaug, TA.TrivialAugmentWide) and tr.transform_train.randaug is tr.randaug
        assert tr.transform_val.randaug is None
        assert (tr.randaug.backend, tr.randaug.fill, tr.randaug.seed) == ("torch", 0, 4)
        assert "Augmentation: TrivialAugmentWide" in capsys.readouterr().out
        train, _ = tr._loaders(3)
        assert tr.randaug.epoch == 3
        loss, _, _, _ = tr.train_epoch(0, train)
        assert math.isfinite(loss) and loss > 0 and tr.last_train_images == 16
    finally:
        tr.close()
