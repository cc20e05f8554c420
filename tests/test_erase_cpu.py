"""Random Erasing without a GPU (--random-erase, data/erase.py): the box arithmetic against a per-sample loop in Python
floats, the choice of the first valid attempt, the Philox4x32-10 words against known answers and a plain-integer
implementation, the torch backend in both modes, the epoch seeding, the command line and two CPU trainer steps."""

import math
import random

import numpy as np
import pytest
import torch

M32 = 0xFFFFFFFF


# ------------------------------------------------------------------ boxes
def loop_boxes(u_apply, u, H, W, p, scale, ratio):
    """torchvision's rule (with timm's count), one sample at a time in Python floats."""
    B, N = len(u), len(u[0])
    out = np.zeros((B, N, 4), dtype=np.int64)
    for b in range(B):
        if not (u_apply[b] < p):
            continue
        for n in range(N):
            for a0, a1, a2, a3 in u[b][n]:
                area = H * W * (scale[0] + a0 * (scale[1] - scale[0])) / N
                ar = math.exp(math.log(ratio[0]) + a1 * (math.log(ratio[1]) - math.log(ratio[0])))
                h, w = round(math.sqrt(area * ar)), round(math.sqrt(area / ar))
                if not (h < H and w < W):
                    continue
                top = min(H - h, math.floor(a2 * (H - h + 1)))
                left = min(W - w, math.floor(a3 * (W - w + 1)))
                if h > 0 and w > 0:
                    out[b, n] = (top, left, h, w)
                break
    return out


@pytest.mark.parametrize("H,W,N,scale,ratio", [(224, 224, 1, (0.02, 0.33), (0.3, 3.3)),
                                               (33, 71, 4, (0.02, 0.33), (0.3, 3.3)),
                                               (16, 16, 2, (0.5, 1.0), (0.3, 3.3)),
                                               (5, 7, 3, (0.001, 0.05), (0.1, 10.0))])
def test_boxes_equal_python_loop(H, W, N, scale, ratio):
    from imagent_amd.data.erase import params_from_uniforms
    g = torch.Generator().manual_seed(H * 100 + W + N)
    B = 400
    u_apply = torch.rand(B, generator=g)
    u = torch.rand((B, N, 10, 4), generator=g)
    u[0, 0, :, 2:] = 0.0  # the corners
    u[1, 0, :, 2:] = 1.0 - 2.0 ** -24
    boxes = params_from_uniforms(u_apply, u, H, W, 0.7, scale, ratio)
    assert boxes.dtype == torch.int32 and boxes.shape == (B, N, 4)
    want = loop_boxes(u_apply.double().tolist(), u.double().tolist(), H, W, 0.7, scale, ratio)
    assert np.array_equal(boxes.numpy(), want)
    t, l, h, w = (boxes[..., i] for i in range(4))
    assert ((t >= 0) & (l >= 0) & (t + h <= H) & (l + w <= W)).all()
    assert (h > 0).any() and ((h == 0) == (w == 0)).all()


def _attempt(valid):
    # scale (0.9, 1.0), 32 x 32: ratio 3.3 (u1 = 1) gives h = round(sqrt(>= 921.6 x 3.3)) >= 55: invalid;
    # ratio sqrt(0.3 x 3.3) = 0.995 (u1 = 0.5) at share 0.9 (u0 = 0) gives h = w = 30: valid
    return [0.0, 0.5, 0.25, 0.75] if valid else [0.5, 1.0, 0.1, 0.1]


@pytest.mark.parametrize("k", range(10))
def test_first_valid_attempt_is_chosen(k):
    from imagent_amd.data.erase import params_from_uniforms
    H = W = 32
    scale, ratio = (0.9, 1.0), (0.3, 3.3)
    # attempts 0 .. k - 1 invalid, k valid, and every later one valid too but at another place
    rows = [_attempt(False)] * k + [_attempt(True)] + [[0.0, 0.5, 0.9, 0.9]] * (9 - k)
    u = torch.tensor(rows, dtype=torch.float64).view(1, 1, 10, 4)
    box = params_from_uniforms(torch.zeros(1), u, H, W, 1.0, scale, ratio)[0, 0].tolist()
    hw = round(math.sqrt(H * W * 0.9))
    assert hw < H and box == [math.floor(0.25 * (H - hw + 1)), math.floor(0.75 * (W - hw + 1)), hw, hw], box
    assert np.array_equal(loop_boxes([0.0], u.tolist(), H, W, 1.0, scale, ratio)[0, 0], box)


def test_no_valid_attempt_is_the_empty_box():
    from imagent_amd.data.erase import params_from_uniforms
    u = torch.tensor([_attempt(False)] * 10, dtype=torch.float64).view(1, 1, 10, 4)
    assert params_from_uniforms(torch.zeros(1), u, 32, 32, 1.0, (0.9, 1.0), (0.3, 3.3)).tolist() == [[[0, 0, 0, 0]]]
    # a box that rounds to no pixel is stored as the empty box too
    u = torch.tensor([[0.0, 0.0, 0.5, 0.5]] * 10, dtype=torch.float64).view(1, 1, 10, 4)
    assert params_from_uniforms(torch.zeros(1), u, 8, 8, 1.0, (0.001, 0.001), (0.05, 0.05)).tolist() == [[[0, 0, 0, 0]]]


def test_apply_probability():
    from imagent_amd.data.erase import erase_params
    g = torch.Generator().manual_seed(5)
    boxes, keys = erase_params(512, 224, 224, 0.0, generator=g)
    assert not boxes.any() and keys.dtype == torch.int32 and keys.shape == (512, 2)
    # p = 1: an attempt fails only when share x ratio >= 1, under 0.3 % of attempts; ten in a row never
    boxes, keys = erase_params(10000, 224, 224, 1.0, generator=g)
    assert (boxes[..., 2] > 0).all() and (boxes[..., 3] > 0).all()
    assert (keys < 0).any() and (keys > 0).any() and len(keys.unique()) > 19000  # the whole int32 range
    share = (boxes[:, 0, 2] * boxes[:, 0, 3]).double().mean().item() / 224 ** 2
    assert abs(share - 0.175) < 0.01, share  # the mean of uniform (0.02, 0.33), less what the rare misses shift
    boxes, _ = erase_params(4000, 224, 224, 0.25, count=3, generator=g)
    some = (boxes[..., 2] > 0).any(1)
    assert abs(some.double().mean().item() - 0.25) < 0.04
    assert ((boxes[..., 2] > 0).all(1) == some).all()  # all of a sample's boxes or none (at these small shares)


# ------------------------------------------------------------------ Philox4x32-10
def philox_int(counter, key):
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((M32,) * 4, (M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    from imagent_amd.data.erase import philox4x32_10
    for counter, key, want in KNOWN:
        assert tuple(philox_int(counter, key)) == want
        got = philox4x32_10(torch.tensor(counter, dtype=torch.int64), torch.tensor(key, dtype=torch.int64))
        assert tuple(got.tolist()) == want
    # int32 keys are read as uint32 words
    got = philox4x32_10(torch.full((4,), M32, dtype=torch.int64), torch.tensor([-1, -1], dtype=torch.int32))
    assert tuple(got.tolist()) == KNOWN[1][2]


def test_philox_random_pairs():
    from imagent_amd.data.erase import philox4x32_10
    rng = random.Random(11)
    cs = [[rng.getrandbits(32) for _ in range(4)] for _ in range(1000)]
    ks = [[rng.getrandbits(32) for _ in range(2)] for _ in range(1000)]
    got = philox4x32_10(torch.tensor(cs, dtype=torch.int64), torch.tensor(ks, dtype=torch.int64))
    assert got.tolist() == [philox_int(c, k) for c, k in zip(cs, ks)]


def test_noise_words_use_the_pixel_index_and_the_sample_key():
    from imagent_amd.data.erase import noise_words
    keys = torch.tensor([[5, -7], [2 ** 31 - 1, -2 ** 31]], dtype=torch.int32)
    w = noise_words(keys, 3, 5)
    assert w.shape == (2, 3, 5, 4)
    for b, y, x in ((0, 0, 0), (0, 2, 4), (1, 1, 3)):
        k = [int(v) & M32 for v in keys[b]]
        assert w[b, y, x].tolist() == philox_int([y * 5 + x, 0, 0, 0], k)


# ------------------------------------------------------------------ the torch backend
def _x(B, H, W, seed=0):
    return torch.randn((B, 3, H, W), generator=torch.Generator().manual_seed(seed))


def test_const_mode_is_exact():
    from imagent_amd.data.erase import erase_torch
    x = _x(3, 5, 7)
    boxes = torch.tensor([[[1, 2, 3, 4], [0, 0, 0, 0]], [[0, 0, 0, 0], [0, 0, 0, 0]], [[0, 0, 5, 7], [4, 6, 1, 1]]],
                         dtype=torch.int32)
    for dtype in (torch.float32, torch.bfloat16):
        xd = x.to(dtype)
        out = erase_torch(xd, boxes, None, "const", 0.3)
        want = xd.clone()
        want[0, :, 1:4, 2:6] = 0.3
        want[2] = 0.3
        assert out.dtype == dtype and torch.equal(out, want) and out.data_ptr() != xd.data_ptr()
        assert torch.equal(xd, x.to(dtype))  # the input is left as it was
    assert torch.equal(erase_torch(x, boxes, None)[0, :, 1:4, 2:6], torch.zeros(3, 3, 4))  # the default value 0


def test_pixel_mode_moments():
    """A whole 64 x 64 image x 4 samples, every channel: n = 49152 values; the mean within 5 / sqrt(n) of 0, the
    variance within 5 sqrt(2 / n) of 1 (five standard errors of each)."""
    from imagent_amd.data.erase import erase_torch
    B, H, W = 4, 64, 64
    x = torch.full((B, 3, H, W), 100.0)
    boxes = torch.tensor([[[0, 0, H, W]]] * B, dtype=torch.int32)
    keys = torch.tensor([[1, 2], [3, 4], [-5, 6], [7, -8]], dtype=torch.int32)
    out = erase_torch(x, boxes, keys, "pixel").double()
    n = out.numel()
    assert (out != 100.0).all() and out.abs().max() < 6.0
    assert abs(out.mean().item()) < 5 / math.sqrt(n)
    assert abs(out.var().item() - 1.0) < 5 * math.sqrt(2 / n)
    assert not torch.equal(out[0], out[1])  # another key, other values
    for c in range(3):  # and each channel alone is no constant copy of another
        assert abs(out[:, c].mean().item()) < 5 / math.sqrt(n / 3)
    assert abs(torch.corrcoef(torch.stack([out[:, 0].flatten(), out[:, 1].flatten()]))[0, 1].item()) < 0.04


def test_overlapping_boxes_in_either_order():
    from imagent_amd.data.erase import erase_torch
    x = _x(2, 9, 11, seed=3)
    keys = torch.tensor([[9, 9], [1, 0]], dtype=torch.int32)
    b = torch.tensor([[[1, 1, 5, 6], [3, 4, 5, 6]]] * 2, dtype=torch.int32)
    for mode in ("const", "pixel"):
        a = erase_torch(x, b, keys, mode, 1.5)
        assert torch.equal(a, erase_torch(x, b.flip(1), keys, mode, 1.5))
        # and equals the two boxes applied one after the other
        two = erase_torch(erase_torch(x, b[:, :1], keys, mode, 1.5), b[:, 1:], keys, mode, 1.5)
        assert torch.equal(a, two)
        assert torch.equal(a[:, :, 0], x[:, :, 0]) and torch.equal(a[:, :, :, 0], x[:, :, :, 0])


def test_set_epoch_repeats_the_draws():
    from imagent_amd.data.erase import BatchEraser
    from imagent_amd.data.mix import BatchMixer
    from imagent_amd.data.randaug import RandAugment

    def draws(seed, rank, epoch):
        e = BatchEraser("torch", 0.5, count=2, seed=seed, rank=rank)
        e.set_epoch(epoch)
        return e.draw(16, 32, 32, "cpu"), e.draw(16, 32, 32, "cpu")

    same = lambda a, b: all(torch.equal(p, q) for s, t in zip(a, b) for p, q in zip(s, t))  # noqa: E731
    assert same(draws(1, 0, 3), draws(1, 0, 3))
    assert not same(draws(1, 0, 3), draws(1, 0, 4)) and not same(draws(1, 0, 3), draws(1, 1, 3))
    assert not same(draws(1, 0, 3), draws(2, 0, 3))
    first, second = draws(1, 0, 3)
    assert not torch.equal(first[1], second[1])
    e = BatchEraser("torch", 0.5, seed=1)
    d0 = e.draw(8, 32, 32, "cpu")
    e.set_epoch(0)
    assert same([d0], [e.draw(8, 32, 32, "cpu")])  # a re-seed in the middle of an epoch starts it again
    # a stream of its own
    seeds = {BatchEraser("torch", 0.5, seed=3, rank=2)._epoch_seed(),
             BatchMixer("torch", 0.2, seed=3, rank=2)._epoch_seed(), RandAugment("torch", seed=3, rank=2)._epoch_seed()}
    assert len(seeds) == 3
    # the call draws what draw() draws, and explicit params pass through
    e1, e2 = BatchEraser("torch", 1.0, mode="pixel", seed=4), BatchEraser("torch", 1.0, mode="pixel", seed=4)
    x = _x(8, 32, 32)
    from imagent_amd.data.erase import erase_torch
    assert torch.equal(e1(x), erase_torch(x, *e2.draw(8, 32, 32, "cpu"), "pixel"))
    with pytest.raises(ValueError):
        BatchEraser("cuda", 0.5)
    for bad in (dict(p=1.5), dict(p=0.5, scale=(0.0, 0.3)), dict(p=0.5, scale=(0.5, 0.3)),
                dict(p=0.5, scale=(0.5, 1.3)), dict(p=0.5, ratio=(0.0, 1.0)), dict(p=0.5, ratio=(2.0, 1.0)),
                dict(p=0.5, count=0), dict(p=0.5, count=5), dict(p=0.5, mode="noise"),
                dict(p=0.5, value=float("nan"))):
        with pytest.raises(ValueError):
            BatchEraser("torch", **bad)


# ------------------------------------------------------------------ command line, trainer
COMMON = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
          "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--quiet-banner", "--tb-dir", "",
          "--device", "cpu", "--kernels", "torch", "--launcher", "single"]


def test_cli_flags():
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    p = build_parser()
    a = p.parse_args(COMMON)
    assert a.random_erase == 0.0 and list(a.erase_scale) == [0.02, 0.33] and list(a.erase_ratio) == [0.3, 3.3]
    assert a.erase_count == 1 and a.erase_mode == "const" and a.erase_value == 0.0
    a = p.parse_args(COMMON + ["--random-erase", "0.1", "--erase-scale", "0.1", "0.2", "--erase-ratio", "0.5", "2",
                               "--erase-count", "3", "--erase-mode", "pixel", "--erase-value", "-1.5"])
    assert a.random_erase == 0.1 and list(a.erase_scale) == [0.1, 0.2] and list(a.erase_ratio) == [0.5, 2.0]
    assert a.erase_count == 3 and a.erase_mode == "pixel" and a.erase_value == -1.5
    with pytest.raises(SystemExit):
        p.parse_args(COMMON + ["--erase-mode", "noise"])
    for bad, flag in ((["--random-erase", "-0.1"], "--random-erase"), (["--random-erase", "1.5"], "--random-erase"),
                      (["--random-erase", "0.5", "--erase-scale", "0", "0.3"], "--erase-scale"),
                      (["--random-erase", "0.5", "--erase-scale", "0.4", "0.3"], "--erase-scale"),
                      (["--random-erase", "0.5", "--erase-scale", "0.4", "1.3"], "--erase-scale"),
                      (["--random-erase", "0.5", "--erase-ratio", "0", "3"], "--erase-ratio"),
                      (["--random-erase", "0.5", "--erase-ratio", "3", "2"], "--erase-ratio"),
                      (["--random-erase", "0.5", "--erase-count", "0"], "--erase-count"),
                      (["--random-erase", "0.5", "--erase-count", "5"], "--erase-count"),
                      (["--random-erase", "0.5", "--erase-value", "nan"], "--erase-value"),
                      (["--random-erase", "0.5", "--hip-graph"], "--hip-graph")):
        with pytest.raises(SystemExit) as e:
            Trainer(p.parse_args(COMMON + bad))
        assert flag in str(e.value), (bad, e.value)
    with pytest.raises(SystemExit) as e:
        Trainer(p.parse_args(COMMON + ["--random-erase", "0.5", "--hip-graph"]))
    assert "the per-batch draws are not fed into a captured step" in str(e.value)  # the mix flags' sentence


def test_trainer_two_steps(tmp_path, monkeypatch, capsys):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    args = COMMON + ["--random-erase", "1", "--erase-mode", "pixel", "--mixup", "0.2", "--max-steps", "2", "--seed",
                     "5", "--log-interval", "0"]
    tr = Trainer(build_parser().parse_args(args))
    try:
        e = tr.eraser
        assert e is not None and e.backend == "torch"
        assert (e.p, e.count, e.mode, e.seed, e.rank) == (1.0, 1, "pixel", 5, 0)
        assert "Augmentation: Random Erasing with probability 1, 1 box of scale (0.02, 0.33)" in capsys.readouterr().out
        order, erase, mix = [], type(e).__call__, type(tr.mixer).__call__
        monkeypatch.setattr(type(e), "__call__",
                            lambda s, x, params=None: (order.append("erase"), erase(s, x, params))[1])
        monkeypatch.setattr(type(tr.mixer), "__call__",
                            lambda s, x, y, params=None: (order.append("mix"), mix(s, x, y, params))[1])
        train, val = tr._loaders(2)
        assert e.epoch == 2
        loss, _, _, _ = tr.train_epoch(0, train)
        assert math.isfinite(loss) and loss > 0, loss
        assert order == ["erase", "mix"] * 2 and tr.last_train_images == 16
        vloss, _, _, _ = tr.validate(val)  # validation never erases
        assert math.isfinite(vloss) and len(order) == 4
    finally:
        tr.close()
    tr = Trainer(build_parser().parse_args(COMMON))  # without the flag: no stage
    try:
        assert tr.eraser is None
    finally:
        tr.close()
