"""Mixup / CutMix without a GPU (--mixup / --cutmix, data/mix.py): the box and adjusted-lam arithmetic against a
per-sample loop of the published rule in Python floats, the Beta draws' moments, the kinds, the epoch seeding, the
torch backend of ``BatchMixer`` against the definition, the two-label loss of the torch path, the command line and one
end-to-end CPU run."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ boxes and adjusted lam
def loop_params(mixed, cut, u_pos, lam, H, W):
    """The published CutMix rule, one sample at a time in Python floats -> (lam float32, boxes)."""
    lams, boxes = [], []
    for m, c, (uy, ux), l in zip(mixed, cut, u_pos, lam):
        if not m:
            lams.append(1.0), boxes.append((0, 0, 0, 0))
            continue
        if not c:
            lams.append(l), boxes.append((0, 0, 0, 0))
            continue
        r = math.sqrt(1.0 - l)
        ch, cw = int(H * r), int(W * r)
        cy, cx = min(int(uy * H), H - 1), min(int(ux * W), W - 1)
        y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
        x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
        if y1 - y0 <= 0 or x1 - x0 <= 0:
            lams.append(1.0), boxes.append((0, 0, 0, 0))
        else:
            lams.append(1.0 - (y1 - y0) * (x1 - x0) / (H * W)), boxes.append((y0, x0, y1 - y0, x1 - x0))
    return np.asarray(lams, dtype=np.float64).astype(np.float32), np.asarray(boxes, dtype=np.int32)


def _check_against_loop(mixed, cut, u_pos, lam, H, W):
    from imagent_amd.data.mix import params_from_uniforms
    n = len(lam)
    pair = torch.arange(n).flip(0)
    p, l, b = params_from_uniforms(torch.tensor(mixed), torch.tensor(cut), torch.tensor(u_pos, dtype=torch.float64),
                                   torch.tensor(lam, dtype=torch.float64), pair, H, W)
    assert p.dtype == torch.int32 and l.dtype == torch.float32 and b.dtype == torch.int32
    assert torch.equal(p, pair.to(torch.int32)) and b.shape == (n, 4)
    rl, rb = loop_params(mixed, cut, u_pos, lam, H, W)
    assert np.array_equal(b.numpy(), rb), (b.numpy(), rb)
    assert np.array_equal(l.numpy(), rl), (l.numpy(), rl)
    return l.numpy(), b.numpy()


def test_boxes_equal_python_loop_edge_cases():
    H, W = 8, 10
    #        mixed  cut    (uy, ux)       lam
    cases = [(True, True, (0.0, 0.5), 0.5),      # clipped at the top
             (True, True, (0.99, 0.5), 0.5),     # at the bottom
             (True, True, (0.5, 0.0), 0.5),      # at the left
             (True, True, (0.5, 0.99), 0.5),     # at the right
             (True, True, (0.0, 0.0), 0.3),      # a corner: two edges
             (True, True, (0.99, 0.99), 0.3),
             (True, True, (0.5, 0.5), 0.75),     # interior, unclipped
             (True, True, (0.5, 0.5), 1.0),      # lam 1: r = 0, nothing to paste -> the empty box
             (True, True, (0.5, 0.5), 0.0),      # lam 0: the whole image
             (True, True, (0.3, 0.7), 0.995),    # int(H r) = 0: the empty box, lam back to 1
             (True, False, (0.5, 0.5), 0.25),    # Mixup keeps lam, empty box
             (False, False, (0.5, 0.5), 0.25),   # not mixed
             (False, True, (0.5, 0.5), 0.25)]
    mixed, cut, u_pos, lam = (list(c) for c in zip(*cases))
    cut = [c and m for c, m in zip(cut, mixed)]
    l, b = _check_against_loop(mixed, cut, u_pos, lam, H, W)
    assert b[0].tolist() == [0, 2, 2, 6] and b[1][0] + b[1][2] == H and b[2][1] == 0 and b[3][1] + b[3][3] == W
    assert b[7].tolist() == [0, 0, 0, 0] and l[7] == 1.0
    assert b[8].tolist() == [0, 0, H, W] and l[8] == 0.0
    assert b[9].tolist() == [0, 0, 0, 0] and l[9] == 1.0
    assert b[10].tolist() == [0, 0, 0, 0] and l[10] == np.float32(0.25)
    assert l[11] == 1.0 and l[12] == 1.0 and not b[11:].any()


@pytest.mark.parametrize("H,W", [(7, 5), (32, 32), (224, 224), (37, 64)])
def test_boxes_equal_python_loop_random(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W)
    n = 500
    mixed = (torch.rand(n, generator=g) < 0.8).tolist()
    cut = [(c and m) for c, m in zip((torch.rand(n, generator=g) < 0.6).tolist(), mixed)]
    u_pos = torch.rand((n, 2), generator=g, dtype=torch.float32).double().tolist()
    lam = torch.rand(n, generator=g, dtype=torch.float64).tolist()
    l, b = _check_against_loop(mixed, cut, u_pos, lam, H, W)
    assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 0] + b[:, 2] <= H).all() \
        and (b[:, 1] + b[:, 3] <= W).all()
    assert ((l >= 0) & (l <= 1)).all()


# ------------------------------------------------------------------ the draws
def test_beta_draws_have_the_right_moments():
    """Beta(0.2, 0.2): mean 0.5, variance 1 / (4 (2 alpha + 1)) = 0.17857; float64 gammas, no NaN."""
    from imagent_amd.data.mix import beta_draws, mix_params
    g = torch.Generator().manual_seed(1234)
    n, alpha = 100_000, 0.2
    lam = beta_draws(torch.full((n,), alpha, dtype=torch.float64), g)
    assert lam.dtype == torch.float64 and not torch.isnan(lam).any()
    assert ((lam >= 0) & (lam <= 1)).all()
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    print(f"Beta({alpha}, {alpha}) x {n}: mean {lam.mean().item():.5f}, variance {lam.var().item():.5f} (exact {var:.5f})")
    assert abs(lam.mean().item() - 0.5) < 0.01
    assert abs(lam.var().item() - var) < 0.05 * var
    # both gammas 0 -> 0.5, never NaN (an alpha small enough that float64 underflows too)
    tiny = beta_draws(torch.full((1000,), 1e-4, dtype=torch.float64), g)
    assert not torch.isnan(tiny).any() and ((tiny >= 0) & (tiny <= 1)).all()
    # through mix_params (all Mixup): the same distribution in the returned float32 lam
    _, l32, boxes = mix_params(n, 32, 32, alpha, 0.0, generator=torch.Generator().manual_seed(5))
    assert l32.dtype == torch.float32 and not torch.isnan(l32).any() and not boxes.any()
    assert abs(l32.double().mean().item() - 0.5) < 0.01 and abs(l32.double().var().item() - var) < 0.05 * var


def test_mix_params_kinds():
    from imagent_amd.data.mix import mix_params
    B, H, W = 4000, 24, 40

    def draw(mu, cm, prob=1.0, sw=0.5, seed=0):
        return mix_params(B, H, W, mu, cm, prob, sw, torch.Generator().manual_seed(seed), "cpu")

    pair, lam, boxes = draw(0.2, 1.0, prob=0.0)            # prob 0: nothing is mixed
    assert (lam == 1).all() and not boxes.any()
    assert pair.dtype == torch.int32 and sorted(pair.tolist()) == list(range(B))  # a permutation of the batch
    pair, lam, boxes = draw(0.4, 0.0)                      # Mixup only: never a box
    assert not boxes.any() and (lam < 1).float().mean() > 0.9
    pair, lam, boxes = draw(0.0, 1.0)                      # CutMix only: a box, or lam 1 with the empty one
    has = (boxes[:, 2] > 0) & (boxes[:, 3] > 0)
    assert has.float().mean() > 0.9 and (lam[~has] == 1).all() and not boxes[~has].any()
    area = (boxes[:, 2] * boxes[:, 3]).double()
    assert torch.equal(lam[has], (1.0 - area[has] / (H * W)).float())
    pair, lam, boxes = draw(0.4, 1.0, sw=0.5)              # both: about half of each kind
    has = (boxes[:, 2] > 0) & (boxes[:, 3] > 0)
    assert 0.4 < has.float().mean() < 0.55
    pair, lam, boxes = draw(0.4, 1.0, prob=0.5, sw=1.0)    # half mixed, all of those CutMix
    has = (boxes[:, 2] > 0) & (boxes[:, 3] > 0)
    assert 0.4 < has.float().mean() < 0.55 and (lam[~has] == 1).all()
    pair, lam, boxes = draw(0.0, 0.0)                      # both off
    assert (lam == 1).all() and not boxes.any()
    for bad in ((-0.1, 0.0, 1.0, 0.5), (0.0, -1.0, 1.0, 0.5), (0.2, 0.2, 1.5, 0.5), (0.2, 0.2, 1.0, -0.1)):
        with pytest.raises(ValueError):
            mix_params(4, 8, 8, *bad)


def test_set_epoch_repeats_the_draws():
    from imagent_amd.data.mix import BatchMixer

    def draws(seed, rank, epoch, again=None):
        m = again or BatchMixer("torch", 0.2, 1.0, seed=seed, rank=rank)
        m.set_epoch(epoch)
        return m, [m.draw(16, 32, 32, "cpu") for _ in range(2)]

    def same(a, b):
        return all(torch.equal(s, t) for p, q in zip(a, b) for s, t in zip(p, q))

    m, d0 = draws(3, 0, 0)
    _, d0b = draws(3, 0, 0, again=m)   # set_epoch on the live generator
    _, d0c = draws(3, 0, 0)            # and a fresh mixer: a resumed run
    assert same(d0, d0b) and same(d0, d0c)
    assert not same(d0[:1], d0[1:])    # successive batches differ
    assert not same(d0, draws(3, 0, 1)[1]) and not same(d0, draws(3, 1, 0)[1]) and not same(d0, draws(4, 0, 0)[1])
    # other constants than the input transform's generator
    from imagent_amd.data.loader import InputTransform
    t = InputTransform("torch", (32, 32), seed=3, rank=0)
    assert t._epoch_seed() != m._epoch_seed()


# ------------------------------------------------------------------ the torch backend
def test_torch_backend_matches_definition():
    from imagent_amd.data.mix import BatchMixer
    g = torch.Generator().manual_seed(0)
    x = torch.randn((3, 3, 5, 7), generator=g)
    y = torch.tensor([4, 9, 2])
    pair = torch.tensor([2, 1, 0], dtype=torch.int32)           # sample 1 is its own partner
    lam = torch.tensor([0.3, 0.5, 0.6], dtype=torch.float32)
    boxes = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0], [1, 3, 2, 3]], dtype=torch.int32)
    out, (ya, yb, l) = BatchMixer("torch", 0.2, 1.0)(x, y, params=(pair, lam, boxes))
    assert torch.equal(ya, y) and torch.equal(yb, y[pair.long()]) and torch.equal(l, lam)
    ref = x.clone()
    ref[0] = lam[0] * x[0] + (1 - lam[0]) * x[2]
    ref[1] = lam[1] * x[1] + (1 - lam[1]) * x[1]
    ref[2, :, 1:3, 3:6] = x[0, :, 1:3, 3:6]
    assert out.shape == x.shape and out.dtype == x.dtype
    assert torch.allclose(out[:2], ref[:2], rtol=0, atol=1e-6)
    assert torch.equal(out[2], ref[2])                           # a select: exact
    # lam 1 / lam 0 with the empty box: the sample / its partner
    out, _ = BatchMixer("torch", 0.2, 0.0)(x, y, params=(pair, torch.tensor([1.0, 1.0, 0.0]), torch.zeros_like(boxes)))
    assert torch.equal(out[0], x[0]) and torch.equal(out[1], x[1]) and torch.equal(out[2], x[0])
    # own draws: shapes, dtypes, a permutation
    out, (ya, yb, l) = BatchMixer("torch", 0.2, 1.0, seed=1)(x, y)
    assert out.shape == x.shape and l.shape == (3,) and l.dtype == torch.float32 and sorted(yb.tolist()) == [2, 4, 9]


# ------------------------------------------------------------------ the two-label loss of the torch path
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_step_runner_pair_loss(smoothing):
    from imagent_amd.train.engine import StepRunner
    from imagent_amd.train.meters import DeviceMetrics
    g = torch.Generator().manual_seed(2)
    B, NC = 16, 10
    z = torch.randn((B, NC), generator=g) * 2
    ya = torch.randint(0, NC, (B,), generator=g)
    yb = torch.randint(0, NC, (B,), generator=g)
    ya[:3] = z[:3].argmax(1)
    yb[3:6] = z[3:6].argmax(1)
    lam = torch.rand(B, generator=g)
    lam[0], lam[1], lam[3], lam[4] = 1.0, 0.7, 0.0, 0.2
    met = DeviceMetrics("cpu")
    run = StepRunner(None, None, met, "torch", smoothing)
    loss = run.loss(z, (ya, yb, lam))
    ref = (lam * F.cross_entropy(z, ya, reduction="none", label_smoothing=smoothing) +
           (1 - lam) * F.cross_entropy(z, yb, reduction="none", label_smoothing=smoothing)).mean()
    assert abs(loss.item() - ref.item()) < 1e-5
    dom = torch.where(lam >= 0.5, ya, yb)
    top5 = z.topk(5, 1).indices
    assert met.buf[1].item() == (top5[:, 0] == dom).sum().item() >= 5
    assert met.buf[2].item() == (top5 == dom[:, None]).any(1).sum().item()
    assert met.buf[3].item() == B and abs(met.buf[0].item() - ref.item() * B) < 1e-4
    # a plain label tensor still takes the one-label path
    one = run.loss(z, ya)
    assert abs(one.item() - F.cross_entropy(z, ya, label_smoothing=smoothing).item()) < 1e-6


# ------------------------------------------------------------------ command line, trainer
COMMON = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
          "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--quiet-banner", "--tb-dir", "",
          "--device", "cpu", "--kernels", "torch", "--launcher", "single"]


def test_cli_flags():
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    p = build_parser()
    a = p.parse_args(COMMON)
    assert a.mixup == 0.0 and a.cutmix == 0.0 and a.mix_prob == 1.0 and a.mix_switch_prob == 0.5
    a = p.parse_args(COMMON + ["--mixup", "0.2", "--cutmix", "1.0", "--mix-prob", "0.8", "--mix-switch-prob", "0.3"])
    assert a.mixup == 0.2 and a.cutmix == 1.0 and a.mix_prob == 0.8 and a.mix_switch_prob == 0.3
    for bad, flag in ((["--mixup", "-0.1"], "--mixup"), (["--cutmix", "-1"], "--cutmix"),
                      (["--mixup", "0.2", "--mix-prob", "1.5"], "--mix-prob"),
                      (["--mixup", "0.2", "--mix-prob", "-0.5"], "--mix-prob"),
                      (["--cutmix", "1", "--mix-switch-prob", "2"], "--mix-switch-prob"),
                      (["--mixup", "0.2", "--hip-graph"], "--hip-graph"),
                      (["--cutmix", "1.0", "--hip-graph"], "--hip-graph")):
        with pytest.raises(SystemExit) as e:
            Trainer(p.parse_args(COMMON + bad))
        assert flag in str(e.value), (bad, e.value)


def test_trainer_builds_the_mixer(tmp_path, monkeypatch, capsys):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        monkeypatch.delenv(k, raising=False)
    tr = Trainer(build_parser().parse_args(COMMON + ["--mixup", "0.2", "--cutmix", "1.0", "--seed", "5"]))
    try:
        m = tr.mixer
        assert m is not None and m.backend == "torch" and (m.mixup_alpha, m.cutmix_alpha) == (0.2, 1.0)
        assert (m.prob, m.switch_prob, m.seed, m.rank) == (1.0, 0.5, 5, 0)
        assert "Augmentation: Mixup alpha 0.2 / CutMix alpha 1" in capsys.readouterr().out
        tr._loaders(2)
        assert m.epoch == 2
    finally:
        tr.close()
    tr = Trainer(build_parser().parse_args(COMMON))   # without the flags: no mixer
    try:
        assert tr.mixer is None
    finally:
        tr.close()


def test_one_epoch_cpu_run(tmp_path):
    """Started the way tests/test_engine_cpu.py starts its runs."""
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    args = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
            "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--log-interval", "3",
            "--quiet-banner", "--tb-dir", "", "--epochs", "1", "--kernels", "torch", "--mixup", "0.2", "--cutmix", "1.0",
            "--label-smoothing", "0.1", "--max-steps", "3"]
    r = subprocess.run([sys.executable, "-m", "imagent_amd.cli"] + args, cwd=tmp_path, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    out = r.stdout
    assert "Augmentation: Mixup alpha 0.2 / CutMix alpha 1" in out and "Epoch 1 Summary: " in out
    import re
    tl, vl = re.search(r"Train loss: (\S+) ; Test loss: (\S+)", out).groups()
    assert math.isfinite(float(tl)) and float(tl) > 0 and math.isfinite(float(vl)), out[-2000:]
