"""--model-ema on the CPU: the flat-op path of train/ema.py against a per-tensor reference, the warm-up
schedule, the bucket re-layout, the checkpoint round trip, the in-place swap, and the command line."""

import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Tiny(nn.Module):
    """One 4-D conv weight (channels-last in the arena), one 1-D and one 2-D parameter; BatchNorm buffers."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(5, 7, 3, bias=False)
        self.bn = nn.BatchNorm2d(7, affine=False)
        self.scale = nn.Parameter(torch.randn(7))
        self.fc = nn.Linear(11, 3, bias=False)


def _tiny(seed=0, order=(2, 0, 1)):
    from imagent_amd.models.arena import ParamArena
    torch.manual_seed(seed)
    m = Tiny()
    with torch.no_grad():
        m.bn.running_mean.normal_()
        m.bn.running_var.uniform_(0.5, 2.0)
    return m, ParamArena(list(m.named_parameters()), "cpu", order=list(order))


def _drift_buffers(m, g):
    with torch.no_grad():
        m.bn.running_mean.add_(torch.randn(7, generator=g))
        m.bn.running_var.mul_(torch.rand(7, generator=g) + 0.5)
        m.bn.num_batches_tracked.add_(1)


def test_fixed_decay_matches_per_tensor_lerp():
    from imagent_amd.train.ema import ModelEma
    from imagent_amd.train.optim import FlatSGD
    d = 0.9
    m, ar = _tiny()
    opt = FlatSGD(ar, lr=0.1, momentum=0.9, weight_decay=1e-4, native=False)
    opt.ema = ema = ModelEma(ar, m, d)
    assert len(ar.params) == 3 and sorted(len(s) for s in ar.shapes) == [1, 2, 4]
    ref = {n: p.detach().clone() for n, p in m.named_parameters()}
    bref = {"bn.running_mean": m.bn.running_mean.clone(), "bn.running_var": m.bn.running_var.clone()}
    assert ema.buf_names == list(bref)  # float buffers only: num_batches_tracked is not averaged
    g = torch.Generator().manual_seed(1)
    for step in range(5):
        ar.G.copy_(torch.randn(ar.total, generator=g))
        _drift_buffers(m, g)
        opt.step()
        for n, p in m.named_parameters():
            ref[n].lerp_(p.detach(), 1 - d)
        for n, b in m.named_buffers():
            if n in bref:
                bref[n].lerp_(b, 1 - d)
        assert ema.updates == step + 1
    for i, n in enumerate(ar.names):
        assert torch.equal(ar.view(ema.E, i), ref[n]), n
        assert not torch.equal(ar.view(ema.E, i), ar.view(ar.P, i)), n
    for i, n in enumerate(ema.buf_names):
        assert torch.equal(ema._buf_slice(i), bref[n]), n


def test_one_update_per_step_for_every_optimizer_kind():
    """FlatLARS and the torch.optim family update the average after their own step, with the same math."""
    from imagent_amd.train.ema import ModelEma
    from imagent_amd.train.optim import build_optimizer
    for name in ("lars", "adam"):
        m, ar = _tiny(seed=3)
        opt = build_optimizer(name, ar, lr=0.01)
        opt.native = False
        opt.ema = ema = ModelEma(ar, m, 0.75)
        before = ar.P.clone()
        ar.G.copy_(torch.randn(ar.total, generator=torch.Generator().manual_seed(4)))
        opt.step()
        assert ema.updates == 1 and not torch.equal(ar.P, before)
        assert torch.equal(ema.E, before.clone().lerp_(ar.P, 0.25)), name


def test_warmup_schedule():
    from imagent_amd.train.ema import ModelEma
    m, ar = _tiny()
    ema = ModelEma(ar, m, 0.3, warmup=True)
    want = [1 / 10, 2 / 11, 3 / 12, 4 / 13]
    got = []
    for t in range(4):
        assert ema.updates == t
        got.append(ema.decay_at(t))
        # the kernel argument: 1 - d_t formed in double precision and rounded once to fp32
        assert ema.omd() == torch.tensor(1.0 - min(0.3, want[t]), dtype=torch.float64).to(torch.float32).item()
        ema.update()
    assert got == [0.1, 2 / 11, 0.25, 0.3]  # (1 + t) / (10 + t) until it passes DECAY = 0.3 at t = 3
    assert want[3] > 0.3 > want[2]
    assert all(ema.decay_at(t) == 0.3 for t in range(3, 50))
    big = ModelEma(ar, m, 0.9999, warmup=True)
    assert [big.decay_at(t) for t in range(4)] == want
    assert big.decay_at(10 ** 6) == 0.9999
    fixed = ModelEma(ar, m, 0.9999)
    assert fixed.decay_at(0) == 0.9999 and fixed.omd() == torch.tensor(1 - 0.9999, dtype=torch.float64).float().item()


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_decay_out_of_range(bad):
    from imagent_amd.train.ema import ModelEma
    m, ar = _tiny()
    with pytest.raises(ValueError):
        ModelEma(ar, m, bad)


def test_relayout_keeps_every_tensor_under_its_name():
    from imagent_amd.train.ema import ModelEma
    m, ar = _tiny(order=(0, 1, 2))
    ema = ModelEma(ar, m, 0.5)
    ema.E.copy_(torch.randn(ar.total, generator=torch.Generator().manual_seed(2)))
    before = {n: ar.view(ema.E, i).clone() for i, n in enumerate(ar.names)}
    old_offsets = list(ar.offsets)
    ema.set_flats(ar.relayout([2, 1, 0], ema.flats()))
    assert ar.offsets != old_offsets and ema.E.numel() == ar.total
    for i, n in enumerate(ar.names):
        assert torch.equal(ar.view(ema.E, i), before[n]), n


def test_checkpoint_round_trip(tmp_path):
    from imagent_amd.train.ema import ModelEma
    m, ar = _tiny()
    ema = ModelEma(ar, m, 0.9, warmup=True)
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        ar.P.add_(torch.randn(ar.total, generator=g))
        _drift_buffers(m, g)
        ema.update()
    torch.save({"extra": {"ema": ema.state_dict()}}, tmp_path / "s.pt")
    sd = torch.load(tmp_path / "s.pt", map_location="cpu", weights_only=True)["extra"]["ema"]
    assert set(sd["params"]) == set(ar.names) and set(sd["buffers"]) == {"bn.running_mean", "bn.running_var"}
    m2, ar2 = _tiny(seed=9, order=(1, 2, 0))  # another layout: the state is keyed by name
    ema2 = ModelEma(ar2, m2, 0.9, warmup=True)
    ema2.load_state_dict(sd)
    assert ema2.updates == 3 and ema2.omd() == ema.omd()
    for i, n in enumerate(ar.names):
        assert torch.equal(ar2.view(ema2.E, ar2.names.index(n)), ar.view(ema.E, i)), n
    assert torch.equal(ema2.B, ema.B)


def test_swap_twice_restores():
    from imagent_amd.train.ema import ModelEma
    m, ar = _tiny()
    calls = []
    ema = ModelEma(ar, m, 0.9, refresh=lambda: calls.append(1))
    g = torch.Generator().manual_seed(6)
    ar.P.add_(torch.randn(ar.total, generator=g))
    _drift_buffers(m, g)
    ema.update()
    P0, E0, B0 = ar.P.clone(), ema.E.clone(), ema.B.clone()
    bufs0 = [b.clone() for b in m.buffers()]
    ptrs = [b.data_ptr() for b in m.buffers()] + [ar.P.data_ptr()]
    ema.swap()
    assert torch.equal(ar.P, E0) and torch.equal(ema.E, P0) and not torch.equal(P0, E0)
    assert torch.equal(m.bn.running_mean, B0[:7]) and torch.equal(m.bn.running_var, B0[7:])
    assert torch.equal(ema.B, torch.cat([bufs0[0], bufs0[1]]))
    assert torch.equal(m.conv.weight, ar.view(E0, ar.names.index("conv.weight")))  # the model's parameters are views of P: they follow
    assert m.bn.num_batches_tracked.item() == bufs0[2].item()
    ema.swap()
    assert torch.equal(ar.P, P0) and torch.equal(ema.E, E0) and torch.equal(ema.B, B0)
    for b, b0 in zip(m.buffers(), bufs0):
        assert torch.equal(b, b0)
    assert ptrs == [b.data_ptr() for b in m.buffers()] + [ar.P.data_ptr()]  # in place: no pointer moved
    assert len(calls) == 2


# ------------------------------------------------------------------ command line (CPU, --kernels torch)
COMMON = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
          "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--log-interval", "3",
          "--quiet-banner"]


def _cli(args, cwd, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, "-m", "imagent_amd.cli"] + COMMON + ["--kernels", "torch", "--device",
                                                                                "cpu"] + args,
                          cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                          timeout=timeout)


def test_cli_two_epochs_save_and_resume(tmp_path):
    r = _cli(["--model-ema", "0.9", "--epochs", "2", "--tb-dir", str(tmp_path / "tb"), "--checkpoint-dir",
              str(tmp_path), "--save-model"], tmp_path)
    assert r.returncode == 0, r.stdout[-4000:]
    out = r.stdout
    assert out.count("\tEMA Test loss: ") == 2 and out.count(" ; EMA Test top1 accuracy: ") == 2
    assert out.count(" ; EMA Test top5 accuracy: ") == 2
    assert out.count("\tTrain top1 accuracy: ") == 2  # the raw lines as before
    assert "\t Best EMA Test top1 accuracy: " in out
    assert os.path.isdir(tmp_path / "tb" / "Loss_val_ema") and os.path.isdir(tmp_path / "tb" / "Top1 accuracy_val_ema")
    sd = torch.load(tmp_path / "imagenet_FR_resnet18_ema.pt", map_location="cpu", weights_only=True)
    assert len(sd) == 122 and all(k.startswith("module.") for k in sd)
    raw = torch.load(tmp_path / "imagenet_FR_resnet18.pt", map_location="cpu", weights_only=True)
    assert list(raw) == list(sd)
    assert not torch.equal(raw["module.conv1.weight"], sd["module.conv1.weight"])
    from imagent_amd.models import resnet
    from imagent_amd.utils.checkpoint import load_reference_weights
    load_reference_weights(resnet.build("resnet18", num_classes=10), str(tmp_path / "imagenet_FR_resnet18_ema.pt"))
    st = torch.load(tmp_path / "state_resnet18.pt", map_location="cpu", weights_only=True)
    assert st["extra"]["ema"]["updates"] == 12  # 2 epochs x 48 / 8 steps
    assert "ema_top1" in st["best"] and "ema_epoch_top1" in st["best"]
    # the state holds the RAW weights (the average was swapped out again before it was written)
    assert not torch.equal(st["model"]["conv1.weight"], st["extra"]["ema"]["params"]["conv1.weight"]
                           .view(64, 7, 7, 3).permute(0, 3, 1, 2))

    r2 = _cli(["--model-ema", "0.9", "--epochs", "3", "--tb-dir", "", "--checkpoint-dir", str(tmp_path), "--resume",
               str(tmp_path / "state_resnet18.pt")], tmp_path)
    assert r2.returncode == 0, r2.stdout[-4000:]
    assert "Model EMA: resumed the average after 12 updates" in r2.stdout
    assert "Epoch 3 Summary: " in r2.stdout and r2.stdout.count("\tEMA Test loss: ") == 1
    st2 = torch.load(tmp_path / "state_resnet18.pt", map_location="cpu", weights_only=True)
    assert st2["extra"]["ema"]["updates"] == 18


def test_cli_resume_without_an_average_starts_from_the_weights(tmp_path):
    r = _cli(["--epochs", "1", "--tb-dir", "", "--checkpoint-dir", str(tmp_path)], tmp_path)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "EMA" not in r.stdout  # flag off: no new output
    r2 = _cli(["--model-ema", "0.5", "--model-ema-warmup", "--epochs", "2", "--tb-dir", "", "--resume",
               str(tmp_path / "state_resnet18.pt")], tmp_path)
    assert r2.returncode == 0, r2.stdout[-4000:]
    assert "holds no average; it starts from the loaded weights" in r2.stdout
    assert r2.stdout.count("\tEMA Test loss: ") == 1


@pytest.mark.parametrize("flags,needle", [
    (["--model-ema", "1.0"], "--model-ema"),
    (["--model-ema", "-0.1"], "--model-ema"),
    (["--model-ema", "0.9", "--model-ema-warmup", "--hip-graph"], "--model-ema-warmup"),
    (["--model-ema-warmup"], "--model-ema-warmup"),
])
def test_cli_refuses(tmp_path, flags, needle):
    r = _cli(flags + ["--epochs", "1", "--tb-dir", ""], tmp_path, timeout=120)
    assert r.returncode != 0
    assert needle in r.stdout and "Epoch 1 Summary" not in r.stdout and "Initialize" not in r.stdout, r.stdout[-2000:]
