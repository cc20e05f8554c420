"""FlatAdam / FlatLAMB on the CPU (train/optim.py, the ``native=False`` flat-op path): against torch.optim.Adam /
AdamW and a per-parameter float64 LAMB reference, the bucket re-layout, the name-keyed checkpoint, a stock
``"kind": "torch"`` Adam checkpoint, the EMA hook, and the command line."""

import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(seed=0):
    torch.manual_seed(seed)
    a = nn.Parameter(torch.randn(5, 3, 3, 3).contiguous(memory_format=torch.channels_last))
    b = nn.Parameter(torch.randn(7))
    return [("w", a), ("b", b)]


def _net(seed=0):
    """One 4-D, one 2-D and three 1-D parameters (conv weight and bias, BatchNorm affine, a bias-free linear)."""
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Flatten(), nn.Linear(8, 5, bias=False))


def _arena(net, order=None):
    from imagent_amd.models.arena import ParamArena
    return ParamArena(list(net.named_parameters()), torch.device("cpu"), order=order)


def _by_name(ar, flat):
    return {n: ar.view(flat, i).clone() for i, n in enumerate(ar.names)}


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_flat_adam_matches_torch(decoupled):
    from imagent_amd.models.arena import ParamArena
    from imagent_amd.train.optim import FlatAdam
    named = _params()
    ref = [nn.Parameter(p.detach().clone()) for _, p in named]
    ar = ParamArena(named, "cpu", order=[1, 0])
    opt = FlatAdam(ar, 0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled=decoupled)
    assert not opt.native and opt.flats() == []
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    ropt = cls(ref, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    worst = 0.0
    for step in range(5):
        grads = [torch.randn_like(r) for r in ref]
        opt.zero_grad()
        for (_, p), g in zip(named, grads):
            p.grad.add_(g)  # the gradients live in the arena
        for r, g in zip(ref, grads):
            r.grad = g.clone()
        opt.step()
        ropt.step()
        assert opt.steps == step + 1
    for (_, p), r in zip(named, ref):
        worst = max(worst, (p.detach() - r.detach()).abs().max().item())
        torch.testing.assert_close(p.detach(), r.detach(), rtol=1e-5, atol=1e-7)
    print(f"decoupled={decoupled}: worst |p - torch| = {worst:.3g}")
    assert len(opt.flats()) == 2 and all(t.shape == ar.P.shape for t in opt.flats())
    # padding: still zero in the parameters and both moments
    pad = torch.ones(ar.total, dtype=torch.bool)
    for i in range(len(ar.params)):
        pad[ar.offsets[i]:ar.offsets[i] + ar.numels[i]] = False
    assert pad.any() and all((t[pad] == 0).all() for t in (ar.P, opt.m, opt.v))


def test_grad_scale_is_the_gradient_scaled():
    from imagent_amd.train.optim import FlatAdam, FlatLAMB
    for cls in (FlatAdam, FlatLAMB):
        a, b = _arena(_net()), _arena(_net())
        oa, ob = cls(a, 0.01, native=False), cls(b, 0.01, native=False)
        oa.grad_scale = 0.25  # a power of two: scaling commutes with every rounding
        for s in range(3):
            g = torch.randn(a.total, generator=torch.Generator().manual_seed(s))
            for i in range(len(a.params)):  # (the padding of G stays zero)
                a.flat_slice(a.G, i).copy_(a.flat_slice(g, i))
                b.flat_slice(b.G, i).copy_(a.flat_slice(g, i) * 0.25)
            oa.step()
            ob.step()
        assert torch.equal(a.P, b.P), cls.__name__


def _lamb_reference(ws, ms, vs, grads, t, lr, b1, b2, eps, wd, mgn, gs=1.0):
    """One LAMB step per parameter in float64 (apex FusedLAMB / timm Lamb with the no-decay filter)."""
    gn = gs * math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    c = mgn / gn if (mgn > 0 and gn > mgn) else 1.0
    trusts = []
    for w, m, v, g in zip(ws, ms, vs, grads):
        gg = g.double() * gs * c
        m.mul_(b1).add_(gg, alpha=1 - b1)
        v.mul_(b2).add_(gg * gg, alpha=1 - b2)
        r = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
        trust = 1.0
        if w.dim() > 1:
            r = r + wd * w
            wn, rn = w.norm().item(), r.norm().item()
            if wn > 0 and rn > 0:
                trust = wn / rn
        trusts.append(trust)
        w.sub_(r, alpha=lr * trust)
    return c, trusts


@pytest.mark.parametrize("mgn,gscale", [(1.0, 1.0), (1.0, 1e-3), (0.0, 1.0)], ids=["clipped", "not-clipped", "clip-off"])
def test_flat_lamb_matches_reference(mgn, gscale):
    from imagent_amd.train.optim import FlatLAMB
    net = _net()
    ar = _arena(net, order=[2, 0, 4, 1, 3])
    with torch.no_grad():
        net[1].weight.zero_()  # a zero tensor (1-D): stays finite
    lr, b1, b2, eps, wd = 0.02, 0.9, 0.99, 1e-6, 1e-2
    opt = FlatLAMB(ar, lr, betas=(b1, b2), eps=eps, weight_decay=wd, max_grad_norm=mgn)
    assert not opt.native
    ws = [p.detach().double().clone() for p in net.parameters()]
    ms, vs = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
    clipped = []
    for t in range(1, 5):
        grads = [torch.randn_like(p) * gscale for p in net.parameters()]
        for p, g in zip(net.parameters(), grads):
            p.grad.copy_(g)
        opt.step()
        c, trusts = _lamb_reference(ws, ms, vs, grads, t, lr, b1, b2, eps, wd, mgn)
        clipped.append(c < 1.0)
        for p, tr in zip(net.parameters(), trusts):
            assert p.dim() > 1 or tr == 1.0
        assert any(tr != 1.0 for tr in trusts)
    assert all(clipped) if (mgn > 0 and gscale == 1.0) else not any(clipped)
    for p, w in zip(net.parameters(), ws):
        assert torch.isfinite(p).all()
        torch.testing.assert_close(p.detach().double(), w, rtol=1e-5, atol=1e-7)
    # 1-D tensors are not decayed: with a zero gradient history they would not move at all
    net2 = _net(1)
    ar2 = _arena(net2)
    o2 = FlatLAMB(ar2, lr, weight_decay=0.5, max_grad_norm=mgn)
    before = {n: p.detach().clone() for n, p in net2.named_parameters()}
    o2.step()  # G == 0
    for n, p in net2.named_parameters():
        assert torch.equal(p.detach(), before[n]) == (p.dim() == 1), n


@pytest.mark.parametrize("kind", ["adam", "adamw", "lamb"])
def test_relayout_mid_run_gives_the_same_result_by_name(kind):
    from imagent_amd.train.optim import build_optimizer
    na, nb = _net(), _net()
    a, b = _arena(na, order=[0, 1, 2, 3, 4]), _arena(nb, order=[4, 2, 0, 3, 1])
    oa, ob = build_optimizer(kind, a, 0.01, weight_decay=1e-2), build_optimizer(kind, b, 0.01, weight_decay=1e-2)
    assert type(oa).__name__ == ("FlatLAMB" if kind == "lamb" else "FlatAdam")
    gen = torch.Generator().manual_seed(3)
    for step in range(4):
        if step == 2:
            old = list(a.offsets)
            oa.set_flats(a.relayout([3, 1, 4, 0, 2], oa.flats()))
            assert a.offsets != old and oa.m.numel() == a.total
        for pa, pb in zip(na.parameters(), nb.parameters()):
            g = torch.randn(pa.shape, generator=gen)
            pa.grad.copy_(g)
            pb.grad.copy_(g)
        oa.step()
        ob.step()
    for flat_a, flat_b in ((a.P, b.P), (oa.m, ob.m), (oa.v, ob.v)):
        x, y = _by_name(a, flat_a), _by_name(b, flat_b)
        for n in a.names:
            if kind == "lamb":  # the clip factor's global norm sums the arena in its own order
                torch.testing.assert_close(x[n], y[n], rtol=1e-6, atol=1e-8)
            else:
                assert torch.equal(x[n], y[n]), n


@pytest.mark.parametrize("kind", ["adam", "adamw", "lamb"])
def test_state_round_trips_by_name_and_continues_bit_identically(kind, tmp_path):
    from imagent_amd.train.optim import build_optimizer
    na, nb = _net(), _net(5)
    a, b = _arena(na), _arena(nb, order=[4, 2, 0, 3, 1])
    oa = build_optimizer(kind, a, 0.01, weight_decay=1e-2, betas=(0.8, 0.95), opt_eps=1e-5)
    gen = torch.Generator().manual_seed(4)
    for _ in range(3):
        for p in na.parameters():
            p.grad.copy_(torch.randn(p.shape, generator=gen))
        oa.step()
    torch.save({"optimizer": oa.state_dict()}, tmp_path / "s.pt")
    sd = torch.load(tmp_path / "s.pt", map_location="cpu", weights_only=True)["optimizer"]
    assert sd["kind"] == ("lamb" if kind == "lamb" else "adam") and sd["steps"] == 3
    assert set(sd["m"]) == set(a.names) == set(sd["v"])
    # b: another layout; c: the layout of a. Other hyper-parameters in both: the file's hold
    nc = _net(6)
    c = _arena(nc)
    ob, oc = build_optimizer(kind, b, 0.5), build_optimizer(kind, c, 0.5)
    for net, o in ((nb, ob), (nc, oc)):
        o.load_state_dict(sd)
        with torch.no_grad():
            for pa, pb in zip(na.parameters(), net.parameters()):
                pb.copy_(pa)
        assert o.steps == 3 and o.param_groups[0]["betas"] == (0.8, 0.95) and o.param_groups[0]["eps"] == 1e-5
        assert o.param_groups[0]["lr"] == 0.01
    assert torch.equal(oc.m, oa.m) and torch.equal(oc.v, oa.v)
    for pa, pb, pc in zip(na.parameters(), nb.parameters(), nc.parameters()):
        g = torch.randn(pa.shape, generator=gen)
        for p in (pa, pb, pc):
            p.grad.copy_(g)
    for o in (oa, ob, oc):
        o.step()
    assert torch.equal(c.P, a.P) and torch.equal(oc.m, oa.m) and torch.equal(oc.v, oa.v)
    x, y = _by_name(a, a.P), _by_name(b, b.P)
    for n in a.names:
        if kind == "lamb":  # the clip factor's global norm sums the arena in its own order
            torch.testing.assert_close(x[n], y[n], rtol=1e-6, atol=1e-8)
        else:
            assert torch.equal(x[n], y[n]), n
    # a state saved before the first step holds no moments
    fresh = build_optimizer(kind, _arena(_net()), 0.1)
    oc.load_state_dict(fresh.state_dict())
    assert oc.m is None and oc.steps == 0 and oc.flats() == []


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_stock_torch_adam_checkpoint_loads(decoupled, tmp_path):
    """A --resume file of the stock route (TorchOptimizer over the arena views: ``"kind": "torch"``, torch's
    index-keyed state) loads into FlatAdam; the next step matches stock Adam's next step."""
    from imagent_amd.models.arena import ParamArena
    from imagent_amd.train.optim import FlatAdam, TorchOptimizer
    named = _params()
    ar = ParamArena(named, "cpu", order=[1, 0])
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    stock = TorchOptimizer(ar, cls(ar.params, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2))
    gen = torch.Generator().manual_seed(7)
    for _ in range(3):
        ar.G.zero_()
        for _, p in named:
            p.grad.add_(torch.randn(p.shape, generator=gen))
        stock.step()
    torch.save({"optimizer": stock.state_dict()}, tmp_path / "s.pt")
    sd = torch.load(tmp_path / "s.pt", map_location="cpu", weights_only=True)["optimizer"]
    assert sd["kind"] == "torch"
    named2 = _params(1)
    ar2 = ParamArena(named2, "cpu", order=[0, 1])
    with torch.no_grad():
        for (_, p), (_, q) in zip(named, named2):
            q.copy_(p)
    flat = FlatAdam(ar2, 0.5, betas=(0.5, 0.5), eps=1.0, weight_decay=0.0, decoupled=decoupled)
    flat.load_state_dict(sd)
    assert flat.steps == 3 and flat.param_groups[0]["lr"] == 0.01 and flat.param_groups[0]["betas"] == (0.9, 0.999)
    assert torch.equal(ar2.view(flat.m, 0), stock.opt.state[ar.params[0]]["exp_avg"])
    for (_, p), (_, q) in zip(named, named2):
        g = torch.randn(p.shape, generator=gen)
        p.grad.copy_(g)
        q.grad.copy_(g)
    before = ar2.P.clone()
    stock.step()
    flat.step()
    assert flat.steps == 4 and not torch.equal(before, ar2.P)
    for (_, p), (_, q) in zip(named, named2):
        torch.testing.assert_close(q.detach(), p.detach(), rtol=1e-5, atol=1e-7)


def test_ema_is_updated_once_per_step():
    from imagent_amd.train.ema import ModelEma
    from imagent_amd.train.optim import build_optimizer
    for name in ("lamb", "adam", "adamw"):
        net = _net(3)
        ar = _arena(net)
        calls = []
        opt = build_optimizer(name, ar, lr=0.01, after_step=lambda: calls.append(1))
        opt.ema = ema = ModelEma(ar, net, 0.75)
        for s in range(2):
            before, e0 = ar.P.clone(), ema.E.clone()
            for p in net.parameters():
                p.grad.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(4 + s)))
            opt.step()
            assert ema.updates == s + 1 and len(calls) == s + 1 and not torch.equal(ar.P, before), name
            assert torch.equal(ema.E, e0.lerp_(ar.P, 0.25)), name


def test_build_optimizer_routes_and_defaults():
    from imagent_amd.train.optim import FlatAdam, FlatLAMB, TorchOptimizer, build_optimizer
    ar = _arena(_net())
    o = build_optimizer("adam", ar, 0.1)
    assert type(o) is FlatAdam and not o.param_groups[0]["decoupled"] and o.param_groups[0]["eps"] == 1e-8
    o = build_optimizer("adamw", ar, 0.1)
    assert type(o) is FlatAdam and o.param_groups[0]["decoupled"] and o.param_groups[0]["betas"] == (0.9, 0.999)
    o = build_optimizer("lamb", ar, 0.1)
    assert type(o) is FlatLAMB and o.param_groups[0]["eps"] == 1e-6 and o.param_groups[0]["max_grad_norm"] == 1.0
    assert o.launches() == 3
    o = build_optimizer("lamb", ar, 0.1, lamb_max_grad_norm=0.0, betas=(0.9, 0.99), opt_eps=1e-4)
    assert o.launches() == 2 and o.param_groups[0]["betas"] == (0.9, 0.99) and o.param_groups[0]["eps"] == 1e-4
    assert type(build_optimizer("nadam", ar, 0.1)) is TorchOptimizer
    for bad in (dict(betas=(1.0, 0.9)), dict(opt_eps=0.0), dict(lamb_max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            build_optimizer("lamb", ar, 0.1, **bad)


# ------------------------------------------------------------------ command line (CPU, --kernels torch)
COMMON = ["--arch", "resnet18", "--image-size", "32", "--data", "synthetic", "--synthetic-train-size", "48",
          "--synthetic-val-size", "16", "--batch-size", "8", "--num-classes", "10", "--log-interval", "3",
          "--quiet-banner", "--kernels", "torch", "--device", "cpu"]


def test_cli_parses_the_flags():
    from imagent_amd.cli import build_parser
    p = build_parser()
    a = p.parse_args(COMMON + ["--optimizer", "lamb", "--betas", "0.9", "0.99", "--opt-eps", "1e-6",
                               "--lamb-max-grad-norm", "0"])
    assert a.optimizer == "lamb" and a.betas == [0.9, 0.99] and a.opt_eps == 1e-6 and a.lamb_max_grad_norm == 0.0
    a = p.parse_args(COMMON + ["--optimizer", "adamw"])
    assert a.betas == [0.9, 0.999] and a.opt_eps is None and a.lamb_max_grad_norm == 1.0


@pytest.mark.parametrize("flags,needle", [
    (["--optimizer", "lamb", "--hip-graph"], "--hip-graph"),
    (["--optimizer", "adam", "--hip-graph"], "--hip-graph"),
    (["--optimizer", "adamw", "--hip-graph"], "--hip-graph"),
    (["--optimizer", "lamb", "--betas", "0.9", "1.0"], "--betas"),
    (["--optimizer", "adam", "--opt-eps", "0"], "--opt-eps"),
    (["--optimizer", "lamb", "--lamb-max-grad-norm", "-1"], "--lamb-max-grad-norm"),
])
def test_trainer_refuses_up_front(flags, needle):
    from imagent_amd.cli import build_parser
    from imagent_amd.train.engine import Trainer
    with pytest.raises(SystemExit) as e:
        Trainer(build_parser().parse_args(COMMON + flags))
    assert needle in str(e.value), e.value
    if needle == "--hip-graph":
        assert f"--optimizer {flags[1]}" in str(e.value), e.value
    Trainer._check_optimizer(build_parser().parse_args(COMMON + ["--optimizer", "lars", "--hip-graph"]))  # captured


def test_cli_lamb_trains(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, "-m", "imagent_amd.cli"] + COMMON +
                       ["--optimizer", "lamb", "--lr", "0.002", "--wd", "0.01", "--model-ema", "0.9", "--epochs", "1",
                        "--tb-dir", "", "--checkpoint-dir", str(tmp_path)],
                       cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    out = r.stdout
    assert "Optimizer: lamb (betas 0.9 0.999, eps 1e-06): per-tensor torch ops" in out
    assert "Epoch 1 Summary: " in out
    line = [ln for ln in out.splitlines() if ln.startswith("\tTrain loss: ")]
    assert len(line) == 1, out[-2000:]
    loss = float(line[0].split("Train loss: ")[1].split(" ;")[0])
    assert math.isfinite(loss) and 0.0 < loss < 20.0
    st = torch.load(tmp_path / "state_resnet18.pt", map_location="cpu", weights_only=True)
    assert st["optimizer"]["kind"] == "lamb" and st["optimizer"]["steps"] == 6
    assert st["extra"]["ema"]["updates"] == 6
    assert set(st["optimizer"]["m"]) == {k for k in st["model"] if "running" not in k and "num_batches" not in k}
