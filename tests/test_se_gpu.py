"""The squeeze-and-excitation block tail (csrc/kernels/se.hip, ops/se.py) against fp64, SE models against the torch
backend, and the trainer with an SE arch under --hip-graph."""

import copy
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from exact_ref import ints

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, H, C, downsample): odd HW = 49, N no multiple of the 16-sample tile, R = 128 | R = 8 below one MFMA tile, HW split
# over blocks | R = 16, the shortcut through the mode-0 BatchNorm | a single sample
CASES = [(3, 7, 2048, False), (2, 56, 64, False), (5, 14, 256, True), (1, 28, 512, False)]
IDS = ["3x7x2048", "2x56x64", "5x14x256-ds", "1x28x512"]
FLOOR = 2.0 ** -9  # half a bf16 ulp


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _bn(C, x, seed):
    """A BatchNorm2d with non-trivial gamma / beta, zeroed gradient slots and a workspace whose slab holds the conv
    epilogue's sums of ``x`` (around the shift 0 of a fresh BatchNorm)."""
    from imagent_amd.models.resnet import BatchNorm2d, BNWork
    from imagent_amd.ops import _lib
    g = torch.Generator().manual_seed(seed)
    bn = BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.5)
    bn.weight.grad, bn.bias.grad = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    bn.work = BNWork(torch.zeros(_lib.STAT_SLOTS, 2, C, device=DEV), torch.zeros(2, C, device=DEV),
                     torch.zeros(2, C, device=DEV),
                     torch.zeros(_lib.kernels().imk_bn_bwd_scratch_floats(C), device=DEV))
    xd = x.double().reshape(-1, C)
    bn.work.slab[0, 0].copy_(xd.sum(0))
    bn.work.slab[0, 1].copy_((xd * xd).sum(0))
    return bn


def _se(C, seed):
    """An SEModule with bf16-representable weights, non-zero biases, its bf16 shadows and zeroed gradient slots."""
    from imagent_amd.models.resnet import SEModule
    torch.manual_seed(seed)
    se = SEModule(C).to(DEV)
    with torch.no_grad():
        for fc in (se.fc1, se.fc2):
            fc.weight.copy_(fc.weight.to(torch.bfloat16).float())
            fc.bias.normal_(0.0, 0.5)
            fc.w_bf16 = fc.weight.to(torch.bfloat16).flatten().contiguous()
    for p in se.parameters():
        p.grad = torch.zeros_like(p)
    return se


def _norm(x, b, gamma, beta):
    mean, var = x.mean((0, 1, 2)), x.var((0, 1, 2), unbiased=False)
    return (x - mean) * torch.rsqrt(var + b.eps) * gamma + beta


def _compose(t, bn, dbn, se, dtype):
    """The tail with stock torch ops in ``dtype`` and autograd, from the bf16 a, idt and dout the HIP path is given:
    every tensor that path returns. A downsample block's shortcut is the materialised bf16 output of its BatchNorm
    (``t["idt"]``); its gradient g then goes back through that BatchNorm (dAd)."""
    def leaf(v):
        return v.detach().to(dtype).requires_grad_()

    a, gamma, beta, idt = leaf(t["a"]), leaf(bn.weight), leaf(bn.bias), leaf(t["idt"])
    w1, b1, w2, b2 = leaf(se.fc1.weight), leaf(se.fc1.bias), leaf(se.fc2.weight), leaf(se.fc2.bias)
    u = _norm(a, bn, gamma, beta)
    h = F.relu(u.mean((1, 2)) @ w1.flatten(1).t() + b1)
    s = torch.sigmoid(h @ w2.flatten(1).t() + b2)
    out = F.relu(s[:, None, None, :] * u + idt)
    out.backward(t["dout"].to(dtype))
    r = dict(out=out.detach(), dA=a.grad, g=idt.grad, dW1=w1.grad, db1=b1.grad, dW2=w2.grad, db2=b2.grad,
             dgamma=gamma.grad, dbeta=beta.grad)
    if dbn is not None:
        ad = leaf(t["ad"])
        _norm(ad, dbn, dbn.weight.detach().to(dtype), dbn.bias.detach().to(dtype)).backward(idt.grad)
        r["dAd"] = ad.grad
    return r


def _hip(t, bn, dbn, se):
    from imagent_amd.ops.bn import bn_act_backward
    from imagent_amd.ops.se import se_tail_backward, se_tail_forward
    for p in list(se.parameters()) + [bn.weight, bn.bias]:
        p.grad.zero_()
    bn.work.save.zero_()  # the slab's sums were taken around the shift 0
    if dbn is not None:
        dbn.work.scratch.zero_()
    out, saved = se_tail_forward(t["a"], bn, t["idt"], se)
    dA, g = se_tail_backward(t["dout"], saved, bn, se)
    r = dict(out=out, dA=dA, g=g, dW1=se.fc1.weight.grad, db1=se.fc1.bias.grad, dW2=se.fc2.weight.grad,
             db2=se.fc2.bias.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad)
    if dbn is not None:
        r["dAd"] = bn_act_backward(g, t["ad"], None, None, dbn, None, 0, False)[0]
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in r.items()}


@pytest.mark.parametrize("N,H,C,ds", CASES, ids=IDS)
def test_se_tail_matches_fp64(N, H, C, ds):
    """out, dA, g (and a downsample block's shortcut gradient), the four SE gradients and dgamma / dbeta of
    se_tail_forward / se_tail_backward: per tensor, the relative L2 distance to the fp64 composition is at most twice
    that of the same composition in fp32 on the device with its activation outputs rounded to bf16, or 2^-9. Two
    calls give the same bits.

    Measured distances (HIP / fp32 torch): profiles/se.md."""
    gen = torch.Generator().manual_seed(C + N)

    def rnd(scale=1.0, shift=0.0):
        return (torch.randn(N, H, H, C, generator=gen) * scale + shift).to(torch.bfloat16).to(DEV)

    t = dict(a=rnd(1.5, 0.3), idt=rnd(), ad=rnd(2.0, -0.2), dout=rnd())
    bn, se = _bn(C, t["a"], 1), _se(C, 2)
    dbn = _bn(C, t["ad"], 3) if ds else None
    if ds:  # the shortcut as the block materialises it: the mode-0 BatchNorm pass without ReLU
        from imagent_amd.ops.bn import bn_act_forward
        t["idt"] = bn_act_forward(t["ad"], None, dbn, None, 0, False)
        assert _rel(t["idt"], _norm(t["ad"].double(), dbn, dbn.weight.double(), dbn.bias.double())) < FLOOR
    ref = _compose(t, bn, dbn, se, torch.float64)
    f32 = _compose(t, bn, dbn, se, torch.float32)
    acts = ("out", "dA", "g", "dAd")
    got = _hip(t, bn, dbn, se)
    again = _hip(t, bn, dbn, se)
    bad = []
    for k, v in ref.items():
        base = _rel(f32[k].to(torch.bfloat16) if k in acts else f32[k], v)
        err = _rel(got[k].reshape(v.shape), v)
        print(f"{k:7s} hip {err:.3e}  fp32 torch {base:.3e}")
        if not err <= max(2.0 * base, FLOOR):
            bad.append((k, err, base))
    assert not bad, bad
    assert all(torch.equal(got[k], again[k]) for k in got), [k for k in got if not torch.equal(got[k], again[k])]


@pytest.mark.parametrize("N,H,C,ds", CASES, ids=IDS)
def test_se_pooled_sums_exact(N, H, C, ds):
    """Small-integer a and dout, a 0 / 1 mask: every partial sum is exact in fp32, so X1, G1, G2 and g equal fp64."""
    from imagent_amd.ops.se import se_bwd_reduce, se_squeeze
    a, dout = ints((N, H, H, C), -4, 4, 11, DEV), ints((N, H, H, C), -3, 3, 12, DEV)
    out = ints((N, H, H, C), 0, 1, 13, DEV)
    X1 = se_squeeze(a)
    g, G = se_bwd_reduce(dout, out, a)
    gm = dout.double() * out.double()
    assert (gm.abs() * a.double().abs()).sum((1, 2)).max().item() < 2 ** 24  # the exactness precondition
    assert torch.equal(X1.double(), a.double().sum((1, 2)))
    assert torch.equal(g.double(), gm)
    assert torch.equal(G[0].double(), gm.sum((1, 2))) and torch.equal(G[1].double(), (gm * a.double()).sum((1, 2)))


def _grads(model, x, lab, autocast=False):
    for p in model.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = model(x)
    F.cross_entropy(logits.float(), lab).backward()
    return logits.float(), {n: p.grad.float().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-op"])
@pytest.mark.parametrize("arch", ["seresnet18", "seresnext50_32x4d"])
def test_se_model_step_matches_torch(arch, fused):
    """One training step (16 classes, 64x64, batch 4) and the eval logits against the torch backend from the same
    bf16-rounded weights, as test_gconv_gpu.py's test_resnext50_step_matches_torch: per tensor, the relative L2
    distance to the fp32 oracle is at most 2x that of PyTorch's bf16 autocast, or 5e-2 (logits, every parameter
    gradient, eval logits) / 2e-2 (running statistics)."""
    from imagent_amd.models import resnet
    from imagent_amd.models.native import bind_native
    from imagent_amd.ops.misc import normalize_u8
    torch.manual_seed(0)
    ref = resnet.build(arch, num_classes=16).to(DEV)
    model = copy.deepcopy(ref)
    st = bind_native(model, DEV)
    st.fused_blocks = fused
    with torch.no_grad():
        for p_ref, p in zip(ref.parameters(), model.parameters()):
            p_ref.copy_(p.to(torch.bfloat16).float())
    ref_bf = copy.deepcopy(ref)
    B, H = 4, 64
    low = torch.rand(B, 3, 8, 8, device=DEV)
    img = (F.interpolate(low, size=(H, H), mode="bicubic", align_corners=False).clamp(0, 1) * 255)
    img = img.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    lab = torch.randint(0, 16, (B,), device=DEV)
    x = normalize_u8(img, (H, H), 4, (0.5,) * 3, (0.5,) * 3)
    xr = x[..., :3].float().permute(0, 3, 1, 2).contiguous()
    for m in (model, ref, ref_bf):
        m.train()
    st.arena.zero_grad()
    logits = model(x)
    F.cross_entropy(logits, lab).backward()
    l32, g32 = _grads(ref, xr, lab)
    lbf, gbf = _grads(ref_bf, xr, lab, autocast=True)
    assert _rel(logits, l32) < max(5e-2, 2.0 * _rel(lbf, l32))
    assert sum(".se." in n for n in g32) == 4 * len(list(model.blocks()))
    bad = [(n, _rel(p.grad, g32[n]), _rel(gbf[n], g32[n])) for n, p in model.named_parameters()
           if _rel(p.grad, g32[n]) > max(0.05, 2.0 * _rel(gbf[n], g32[n]))]
    assert not bad, bad
    for (n1, b1), (_, b2), (_, b3) in zip(model.named_buffers(), ref.named_buffers(), ref_bf.named_buffers()):
        if "num_batches_tracked" not in n1:
            assert _rel(b1, b2) < max(2e-2, 2.0 * _rel(b3, b2)), n1
    for m in (model, ref, ref_bf):
        m.eval()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ebf = _rel(ref_bf(xr).float(), ref(xr))
        assert _rel(model(x), ref(xr)) < max(5e-2, 2.0 * ebf)


def test_se_trainer_hip_graph(tmp_path):
    """--arch seresnet18 under --hip-graph: three eager steps, the capture and two replays; the losses are finite."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    args = ["--arch", "seresnet18", "--data", "synthetic", "--hip-graph", "--kernels", "hip", "--image-size", "64",
            "--num-classes", "10", "--batch-size", "8", "--synthetic-train-size", "48", "--synthetic-val-size", "8",
            "--epochs", "1", "--lr", "0.05", "--lr-step", "30", "--log-interval", "1", "--quiet-banner", "--tb-dir", ""]
    r = subprocess.run([sys.executable, "-u", "-m", "imagent_amd.cli"] + args, cwd=tmp_path, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    summ = re.findall(r"Train loss: ([0-9.e+-]+|nan|inf) ; Test loss: ([0-9.e+-]+|nan|inf)", r.stdout)
    assert len(summ) == 1 and all(math.isfinite(float(v)) for v in summ[0]), r.stdout[-3000:]
