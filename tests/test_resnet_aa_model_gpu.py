"""One training step and the eval forward of the anti-aliased archs on the HIP kernels (the fused BatchNorm + ReLU +
BlurPool of ops/block.py, the plain pool of the per-op and eval paths, the blur stem) against the torch backend from
the same bf16-rounded weights: exactly the comparison and tolerances of test_resnet_d_model_gpu.py (per tensor, the
relative L2 distance to the fp32 oracle is at most 2x the distance of PyTorch's own bf16 autocast, or 5e-2 for logits /
gradients / eval logits and 2e-2 for the running statistics). 72 px reaches the odd 9 -> 5 and 5 -> 3 maps; on
resnetblur50d the shortcut's ceil-mode average pool and the blur must agree on 5x5.

Measured, seresnetaa18d-fused-64 (the one case that does not hold in every run; ten fresh processes on one MI355X):
the HIP gradient of ``layer2.1.se.fc1.weight`` is 0.2744 from the fp32 oracle in every run, fused and per-op alike
(the kernels use no float atomics on this path), while PyTorch's own bf16-autocast gradient of that tensor moves
between 0.1234 and 0.1560 from run to run, so the bound 2 x autocast moves between 0.247 and 0.312 and the case passed
in 5 of the 10 runs; every other tensor of the case stayed below 0.99 of its bound. The tensor is an SE gate's first
weight (8 reduced channels, 4 images): both bf16 paths are tens of percent from fp32 on it. An arch without the new
code is further out on such tensors at this size (seresnet18d at 64 px, ``layer4.1.se.fc1.bias``: 0.40 against
autocast's 0.04-0.05). The case and the bound stand as set."""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _grads(model, x, lab, autocast=False):
    for p in model.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        logits = model(x)
    F.cross_entropy(logits.float(), lab).backward()
    return logits.float(), {n: p.grad.float().clone() for n, p in model.named_parameters()}


CASES = [(a, f, h) for a in ("resnetblur18", "resnetblur50") for f in (True, False) for h in (72, 64)] + \
    [("resnetblur50d", True, 72), ("resnextblur50_32x4d", True, 64), ("seresnetaa18d", True, 64)]


@pytest.mark.parametrize("arch,fused,H", CASES, ids=[f"{a}-{'fused' if f else 'per-op'}-{h}" for a, f, h in CASES])
def test_resnet_aa_step_matches_torch(arch, fused, H):
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
    B = 4
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
    print("logits", _rel(logits, l32), "autocast", _rel(lbf, l32))
    assert _rel(logits, l32) < max(5e-2, 2.0 * _rel(lbf, l32))
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
