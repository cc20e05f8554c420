"""Times of the SE block tail's launches (ops/se.py) per SE shape of seresnet50 at 224^2, against the time a
device-to-device copy takes to move the same bytes on the same GPU in the same run (the copy roof), and the training
step throughput of seresnet50 beside resnet50. Device events around ``iters`` back-to-back launches after a warm-up.

    python scripts/se_bench.py [--batch 256] [--iters 20] [--steps 10] [--out se_bench.json]

Prints one JSON line per measurement; needs the GPU (no fall-back)."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(56, 256), (28, 512), (14, 1024), (7, 2048)]  # (H = W, C) of layer1..4's block outputs


def _time(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3  # us


def _copy_us(nbytes, iters):
    """A copy that reads nbytes / 2 and writes nbytes / 2."""
    src = torch.empty(max(nbytes // 2, 256), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return _time(lambda: dst.copy_(src), iters)


def tail_times(N, H, C, iters):
    from imagent_amd.models.resnet import BatchNorm2d, BNWork, SEModule
    from imagent_amd.ops import _lib, se as S
    from imagent_amd.ops.bn import bn_scale_shift
    dev = "cuda"
    torch.manual_seed(0)
    a, idt, dout = (torch.randn(N, H, H, C, device=dev).to(torch.bfloat16) for _ in range(3))
    bn, se = BatchNorm2d(C).to(dev), SEModule(C).to(dev)
    for p in list(bn.parameters()) + list(se.parameters()):
        p.grad = torch.zeros_like(p)
    for fc in (se.fc1, se.fc2):
        fc.w_bf16 = fc.weight.detach().to(torch.bfloat16).flatten().contiguous()
    bn.work = BNWork(torch.zeros(_lib.STAT_SLOTS, 2, C, device=dev), torch.zeros(2, C, device=dev),
                     torch.zeros(2, C, device=dev), None)
    x = a.float().reshape(-1, C)
    bn.work.slab[0, 0].copy_(x.sum(0))
    bn.work.slab[0, 1].copy_((x * x).sum(0))
    ss = bn_scale_shift(a, bn)
    HW, R = H * H, se.reduced
    X1 = S.se_squeeze(a)
    z, h, s = S.se_excite_fwd(X1, ss, se, HW)
    out = S.se_scale_add_relu(a, ss, s, idt)
    g, G = S.se_bwd_reduce(dout, out, a)
    dpool, bsum = S.se_excite_bwd(G, X1, ss, z, h, s, bn, se, HW)
    T, nc, w = N * HW * C * 2, N * C * 4, 2 * C * R * 2  # one bf16 tensor, one fp32 [N, C], both bf16 weights
    launches = [
        ("se_squeeze", lambda: S.se_squeeze(a), T + nc),
        ("se_excite_fwd", lambda: S.se_excite_fwd(X1, ss, se, HW), 3 * nc + N * R * 4 + w),
        ("se_scale_add_relu", lambda: S.se_scale_add_relu(a, ss, s, idt), 3 * T + nc),
        ("se_bwd_reduce", lambda: S.se_bwd_reduce(dout, out, a), 4 * T + 2 * nc),
        # reads G1, G2, s (twice), X1, z, dz2; writes dz2, dpool; h / dh twice; weights twice; the fp32 gradients
        ("se_excite_bwd", lambda: S.se_excite_bwd(G, X1, ss, z, h, s, bn, se, HW),
         9 * nc + 4 * N * R * 4 + 2 * w + 2 * 2 * C * R * 4),
        ("se_bn_apply_bwd", lambda: S.se_bn_apply_bwd(g, a, s, dpool, ss, bn, bsum), 3 * T + 2 * nc),
    ]
    rows = []
    for name, fn, nbytes in launches:
        us, roof = _time(fn, iters), _copy_us(nbytes, iters)
        rows.append(dict(kind="launch", name=name, N=N, H=H, C=C, R=R, bytes=nbytes, us=round(us, 1),
                         copy_roof_us=round(roof, 1), of_roof=round(roof / us, 3)))
    return rows


def step_rate(arch, N, steps):
    from imagent_amd.models import resnet
    from imagent_amd.models.native import bind_native
    from imagent_amd.ops.misc import XentFn, normalize_u8
    from imagent_amd.train.optim import FlatSGD
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = resnet.build(arch)
    st = bind_native(m, dev)
    opt = FlatSGD(st.arena, lr=0.1, momentum=0.9, weight_decay=1e-4, after_step=st.refresh_shadows)
    img = torch.randint(0, 256, (N, 224, 224, 3), dtype=torch.uint8, device=dev)
    y = torch.randint(0, 1000, (N,), device=dev)
    met = torch.zeros(4, device=dev)
    m.train()

    def step():
        opt.zero_grad()
        XentFn.apply(m(normalize_u8(img, (224, 224), 4, (0.5,) * 3, (0.5,) * 3)), y, met, 0.0).backward()
        opt.step()

    us = _time(step, steps)
    return dict(kind="step", arch=arch, batch=N, ms=round(us / 1e3, 2), img_per_s=round(N / us * 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("se_bench.py measures on the GPU: none found")
    rows = []
    for H, C in SHAPES:
        rows += tail_times(a.batch, H, C, a.iters)
    for arch in ("resnet50", "seresnet50", "resnet50", "seresnet50"):  # alternating: the spread shows
        rows.append(step_rate(arch, a.batch, a.steps))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
