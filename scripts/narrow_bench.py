"""Times of the ResNet-D kernels at the shapes of resnet50d at 224^2: the narrow stem convs (ops/conv.py nconv_*;
forward, dgrad and wgrad of conv A 4 -> 32 / s2, B 32 -> 32, C 32 -> 64 at 112 x 112) and the shortcut's 2 x 2 average
pool in both directions, each against the MINIMUM traffic of the op (operands read once, the result written once) and
the copy roof of profiles/hbm_roof.md; for the two 32-channel forwards and dgrads also the existing dense route
(``igemm_fwd`` / ``igemm_dgrad``) in the same run; and the training step rate of resnet50d beside resnet50.
Device events around ``iters`` back-to-back launches after a warm-up.

    python scripts/narrow_bench.py [--batch 256] [--iters 20] [--steps 10] [--out narrow_bench.json]

Prints one JSON line per measurement; needs the GPU (no fall-back)."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from se_bench import _time, step_rate  # noqa: E402  (the same timer and training step)

COPY_ROOF = 5.77e12  # bytes / s read + written, profiles/hbm_roof.md
CONVS = [("A", 4, 32, 2, 224), ("B", 32, 32, 1, 112), ("C", 32, 64, 1, 112)]  # name, Ci, Co, stride, input H = W
POOLS = [(56, 256), (28, 512), (14, 1024)]  # (H = W, C) of the inputs of layer2..4's first block


def _row(name, us, nbytes, **kw):
    bps = nbytes / (us * 1e-6)
    return dict(kind="kernel", name=name, us=round(us, 1), min_bytes=nbytes, tb_per_s=round(bps / 1e12, 3),
                of_copy_roof=round(bps / COPY_ROOF, 3), **kw)


def conv_rows(N, iters):
    from imagent_amd.ops import conv as K
    rows = []
    for name, ci, co, s, H in CONVS:
        OH = (H - 1) // s + 1
        x = torch.randn(N, H, H, ci, device="cuda").to(torch.bfloat16)
        dy = torch.randn(N, OH, OH, co, device="cuda").to(torch.bfloat16)
        w = torch.randn(co, 3, 3, ci, device="cuda").to(torch.bfloat16)
        wt = w.permute(3, 1, 2, 0).contiguous()
        dw = torch.zeros(co, 3, 3, ci, device="cuda")
        stats = torch.zeros(32, 2, co, device="cuda")
        bx, by, bw = x.numel() * 2, dy.numel() * 2, w.numel() * 2
        rows.append(_row(f"conv{name} fwd", _time(lambda: K.nconv_fwd(x, w, s, stats=stats), iters), bx + by + bw))
        rows.append(_row(f"conv{name} wgrad", _time(lambda: K.nconv_wgrad(dy, x, dw, s), iters), bx + by + 2 * bw))
        if s == 1:
            rows.append(_row(f"conv{name} dgrad", _time(lambda: K.nconv_dgrad(dy, wt), iters), bx + by + bw))
            rows.append(_row(f"conv{name} fwd dense", _time(lambda: K.igemm_fwd(x, w, 1, 1, 3, 3, stats=stats), iters),
                             bx + by + bw))
            rows.append(_row(f"conv{name} dgrad dense", _time(lambda: K.igemm_dgrad(dy, wt, (H, H), 1, 1, 3, 3), iters),
                             bx + by + bw))
    return rows


def pool_rows(N, iters):
    from imagent_amd.ops.misc import avgpool2_bwd, avgpool2_fwd
    rows = []
    for H, C in POOLS:
        x = torch.randn(N, H, H, C, device="cuda").to(torch.bfloat16)
        y = avgpool2_fwd(x)
        nbytes = (x.numel() + y.numel()) * 2
        rows.append(_row("avgpool2 fwd", _time(lambda: avgpool2_fwd(x), iters), nbytes, H=H, C=C))
        rows.append(_row("avgpool2 bwd", _time(lambda: avgpool2_bwd(y, (H, H)), iters), nbytes, H=H, C=C))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("narrow_bench.py measures on the GPU: none found")
    rows = conv_rows(a.batch, a.iters) + pool_rows(a.batch, a.iters)
    for arch in ("resnet50", "resnet50d", "resnet50", "resnet50d"):  # alternating: the spread shows
        rows.append(step_rate(arch, a.batch, a.steps))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
