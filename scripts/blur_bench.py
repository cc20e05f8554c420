"""Times of the BlurPool kernels (ops/misc.py blurpool_fwd / blurpool_bwd; blurpool.hip) at the shapes of resnetblur50 at
224^2 -- the stride-2 blocks' 56^2 x 128, 28^2 x 256, 14^2 x 512 and the stem's 112^2 x 64 -- each against the MINIMUM
traffic of the op (the input read once, the result written once), the copy roof of profiles/hbm_roof.md and a copy of
the same bytes timed in the same run; the fused BatchNorm + ReLU + BlurPool route of ops/block.py (``bn_scale_shift``
+ the kernel with ss) against the two-pass route (``bn_act_forward`` + the plain pool) in the same run; and the
training step rate of resnetblur50 / resnetaa50d beside resnet50 / resnet50d. Device events around ``iters``
back-to-back launches after a warm-up.

    python scripts/blur_bench.py [--batch 256] [--iters 20] [--steps 10] [--out blur_bench.json]

Prints one JSON line per measurement; needs the GPU (no fall-back)."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from se_bench import _copy_us, _time, step_rate  # noqa: E402  (the same timer, copy and training step)

COPY_ROOF = 5.77e12  # bytes / s read + written, profiles/hbm_roof.md
SHAPES = [(56, 128), (28, 256), (14, 512), (112, 64)]  # (H = W, C) of the pools' inputs


def _row(name, us, nbytes, iters, **kw):
    bps = nbytes / (us * 1e-6)
    return dict(kind="kernel", name=name, us=round(us, 1), min_bytes=nbytes, tb_per_s=round(bps / 1e12, 3),
                of_copy_roof=round(bps / COPY_ROOF, 3), copy_us=round(_copy_us(nbytes, iters), 1), **kw)


def pool_rows(N, iters):
    from imagent_amd.models.resnet import BatchNorm2d, BNWork
    from imagent_amd.ops import _lib
    from imagent_amd.ops.bn import bn_act_forward, bn_scale_shift
    from imagent_amd.ops.misc import blurpool_bwd, blurpool_fwd
    rows = []
    for H, C in SHAPES:
        x = torch.randn(N, H, H, C, device="cuda").to(torch.bfloat16)
        y = blurpool_fwd(x)
        nbytes = (x.numel() + y.numel()) * 2
        kw = dict(H=H, C=C)
        rows.append(_row("blurpool fwd", _time(lambda: blurpool_fwd(x), iters), nbytes, iters, **kw))
        rows.append(_row("blurpool bwd", _time(lambda: blurpool_bwd(y, (H, H)), iters), nbytes, iters, **kw))
        bn = BatchNorm2d(C).to("cuda")
        bn.work = BNWork(torch.zeros(_lib.STAT_SLOTS, 2, C, device="cuda"), torch.zeros(2, C, device="cuda"),
                         torch.zeros(2, C, device="cuda"), None)
        xf = x.float().reshape(-1, C)
        bn.work.slab[0, 0].copy_(xf.sum(0))
        bn.work.slab[0, 1].copy_((xf * xf).sum(0))
        ss = bn_scale_shift(x, bn)
        rows.append(_row("blurpool fwd, BN + ReLU on the load", _time(lambda: blurpool_fwd(x, ss), iters), nbytes,
                         iters, **kw))
        # the two routes of an anti-aliased block from the raw conv output to the pooled tensor, small launches included
        rows.append(_row("route: bn_scale_shift + fused blurpool",
                         _time(lambda: blurpool_fwd(x, bn_scale_shift(x, bn)), iters), nbytes, iters, **kw))
        rows.append(_row("route: bn_act_forward + plain blurpool",
                         _time(lambda: blurpool_fwd(bn_act_forward(x, None, bn, None, 0, True)), iters),
                         nbytes + 2 * x.numel() * 2, iters, **kw))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blur_bench.py measures on the GPU: none found")
    rows = pool_rows(a.batch, a.iters)
    for arch in ("resnet50", "resnetblur50", "resnet50d", "resnetaa50d") * 2:  # alternating: the spread shows
        rows.append(step_rate(arch, a.batch, a.steps))
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
