"""Stand-alone timing of conv3's fused-output launch with the next block's conv1 in it (igemm_fwd(next1=),
conv_stream.hip IG_NEXT1) against the two launches it replaces, plain events, nothing profiled:

python scripts/next_conv1_bench.py [--batch 4096] [--downsample]

One line per arm: us per call and the HBM bytes each moves (operands + results) as TB/s.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def timeit(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--hw", type=int, default=56)
    ap.add_argument("--downsample", action="store_true", help="the residual enters through a per-channel scale")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    from imagent_amd.ops import _lib
    from imagent_amd.ops.conv import igemm_fwd
    dev = "cuda"
    N, H = a.batch, a.hw
    M = N * H * H
    torch.manual_seed(0)
    h = torch.randn(N, H, H, 64, device=dev).to(torch.bfloat16)
    res = torch.randn(N, H, H, 256, device=dev).to(torch.bfloat16)
    w3 = (torch.randn(256, 1, 1, 64, device=dev) * (2.0 / 64) ** 0.5).to(torch.bfloat16)
    w1 = (torch.randn(64, 1, 1, 256, device=dev) * (2.0 / 256) ** 0.5).to(torch.bfloat16)
    aff = torch.stack([torch.empty(256, device=dev).uniform_(0.5, 1.5),
                       torch.empty(256, device=dev).uniform_(-0.5, 0.5)]).contiguous()
    rsc = torch.empty(256, device=dev).uniform_(0.5, 1.5) if a.downsample else None
    out = torch.empty_like(res)
    ym = torch.empty(out.numel() // 8, device=dev, dtype=torch.uint8)
    slab = torch.zeros(_lib.STAT_SLOTS, 2, 64, device=dev)
    a1 = torch.empty(N, H, H, 64, device=dev, dtype=torch.bfloat16)

    def conv3(**kw):
        return igemm_fwd(h, w3, 1, 0, 1, 1, out=out, affine=aff, relu=True, res=res, maskout=ym, res_scale=rsc, **kw)

    def conv1():
        return igemm_fwd(out, w1, 1, 0, 1, 1, stats=slab, out=a1)

    b3 = M * (64 + 256 + 256) * 2 + M * 32  # h, residual, out, mask bits
    b1 = M * (256 + 64) * 2
    bf = b3 + M * 64 * 2
    t3, t1 = timeit(conv3, a.reps), timeit(conv1, a.reps)
    tf = timeit(lambda: conv3(next1=(w1, slab)), a.reps)
    print(f"{N} x {H} x {H}{' (downsample form)' if a.downsample else ''}")
    print(f"conv3 fused output        {t3:9.1f} us  {b3 / t3 * 1e-6:5.2f} TB/s")
    print(f"next conv1 (256 -> 64)    {t1:9.1f} us  {b1 / t1 * 1e-6:5.2f} TB/s")
    print(f"two launches              {t3 + t1:9.1f} us")
    print(f"one launch (next1)        {tf:9.1f} us  {bf / tf * 1e-6:5.2f} TB/s   {100 * (1 - tf / (t3 + t1)):.1f} % less")


if __name__ == "__main__":
    main()
