"""Stand-alone timing of the conv1 dgrad that also forms the previous block's T = g^T h2 (BNBwdFuse(gramt=),
conv_stream.hip modes 6 / 7) against the two launches it replaces -- the same dgrad without T, then gram_T over the
g it wrote -- plain events, nothing profiled:

python scripts/gram_t_fused_bench.py [--batch 4096] [--hw 56]

Per form (K = 64 mode 6, K = 64 mode 7 with the second BN branch, K = 128 with old_sub2): us per call and the HBM
bytes each arm moves (operands + results) as TB/s.
"""

import argparse
import os
import sys
import types

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
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    from imagent_amd.ops import _lib
    from imagent_amd.ops.bn_gram import gram_T
    from imagent_amd.ops.conv import BNBwdFuse, igemm_dgrad
    dev = "cuda"
    N, H, P = a.batch, a.hw, 64
    C4, M = 4 * P, a.batch * a.hw * a.hw
    torch.manual_seed(0)
    nbw = _lib.kernels().imk_bn_bwd_scratch_floats(1)

    def bn():
        return types.SimpleNamespace(
            weight=torch.ones(C4, device=dev), bias=torch.zeros(C4, device=dev),
            work=types.SimpleNamespace(save=torch.stack([torch.zeros(C4, device=dev), torch.ones(C4, device=dev)]),
                                       scratch=torch.zeros(nbw * C4, device=dev)))

    g = torch.randn(N, H, H, C4, device=dev).to(torch.bfloat16)  # the old gradient, accumulated into
    h2 = torch.relu(torch.randn(N, H, H, P, device=dev)).to(torch.bfloat16)
    bits = torch.randint(0, 256, (g.numel() // 8,), device=dev, dtype=torch.uint8)
    T = torch.zeros(C4, P, device=dev)
    print(f"{N} x {H} x {H}, p = {P}")
    for name, K, x2, sub2 in (("K = 64 (mode 6)", 64, False, False), ("K = 64 + second branch (mode 7)", 64, True, False),
                              ("K = 128 old_sub2 (mode 6)", 128, False, True)):
        dy = torch.randn(N, H, H, K, device=dev).to(torch.bfloat16)
        wt = (torch.randn(C4, 1, 1, K, device=dev) * (2.0 / K) ** 0.5).to(torch.bfloat16)
        xb = torch.randn(N, H, H, C4, device=dev).to(torch.bfloat16) if x2 else None
        b1, b2 = bn(), (bn() if x2 else None)

        def dgrad(gt):
            igemm_dgrad(dy, wt, (H, H), 1, 0, 1, 1, out=g, accumulate=True, old_sub2=sub2,
                        bnb=BNBwdFuse(None, b1, y=bits, x2=xb, bn2=b2, gramt=gt))

        # dy, old g (a quarter of it with old_sub2), mask bits, g stored, second-branch x
        bd = M * (K * 2 + C4 * 2 // (4 if sub2 else 1) + C4 // 8 + C4 * 2 + (C4 * 2 if x2 else 0))
        bt = M * (C4 + P) * 2
        bf = bd + M * P * 2
        td = timeit(lambda: dgrad(None), a.reps)
        tt = timeit(lambda: gram_T(g, h2, out=T), a.reps)
        tf = timeit(lambda: dgrad((h2, T)), a.reps)
        print(f"{name}")
        print(f"  conv1 dgrad + BN backward {td:9.1f} us  {bd / td * 1e-6:5.2f} TB/s")
        print(f"  gram_T                    {tt:9.1f} us  {bt / tt * 1e-6:5.2f} TB/s")
        print(f"  two launches              {td + tt:9.1f} us")
        print(f"  one launch (gramt)        {tf:9.1f} us  {bf / tf * 1e-6:5.2f} TB/s   {100 * (1 - tf / (td + tt)):.1f} % less")
        del dy, xb
    assert torch.isfinite(T).all()


if __name__ == "__main__":
    main()
