"""fp8 weight gradient (imk_conv_wgrad_fp8, conv_wgrad_fp8.h) against the default bf16 dispatch (imk_conv_wgrad) on
every ResNet-50 shape `ops.block.fp8_wgrad_ok` covers: isolated time per call and the operand bytes of each.

    python scripts/wgrad_fp8_ab.py [--batch 2048] [--variants 2,1,3,4,5,12]

fp8 variants: 2 (the default dispatch) 64-row stages x 2, 1: 64 x 4, 3: 128 x 2, 4: 64 x 3, 5: 32 x 4 -- fragments
converted to bf16; 11 / 12 / 13: the fp8 MFMA on the bytes (64 x 4 / 64 x 2 / 128 x 2; does not hold the fp32
summation bound on full-range data, profiles/fp8_wgrad.md).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (Ci, H, Co, k, s, calls per step at R50)
SHAPES = [(128, 56, 128, 3, 2, 1), (128, 28, 128, 3, 1, 3), (256, 28, 256, 3, 2, 1), (256, 14, 256, 3, 1, 5),
          (512, 14, 512, 3, 2, 1), (512, 7, 512, 3, 1, 2), (1024, 14, 512, 1, 1, 1), (2048, 7, 512, 1, 1, 2),
          (512, 7, 2048, 1, 1, 3), (512, 28, 1024, 1, 2, 1), (1024, 14, 2048, 1, 2, 1)]


def _time(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--variants", default="2,1,3,4,5,12")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    from imagent_amd.ops.conv import igemm_wgrad, igemm_wgrad_fp8
    dev = "cuda"
    # clock ramp: spin the GPU before the first timed call (as scripts/wgrad_ab.py)
    _a = torch.randn(8192, 8192, device=dev, dtype=torch.bfloat16)
    for _ in range(200):
        _a = _a @ _a.T * 1e-4
    torch.cuda.synchronize()
    variants = [int(v) for v in a.variants.split(",")]
    e_dy = torch.tensor([-10], dtype=torch.int32, device=dev)
    e_x = torch.tensor([-6], dtype=torch.int32, device=dev)
    print("   Ci    H   Co k s | n | bf16 MB | fp8 MB | bf16 us | " + " | ".join(f"f8 v{v} us" for v in variants))
    tot = [0.0] * (len(variants) + 1)
    for ci, h, co, k, s, n in SHAPES:
        pad = k // 2
        oh = (h + 2 * pad - k) // s + 1
        x = torch.randn(a.batch, h, h, ci, device=dev).to(torch.bfloat16)
        dy = torch.randn(a.batch, oh, oh, co, device=dev).to(torch.bfloat16)
        x8 = (x.float() * 2.0 ** 6).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        dy8 = (dy.float() * 2.0 ** 10).clamp(-57344, 57344).to(torch.float8_e5m2).view(torch.uint8)
        dw = torch.zeros(co, k * k * ci, device=dev)
        us = [_time(lambda: igemm_wgrad(dy, x, dw, s, pad, k, k), a.reps)]
        dw.zero_()
        igemm_wgrad(dy, x, dw, s, pad, k, k)
        ref = dw.clone()
        flag = []
        for v in variants:
            dw.zero_()
            assert igemm_wgrad_fp8(dy8, x8, dw, e_dy, e_x, s, pad, k, k, variant=v)
            torch.cuda.synchronize()
            err = ((dw - ref).norm() / ref.norm()).item()  # (quantisation error of the operands: a sanity check)
            flag.append("" if err < 0.1 else "!")
            us.append(_time(lambda: igemm_wgrad_fp8(dy8, x8, dw, e_dy, e_x, s, pad, k, k, variant=v), a.reps))
        for i, u in enumerate(us):
            tot[i] += u * n
        mb = (x.numel() + dy.numel()) / 1e6
        print(f"{ci:5d} {h:4d} {co:4d} {k} {s} | {n} | {2 * mb:7.0f} | {mb:6.0f} | {us[0]:7.1f} | " +
              " | ".join(f"{u:7.1f}{f}" for u, f in zip(us[1:], flag)), flush=True)
    print("per step (us, x calls): bf16 " + f"{tot[0]:.0f} | " +
          " | ".join(f"f8 v{v} {t:.0f}" for v, t in zip(variants, tot[1:])))


if __name__ == "__main__":
    main()
