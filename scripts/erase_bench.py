"""Timing of the Random Erasing kernel (ops.misc.erase_boxes, csrc/kernels/erase.hip) at the production shape, 4096 x
224 x 224 x 4 bf16, in place on one tensor in one process: the probability P in --probs x both modes x --counts boxes
per sample, the draws from data.erase.erase_params at the default scale and ratio. A P = 0 row (every box empty: the
launch and its blocks' four loads) stands beside them.

One event pair per launch, 3 warm-up rounds, the median (and the minimum) of --reps rounds, all cases interleaved
round by round. "MB written" is the erased pixels' bytes, boxes of one sample counted separately (overlaps are
written twice). --step: the in-step cost as img/s -- imagenet.py --data synthetic --arch resnet50 --batch-size 256
with and without --random-erase, run as alternating pairs of fresh processes, the median of the logged interval
throughputs after the first two intervals.

python scripts/erase_bench.py [--batch 4096] [--reps 20] [--step 2] [--dtype bf16] [--out FILE.md]
"""

import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def kernel_table(args, dev):
    from imagent_amd.data.erase import erase_params
    from imagent_amd.ops.misc import erase_boxes
    B, S = args.batch, args.size
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.empty((B, S, S, 4), device=dev, dtype=dtype)
    for i in range(0, B, 256):  # normalised-image-like values, drawn in slices
        x[i:i + 256] = torch.randn((min(256, B - i), S, S, 4), device=dev, generator=g)
    pix = 4 * x.element_size()
    cases = []
    for p in [0.0] + list(args.probs):
        for n in args.counts:
            boxes, keys = erase_params(B, S, S, p, count=n, generator=g, device=dev)
            area = int((boxes[..., 2].long() * boxes[..., 3].long()).sum().item())
            erased = int((boxes[..., 2] > 0).any(1).sum().item())
            for mode in ("const", "pixel"):
                cases.append((p, n, mode, erased, area * pix,
                              lambda b=boxes, k=keys, m=mode: erase_boxes(x, b, k, m, 0.0)))
    times = [[] for _ in cases]
    for _ in range(3):
        for c in cases:
            c[5]()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for i, c in enumerate(cases):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            c[5]()
            e.record()
            e.synchronize()
            times[i].append(s.elapsed_time(e) * 1e3)
    lines = [f"| P ({B} x {S} x {S} x 4 {args.dtype}) | boxes per sample | mode | erased samples | MB written | "
             "median us | min us | TB/s written (median) |", "|---:|---:|---|---:|---:|---:|---:|---:|"]
    for (p, n, mode, erased, nbytes, _), t in zip(cases, times):
        med, mn = statistics.median(t), min(t)
        lines.append(f"| {p:g} | {n} | {mode} | {erased} | {nbytes / 1e6:.1f} | {med:.1f} | {mn:.1f} | "
                     f"{nbytes / med / 1e6:.2f} |")
    return lines + [""]


def step_table(args):
    base = [sys.executable, os.path.join(ROOT, "imagenet.py"), "--data", "synthetic", "--arch", "resnet50",
            "--batch-size", "256", "--epochs", "1", "--max-steps", str(args.step_iters), "--log-interval", "10",
            "--max-val-steps", "1", "--tb-dir", "", "--quiet-banner", "--launcher", "single"]
    flag = ["--random-erase", str(args.step_prob), "--erase-mode", args.step_mode]
    res = {"off": [], "on": []}
    for _ in range(args.step):
        for name, extra in (("off", []), ("on", flag)):
            r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                               timeout=args.step_timeout)
            if r.returncode != 0:
                raise SystemExit(f"imagenet.py {' '.join(extra)} failed:\n{r.stdout[-3000:]}")
            ips = [float(v) for v in re.findall(r"(\d+\.\d+) img/s \|", r.stdout)]
            if len(ips) < 4:
                raise SystemExit(f"too few logged intervals:\n{r.stdout[-3000:]}")
            res[name].append(statistics.median(ips[2:]))
    lines = ["| imagenet.py --data synthetic --arch resnet50 --batch-size 256 | img/s, the runs in order | "
             "median img/s |", "|---|---|---:|"]
    for name, label in (("off", "without the flag"), ("on", " ".join(flag))):
        lines.append(f"| {label} | {', '.join(f'{v:.1f}' for v in res[name])} | {statistics.median(res[name]):.1f} |")
    off, on = statistics.median(res["off"]), statistics.median(res["on"])
    lines += ["", f"In-step cost: {100 * (off - on) / off:.2f} % of the throughput "
                  f"({1e3 * 256 * (1 / on - 1 / off):.3f} ms per 256-image step).", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--probs", type=float, nargs="+", default=[0.1, 0.25, 1.0])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", type=int, default=0, help="pairs of trainer runs (0: the kernel only)")
    ap.add_argument("--step-prob", type=float, default=0.25)
    ap.add_argument("--step-mode", default="pixel", choices=["const", "pixel"])
    ap.add_argument("--step-iters", type=int, default=80)
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("erase_bench needs a GPU: a timing taken elsewhere says nothing")
    lines = kernel_table(args, torch.device("cuda"))
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if args.step > 0:
        lines += step_table(args)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
