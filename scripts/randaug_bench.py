"""Timing of the RandAugment stage (ops.misc.randaug_u8, csrc/kernels/randaug.hip) on the uint8 batch, each figure
against a device copy of the same batch timed in the same process: the copy is one read and one write, the floor of
a uint8 -> uint8 layer.

  per op     the whole batch through one layer of that op at --magnitude (signed ops: the signs alternate over the
             batch): the statistics launch (its blocks exit at once unless the op is Contrast, AutoContrast or
             Equalize), the histogram clear and the apply launch
  stage      the drawn stage, data.randaug.sample_params at --magnitude with --ops layers (default 2)
  copy       out.copy_(batch)

One event pair per call, 3 warm-up rounds, the median (and the minimum) of --reps rounds, all cases interleaved
round by round. --step: the in-step cost as img/s -- imagenet.py --data synthetic --arch resnet50 --batch-size 256
with and without --randaugment, run as alternating pairs of fresh processes, the median of the logged interval
throughputs after the first two intervals.

python scripts/randaug_bench.py [--batch 4096] [--sizes 448 224] [--reps 10] [--step 2] [--out FILE.md]
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


def kernel_tables(args, dev):
    from imagent_amd.data import randaug as RA
    from imagent_amd.ops.misc import randaug_u8
    out_lines = []
    for S in args.sizes:
        B = args.batch
        g = torch.Generator(device=dev).manual_seed(0)
        u8 = torch.empty((B, S, S, 3), device=dev, dtype=torch.uint8)
        for i in range(0, B, 256):
            u8[i:i + 256] = torch.randint(0, 256, (min(256, B - i), S, S, 3), device=dev, generator=g,
                                          dtype=torch.uint8)
        dst = torch.empty_like(u8)
        nbytes = 2 * u8.numel()  # one read, one write
        cases = [("copy", lambda: dst.copy_(u8))]
        for op in range(RA.NUM_OPS):
            rows = [[[op] + RA.op_args(op, args.magnitude, bool(b & 1), S, S)] for b in range(B)]
            p = torch.tensor(rows, dtype=torch.int32).to(dev)
            cases.append((RA.OP_NAMES[op], lambda p=p: randaug_u8(u8, p, 128)))
        p = RA.sample_params(B, args.ops, args.magnitude, S, S, g, dev)
        cases.append((f"stage: {args.ops} drawn layers", lambda p=p: randaug_u8(u8, p, 128)))
        times = [[] for _ in cases]
        for _ in range(3):
            for _, f in cases:
                f()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for i, (_, f) in enumerate(cases):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                e.synchronize()
                times[i].append(s.elapsed_time(e) * 1e3)
        copy_med = statistics.median(times[0])
        out_lines += [f"| case ({B} x {S} x {S} x 3 uint8, magnitude {args.magnitude}) | median us | min us | "
                      "TB/s of one read + one write (median) | times the copy |", "|---|---:|---:|---:|---:|"]
        for (name, _), t in zip(cases, times):
            med, mn = statistics.median(t), min(t)
            layers = args.ops if name.startswith("stage") else 1
            out_lines.append(f"| {name} | {med:.1f} | {mn:.1f} | {layers * nbytes / med / 1e6:.2f} | "
                             f"{med / copy_med:.2f} |")
        out_lines.append("")
        del u8, dst, cases
        torch.cuda.empty_cache()
    return out_lines


def step_table(args):
    base = [sys.executable, os.path.join(ROOT, "imagenet.py"), "--data", "synthetic", "--arch", "resnet50",
            "--batch-size", "256", "--epochs", "1", "--max-steps", str(args.step_iters), "--log-interval", "10",
            "--max-val-steps", "1", "--tb-dir", "", "--quiet-banner", "--launcher", "single"]
    flag = ["--randaugment", str(args.magnitude), "--randaug-ops", str(args.ops)]
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
    lines = ["| imagenet.py --data synthetic --arch resnet50 --batch-size 256 (448 x 448) | img/s, the runs in order | "
             "median img/s |", "|---|---|---:|"]
    for name, label in (("off", "without the flag"), ("on", " ".join(flag))):
        lines.append(f"| {label} | {', '.join(f'{v:.1f}' for v in res[name])} | {statistics.median(res[name]):.1f} |")
    off, on = statistics.median(res["off"]), statistics.median(res["on"])
    lines += ["", f"In-step cost: {100 * (off - on) / off:.2f} % of the throughput "
                  f"({1e3 * 256 * (1 / on - 1 / off):.2f} ms per 256-image step).", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sizes", type=int, nargs="+", default=[448, 224])
    ap.add_argument("--magnitude", type=int, default=9)
    ap.add_argument("--ops", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", type=int, default=0, help="pairs of trainer runs (0: kernels only)")
    ap.add_argument("--step-iters", type=int, default=80)
    ap.add_argument("--step-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench needs a GPU: a timing taken elsewhere says nothing")
    lines = kernel_tables(args, torch.device("cuda"))
    torch.cuda.synchronize()
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
