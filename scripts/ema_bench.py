"""Isolated timing of the --model-ema optimizer launches at the ResNet-50 arena size (25.6 M fp32 parameters), in one
process on the same tensors:

  sgd          imk_sgd alone (the step without --model-ema): 22 B per element (p, g, buf read; p, buf, bf16 shadow
               written)
  ema          imk_ema_flat alone over (E, p): 12 B per element
  sgd + ema    imk_sgd, then imk_ema_flat: what --model-ema runs per step, 34 B per element in two launches

10 warm-up launches, then 50 timed launches per arm and repeat (one event pair per launch for the one-launch arms,
one pair around both launches of the two-launch arm), the median and the minimum of the 50; every arm repeated
--repeats times, the arms interleaved repeat by repeat. TB/s is the arm's bytes over its median. (A fourth arm, one
launch with the average inside sgd_kernel at 30 B per element, was timed by this script when the feature was built
and lost to sgd + ema: profiles/model_ema.md has its numbers and its kernel text.)

python scripts/ema_bench.py [--arch resnet50] [--reps 50] [--repeats 3] [--out FILE.md]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench needs a GPU: a timing taken elsewhere says nothing")
    from imagent_amd.models import resnet
    from imagent_amd.models.arena import _align
    from imagent_amd.ops.misc import ema_flat, sgd_flat
    dev = torch.device("cuda")
    n = sum(_align(p.numel()) for p in resnet.build(args.arch, num_classes=1000).parameters())
    g = torch.Generator(device=dev).manual_seed(0)
    P = torch.randn(n, device=dev, generator=g) * 0.05
    G = torch.randn(n, device=dev, generator=g) * 1e-3
    B = torch.zeros(n, device=dev)
    E = P.clone()
    S = torch.empty(n, device=dev, dtype=torch.bfloat16)
    hp = (1e-3, 0.9, 0.0, 1e-4, False, False, 1.0)
    omd = 1e-4

    def sgd():
        sgd_flat(P, G, B, S, *hp)

    def ema():
        ema_flat(E, P, omd)

    def two():
        sgd_flat(P, G, B, S, *hp)
        ema_flat(E, P, omd)

    arms = [("sgd", sgd, 22), ("ema", ema, 12), ("sgd + ema", two, 34)]
    meds = {name: [] for name, _, _ in arms}
    mins = {name: [] for name, _, _ in arms}
    for _ in range(args.repeats):
        for name, f, _ in arms:
            for _ in range(args.warmup):
                f()
            torch.cuda.synchronize()
            t = []
            for _ in range(args.reps):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                f()
                e.record()
                e.synchronize()
                t.append(s.elapsed_time(e) * 1e3)
            meds[name].append(statistics.median(t))
            mins[name].append(min(t))
    lines = [f"| arm ({args.arch} arena, {n} floats) | B / element | median us per repeat | min us per repeat | "
             "median of medians us | TB/s |", "|---|---:|---|---|---:|---:|"]
    for name, _, bpe in arms:
        m = statistics.median(meds[name])
        lines.append(f"| {name} | {bpe} | {' / '.join(f'{x:.1f}' for x in meds[name])} | "
                     f"{' / '.join(f'{x:.1f}' for x in mins[name])} | {m:.1f} | {n * bpe / m / 1e6:.2f} |")
    extra = statistics.median(meds["sgd + ema"]) - statistics.median(meds["sgd"])
    spread = max(meds["sgd + ema"]) - min(meds["sgd + ema"])
    lines += ["", f"sgd + ema vs sgd alone: {extra:+.1f} us per step for the average "
                  f"(spread of sgd + ema's repeat medians: {spread:.1f} us)"]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
