"""Isolated timing of the fused RandomResizedCrop + normalise kernel (ops.misc.rrc_normalize_u8) against the two
input kernels it stands beside, in one process on the same uint8 tensors: 448^2 records -> 224^2 bf16 at Cp 4,
B = 256 and B = 4096.

  rrc default   boxes from data.augment.sample_boxes, scale (0.08, 1), ratio (3/4, 4/3)
  rrc full      every box the whole image (scale 2 on both axes: the most source rows and taps a record can need)
  normalize     normalize_u8 with a random 224^2 crop (the same-scale crop --random-resized-crop replaces)
  resize        resize_normalize_u8 of the whole image (--record-resize: bilinear, no antialiasing)

One event pair per launch, 3 warm-up launches, the median (and the minimum) of --reps launches, the variants
interleaved round by round. Bytes are what each kernel must move: the source pixels it needs once (the boxes' for
rrc, the crop's for normalize, the image's for resize) plus its output once; TB/s against the 5.77 TB/s copy roof of
profiles/hbm_roof.md. IMAGENT_RRC_BAND / IMAGENT_RRC_LDS_KB variants of the band height / LDS bytes are timed beside
the default with --variants.

python scripts/rrc_bench.py [--batches 256 4096] [--reps 20] [--variants 8:64 4:64] [--out FILE.md]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

COPY_ROOF_TBS = 5.77  # profiles/hbm_roof.md
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--src", type=int, default=448)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--variants", nargs="*", default=["8:64", "4:64"],
                    help="band rows : LDS cap in KB (first = the default)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrc_bench needs a GPU: a timing taken elsewhere says nothing")
    from imagent_amd.data.augment import sample_boxes
    from imagent_amd.ops.misc import normalize_u8, resize_normalize_u8, rrc_normalize_u8
    dev = torch.device("cuda")
    S, O = args.src, args.size
    lines = ["| B | kernel | band : LDS cap KB | median us | min us | GB moved | TB/s (median) | of copy roof |",
             "|---:|---|---|---:|---:|---:|---:|---:|"]
    for B in args.batches:
        g = torch.Generator(device=dev).manual_seed(0)
        u8 = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
        out = torch.empty((B, O, O, 4), device=dev, dtype=torch.bfloat16)
        flip = (torch.rand(B, device=dev, generator=g) < 0.5).to(torch.uint8)
        boxes = sample_boxes(B, S, S, generator=g, device=dev)
        full = torch.tensor([[0, 0, S, S]] * B, dtype=torch.int32, device=dev)
        crop = torch.randint(0, S - O + 1, (B, 2), device=dev, generator=g, dtype=torch.int32)
        ob = out.numel() * 2
        box_bytes = int((boxes[:, 2].long() * boxes[:, 3].long()).sum().item()) * 3

        def rrc(bx, band, kb):
            def f():
                os.environ["IMAGENT_RRC_BAND"], os.environ["IMAGENT_RRC_LDS_KB"] = band, kb
                rrc_normalize_u8(u8, (O, O), 4, MEAN, STD, bx, flip, out=out)
            return f

        cases = []
        for v in args.variants:
            band, kb = v.split(":")
            cases.append(("rrc default boxes", v, rrc(boxes, band, kb), box_bytes + ob))
            cases.append(("rrc full-image boxes", v, rrc(full, band, kb), B * S * S * 3 + ob))
        cases.append(("normalize_u8 random crop", "-",
                      lambda: normalize_u8(u8, (O, O), 4, MEAN, STD, crop, flip, out=out), B * O * O * 3 + ob))
        cases.append(("resize_normalize_u8", "-",
                      lambda: resize_normalize_u8(u8, (O, O), 4, MEAN, STD, flip, out=out), B * S * S * 3 + ob))
        times = [[] for _ in cases]
        for _ in range(3):
            for _, _, fn, _ in cases:
                fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for i, (_, _, fn, _) in enumerate(cases):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                e.synchronize()
                times[i].append(s.elapsed_time(e) * 1e3)
        for (name, v, _, nbytes), t in zip(cases, times):
            med, mn = statistics.median(t), min(t)
            tbs = nbytes / med / 1e6
            lines.append(f"| {B} | {name} | {v} | {med:.1f} | {mn:.1f} | {nbytes / 1e9:.3f} | {tbs:.2f} | "
                         f"{100 * tbs / COPY_ROOF_TBS:.0f} % |")
        del u8, out
        os.environ.pop("IMAGENT_RRC_BAND", None)
        os.environ.pop("IMAGENT_RRC_LDS_KB", None)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
