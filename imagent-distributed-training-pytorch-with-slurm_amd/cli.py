"""Command line: a superset of the reference's flags.

The six reference flags keep their names and defaults (``imagenet.py:435-450``):
``--seed 0 --backend nccl --batch-size 128 (per GPU) --epochs 100 --lr 0.1
--save-model``. The reference's hard-coded choices become flags with the
reference values as defaults (ResNet-18, 448x448, Normalize 0.5/0.5, momentum
0.9, wd 1e-4, step decay 0.1 every 30 epochs, 10 workers, ``../data/imagenet``,
TensorBoard dir ``imagenet_FR``).

Usage::

    python -m imagent_amd.cli --arch resnet50 --image-size 224 --data synthetic
    srun python imagenet.py --backend=nccl          # Slurm, like imagenet.sh
    torchrun --nproc-per-node 8 imagenet.py ...     # single node
"""

from __future__ import annotations

import argparse
import sys


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Imagenet Pytorch (MI355X-native)")
    # --- reference flags (same names, same defaults) ---
    p.add_argument("--seed", default=0, type=int, help="seed for initializing training. ")
    p.add_argument("--backend", type=str, default="nccl", help="c10d backend (nccl == RCCL on ROCm, or gloo)")
    p.add_argument("--batch-size", type=int, default=128, metavar="N", help="input batch size per GPU")
    p.add_argument("--epochs", type=int, default=100, metavar="N")
    p.add_argument("--lr", type=float, default=0.1, metavar="LR")
    p.add_argument("--save-model", action="store_true", default=False, help="save the best model")
    # --- model / data ---
    p.add_argument("--arch", default="resnet18", choices=["resnet18", "resnet34", "resnet50", "resnet101",
                                                           "resnet152"])
    p.add_argument("--image-size", type=int, default=448)
    p.add_argument("--deterministic", action="store_true",
                   help="BatchNorm statistics without float atomics (fixed-order reduction passes): two runs "
                        "from the same state give bit-identical statistics (HIP kernels)")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp8", "fp32"],
                   help="compute dtype. HIP kernels: bf16 (fp32 masters/accumulation), fp8 = e4m3 forward "
                        "convs on the block-scaled MFMA with bf16 backward, fp32 = the reference's precision "
                        "(imagenet.py:312) on the own exact-f32 MFMA kernels (models/native_f32.py; every ResNet "
                        "depth, BatchNorm widths up to 2048 channels). --kernels torch: PyTorch ops (oracle)")
    p.add_argument("--fp8-wgrad", action="store_true",
                   help="with --dtype fp8 --kernels hip: weight gradients as e5m2 dY x e4m3 X on the 1-byte loop for "
                        "the convs whose fp8 forward and fp8 dgrad already write both copies (ops.block.fp8_wgrad_ok; "
                        "IMAGENT_FP8_WGRAD=1 does the same). Off by default")
    p.add_argument("--data", default="imagenet", choices=["imagenet", "records", "synthetic"],
                   help="imagenet: JPEG folders decoded by worker processes; records: train.imrec / val.imrec "
                        "(python -m imagent_amd.data.records) gathered by the native thread pool")
    p.add_argument("--data-root", default=None, help="default: <cwd>/../data/imagenet (imagenet.py:287)")
    p.add_argument("--workers", type=int, default=10, help="decode processes (imagenet) / gather threads (records)")
    p.add_argument("--num-classes", type=int, default=1000, help="synthetic data only")
    p.add_argument("--synthetic-train-size", type=int, default=1281167)
    p.add_argument("--synthetic-val-size", type=int, default=50000)
    p.add_argument("--synthetic-task", default="random", choices=["random", "colour", "mix"],
                   help="random: uniform noise + labels (throughput); colour: learnable class-coloured images; "
                        "mix: overlapping class Gaussians over smooth random bases (Bayes top-1 ~85 %% at 100 classes)")
    p.add_argument("--flip", action="store_true", help="random horizontal flip (reference: none)")
    p.add_argument("--record-resize", action="store_true",
                   help="records stored at another size than --image-size are bilinearly resampled on the GPU "
                        "(fused into the normalise kernel) instead of cropped: e.g. 320^2 records for 448^2 "
                        "training halve the host gather bytes (profiles/loader_throughput.md)")
    p.add_argument("--random-resized-crop", action="store_true",
                   help="RandomResizedCrop train augmentation: a random box per sample (area fraction --rrc-scale, "
                        "aspect --rrc-ratio), resampled to --image-size with an antialiased filter, fused with the "
                        "normalise and --flip in one HIP kernel; validation takes the --val-center-crop box through "
                        "the same antialiased filter. Takes precedence over --record-resize and the same-scale crop. "
                        "Cost at 4096 img, 448^2 -> 224^2: profiles/rrc_normalize.md")
    p.add_argument("--rrc-scale", type=float, nargs=2, default=[0.08, 1.0], metavar=("LO", "HI"),
                   help="RandomResizedCrop: box area as a fraction of the source image")
    p.add_argument("--rrc-ratio", type=float, nargs=2, default=[0.75, 1.3333], metavar=("LO", "HI"),
                   help="RandomResizedCrop: box aspect ratio w / h, log-uniform (relative to the stored image: "
                        "records are aspect-squashed squares)")
    p.add_argument("--val-center-crop", type=float, default=1.0, metavar="FRAC",
                   help="validation: the centred box of this fraction of each side, antialiased to --image-size "
                        "(0.875 = the usual 224 of 256); 1.0 with --random-resized-crop off: the existing path")
    p.add_argument("--source-size", type=int, default=None, metavar="N",
                   help="--data imagenet: the size the JPEG folder loader decodes to (default --image-size), so that "
                        "--random-resized-crop has pixels to crop from; records and synthetic data hold their own")
    p.add_argument("--mixup", type=float, default=0.0, metavar="ALPHA",
                   help="Mixup train augmentation: every sample becomes lam x + (1 - lam) x' with a partner x' of its "
                        "batch, lam ~ Beta(ALPHA, ALPHA), and the loss is taken against both labels (one HIP kernel "
                        "for the batch, one pair of loss kernels; validation never mixes). 0: off. Cost at 4096 img: "
                        "profiles/mix_pairs.md")
    p.add_argument("--cutmix", type=float, default=0.0, metavar="ALPHA",
                   help="CutMix train augmentation: a box of the partner, sqrt(1 - lam) of each side around a uniform "
                        "centre, is pasted into the sample, lam ~ Beta(ALPHA, ALPHA) then set to the share of pixels "
                        "kept. 0: off. With --mixup too, each mixed sample is one or the other (--mix-switch-prob)")
    p.add_argument("--mix-prob", type=float, default=1.0, metavar="P",
                   help="--mixup / --cutmix: the probability that a sample is mixed at all")
    p.add_argument("--mix-switch-prob", type=float, default=0.5, metavar="P",
                   help="--mixup and --cutmix together: the probability that a mixed sample is CutMix")
    p.add_argument("--randaugment", type=int, default=None, metavar="M",
                   help="RandAugment train augmentation at magnitude M (0 .. 30, 31 bins as torchvision's): every "
                        "image goes through --randaug-ops ops drawn uniformly from the 14 of data/randaug.py, with a "
                        "random sign, in integer arithmetic on the uint8 batch as stored -- ahead of the crop, so the "
                        "fused crop + resize + normalise kernel is untouched (two HIP launches per op; validation "
                        "never augments). Absent: off. Not with --hip-graph. Cost: profiles/randaug.md")
    p.add_argument("--randaug-ops", type=int, default=2, metavar="N", help="--randaugment: ops per image (1 .. 4)")
    p.add_argument("--randaug-fill", type=int, default=128, metavar="V",
                   help="--randaugment: the colour (0 .. 255) of pixels a shear, translation or rotation brings in "
                        "from outside the image; 128 is the normalised zero at mean = std = 0.5")
    p.add_argument("--trivialaugment", action="store_true",
                   help="TrivialAugmentWide train augmentation (torchvision's ta_wide): every image goes through one "
                        "op drawn uniformly from the same 14, at a magnitude bin drawn uniformly from 0 .. 30 over the "
                        "wide ranges of data/trivialaug.py, through --randaugment's kernels and in its place (takes "
                        "--randaug-fill; not with --randaugment, not with --hip-graph)")
    p.add_argument("--random-erase", type=float, default=0.0, metavar="P",
                   help="Random Erasing train augmentation: with probability P a sample's model input has "
                        "--erase-count boxes overwritten in place by one HIP kernel, after the normalise / crop kernel "
                        "and before Mixup / CutMix (torchvision's RandomErasing, timm's count and pixel mode; "
                        "validation never erases). 0: off. Not with --hip-graph. Cost: profiles/erase.md")
    p.add_argument("--erase-scale", type=float, nargs=2, default=[0.02, 0.33], metavar=("LO", "HI"),
                   help="--random-erase: the erased share of the image area, 0 < LO <= HI <= 1")
    p.add_argument("--erase-ratio", type=float, nargs=2, default=[0.3, 3.3], metavar=("LO", "HI"),
                   help="--random-erase: the boxes' aspect ratio h / w, log-uniform, 0 < LO <= HI")
    p.add_argument("--erase-count", type=int, default=1, metavar="N",
                   help="--random-erase: boxes per erased sample (1 .. 4), each of the drawn area divided by N")
    p.add_argument("--erase-mode", default="const", choices=["const", "pixel"],
                   help="--random-erase: const -- every erased element becomes --erase-value; pixel -- an independent "
                        "N(0, 1) draw per element, generated in the kernel (Philox4x32-10, Box-Muller)")
    p.add_argument("--erase-value", type=float, default=0.0, metavar="V",
                   help="--random-erase --erase-mode const: the value written, in normalised units (0: the mean "
                        "colour)")
    # --- optimisation ---
    p.add_argument("--optimizer", default="sgd",
                   choices=["sgd", "lars", "lamb", "adam", "adamw", "adagrad", "rmsprop", "adadelta", "asgd", "nadam"],
                   help="sgd, lars, lamb, adam and adamw are fused HIP launches over the flat parameter arena "
                        "(profiles/flat_adam_lamb.md); the others are the stock torch.optim classes. adam, adamw and "
                        "lamb do not combine with --hip-graph (their bias corrections are new kernel arguments on "
                        "every step)")
    p.add_argument("--lars-eta", type=float, default=1e-3, help="LARS trust coefficient")
    p.add_argument("--betas", type=float, nargs=2, default=[0.9, 0.999], metavar=("B1", "B2"),
                   help="adam / adamw / lamb: the decay of the first and second moment")
    p.add_argument("--opt-eps", type=float, default=None, metavar="EPS",
                   help="adam / adamw / lamb: the denominator's epsilon (default 1e-8 for adam and adamw, 1e-6 for "
                        "lamb)")
    p.add_argument("--lamb-max-grad-norm", type=float, default=1.0, metavar="NORM",
                   help="lamb: clip the gradient to this global L2 norm before the moments (one more launch over "
                        "the gradient arena). 0: off")
    p.add_argument("--momentum", type=float, default=0.9)
    p.add_argument("--wd", "--weight-decay", dest="wd", type=float, default=1e-4)
    p.add_argument("--nesterov", action="store_true")
    p.add_argument("--schedule-decay", type=float, default=4e-3, help="Nadam (Keras) schedule decay")
    p.add_argument("--lr-schedule", default="step", choices=["step", "cosine"])
    p.add_argument("--lr-step", type=int, default=30)
    p.add_argument("--lr-gamma", type=float, default=0.1)
    p.add_argument("--warmup-epochs", type=float, default=0.0)
    p.add_argument("--scale-lr", action="store_true", help="lr *= global_batch / 256")
    p.add_argument("--label-smoothing", type=float, default=0.0)
    p.add_argument("--accum-steps", type=int, default=1, help="gradient accumulation micro-batches")
    p.add_argument("--model-ema", type=float, default=0.0, metavar="DECAY",
                   help="keep an exponential moving average of the weights, E += (1 - DECAY) (p - E) once per "
                        "optimizer step, and of the BatchNorm running statistics; every epoch validates the raw "
                        "weights and then the average (EMA Test lines, val_ema TensorBoard series), and --save-model "
                        "also writes the best average as imagenet_FR_<arch>_ema.pt. Two elementwise HIP launches per "
                        "step after the optimizer's. 0: off; else 0 < DECAY < 1 (e.g. 0.9999). Cost: "
                        "profiles/model_ema.md")
    p.add_argument("--model-ema-warmup", action="store_true",
                   help="--model-ema: ramp the decay as min(DECAY, (1 + t) / (10 + t)) over the t updates done, so "
                        "the average forgets the initial weights quickly (not with --hip-graph: a per-step kernel "
                        "argument would re-capture every step)")
    # --- parallelism / runtime ---
    p.add_argument("--launcher", default="auto", choices=["auto", "slurm", "torchrun", "single"])
    p.add_argument("--kernels", default="auto", choices=["auto", "hip", "torch"],
                   help="hip = hand-written MI355X kernels; torch = PyTorch ops (oracle / CPU)")
    p.add_argument("--comm", default="auto", choices=["auto", "rccl", "torch", "local"])
    p.add_argument("--device", default=None)
    p.add_argument("--bucket-mb", type=float, default=16.0)
    p.add_argument("--first-bucket-mb", type=float, default=2.0)
    p.add_argument("--grad-allreduce-dtype", default="fp32", choices=["fp32", "bf16"],
                   help="bf16: all-reduce bf16 copies of the gradient buckets (half the xGMI bytes)")
    p.add_argument("--broadcast-buffers", default="eval", choices=["eval", "always", "never"])
    p.add_argument("--no-rebuild-buckets", dest="rebuild_buckets", action="store_false")
    p.add_argument("--pg-timeout", type=float, default=1800.0)
    p.add_argument("--hip-graph", action="store_true",
                   help="capture each training step in a HIP graph and replay it (1 GPU, step LR schedule)")
    p.add_argument("--step-timeout", type=float, default=0.0,
                   help="hang watchdog: if no training / validation step completes for this many seconds, "
                        "dump all stacks, abort the communicators and exit with status 75")
    p.add_argument("--check-consistency", type=int, default=0,
                   help="every N steps verify parameters are bit-identical across ranks")
    # --- logging / checkpoint ---
    p.add_argument("--log-interval", type=int, default=50)
    p.add_argument("--tb-dir", default="imagenet_FR")
    p.add_argument("--checkpoint-dir", default=None)
    p.add_argument("--resume", default=None)
    p.add_argument("--max-steps", type=int, default=0, help="cap train steps per epoch (0 = full)")
    p.add_argument("--max-val-steps", type=int, default=0)
    p.add_argument("--quiet-banner", action="store_true")
    p.add_argument("--profile", default=None, help="write a torch.profiler trace to this dir")
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from .train.engine import Trainer
    tr = Trainer(args)
    try:
        if args.profile:
            from .utils.profiling import profiled
            with profiled(args.profile):
                tr.run()
        else:
            tr.run()
    finally:
        tr.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
