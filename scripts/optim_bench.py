"""Isolated timing of the optimizer step at the ResNet-50 arena (25,557,056 fp32 parameters + alignment padding), in
one process on one bound model's arenas:

  sgd              FlatSGD, imk_sgd: 22 B per element (p, g, buf read; p, buf, bf16 shadow written) -- for scale
  stock adamw      the route --optimizer adamw took before FlatAdam: TorchOptimizer(torch.optim.AdamW) over the 161
                   parameter views, then refresh_shadows(full=True)
  adam             FlatAdam, imk_adam_flat: 30 B per element (p, g, m, v read; p, m, v, shadow written)
  adam + refresh   FlatAdam with the per-step partial refresh_shadows() it runs in training: the like-for-like
                   counterpart of the stock arm
  lars             FlatLARS, imk_lars_step: 30 B per element (p, g | p, g, buf read; p, buf, shadow written)
  lamb clip        FlatLAMB with the gradient-norm pass: 4 + 24 + 18 = 46 B per element (g | p, g, m, v read; m, v
                   written | p, m, v read; p, shadow written)
  lamb no clip     FlatLAMB, --lamb-max-grad-norm 0: 24 + 18 = 42 B per element

10 warm-up steps, then 50 timed steps per arm (one device-event pair per step), the median of the 50; every arm
repeated --repeats times, the arms interleaved repeat by repeat; median of the repeat medians and their spread
(max - min). TB/s is the arm's bytes (over the parameter elements, padding not counted) over its median; "roof" is
its share of the 6.3 TB/s 2-read-1-write streaming roof (profiles/hbm_roof.md).

python scripts/optim_bench.py [--arch resnet50] [--reps 50] [--repeats 3] [--out FILE.md]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

ROOF_TBS = 6.3  # 2 reads : 1 write (profiles/hbm_roof.md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="resnet50")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs a GPU: a timing taken elsewhere says nothing")
    from imagent_amd.models import resnet
    from imagent_amd.models.native import bind_native
    from imagent_amd.train.optim import FlatAdam, FlatLAMB, FlatLARS, FlatSGD, TorchOptimizer
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = resnet.build(args.arch, num_classes=1000)
    st = bind_native(model, dev)
    ar = st.arena
    n = sum(ar.numels)
    gen = torch.Generator(device=dev).manual_seed(0)
    for i in range(len(ar.params)):  # a gradient in every slice, the padding left zero
        ar.flat_slice(ar.G, i).copy_(torch.randn(ar.numels[i], device=dev, generator=gen) * 1e-3)
    P0 = ar.P.clone()
    lr, wd = 1e-4, 1e-4  # small: hundreds of steps on one gradient must not blow the weights up
    stock = TorchOptimizer(ar, torch.optim.AdamW(ar.params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd),
                           full_refresh=lambda: st.refresh_shadows(full=True))
    arms = [
        ("sgd", FlatSGD(ar, lr, 0.9, 0.0, wd), 22),
        ("stock adamw + full refresh", stock, None),
        ("adam", FlatAdam(ar, lr, weight_decay=wd, decoupled=True), 30),
        ("adam + refresh", FlatAdam(ar, lr, weight_decay=wd, decoupled=True, after_step=st.refresh_shadows), None),
        ("lars", FlatLARS(ar, lr, 0.9, wd), 30),
        ("lamb clip", FlatLAMB(ar, lr, weight_decay=wd, max_grad_norm=1.0), 46),
        ("lamb no clip", FlatLAMB(ar, lr, weight_decay=wd, max_grad_norm=0.0), 42),
    ]
    meds = {name: [] for name, _, _ in arms}
    for _ in range(args.repeats):
        for name, opt, _ in arms:
            ar.P.copy_(P0)
            for _ in range(args.warmup):
                opt.step()
            torch.cuda.synchronize()
            t = []
            for _ in range(args.reps):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                opt.step()
                e.record()
                e.synchronize()
                t.append(s.elapsed_time(e) * 1e3)
            meds[name].append(statistics.median(t))
    assert torch.isfinite(ar.P).all()
    med = {k: statistics.median(v) for k, v in meds.items()}
    spread = {k: max(v) - min(v) for k, v in meds.items()}
    lines = [f"| arm ({args.arch}: {n} parameters, arena {ar.total} floats) | B / element | median us per repeat | "
             "median of medians us | spread us | TB/s | share of the 6.3 TB/s roof |", "|---|---:|---|---:|---:|---:|---:|"]
    tbs = {}
    for name, _, bpe in arms:
        rate = ""
        if bpe is not None:
            tbs[name] = n * bpe / med[name] / 1e6
            rate = f"{tbs[name]:.2f} | {100 * tbs[name] / ROOF_TBS:.0f} %"
        else:
            rate = " | "
        lines.append(f"| {name} | {bpe if bpe is not None else ''} | {' / '.join(f'{x:.1f}' for x in meds[name])} | "
                     f"{med[name]:.1f} | {spread[name]:.1f} | {rate} |")
    a, b = "adam + refresh", "stock adamw + full refresh"
    margin = max(spread[a], spread[b])
    won = med[b] - med[a] > margin
    lines += ["", f"FlatAdam with its per-step refresh vs the stock route: {med[a]:.1f} us against {med[b]:.1f} us, "
                  f"{med[b] - med[a]:+.1f} us per step; the larger of the two spreads is {margin:.1f} us: "
                  + ("the fused launch wins." if won else "NO CASE for the fusion at this margin.")]
    ok = tbs["lamb clip"] >= tbs["lars"] and tbs["lamb no clip"] >= tbs["lars"]
    lines += [f"FlatLAMB by its byte model: {tbs['lamb clip']:.2f} TB/s with clipping, {tbs['lamb no clip']:.2f} "
              f"TB/s without, FlatLARS {tbs['lars']:.2f} TB/s: " +
              ("not below LARS." if ok else "BELOW LARS's (64, T) grid: the chunk table has no case.")]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
