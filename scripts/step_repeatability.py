"""How far one training step repeats: the same ResNet-50 step three times from the same state and batch in one
process (default path: float-atomic BatchNorm statistics), loss / gradient / BN-statistics differences and the
per-parameter gradient differences (largest and smallest). Backs bench.py --dump-outputs' choice of arrays
(profiles/bench_dump_repeatability.md).

    python scripts/step_repeatability.py [BATCH]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from imagent_amd.models import resnet
from imagent_amd.models.native import bind_native
from imagent_amd.ops.misc import XentFn, normalize_u8
from imagent_amd.train.optim import FlatSGD

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
dev = torch.device("cuda:0")
torch.manual_seed(0)
m = resnet.resnet50()
order = list(reversed(range(len(list(m.parameters())))))
st = bind_native(m, dev, order)
st.refresh_shadows(full=True)
ar = st.arena
opt = FlatSGD(ar, lr=0.1, momentum=0.9, weight_decay=1e-4, after_step=st.refresh_shadows)
g = torch.Generator(device="cpu")
g.manual_seed(0)
img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=g).to(dev)
y = torch.randint(0, 1000, (B,), generator=g).to(dev)
met = torch.zeros(4, device=dev)
m.train()
state = [ar.P] + list(m.buffers()) + [x.work.save for x in m.modules()
                                       if getattr(getattr(x, "work", None), "save", None) is not None]
print("state tensors", len(state), "bn saves", len(state) - 1 - len(list(m.buffers())))
state0 = [t.clone() for t in state]
outs = []
for rep in range(3):
    torch._foreach_copy_(state, state0)
    st.refresh_shadows(full=True)
    if opt.buf is not None:
        opt.buf.zero_()
    met.zero_()
    opt.zero_grad()
    loss = XentFn.apply(m(normalize_u8(img, (224, 224), 4, (0.5,) * 3, (0.5,) * 3)), y, met, 0.0)
    loss.backward()
    torch.cuda.synchronize()
    G = ar.G.clone()
    opt.step()
    torch.cuda.synchronize()
    outs.append((G, loss.item(), torch.cat([b.reshape(-1).float() for n, b in m.named_buffers() if "running" in n])))
    print("rep", rep, "loss", loss.item(), "gnorm", G.norm().item())
for r in (1, 2):
    G0, G1 = outs[0][0], outs[r][0]
    print(f"rep0 vs rep{r}: grad rel {((G0 - G1).norm() / G0.norm()).item():.3e} bn stats rel "
          f"{((outs[0][2] - outs[r][2]).norm() / outs[0][2].norm()).item():.3e}")
rows = []
for i, n in enumerate(ar.names):
    a, b = ar.flat_slice(outs[0][0], i), ar.flat_slice(outs[1][0], i)
    rows.append(((a - b).norm().item() / max(a.norm().item(), 1e-30), a.norm().item(), n))
rows.sort(reverse=True)
for r in rows[:12] + rows[-5:]:
    print(f"{r[0]:.3e} |g|={r[1]:.3e} {r[2]}")
