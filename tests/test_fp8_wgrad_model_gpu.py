"""--fp8-wgrad inside a real training step (method of test_model_gpu.py::test_fp8_forward_training_step): the seam
``ops.block.conv_wgrad`` is wrapped, and every fp8 weight gradient is checked exactly -- its operands are the
fake-quantised bf16 tensors at their exponents, its result the fp64 weight gradient of those bytes within the kernel
bound of tests/test_wgrad_fp8_gpu.py."""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _fq_bytes(t, e, fmt):
    """Saturating fake-quantisation of a bf16 tensor to fp8 bytes at scale 2^e."""
    mx, dt = (448.0, torch.float8_e4m3fn) if fmt == "e4m3" else (57344.0, torch.float8_e5m2)
    return (t.float() * 2.0 ** -e).clamp(-mx, mx).to(dt).view(torch.uint8)


def _graph_nodes(root):
    seen, todo = set(), [root]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        todo.extend(f for f, _ in n.next_functions)
    return seen


def _setup(arch, fp8_wgrad):
    from imagent_amd.models import resnet
    from imagent_amd.models.native import bind_native
    torch.manual_seed(11)
    model = resnet.build(arch, num_classes=1000)
    st = bind_native(model, DEV, fp8=True, fp8_wgrad=fp8_wgrad)
    g = torch.Generator(device=DEV).manual_seed(12)
    x = (torch.rand(16, 64, 64, 4, device=DEV, generator=g) * 2 - 1).to(torch.bfloat16)
    x[..., 3] = 0
    lab = torch.randint(0, 1000, (16,), device=DEV, generator=g)
    model.train()
    return model, st, x, lab


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_fp8_wgrad_training_steps(arch, monkeypatch):
    import imagent_amd.ops.block as blk
    from test_wgrad_fp8_gpu import _check, _ref
    model, st, x, lab = _setup(arch, True)
    assert st.fp8.wgrad
    ran = []
    real = blk.conv_wgrad

    def checked(mod, dy, xin, xbn=None, fp8=None):
        if fp8 is None:
            return real(mod, dy, xin, xbn=xbn)
        dy8, e_dy, x8, e_x = fp8
        ed, ex = int(e_dy.item()), int(e_x.item())
        assert torch.equal(x8, _fq_bytes(xin, ex, "e4m3")), tuple(mod.weight.shape)
        assert torch.equal(dy8, _fq_bytes(dy, ed, "e5m2")), tuple(mod.weight.shape)
        torch.cuda.synchronize()
        mod.weight.grad.zero_()
        real(mod, dy, xin, xbn=xbn, fp8=fp8)
        torch.cuda.synchronize()
        ref, S, n = _ref(dy8, x8, ed, ex, mod.kh, mod.stride, mod.padding)
        got = mod.weight.grad.permute(0, 2, 3, 1)  # [Co][KH][KW][Ci], the storage order
        _check(got, torch.zeros_like(got), ref, S, n, f"{arch} {tuple(mod.weight.shape)} s{mod.stride}")
        ran.append(mod)

    monkeypatch.setattr(blk, "conv_wgrad", checked)
    st.arena.zero_grad()
    F.cross_entropy(model(x), lab).backward()
    torch.cuda.synchronize()
    assert not ran, "step 1: no gradient scales yet, every weight gradient is bf16"
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    st.refresh_shadows()  # the optimizer-step hook: this step's amax -> exponents, gradient scales exist from now on
    st.arena.zero_grad()
    F.cross_entropy(model(x), lab).backward()
    torch.cuda.synchronize()
    want = [c for c in model.convs() if blk.fp8_wgrad_ok(c)]
    assert want, "no conv qualifies"
    assert len(ran) == len(want) and {id(c) for c in ran} == {id(c) for c in want}, (len(ran), len(want))
    print(f"{arch}: {len(want)} of {len(model.convs())} convs ran the fp8 weight gradient")
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())


def test_fp8_wgrad_off_changes_nothing(monkeypatch):
    """fp8_wgrad=False: the seam never sees fp8 operands and no block keeps a byte tensor for its backward."""
    import imagent_amd.ops.block as blk
    model, st, x, lab = _setup("resnet50", False)
    assert not st.fp8.wgrad
    real = blk.conv_wgrad
    calls = []

    def watched(mod, dy, xin, xbn=None, fp8=None):
        calls.append(fp8 is not None)
        return real(mod, dy, xin, xbn=xbn, fp8=fp8)

    monkeypatch.setattr(blk, "conv_wgrad", watched)
    for step in range(2):
        st.arena.zero_grad()
        loss = F.cross_entropy(model(x), lab)
        nodes = [n for n in _graph_nodes(loss.grad_fn) if type(n).__name__ == "BlockFnBackward"]
        assert len(nodes) == len(list(model.blocks()))
        for n in nodes:
            assert n.wg8 is None
            assert all(t is None or t.dtype != torch.uint8 for t in n.saved_tensors)
        loss.backward()
        torch.cuda.synchronize()
        st.refresh_shadows()
    assert calls and not any(calls)


def test_cli_epoch_with_fp8_wgrad(tmp_path):
    """imagenet.py --dtype fp8 --fp8-wgrad, one short synthetic epoch: exits 0, finite summaries, and the count of
    covered convs is printed once."""
    import math
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(root, "imagenet.py"), "--data", "synthetic", "--arch", "resnet18",
                        "--dtype", "fp8", "--fp8-wgrad", "--kernels", "hip", "--image-size", "64",
                        "--synthetic-train-size", "128", "--synthetic-val-size", "32", "--batch-size", "16",
                        "--num-classes", "10", "--epochs", "1", "--tb-dir", "", "--quiet-banner"],
                       cwd=tmp_path, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-4000:]
    out = r.stdout
    m = re.findall(r"fp8 weight gradients: (\d+) of (\d+) convs", out)
    assert len(m) == 1 and int(m[0][0]) == 10 and int(m[0][1]) == 20, m
    s = re.search(r"Train loss: (\S+) ; Test loss: (\S+)", out)
    assert s and math.isfinite(float(s.group(1))) and math.isfinite(float(s.group(2))), out[-2000:]
