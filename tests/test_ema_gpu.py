"""--model-ema on the GPU: the stand-alone EMA, the swap and the multi-tensor buffer kernel element for element,
then the whole feature on ResNet-18 / ResNet-50. (There is no fused SGD + EMA kernel to test: it measured no faster
than imk_sgd followed by imk_ema_flat, profiles/model_ema.md, and was dropped; the optimizer launch is the unchanged
imk_sgd, which tests/test_kernels_gpu.py covers.)

Exact tests use dyadic inputs: p, E multiples of 2^-6 below 2^10 and omd = 0.25. Then p - E is a multiple of 2^-6
below 2^11 and E + omd (p - E) a multiple of 2^-8 below 2^11: at most 19 significant bits, so every intermediate
is exact with or without FMA contraction and the kernels must equal the CPU computation bit for bit.

Random inputs are held to float64 arithmetic on the same fp32 inputs and the same fp32-rounded omd, within
8 * 2^-24 * max(|e|, |p|) elementwise: e += omd * (p - e) is three fp32 roundings (subtract, multiply, add; two
with the multiply-add contracted) on operands bounded by 2 max, under 5 * 2^-24 * max in all.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

# n = 3: tail only; 1027: body + tail, several blocks; BIG: one element group past what the 8192-block grid covers
# in one sweep (8192 blocks x 256 threads x 4 floats), so the grid-stride loop's second trip runs
BIG = 8192 * 256 * 4 + 1024 + 3
SIZES = [3, 1027, BIG]
U = 2.0 ** -24
OMD = 0.25


def _dyadic(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(-2 ** 16 + 1, 2 ** 16, (n,), generator=g).float() * 2.0 ** -6
    e = torch.randint(-2 ** 16 + 1, 2 ** 16, (n,), generator=g).float() * 2.0 ** -6
    return p, e


def _random(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g), torch.randn(n, generator=g)


@pytest.mark.parametrize("n", SIZES)
def test_ema_flat_exact_and_within_bound(n):
    from imagent_amd.ops.misc import ema_flat
    p, e = _dyadic(n, seed=n + 2)
    E = e.to(DEV)
    Pd = p.to(DEV)
    ema_flat(E, Pd, OMD)
    torch.cuda.synchronize()
    assert torch.equal(E.cpu(), e + OMD * (p - e)) and torch.equal(Pd.cpu(), p)
    omd = torch.tensor(1.0 - 0.9999, dtype=torch.float64).float().item()
    p, e = _random(n, seed=n + 3)
    E = e.to(DEV)
    ema_flat(E, p.to(DEV), omd)
    torch.cuda.synchronize()
    ref = e.double() + omd * (p.double() - e.double())
    err, top = (E.cpu().double() - ref).abs(), torch.maximum(e.abs(), p.abs()).double()
    print(f"n={n}: worst |E - ref| / (2^-24 max) = {(err / (U * top).clamp_min(1e-300)).max().item():.3f}")
    assert (err <= 8 * U * top).all()
    assert not torch.equal(E.cpu(), e)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "no_shadow"])
def test_swap(n, shadow):
    from imagent_amd.ops.misc import ema_swap
    p, e = _random(n, seed=n + 4)
    P, E = p.to(DEV), e.to(DEV)
    S = torch.full((n,), -7.0, dtype=torch.bfloat16, device=DEV) if shadow else None
    ema_swap(P, E, S)
    torch.cuda.synchronize()
    assert torch.equal(P.cpu(), e) and torch.equal(E.cpu(), p)
    if shadow:
        assert torch.equal(S.cpu(), e.to(torch.bfloat16))
    ema_swap(P, E, S)
    torch.cuda.synchronize()
    assert torch.equal(P.cpu(), p) and torch.equal(E.cpu(), e)
    if shadow:
        assert torch.equal(S.cpu(), p.to(torch.bfloat16))


def test_buffer_table_ema_and_swap_leave_neighbours_alone():
    """Tensors of 3, 64 and 2048 floats in one table; guard values around every region of the flat side buffer and
    around every buffer."""
    from imagent_amd.ops.misc import ema_buf_table, ema_bufs
    sizes, gaps, GUARD = [3, 64, 2048], [5, 7, 1, 9], 12345.0
    g = torch.Generator().manual_seed(7)
    offsets, o = [], gaps[0]
    for n, gap in zip(sizes, gaps[1:]):
        offsets.append(o)
        o += n + gap
    flat0 = torch.full((o,), GUARD)
    pool0 = torch.full((o,), -GUARD)  # the buffers: slices of one allocation, guards between them too
    for n, off in zip(sizes, offsets):
        flat0[off:off + n] = torch.randint(-2 ** 16 + 1, 2 ** 16, (n,), generator=g).float() * 2.0 ** -6
        pool0[off:off + n] = torch.randint(-2 ** 16 + 1, 2 ** 16, (n,), generator=g).float() * 2.0 ** -6
    flat, pool = flat0.to(DEV), pool0.to(DEV)
    bufs = [pool[off:off + n] for n, off in zip(sizes, offsets)]
    table = ema_buf_table(bufs, offsets, DEV)
    ema_bufs(table, 3, max(sizes), flat, OMD, swap=False)
    torch.cuda.synchronize()
    want = flat0.clone()
    for n, off in zip(sizes, offsets):
        want[off:off + n] = flat0[off:off + n] + OMD * (pool0[off:off + n] - flat0[off:off + n])
    assert torch.equal(flat.cpu(), want) and torch.equal(pool.cpu(), pool0)
    assert (want != flat0).sum() > 2000
    ema_bufs(table, 3, max(sizes), flat, 0.0, swap=True)
    torch.cuda.synchronize()
    sw_flat, sw_pool = want.clone(), pool0.clone()
    for n, off in zip(sizes, offsets):
        sw_flat[off:off + n] = pool0[off:off + n]
        sw_pool[off:off + n] = want[off:off + n]
    assert torch.equal(flat.cpu(), sw_flat) and torch.equal(pool.cpu(), sw_pool)
    ema_bufs(table, 3, max(sizes), flat, 0.0, swap=True)
    torch.cuda.synchronize()
    assert torch.equal(flat.cpu(), want) and torch.equal(pool.cpu(), pool0)


# ------------------------------------------------------------------ model level
def _by_name(arena, flat):
    return {n: arena.flat_slice(flat, i).clone() for i, n in enumerate(arena.names)}


@pytest.mark.parametrize("arch,relayout", [("resnet18", False), ("resnet50", False), ("resnet18", True)],
                         ids=["resnet18", "resnet50", "resnet18-relayout"])
def test_model_ema_train_swap_eval_restore(arch, relayout, tmp_path):
    """Three training steps with ModelEma(0.5) on the optimizer (64 x 64 images, batch 16, deterministic
    mode, as tests/test_model_gpu.py builds its models); ``relayout``: a forced bucket re-layout between steps 1 and
    2, which the average has to follow.

    * E and the averaged BatchNorm statistics against the float64 recursion over the per-step clones of P and of
      the buffers. With omd = 0.5 the multiply is exact and one update rounds twice, under 2 * 2^-24 * M with M the
      largest magnitude the element took in any clone (E is a convex combination of them); an earlier step's error
      is halved by each later one, so three steps stay under 3.5 * 2^-24 * M, inside the 8 * 2^-24 * M bound.
    * swapped in, the eval logits equal bit for bit those of a freshly bound model that loaded the file save_best
      wrote; swapped back, P, S and every buffer are bit-identical to before.
    * the fourth step after the swap pair updates P like the fourth step of a twin that never swapped: the twin is
      the same step-3 state restored, and the two updates may differ by what two runs of one step differ by in
      this mode, <= 1e-5 relative (the weight gradients' split-K fp32 atomics, test_deterministic_step_reproducible).
    """
    from imagent_amd.data.loader import InputTransform
    from imagent_amd.models import resnet
    from imagent_amd.models.native import bind_native
    from imagent_amd.ops import conv as cv
    from imagent_amd.parallel.comm import LocalCommunicator
    from imagent_amd.parallel.ddp import DataParallel
    from imagent_amd.train.ema import ModelEma
    from imagent_amd.train.engine import StepRunner, apply_relayout
    from imagent_amd.train.meters import DeviceMetrics
    from imagent_amd.train.optim import FlatSGD
    from imagent_amd.utils.checkpoint import load_reference_weights, save_best
    prev = cv.deterministic()
    cv.set_deterministic(True)
    try:
        torch.manual_seed(41)
        model = resnet.build(arch, num_classes=1000)
        st = bind_native(model, DEV)
        ar = st.arena
        ddp = DataParallel(model, ar, LocalCommunicator(), rebuild_buckets=False)
        opt = FlatSGD(ar, lr=0.05, momentum=0.9, weight_decay=1e-4, after_step=st.refresh_shadows)
        opt.ema = ema = ModelEma(ar, model, 0.5, refresh=st.refresh_shadows)
        assert ema.native and ema.omd() == 0.5
        runner = StepRunner(ddp, opt, DeviceMetrics(DEV), "hip")
        tf = InputTransform("hip", (64, 64), cpad=resnet.ResNet.STEM_CPAD)
        g = torch.Generator(device=DEV).manual_seed(42)
        u8 = torch.randint(0, 256, (4, 16, 64, 64, 3), dtype=torch.uint8, device=DEV, generator=g)
        y = torch.randint(0, 1000, (4, 16), device=DEV, generator=g)
        fbufs = {n: b for n, b in model.named_buffers() if b.dtype == torch.float32}
        assert ema.buf_names == list(fbufs) and len(fbufs) == 2 * len(model.batchnorms())
        model.train()

        ref = {n: t.double() for n, t in _by_name(ar, ar.P).items()}
        top = {n: t.abs() for n, t in _by_name(ar, ar.P).items()}
        bref = {n: b.detach().double().reshape(-1) for n, b in fbufs.items()}
        btop = {n: b.detach().abs().reshape(-1) for n, b in fbufs.items()}
        for step in range(3):
            if relayout and step == 1:
                old = list(ar.offsets)
                ddp.pending_relayout = list(reversed(ar.order))
                apply_relayout(ddp, opt, ema, st)
                assert ar.offsets != old and ema.E.numel() == ar.total and ddp.pending_relayout is None
            runner.train_step([(tf(u8[step]), y[step])])
            torch.cuda.synchronize()
            for n, pk in _by_name(ar, ar.P).items():
                ref[n] += 0.5 * (pk.double() - ref[n])
                top[n] = torch.maximum(top[n], pk.abs())
            for n, b in fbufs.items():
                bref[n] += 0.5 * (b.double().reshape(-1) - bref[n])
                btop[n] = torch.maximum(btop[n], b.abs().reshape(-1))
        assert ema.updates == 3
        worst = 0.0
        for n, ek in _by_name(ar, ema.E).items():
            err = (ek.double() - ref[n]).abs()
            worst = max(worst, (err / (U * top[n].double()).clamp_min(1e-300)).max().item())
            assert (err <= 8 * U * top[n].double()).all(), n
        for i, n in enumerate(ema.buf_names):
            err = (ema._buf_slice(i).double() - bref[n]).abs()
            worst = max(worst, (err / (U * btop[n].double()).clamp_min(1e-300)).max().item())
            assert (err <= 8 * U * btop[n].double()).all(), n
        print(f"{arch}: worst |E - ref| / (2^-24 M) = {worst:.3f}")
        assert not torch.equal(ema.E, ar.P)

        # the state after step 3, and the twin's fourth step from it
        state_t = [ar.P, opt.buf, st.save_ws, ema.E, ema.B] + list(model.buffers())
        state = [t.clone() for t in state_t]
        S3 = ar.S.clone()
        runner.train_step([(tf(u8[3]), y[3])])
        torch.cuda.synchronize()
        upd_twin = ar.P - state[0]
        for dst, src in zip(state_t, state):
            dst.copy_(src)
        st.refresh_shadows(full=True)
        ema.updates = 3
        torch.cuda.synchronize()
        assert torch.equal(ar.S, S3)

        # the average swapped in: the eval forward, and the file save_best writes
        x = tf(u8[3])
        ema.swap()
        assert torch.equal(ar.P, state[3]) and torch.equal(ema.E, state[0])
        assert torch.equal(ar.S, state[3].to(torch.bfloat16))
        for i, n in enumerate(ema.buf_names):
            assert torch.equal(fbufs[n].reshape(-1), state[4][ema.buf_offsets[i]:][:fbufs[n].numel()]), n
        model.eval()
        with torch.no_grad():
            logits = model(x).float().clone()
        path = save_best(model, arch, str(tmp_path), name=f"imagenet_FR_{arch}_ema.pt")
        model.train()
        ema.swap()
        torch.cuda.synchronize()
        for t, t0 in zip(state_t, state):
            assert torch.equal(t, t0)
        assert torch.equal(ar.S, S3)

        model2 = resnet.build(arch, num_classes=1000)
        load_reference_weights(model2, path)
        bind_native(model2, DEV)
        model2.eval()
        with torch.no_grad():
            logits2 = model2(x).float()
        torch.cuda.synchronize()
        assert torch.isfinite(logits).all() and logits.abs().max() > 0
        assert torch.equal(logits, logits2)

        # the fourth step, after the swap pair
        runner.train_step([(tf(u8[3]), y[3])])
        torch.cuda.synchronize()
        upd = ar.P - state[0]
        e = ((upd - upd_twin).norm() / upd_twin.norm()).item()
        print(f"{arch}: fourth step after the swap pair vs the twin: rel {e:.3g}")
        assert upd_twin.abs().max() > 0 and e <= 1e-5, e
        assert ema.updates == 4
    finally:
        cv.set_deterministic(prev)
