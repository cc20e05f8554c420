"""FlatAdam / FlatLAMB on the GPU (csrc/kernels/optim.hip imk_adam_flat, imk_lamb_step): the kernels element for
element, the optimizers against their CPU path, and both on ResNet-18 with the EMA, a bucket re-layout and a
checkpoint round trip.

Every elementwise bound is against float64 arithmetic on the same fp32 inputs and the same fp32-rounded scalar
arguments, and each stage takes the kernel's OWN output of the previous stage as its input, so a bound counts only
that stage's roundings. U = 2^-24. The float64 references run on the device (torch float64 ops): they are the
yardstick, not the code under test.

Summation bound: a float sum of non-negative terms whose longest addition chain has L additions, each term itself
carrying k roundings, is within (k + L) U of the exact sum (to first order in U). L is computed below from the
kernels' exported launch geometry (imk_optim_const): for a per-tensor norm, the additions of one thread (one per
element it owns: chunk / threads, plus one for a tail element), 6 wave steps, the waves of a block, and one atomic
per chunk of the tensor; for the gradient norm, 4 per trip of the grid-stride loop, 6 wave steps, the waves of a
block, and one atomic per block.
"""

import math
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _const(which):
    from imagent_amd.ops import _lib
    v = _lib.kernels().imk_optim_const(which)
    assert v > 0
    return v


def _sizes():
    # 3: tail only; 1027: body + tail, several blocks; BIG: one vector group past what one sweep of the capped grid
    # covers (cap blocks x 256 threads x 4 floats), plus 1024 + 3: the grid-stride second trip and the tail both run
    return [3, 1027, _const(3) * 256 * 4 + 1024 + 3]


def _grads(n, gen):
    """Magnitudes spread over 1e-7 .. 10."""
    mag = 10.0 ** (torch.rand(n, device=DEV, generator=gen) * 8.0 - 7.0)
    return torch.randn(n, device=DEV, generator=gen) * mag


def _ratio(err, bound):
    return (err / bound.clamp_min(1e-300)).max().item()


# ------------------------------------------------------------------ 1. adam_flat, element for element
LR, B1, B2, EPS, WD, GS = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.5


def _adam_scalars(t, lr=LR):
    return dict(step_size=_f32(lr / (1.0 - B1 ** t)), rbc2=_f32(1.0 / math.sqrt(1.0 - B2 ** t)), eps=_f32(EPS),
                beta2=_f32(B2), omb1=_f32(1.0 - B1), omb2=_f32(1.0 - B2), wd=_f32(WD), lr_wd=_f32(1.0 - lr * WD))


@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "no_shadow"])
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("decoupled", [0, 1], ids=["l2", "decoupled"])
@pytest.mark.parametrize("size", [0, 1, 2], ids=["n3", "n1027", "big"])
def test_adam_flat_elementwise(size, decoupled, t, shadow):
    from imagent_amd.ops.misc import adam_flat
    n = _sizes()[size]
    gen = torch.Generator(device=DEV).manual_seed(1000 * size + 100 * decoupled + 10 * t + shadow)
    p = torch.randn(n, device=DEV, generator=gen)
    g = _grads(n, gen)
    if t == 1:
        m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    else:
        m = _grads(n, gen) * 0.3
        v = _grads(n, gen).square() * 0.1
    assert (v >= 0).all()
    s = _adam_scalars(t)
    P, G, M, V = p.clone(), g.clone(), m.clone(), v.clone()
    S = torch.full((n,), -7.0, dtype=torch.bfloat16, device=DEV) if shadow else None
    adam_flat(P, G, M, V, S, s["step_size"], s["rbc2"], s["eps"], s["beta2"], s["omb1"], s["omb2"], s["wd"],
              s["lr_wd"], bool(decoupled), GS)
    torch.cuda.synchronize()
    pd, gd, md, vd = p.double(), g.double(), m.double(), v.double()
    if decoupled:
        gp, A, pw = gd * GS, (gd * GS).abs(), pd * s["lr_wd"]
    else:
        gp, A, pw = gd * GS + s["wd"] * pd, (gd * GS).abs() + s["wd"] * pd.abs(), pd
    m_ref = md + s["omb1"] * (gp - md)
    v_ref = s["beta2"] * vd + s["omb2"] * gp * gp
    rm = _ratio((M.double() - m_ref).abs(), U * torch.maximum(md.abs(), A))
    rv = _ratio((V.double() - v_ref).abs(), U * torch.maximum(vd, A * A))
    upd = s["step_size"] * (M.double() / (V.double().sqrt() * s["rbc2"] + s["eps"]))  # from the kernel's m', v'
    rp = _ratio((P.double() - (pw - upd)).abs(), U * torch.maximum(pd.abs(), upd.abs()))
    print(f"n={n} decoupled={decoupled} t={t}: worst ratios to U * scale: m {rm:.3f} (6), v {rv:.3f} (8), "
          f"p {rp:.3f} (12)")
    assert rm <= 6 and rv <= 8 and rp <= 12
    assert not torch.equal(P, p) and (V >= 0).all()
    assert torch.equal(G, g)  # read only
    if shadow:
        assert torch.equal(S, P.to(torch.bfloat16))


@pytest.mark.parametrize("decoupled", [0, 1], ids=["l2", "decoupled"])
def test_adam_flat_keeps_zero_padding_zero(decoupled):
    from imagent_amd.ops.misc import adam_flat
    n = 1027
    P, G, M, V = (torch.zeros(n, device=DEV) for _ in range(4))
    S = torch.full((n,), -7.0, dtype=torch.bfloat16, device=DEV)
    for t in (1, 2):
        s = _adam_scalars(t)
        adam_flat(P, G, M, V, S, s["step_size"], s["rbc2"], s["eps"], s["beta2"], s["omb1"], s["omb2"], s["wd"],
                  s["lr_wd"], bool(decoupled), GS)
    torch.cuda.synchronize()
    for x in (P, G, M, V, S):
        assert (x == 0).all() and torch.isfinite(x.float()).all()


# ------------------------------------------------------------------ 2. lamb_step over a table
def _lamb_arena():
    import torch.nn as nn

    from imagent_amd.models.arena import ParamArena
    from imagent_amd.ops.misc import lamb_chunk
    chunk = lamb_chunk()
    gen = torch.Generator().manual_seed(11)
    shapes = [("v3", (3,)), ("v64", (64,)), ("conv", (5, 3, 3, 3)), ("fc", (1000, 7)),
              ("wide", (1, 3 * chunk + 5)), ("zero", (16, 9))]
    named = []
    for name, shp in shapes:
        w = torch.zeros(shp) if name == "zero" else torch.randn(shp, generator=gen)
        named.append((name, nn.Parameter(w)))
    ar = ParamArena(named, torch.device(DEV), order=[3, 0, 5, 2, 4, 1], with_shadow=True)
    ar.S.copy_(ar.P)
    assert ar.numels[2] % 4 == 3 and ar.numels[4] > 3 * chunk and ar.numels[4] % chunk == 5
    return ar, chunk


def _pad_mask(ar):
    pad = torch.ones(ar.total, dtype=torch.bool, device=DEV)
    for i in range(len(ar.params)):
        pad[ar.offsets[i]:ar.offsets[i] + ar.numels[i]] = False
    assert pad.any()
    return pad


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("mode", ["clipped", "not_clipped", "clip_off"])
def test_lamb_step_over_a_table(mode, t):
    """L (see the module docstring), from imk_optim_const: chunk 4096 and 256 threads give 16 + 1 additions per
    thread, 6 wave steps, 4 waves and ceil(n / 4096) atomics per tensor norm -- 31 for the 12,293-element tensor."""
    from imagent_amd.ops.misc import lamb_step, lamb_table
    ar, chunk = _lamb_arena()
    threads, gcap = _const(1), _const(2)
    T = len(ar.params)
    zi = ar.names.index("zero")
    gen = torch.Generator(device=DEV).manual_seed(20 + t)
    pad = _pad_mask(ar)
    g = _grads(ar.total, gen)
    g[pad] = 0
    ar.flat_slice(g, zi).zero_()
    ar.G.copy_(g)
    m, v = torch.zeros_like(ar.P), torch.zeros_like(ar.P)
    if t > 1:
        m.copy_(_grads(ar.total, gen) * 0.3)
        v.copy_(_grads(ar.total, gen).square() * 0.1)
        for x in (m, v):
            x[pad] = 0
            ar.flat_slice(x, zi).zero_()
    lr, wd, eps = 0.01, _f32(1e-2), _f32(1e-6)
    gnorm = GS * g.double().norm().item()
    mgn = {"clipped": _f32(gnorm / 3.0), "not_clipped": _f32(gnorm * 3.0), "clip_off": 0.0}[mode]
    c1, c2 = _f32(1.0 / (1.0 - B1 ** t)), _f32(1.0 / math.sqrt(1.0 - B2 ** t))
    omb1, omb2, beta2, lr32 = _f32(1.0 - B1), _f32(1.0 - B2), _f32(B2), _f32(lr)
    p0, m0, v0 = ar.P.clone(), m.clone(), v.clone()
    tab = lamb_table(ar, m, v)
    assert tab.nchunks == sum((n + chunk - 1) // chunk for n in ar.numels) and tab.count == T
    lamb_step(tab, lr32, beta2, omb1, omb2, c1, c2, eps, wd, mgn, GS)
    torch.cuda.synchronize()
    norms = tab.norms.double().cpu()
    assert torch.isfinite(norms).all()
    waves = threads // 64

    # the gradient norm and the clip factor
    c = 1.0
    if mode == "clip_off":
        assert norms[2 * T].item() == 0.0  # pass A is not launched
    else:
        n4 = (ar.total + 3) // 4
        grid = min(gcap, (n4 + threads - 1) // threads)
        L = 4 * ((n4 + grid * threads - 1) // (grid * threads)) + 6 + waves + grid
        ref = g.double().square().sum().item()
        r = abs(norms[2 * T].item() - ref) / (U * ref)
        print(f"{mode} t={t}: sum g^2 ratio {r:.3f} ({2 + L})")
        assert r <= 2 + L
        gn = GS * math.sqrt(norms[2 * T].item())
        if gn > mgn:
            c = mgn / gn
        assert (c < 1.0) == (mode == "clipped")
        if mode == "clipped":
            assert abs(c - 1.0 / 3.0) < 1e-4

    worst = dict(m=0.0, v=0.0, w2=0.0, r2=0.0, w=0.0)
    for i, name in enumerate(ar.names):
        n = ar.numels[i]
        adapt = len(ar.shapes[i]) > 1
        wdi = wd if adapt else 0.0
        w, gi = ar.flat_slice(p0, i).double(), ar.flat_slice(g, i).double()
        mi, vi = ar.flat_slice(m0, i).double(), ar.flat_slice(v0, i).double()
        mk, vk = ar.flat_slice(m, i).double(), ar.flat_slice(v, i).double()  # the kernel's m', v'
        gp = gi * GS * c
        A = gp.abs()
        worst["m"] = max(worst["m"], _ratio((mk - (mi + omb1 * (gp - mi))).abs(), U * torch.maximum(mi.abs(), A)))
        worst["v"] = max(worst["v"], _ratio((vk - (beta2 * vi + omb2 * gp * gp)).abs(),
                                            U * torch.maximum(vi, A * A)))
        L = (chunk // threads + 1) + 6 + waves + (n + chunk - 1) // chunk
        q = (mk * c1) / (vk.sqrt() * c2 + eps)
        r = q + wdi * w
        w2, r2 = w.square().sum().item(), r.square().sum().item()
        r2_bound = (q.abs() + wdi * w.abs()).square().sum().item()
        if w2 > 0:
            worst["w2"] = max(worst["w2"], abs(norms[i].item() - w2) / (U * w2) / (2 + L))
            assert abs(norms[i].item() - w2) <= (2 + L) * U * w2, name
        else:
            assert norms[i].item() == 0.0, name
        if r2_bound > 0:
            worst["r2"] = max(worst["r2"], abs(norms[T + i].item() - r2) / (U * r2_bound) / (17 + L))
            assert abs(norms[T + i].item() - r2) <= (17 + L) * U * r2_bound, name
        else:
            assert norms[T + i].item() == 0.0, name
        wn, rn = math.sqrt(norms[i].item()), math.sqrt(norms[T + i].item())
        trust = wn / rn if (adapt and wn > 0 and rn > 0) else 1.0
        assert adapt or (trust == 1.0 and wdi == 0.0)
        step = lr32 * trust
        wk = ar.flat_slice(ar.P, i).double()
        scale = torch.maximum(w.abs(), step * (q.abs() + wdi * w.abs()))
        worst["w"] = max(worst["w"], _ratio((wk - (w - step * r)).abs(), U * scale))
        if name == "zero":
            assert (wk == 0).all() and (mk == 0).all() and (vk == 0).all()
        else:
            assert not torch.equal(wk, w), name
    print(f"{mode} t={t}: worst ratios: m {worst['m']:.3f} (6), v {worst['v']:.3f} (8), w {worst['w']:.3f} (16); "
          f"norms, as a share of their bound: w^2 {worst['w2']:.3f}, r^2 {worst['r2']:.3f}")
    assert worst["m"] <= 6 and worst["v"] <= 8 and worst["w"] <= 16
    for x in (ar.P, m, v):
        assert torch.isfinite(x).all() and (x[pad] == 0).all()
    assert (ar.S[pad] == 0).all()
    assert torch.equal(ar.G, g)  # read only
    assert torch.equal(ar.S, ar.P.to(torch.bfloat16))


# ------------------------------------------------------------------ 3. the optimizers against their CPU path
@pytest.mark.parametrize("kind", ["adam", "adamw", "lamb"])
def test_native_matches_cpu_math(kind):
    import torch.nn as nn

    from imagent_amd.models.arena import ParamArena
    from imagent_amd.train.optim import FlatAdam, FlatLAMB
    torch.manual_seed(3)
    nets = [nn.Sequential(nn.Conv2d(16, 32, 3), nn.BatchNorm2d(32), nn.Flatten(), nn.Linear(32, 10))
            for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    ar_g = ParamArena(list(nets[0].named_parameters()), torch.device(DEV), with_shadow=True)
    ar_c = ParamArena(list(nets[1].named_parameters()), torch.device("cpu"))

    def make(ar, **kw):
        if kind == "lamb":
            return FlatLAMB(ar, lr=0.02, weight_decay=1e-2, max_grad_norm=1.0, **kw)
        return FlatAdam(ar, lr=0.01, weight_decay=1e-2, decoupled=kind == "adamw", **kw)
    og, oc = make(ar_g), make(ar_c, native=False)
    assert og.native and not oc.native
    og.grad_scale = oc.grad_scale = 0.5
    pad = _pad_mask(ar_g).cpu()
    for _ in range(3):
        g = torch.randn(ar_c.total)
        g[pad] = 0
        ar_c.G.copy_(g)
        ar_g.G.copy_(g.to(DEV))
        og.step()
        oc.step()
    assert og.steps == 3
    for x, y in ((ar_g.P, ar_c.P), (og.m, oc.m), (og.v, oc.v)):
        assert torch.allclose(x.cpu(), y, rtol=1e-4, atol=1e-6)
    assert torch.equal(ar_g.S.cpu(), ar_g.P.cpu().to(torch.bfloat16))
    assert torch.equal(ar_g.G.cpu(), ar_c.G)


# ------------------------------------------------------------------ 4. model level
def _by_name(arena, flat):
    return {n: arena.flat_slice(flat, i).clone() for i, n in enumerate(arena.names)}


@pytest.mark.parametrize("kind", ["adamw", "lamb"])
def test_model_three_steps_relayout_ema_and_resume(kind, tmp_path):
    """ResNet-18, 64 x 64, batch 16, deterministic mode, ModelEma(0.5) on the optimizer, a forced bucket re-layout
    between steps 1 and 2 (as tests/test_ema_gpu.py builds it). After every step the gradient arena is copied by name
    into a CPU twin arena in the original order, whose native=False optimizer then steps: P, m, v agree by name.
    The EMA against its float64 recursion (8 U M, as test_ema_gpu.py). Then a checkpoint round trip into a fresh
    optimizer: its fourth step moves P like the fourth step of the un-reloaded optimizer from the same state,
    within what two runs of one step differ by in this mode (<= 1e-5 relative)."""
    from imagent_amd.data.loader import InputTransform
    from imagent_amd.models import resnet
    from imagent_amd.models.arena import ParamArena
    from imagent_amd.models.native import bind_native
    from imagent_amd.ops import conv as cv
    from imagent_amd.parallel.comm import LocalCommunicator
    from imagent_amd.parallel.ddp import DataParallel
    from imagent_amd.train.ema import ModelEma
    from imagent_amd.train.engine import StepRunner, apply_relayout
    from imagent_amd.train.meters import DeviceMetrics
    from imagent_amd.train.optim import FlatAdam, FlatLAMB
    from imagent_amd.utils.checkpoint import load_state, save_state

    def make(ar, **kw):
        if kind == "lamb":
            return FlatLAMB(ar, lr=0.005, weight_decay=1e-2, max_grad_norm=1.0, **kw)
        return FlatAdam(ar, lr=0.001, weight_decay=1e-2, decoupled=True, **kw)
    prev = cv.deterministic()
    cv.set_deterministic(True)
    try:
        torch.manual_seed(41)
        model = resnet.build("resnet18", num_classes=1000)
        st = bind_native(model, DEV)
        ar = st.arena
        ddp = DataParallel(model, ar, LocalCommunicator(), rebuild_buckets=False)
        opt = make(ar, after_step=st.refresh_shadows)
        opt.ema = ema = ModelEma(ar, model, 0.5, refresh=st.refresh_shadows)
        assert opt.native and ema.native
        runner = StepRunner(ddp, opt, DeviceMetrics(DEV), "hip")
        tf = InputTransform("hip", (64, 64), cpad=resnet.ResNet.STEM_CPAD)
        gen = torch.Generator(device=DEV).manual_seed(42)
        u8 = torch.randint(0, 256, (4, 16, 64, 64, 3), dtype=torch.uint8, device=DEV, generator=gen)
        y = torch.randint(0, 1000, (4, 16), device=DEV, generator=gen)
        model.train()

        # the CPU twin: the same parameters by name, in the original order
        twin_named = [(n, torch.nn.Parameter(torch.zeros(ar.shapes[i]))) for i, n in enumerate(ar.names)]
        twin = ParamArena(twin_named, torch.device("cpu"))
        for i, n in enumerate(ar.names):
            twin.flat_slice(twin.P, i).copy_(ar.flat_slice(ar.P, i).cpu())
        topt = make(twin, native=False)

        ref = {n: t.double() for n, t in _by_name(ar, ar.P).items()}
        top = {n: t.abs() for n, t in _by_name(ar, ar.P).items()}
        for step in range(3):
            if step == 1:
                old = list(ar.offsets)
                ddp.pending_relayout = list(reversed(ar.order))
                apply_relayout(ddp, opt, ema, st)
                assert ar.offsets != old and opt.m.numel() == ar.total and ddp.pending_relayout is None
            runner.train_step([(tf(u8[step]), y[step])])
            torch.cuda.synchronize()
            for i, n in enumerate(ar.names):
                twin.flat_slice(twin.G, i).copy_(ar.flat_slice(ar.G, i).cpu())
            topt.step()
            for n, pk in _by_name(ar, ar.P).items():
                ref[n] += 0.5 * (pk.double() - ref[n])
                top[n] = torch.maximum(top[n], pk.abs())
            for flat, tflat, what in ((ar.P, twin.P, "P"), (opt.m, topt.m, "m"), (opt.v, topt.v, "v")):
                for i, n in enumerate(ar.names):
                    a, b = ar.flat_slice(flat, i).cpu(), twin.flat_slice(tflat, i)
                    assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), (step, what, n, (a - b).abs().max().item())
            assert torch.equal(ar.S, ar.P.to(torch.bfloat16))
        assert ema.updates == 3 and opt.steps == 3
        assert opt.m.abs().max() > 0 and opt.v.abs().max() > 0
        worst = 0.0
        for n, ek in _by_name(ar, ema.E).items():
            err = (ek.double() - ref[n]).abs()
            worst = max(worst, _ratio(err, U * top[n].double()))
            assert (err <= 8 * U * top[n].double()).all(), n
        print(f"{kind}: worst |E - ref| / (2^-24 M) = {worst:.3f}")

        # the state after step 3 in a file; the un-reloaded optimizer's fourth step from it
        path = save_state(str(tmp_path / "state.pt"), model, opt, 0, {})
        state_t = [ar.P, opt.m, opt.v, st.save_ws, ema.E, ema.B] + list(model.buffers())
        state = [t.clone() for t in state_t]
        runner.train_step([(tf(u8[3]), y[3])])
        torch.cuda.synchronize()
        upd_twin = ar.P - state[0]
        for dst, src in zip(state_t, state):
            dst.copy_(src)
        ema.updates = 3

        # a fresh optimizer loads the file (the model's weights and buffers with it)
        opt2 = make(ar, after_step=st.refresh_shadows)
        opt2.param_groups[0]["lr"] = 123.0  # the file's holds
        opt2.ema = ema
        load_state(path, model, opt2)
        st.refresh_shadows(full=True)
        torch.cuda.synchronize()
        assert opt2.steps == 3 and opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
        assert torch.equal(ar.P, state[0]) and torch.equal(opt2.m, state[1]) and torch.equal(opt2.v, state[2])
        runner2 = StepRunner(ddp, opt2, DeviceMetrics(DEV), "hip")
        runner2.train_step([(tf(u8[3]), y[3])])
        torch.cuda.synchronize()
        upd = ar.P - state[0]
        e = ((upd - upd_twin).norm() / upd_twin.norm()).item()
        print(f"{kind}: fourth step after the reload vs the un-reloaded one: rel {e:.3g}")
        assert upd_twin.abs().max() > 0 and e <= 1e-5, e
        assert opt2.steps == 4 and ema.updates == 4
    finally:
        cv.set_deterministic(prev)
