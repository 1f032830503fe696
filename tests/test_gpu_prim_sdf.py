"""RoundBoxSDF and CapsuleSDF (sdfs.py:46-86) on the HIP path: nrt_sdf_create_round_boxes /
_capsules, the lane-per-ray kernels k_prim_intersect / k_prim_normals / k_prim_occlusion /
k_prim_eval, and the training kernels nrt_prim_smoothmin_*.

* the march, the coarse scan, the normals and the shadow march against the oracle's MarchedSDF
  on the float32 torch restatement of the two formulas (bars of test_bare_mlp_sdf_march_matches_
  oracle: <= 2 hit + step flips of 1,600 rays, t / p / n <= 1e-4 on agreeing hits, throughput
  within 0.1 on >= 99.5 % of the rays);
* bit-equal results across the precision settings (no MLP to lower) and the "prim_march" schedules;
* against the callable path, SDF(sdf=lambda p: restatement(p));
* the smooth-min kernels against float64 autograd (the rule of test_gpu_sphere_smoothmin.py:
  err <= max(1e-5 scale, 4 e32), e32 the float32 torch error);
* training through SDF.intersect (eikonal and throughput terms, an optimiser step and the
  device-side table refresh), and a pathtrace render against oracle.render.

Float32 oracle against float64 oracle, and against the float32 oracle with the primitives summed
in a permuted order, for these inputs (measured on the CPU): 0 hit flips, 0 step flips, t <= 6e-7,
n <= 1e-5, throughput <= 1e-4 -- the reference alone sits far inside every bar."""
import ctypes
import functools
import random

import pytest
import torch
import torch.nn.functional as F

from oracle import pathtracer_ref as R
from oracle import recipes
from tests.helpers import lib_opt as _lib_opt
from tests.report import report
from tests.test_prim_sdf_host import box_ref, cap_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _fp32():
    from neural_raytracing_amd import set_precision
    set_precision("fp32")
    yield
    set_precision("fp32")


def _camera_rays(n, seed, eye=(0.0, 0.1, 1.0), spread=0.9):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor(eye).expand(1, n, n, 1, 3)
    d = F.normalize(torch.cat([torch.rand(1, n, n, 1, 2, generator=g) * spread - spread / 2,
                               -torch.ones(1, n, n, 1, 1)], -1), dim=-1)
    return torch.cat([o, d], -1)


# ---- the parameter sets (CPU tensors, drawn in the reference constructors' order) -------------

def _box_params(n=32, seed=41):
    torch.manual_seed(seed)
    c = 0.3 * torch.rand(n, 3) - 0.15
    b = 0.2 * torch.rand(n, 3)
    radii = 0.2 * torch.rand(n) - 0.1
    tfs = 0.1 * torch.randn(n, 3, 3)
    return dict(kind="box", c=c, b=b, radii=radii, tfs=tfs)


def _cap_params(n, seed):
    torch.manual_seed(seed)
    a = 0.1 * torch.rand(n, 3) - 0.05
    b = 0.1 * torch.rand(n, 3) - 0.05
    r = 0.1 * torch.rand(n) - 0.05
    return dict(kind="cap", a=a, b=b, r=r)


SETS = {
    "box": (lambda: _box_params(32, 41), 0.9),
    "capsule_a": (lambda: _cap_params(64, 105), 3.0),
    "capsule_b": (lambda: _cap_params(8, 49), 0.9),
}


def _restatement(prm, device="cpu", dtype=torch.float32):
    """p -> sdf(p): the torch restatement on copies of the set's tensors."""
    if prm["kind"] == "box":
        c, b, t = (prm[k].to(device, dtype) for k in ("c", "b", "tfs"))
        return lambda p: box_ref(p, c, b, t)
    a, b, r = (prm[k].to(device, dtype) for k in ("a", "b", "r"))
    return lambda p: cap_ref(p, a, b, r)


def _module(prm, requires_grad=False):
    from neural_raytracing_amd.pathtracer.shapes import CapsuleSDF, RoundBoxSDF
    with torch.no_grad():
        if prm["kind"] == "box":
            m = RoundBoxSDF(n=prm["c"].shape[0], device="cpu")
            m.centers.copy_(prm["c"]); m.b.copy_(prm["b"]); m.radii.copy_(prm["radii"])
            m.tfs.copy_(prm["tfs"])
        else:
            m = CapsuleSDF(n=prm["a"].shape[0], device="cpu")
            m.a.copy_(prm["a"]); m.b.copy_(prm["b"]); m.radii.copy_(prm["r"])
    m = m.cuda()
    for q in m.parameters():
        q.requires_grad_(requires_grad)
    return m


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's results for a set, computed once: primary march (jitter of random.seed(12)),
    the scan-free march and the shadow march."""
    make, spread = SETS[name]
    prm = make()
    rays = _camera_rays(40, 3, spread=spread)
    ref = R.MarchedSDF(sdf=_restatement(prm), max_steps=64)
    random.seed(12)
    jit = random.random()
    g = torch.Generator().manual_seed(9)
    max_t = 0.6 + 1.2 * torch.rand(rays.shape[:-1] + (1,), generator=g)
    with torch.no_grad():
        it, hit = ref.intersect(rays, primary=True, jitter=jit)
        it2, hit2 = ref.intersect(rays, primary=False)
        vis = ref.intersect_test(rays, max_t=max_t)
    return dict(prm=prm, rays=rays, it=it, hit=hit, it2=it2, hit2=hit2, max_t=max_t, vis=vis)


def _march_bars(tag, it, hit, rit, rhit, primary):
    hit, rhit = hit.cpu().reshape(-1), rhit.reshape(-1)
    flips = int((hit != rhit).sum())
    t, rt = it.t.cpu().reshape(-1), rit.t.reshape(-1)
    step = (hit & rhit) & ((t - rt).abs() > 1e-4)
    m = (hit & rhit) & ~step
    t_err = (t[m] - rt[m]).abs().max().item()
    n_err = (it.n.cpu().reshape(-1, 3)[m] - rit.n.reshape(-1, 3)[m]).abs().max().item()
    p_err = (it.p.cpu().reshape(-1, 3)[m] - rit.p.reshape(-1, 3)[m]).abs().max().item()
    stats = dict(rays=hit.numel(), hits=int(rhit.sum()), flips=flips, step_flips=int(step.sum()),
                 t_maxabs=t_err, n_maxabs=n_err, p_maxabs=p_err)
    thr = None
    if primary:
        thr = (it.throughput.cpu().reshape(-1) - rit.throughput.reshape(-1)).abs()
        stats.update(thr_maxabs=thr.max().item(), thr_over_0p1=int((thr > 0.1).sum()))
    report(tag, **stats)
    print(tag, stats)
    assert 0.15 < rhit.float().mean() < 0.85
    assert flips + int(step.sum()) <= 2
    assert t_err <= 1e-4 and p_err <= 1e-4 and n_err <= 1e-4
    if primary:
        assert (thr <= 0.1).float().mean() >= 0.995


@pytest.mark.parametrize("name", list(SETS))
def test_prim_march_matches_oracle(name):
    """SDF(sdf=RoundBoxSDF / CapsuleSDF).intersect and intersect_test vs MarchedSDF on the
    restatement (sdfs.py:111-181, 232-249)."""
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.shapes import SDF
    o = _oracle(name)
    shape = SDF(sdf=_module(o["prm"]), max_steps=64)
    rays = o["rays"].cuda()
    _lib.profile_enable(True)
    _lib.profile_reset()
    random.seed(12)
    with torch.no_grad():
        it, hit = shape.intersect(rays, primary=True)
    launches = _lib.profile_read("k_prim_normals")[1]
    _lib.profile_enable(False)
    assert launches == 1, "the new kinds must run on the lane-per-ray kernels"
    _march_bars(f"prim_march[{name}]", it, hit, o["it"], o["hit"], True)
    raw = it.raw_normals
    assert raw is not None and raw.shape == (int(hit.sum()), 3)
    with torch.no_grad():
        it2, hit2 = shape.intersect(rays, primary=False)
    _march_bars(f"prim_march_scan_free[{name}]", it2, hit2, o["it2"], o["hit2"], False)
    with torch.no_grad():
        vis = shape.intersect_test(rays, max_t=o["max_t"].cuda()).cpu()
    diff = int((vis != o["vis"]).sum())
    report(f"prim_occlusion[{name}]", rays=vis.numel(), visible=int(o["vis"].sum()), flips=diff)
    assert diff <= 2


# ---- precision and schedule invariance ----------------------------------------------------------

def _raw_intersect(mod, flat, steps, scan_max_t):
    """nrt_sdf_intersect as SDF.intersect's training call makes it (scan_index requested)."""
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.shapes.sdfs import march_handle
    P, dev = flat.shape[0], flat.device
    h = march_handle(mod)
    t = torch.empty(P, device=dev)
    hit = torch.empty(P, dtype=torch.uint8, device=dev)
    p, n, raw, wi = (torch.empty(P, 3, device=dev) for _ in range(4))
    thr = torch.empty(P, device=dev)
    hit_idx = torch.empty(P, dtype=torch.int32, device=dev)
    hit_count = torch.zeros(1, dtype=torch.int32, device=dev)
    scan_idx = torch.full((P,), -1, dtype=torch.int32, device=dev)
    lib = _lib.load(require_device=True)
    ws = torch.empty(max(lib.nrt_intersect_workspace_bytes(h, P), 1), dtype=torch.uint8, device=dev)
    mp = _lib.MarchParams(steps, 1e-3, 10.0, 1, scan_max_t, _lib.precision_code(),
                          scan_idx.data_ptr())
    _lib.call("nrt_sdf_intersect", h, _lib.ptr(flat), P, ctypes.byref(mp), _lib.ptr(t),
              _lib.ptr(hit), _lib.ptr(p), _lib.ptr(n), _lib.ptr(raw), _lib.ptr(wi), _lib.ptr(thr),
              _lib.ptr(hit_idx), _lib.ptr(hit_count), _lib.ptr(ws), _lib.stream())
    torch.cuda.synchronize()
    assert int(hit_count.item()) == int(hit.sum())
    return dict(t=t, hit=hit, thr=thr, n=n, p=p, raw=raw, scan_idx=scan_idx)


@pytest.mark.parametrize("name", ["box", "capsule_a"])
@pytest.mark.parametrize("P", [1369, 1])  # ragged (21 waves + 25 rays) and a single ray
def test_prim_results_do_not_depend_on_precision_or_schedule(name, P):
    """t, hit, throughput, n and the training call's scan_idx are the same bits at every
    set_precision (FP32 arithmetic throughout: no MLP to lower, no fast exp) and for every
    "prim_march" schedule (2: the LDS copy of the table, 1: constant cache, 0: per-wave kernels)."""
    from neural_raytracing_amd import set_precision
    make, spread = SETS[name]
    mod = _module(make())
    flat = _camera_rays(37, 5, spread=spread).reshape(-1, 6)[:P].contiguous().cuda()
    base = None
    for prec in ("fp32", "fp16", "mixed"):
        for sched in (1, 0, 2):
            set_precision(prec)
            _lib_opt("prim_march", sched)
            with torch.no_grad():
                out = _raw_intersect(mod, flat, 64, 2.2 + 0.37 * (2 / 128))
            if base is None:
                base = out
                assert int(out["scan_idx"].min()) >= 0 and int(out["scan_idx"].max()) <= 128
                if P > 1:
                    assert 0 < int(out["hit"].sum()) < P
                continue
            for k in ("t", "hit", "thr", "n", "p", "raw", "scan_idx"):
                assert torch.equal(out[k], base[k]), (prec, sched, k)
    set_precision("fp32")
    _lib_opt("prim_march", 1)


@pytest.mark.parametrize("name", ["box", "capsule_a"])
def test_prim_eval_grad_and_occlusion_schedules(name):
    """nrt_sdf_eval / nrt_sdf_grad / nrt_sdf_occlusion: the three schedules give the same bits,
    and the values equal the restatement to FP32 rounding."""
    from neural_raytracing_amd.pathtracer.shapes import SDF
    make, spread = SETS[name]
    prm = make()
    mod = _module(prm)
    g = torch.Generator().manual_seed(4)
    p = (0.5 * (torch.rand(3001, 3, generator=g) * 2 - 1))
    rays = _camera_rays(33, 8, spread=spread)
    outs = []
    for sched in (1, 0, 2):
        _lib_opt("prim_march", sched)
        shape = SDF(sdf=mod, max_steps=32)
        with torch.no_grad():
            outs.append((mod(p.cuda()), shape.autograd_diff(p.cuda()),
                         shape.intersect_test(rays.cuda(), max_t=1.5)))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)
    _lib_opt("prim_march", 1)
    want = _restatement(prm, dtype=torch.float64)(p.double())
    assert (outs[0][0].cpu().double() - want).abs().max().item() <= 1e-5
    q = p.double().requires_grad_(True)
    (gw,) = torch.autograd.grad(_restatement(prm, dtype=torch.float64)(q).sum(), q)
    assert (outs[0][1].cpu().double() - gw).abs().max().item() <= 1e-4


# ---- against the callable path -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box", "capsule_a"])
def test_prim_march_matches_the_callable_path(name):
    """SDF(sdf=lambda p: restatement(p)) marches through _intersect_callable (torch evaluations
    between nrt_march_callable_step launches): same hit mask up to 2 rays, t <= 1e-4 on agreeing
    hits."""
    from neural_raytracing_amd.pathtracer.shapes import SDF
    make, spread = SETS[name]
    prm = make()
    rays = _camera_rays(40, 3, spread=spread).cuda()
    f = _restatement(prm, device="cuda")
    random.seed(12)
    with torch.no_grad():
        it, hit = SDF(sdf=_module(prm), max_steps=64).intersect(rays, primary=True)
    random.seed(12)
    with torch.no_grad():
        cit, chit = SDF(sdf=lambda p: f(p), max_steps=64).intersect(rays, primary=True)
    both = (hit & chit).reshape(-1)
    flips = int((hit != chit).sum())
    dt = (it.t.reshape(-1)[both] - cit.t.reshape(-1)[both]).abs().max().item()
    report(f"prim_vs_callable[{name}]", rays=hit.numel(), hits=int(chit.sum()), flips=flips,
           t_maxabs=dt)
    assert int(chit.sum()) > 100
    assert flips <= 2
    assert dt <= 1e-4


def test_prim_table_over_the_limit_marches_as_a_callable():
    """A RoundBoxSDF of 1025 boxes is no HIP SDF kind: SDF.intersect evaluates its forward (the
    torch restatement) between the callable-step kernels; same march as the oracle's."""
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.shapes import SDF, RoundBoxSDF
    from neural_raytracing_amd.pathtracer.shapes.sdfs import is_hip_sdf
    torch.manual_seed(1)
    mod = RoundBoxSDF(n=1025, device="cpu")
    c, b, t = (x.detach().clone() for x in (mod.centers, mod.b, mod.tfs))
    mod = mod.cuda().requires_grad_(False)
    assert not is_hip_sdf(mod)
    rays = _camera_rays(16, 3, spread=2.0)  # 153 of the 256 rays hit
    steps = 32
    _lib.profile_enable(True)
    _lib.profile_reset()
    with torch.no_grad():
        it, hit = SDF(sdf=mod, max_steps=steps).intersect(rays.cuda(), primary=False)
    launches = _lib.profile_read("k_march_step")[1]
    _lib.profile_enable(False)
    assert launches == steps + 1
    with torch.no_grad():
        rit, rhit = R.MarchedSDF(sdf=lambda p: box_ref(p, c, b, t), max_steps=steps).intersect(
            rays, primary=False)
    hit, rhit = hit.cpu().reshape(-1), rhit.reshape(-1)
    dt = (it.t.cpu().reshape(-1) - rit.t.reshape(-1)).abs()
    step = (hit & rhit) & (dt > 1e-4)
    assert 20 < int(rhit.sum()) < rhit.numel()
    assert int((hit != rhit).sum()) + int(step.sum()) <= 2
    assert dt[(hit & rhit) & ~step].max().item() <= 1e-4


# ---- the smooth-min kernels against float64 autograd ---------------------------------------------

def _sm_params(kind, n):
    torch.manual_seed(3 + n)
    if kind == "box":
        c = 0.3 * torch.rand(n, 3) - 0.15
        b = 0.2 * torch.rand(n, 3)
        t = 0.1 * torch.randn(n, 3, 3)
        return c, b, t
    a = 0.1 * torch.rand(n, 3) - 0.05
    b = 0.1 * torch.rand(n, 3) - 0.05
    r = 0.1 * torch.rand(n) - 0.05
    assert float(((b - a) ** 2).sum(-1).min()) > 1e-5
    return a, b, r


def _sm_ref(kind, p, A, B, C):
    """value and create_graph gradient in the input dtype (torch autograd)."""
    q = p.clone().requires_grad_(True)
    v = box_ref(q, A, B, C) if kind == "box" else cap_ref(q, A, B, C)
    (g,) = torch.autograd.grad(v, q, torch.ones_like(v), create_graph=True)
    return v, g


def _keep(kind, p, A, B, C):
    """Points to compare, decided in float64: away from the 1e-4 clamp boundary of the smooth-min
    and, for boxes, from the kinks of the expression (abs, the two clamps, the max), where a
    float32 and a float64 evaluation can take different branches and one point moves a parameter
    gradient by O(1)."""
    p, A, B, C = (x.double() for x in (p, A, B, C))
    if kind == "box":
        T = C + torch.eye(3, dtype=torch.float64).unsqueeze(0)
        u = torch.einsum("ijk,bk->ibj", T, p) - A.unsqueeze(1)
        q = u.abs() - B.unsqueeze(1)
        srt = q.sort(dim=-1).values
        mq = srt[..., 2]
        sd = q.clamp(min=1e-7).norm(dim=-1) + mq.clamp(max=-1e-7)
        kink = (u.abs() < 1e-5).any(-1) | ((q - 1e-7).abs() < 1e-5).any(-1) | \
            ((mq + 1e-7).abs() < 1e-5) | ((srt[..., 2] - srt[..., 1]) < 1e-5)
        kink = kink.any(0)
    else:
        pa = p.unsqueeze(0) - A.unsqueeze(1)
        ba = (B - A).unsqueeze(1)
        h = (pa * ba).sum(-1, keepdim=True) / (ba * ba).sum(-1, keepdim=True).clamp(0, 1)
        sd = (pa - ba * h).norm(dim=-1) - C.unsqueeze(-1)
        kink = torch.zeros(p.shape[0], dtype=torch.bool)
    S = (-16.0 * sd).exp().sum(0)
    edge = (S - 1e-4).abs() <= 1e-3 * 1e-4
    return ~(kink | edge), S < 1e-4


@pytest.mark.parametrize("P", [1, 77, 5000, 20000])  # 20,000: five point slices in the backward
@pytest.mark.parametrize("n", [1, 32, 64])
@pytest.mark.parametrize("kind", ["box", "capsule"])
def test_prim_smoothmin_matches_float64_autograd(kind, n, P):
    from neural_raytracing_amd.pathtracer.differentiable import (PRIM_CAPSULE, PRIM_ROUND_BOX,
                                                                 _PrimSmoothMinFn)
    code = PRIM_ROUND_BOX if kind == "box" else PRIM_CAPSULE
    A, B, C = _sm_params(kind, n)
    g = torch.Generator().manual_seed(P)
    p = 0.6 * (torch.rand(P, 3, generator=g) * 2 - 1)
    p[: P // 10] *= 40.0  # far away: the clamp (no gradient)
    dv = torch.randn(P, generator=g)
    dg = torch.randn(P, 3, generator=g)
    keep, clamped = _keep(kind, p, A, B, C)
    dropped = 1.0 - keep.float().mean().item()
    print(f"smoothmin[{kind},n={n},P={P}] dropped {dropped:.4f}, clamped {int(clamped.sum())}")
    assert dropped <= 0.02
    p, dv, dg, clamped = p[keep].contiguous(), dv[keep], dg[keep], clamped[keep]
    # float64 reference of values and of every parameter gradient of J = dv . v + dg . g
    a64, b64, c64 = (x.double().requires_grad_(True) for x in (A, B, C))
    v64, g64 = _sm_ref(kind, p.double(), a64, b64, c64)
    (dv.double() * v64).sum().add((dg.double() * g64).sum()).backward()
    # fp32 torch, for the tolerance scale
    a32, b32, c32 = (x.clone().requires_grad_(True) for x in (A, B, C))
    v32, g32 = _sm_ref(kind, p, a32, b32, c32)
    (dv * v32).sum().add((dg * g32).sum()).backward()
    # fused
    am, bm, cm = (x.cuda().requires_grad_(True) for x in (A, B, C))
    v, gr = _PrimSmoothMinFn.apply(p.cuda().contiguous(), code, am, bm, cm)
    (dv.cuda() * v).sum().add((dg.cuda() * gr).sum()).backward()

    def close(got, want, ref32, what):
        scale = max(1.0, want.abs().max().item())
        err = (got.detach().cpu().double() - want.detach()).abs().max().item()
        e32 = (ref32.detach().double() - want.detach()).abs().max().item()
        print(f"  {what}: err {err:.3e} e32 {e32:.3e} scale {scale:.3e}")
        assert err <= max(1e-5 * scale, 4 * e32), (what, err, e32, scale)
    close(v, v64, v32, "value")
    close(gr, g64, g32, "grad")
    close(am.grad, a64.grad, a32.grad, "dA")
    close(bm.grad, b64.grad, b32.grad, "dB")
    close(cm.grad, c64.grad, c32.grad, "dC")
    if P >= 77:
        assert clamped.any()
    if clamped.any():  # clamped points: constant value, exactly zero gradient
        assert gr.detach().cpu()[clamped].abs().max().item() == 0.0


@pytest.mark.parametrize("kind", ["box", "capsule"])
def test_prim_smoothmin_value_only_and_grad_only(kind):
    """A loss on one output only (the other's gradient is None / zero): same as float64."""
    from neural_raytracing_amd.pathtracer.differentiable import (PRIM_CAPSULE, PRIM_ROUND_BOX,
                                                                 _PrimSmoothMinFn)
    code = PRIM_ROUND_BOX if kind == "box" else PRIM_CAPSULE
    A, B, C = _sm_params(kind, 32)
    g = torch.Generator().manual_seed(11)
    p = 0.4 * (torch.rand(900, 3, generator=g) * 2 - 1)
    p = p[_keep(kind, p, A, B, C)[0]].contiguous()
    for which in ("value", "grad"):
        a64, b64, c64 = (x.double().requires_grad_(True) for x in (A, B, C))
        v64, g64 = _sm_ref(kind, p.double(), a64, b64, c64)
        (v64.sum() if which == "value" else g64.square().sum()).backward()
        a32, b32, c32 = (x.clone().requires_grad_(True) for x in (A, B, C))
        v32, g32 = _sm_ref(kind, p, a32, b32, c32)
        (v32.sum() if which == "value" else g32.square().sum()).backward()
        am, bm, cm = (x.cuda().requires_grad_(True) for x in (A, B, C))
        v, gr = _PrimSmoothMinFn.apply(p.cuda(), code, am, bm, cm)
        (v.sum() if which == "value" else gr.square().sum()).backward()
        for got, want, r32 in ((am.grad, a64.grad, a32.grad), (bm.grad, b64.grad, b32.grad),
                               (cm.grad, c64.grad, c32.grad)):
            scale = max(1.0, want.abs().max().item())
            err = (got.cpu().double() - want).abs().max().item()
            e32 = (r32.double() - want).abs().max().item()
            assert err <= max(1e-5 * scale, 4 * e32), (which, err, e32, scale)


@pytest.mark.parametrize("kind", ["box", "capsule"])
def test_prim_smoothmin_deterministic_and_empty(kind):
    from neural_raytracing_amd.pathtracer.differentiable import (PRIM_CAPSULE, PRIM_ROUND_BOX,
                                                                 _PrimSmoothMinFn)
    code = PRIM_ROUND_BOX if kind == "box" else PRIM_CAPSULE
    A, B, C = _sm_params(kind, 64)
    p = (0.5 * (torch.rand(20000, 3) * 2 - 1)).cuda()
    dg = torch.randn(20000, 3).cuda()
    outs = []
    for _ in range(2):
        am, bm, cm = (x.cuda().requires_grad_(True) for x in (A, B, C))
        v, gr = _PrimSmoothMinFn.apply(p, code, am, bm, cm)
        (dg * gr).sum().add(v.sum()).backward()
        outs.append((v.detach().clone(), gr.detach().clone(), am.grad.clone(), bm.grad.clone(),
                     cm.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    am, bm, cm = (x.cuda().requires_grad_(True) for x in (A, B, C))
    v, gr = _PrimSmoothMinFn.apply(torch.zeros(0, 3, device="cuda"), code, am, bm, cm)
    assert v.numel() == 0 and gr.shape == (0, 3)
    (v.sum() + gr.sum()).backward()
    assert float(am.grad.abs().max()) == 0.0 and float(cm.grad.abs().max()) == 0.0


# ---- training through SDF.intersect --------------------------------------------------------------

def _box_ref_params(prm, dtype):
    return [prm[k].to(dtype).clone().requires_grad_(True) for k in ("c", "b", "tfs")]


def _close_grads(got, want64, want32, tag):
    for name, g, w64, w32 in zip(("centers", "b", "tfs"), got, want64, want32):
        scale = max(1.0, w64.abs().max().item())
        err = (g.detach().cpu().double() - w64).abs().max().item()
        e32 = (w32.double() - w64).abs().max().item()
        print(f"{tag} d{name}: err {err:.3e} e32 {e32:.3e} scale {scale:.3e}")
        assert err <= max(1e-5 * scale, 4 * e32), (tag, name, err, e32, scale)


def test_prim_training_eikonal_term():
    """((raw_normals.norm - 1)^2).mean() through SDF.intersect backpropagates to centers, b and
    tfs (the double backward of the normal, nrt_prim_smoothmin_backward); against float64 autograd
    of the restatement at the product's own hit points o + t d.  radii gets no gradient."""
    from neural_raytracing_amd.pathtracer.shapes import SDF
    o = _oracle("box")
    mod = _module(o["prm"], requires_grad=True)
    rays = o["rays"]
    random.seed(12)
    it, hit = SDF(sdf=mod, max_steps=64).intersect(rays.cuda(), primary=True)
    raw = it.raw_normals
    assert raw.requires_grad and raw.shape == (int(hit.sum()), 3)
    ((raw.norm(dim=-1) - 1) ** 2).mean().backward()
    assert mod.radii.grad is None
    flat = rays.reshape(-1, 6)
    h = hit.cpu().reshape(-1)
    t = it.t.detach().cpu().reshape(-1)
    ph = (flat[:, :3] + t.unsqueeze(-1) * flat[:, 3:])[h]
    wants = []
    for dtype in (torch.float64, torch.float32):
        c, b, tf = _box_ref_params(o["prm"], dtype)
        q = ph.to(dtype).requires_grad_(True)
        out = box_ref(q, c, b, tf)
        (g,) = torch.autograd.grad(out, q, torch.ones_like(out), create_graph=True)
        ((g.norm(dim=-1) - 1) ** 2).mean().backward()
        wants.append((c.grad, b.grad, tf.grad))
        if dtype == torch.float64:
            r_err = (raw.detach().cpu().double() - g.detach()).abs().max().item()
            assert r_err <= 1e-4, r_err
    _close_grads((mod.centers.grad, mod.b.grad, mod.tfs.grad), wants[0], wants[1], "eikonal")
    assert float(mod.tfs.grad.abs().max()) > 0


def test_prim_training_throughput_term():
    """sum over the rays whose throughput agrees with the float32 oracle's coarse scan (same
    jitter; >= 99.5 % must) of sigmoid(throughput): parameter gradients against the oracle's, held
    to the float64 oracle with the float32 oracle's own error as the scale."""
    from neural_raytracing_amd.pathtracer.shapes import SDF
    o = _oracle("box")
    mod = _module(o["prm"], requires_grad=True)
    rays = o["rays"]
    random.seed(12)
    jit = random.random()
    random.seed(12)
    it, _ = SDF(sdf=mod, max_steps=64).intersect(rays.cuda(), primary=True)
    thr = it.throughput.reshape(-1)
    origin, direction = rays.split(3, dim=-1)
    res = {}
    for dtype in (torch.float32, torch.float64):
        c, b, tf = _box_ref_params(o["prm"], dtype)
        ref = R.MarchedSDF(sdf=lambda p: box_ref(p, c, b, tf), max_steps=64)
        val, _ = ref.coarse_scan(origin.to(dtype), direction.to(dtype), jitter=jit)
        res[dtype] = ((-1000 * val).reshape(-1), (c, b, tf))
    mask = (thr.detach().cpu() - res[torch.float32][0].detach()).abs() <= 0.1
    assert mask.float().mean().item() >= 0.995
    thr[mask.cuda()].sigmoid().sum().backward()
    wants = {}
    for dtype, (val, params) in res.items():
        val[mask].sigmoid().sum().backward()
        wants[dtype] = [q.grad for q in params]
    _close_grads((mod.centers.grad, mod.b.grad, mod.tfs.grad), wants[torch.float64],
                 wants[torch.float32], "throughput")
    assert float(mod.centers.grad.abs().max()) > 0


@pytest.mark.parametrize("name", ["box", "capsule_b"])
def test_prim_optimiser_step_refreshes_the_table(name):
    """After opt.step() the next march sees the new table (nrt_sdf_refresh_round_boxes /
    _capsules, stream-ordered, no host round trip): the training handle is the same object and
    evaluates to the restatement at the new parameters."""
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.shapes import SDF
    from neural_raytracing_amd.pathtracer.shapes.sdfs import train_sdf_handle
    make, spread = SETS[name]
    mod = _module(make(), requires_grad=True)
    shape = SDF(sdf=mod, max_steps=64)
    rays = _camera_rays(24, 3, spread=spread).cuda()
    # Adam: every parameter that takes a gradient moves by about lr, whatever the gradient's scale
    opt = torch.optim.Adam([q for q in mod.parameters()], lr=5e-3)
    random.seed(5)
    it, hit = shape.intersect(rays, primary=True)
    h0 = train_sdf_handle(mod).value
    assert int(hit.sum()) > 20
    loss = ((it.raw_normals.norm(dim=-1) - 1) ** 2).mean() + it.throughput.sigmoid().mean()
    loss.backward()

    def restate(q):
        if name == "box":
            return box_ref(q, mod.centers, mod.b, mod.tfs)
        return cap_ref(q, mod.a, mod.b, mod.radii)
    g = torch.Generator().manual_seed(2)
    p = (0.4 * (torch.rand(777, 3, generator=g) * 2 - 1)).cuda()
    with torch.no_grad():
        old = restate(p)
    opt.step()
    h1 = train_sdf_handle(mod)  # the same handle, its table rewritten on the device
    assert h1.value == h0
    out = torch.empty(777, device="cuda")
    _lib.call("nrt_sdf_eval", h1, _lib.ptr(p), 777, _lib.ptr(out), _lib.precision_code(),
              _lib.stream())
    with torch.no_grad():
        want = restate(p)
        assert (want - old).abs().max().item() > 1e-3  # the step moved the surface
        assert (out - want).abs().max().item() <= 1e-5
        assert (mod(p) - want).abs().max().item() <= 1e-5  # the render handle re-packs too
    # the next march runs on the refreshed table: the same bits as a march of a module built
    # from the new parameters (a host-packed table)
    random.seed(5)
    it2, hit2 = shape.intersect(rays, primary=True)
    assert train_sdf_handle(mod).value == h0
    fresh = type(mod)(n=next(mod.parameters()).shape[0], device="cpu")
    fresh.load_state_dict({k: v.detach().cpu() for k, v in mod.state_dict().items()})
    fresh = fresh.cuda().requires_grad_(False)
    random.seed(5)
    with torch.no_grad():
        it3, hit3 = SDF(sdf=fresh, max_steps=64).intersect(rays, primary=True)
    assert torch.equal(hit2, hit3) and torch.equal(it2.t.detach(), it3.t)


# ---- end to end ----------------------------------------------------------------------------------

@pytest.mark.parametrize("w_isect", [False, True])
def test_prim_render_matches_oracle(w_isect):
    """pathtrace (48x48, four 24x24 tiles, NeRFCamera, Direct, Diffuse, PointLights) over
    SDF(sdf=RoundBoxSDF) against oracle.render on the restatement: <= 1e-4 abs per channel on the
    pixels whose marches agree, at most 2 pixels whose marches do not."""
    import neural_raytracing_amd.pathtracer as pt
    from neural_raytracing_amd.pathtracer.bsdf import Diffuse
    from neural_raytracing_amd.pathtracer.integrators import Direct
    from neural_raytracing_amd.pathtracer.lights import PointLights
    from neural_raytracing_amd.pathtracer.shapes import SDF
    prm = _box_params(32, 41)
    loc = (0.15, 1.4, 0.4)
    size = 48
    c2w = recipes.look_at_c2w((0.0, 0.7, 0.9)).unsqueeze(0)
    focal = recipes.nerf_focal(size)
    oshape = R.MarchedSDF(sdf=_restatement(prm), max_steps=64)
    olight = R.PointLightRef(location=loc, scale=5.0)
    ocam = R.NeRFCameraRef(c2w, focal)
    random.seed(8)
    with torch.no_grad():
        want = R.render(oshape, olight, ocam, R.DirectRef(), R.DiffuseRef(), size=size,
                        chunk_size=24, background=0.0, with_noise=0.0, w_isect=w_isect)
    shape = SDF(sdf=_module(prm), max_steps=64)
    cam = pt.cameras.NeRFCamera(cam_to_world=c2w.cuda(), focal=focal, device="cuda")
    lights = PointLights(location=list(loc), scale=5.0, device="cuda")
    random.seed(8)
    with torch.no_grad():
        got, _ = pt.pathtrace(shape, lights, cam, Direct(), bsdf=Diffuse(device="cuda"), size=size,
                              chunk_size=24, bundle_size=1, background=0, with_noise=0.0,
                              w_isect=w_isect, silent=True)
    got = got.cpu().reshape(want.shape)
    # which pixels' marches agree: the primary march, and with shadow rays the shadow march, of
    # both sides on the oracle's rays
    rays = ocam.sample_positions(R._tile_positions(0, 0, size), size, 0.0, None)
    with torch.no_grad():
        oit, ohit = oshape.intersect(rays, primary=False)
        _, hit = shape.intersect(rays.cuda(), primary=False)
        agree = (hit.cpu() == ohit)
        if w_isect:
            ds, _ = olight.sample_direction(oit, ohit)
            srays = torch.cat([oit.p, ds.d], dim=-1)
            mt = ds.dist.reshape_as(ohit)[..., None]
            ovis = oshape.intersect_test(srays, max_t=mt)
            vis = shape.intersect_test(srays.cuda(), max_t=mt.cuda()).cpu()
            agree = agree & ((vis == ovis) | ~ohit)
    agree = agree.reshape(size, size)
    err = (got - want).abs().amax(-1).reshape(size, size)
    lit = int((want.abs().amax(-1) > 1e-3).sum())
    report(f"prim_render[w_isect={w_isect}]", pixels=err.numel(), lit=lit,
           disagreeing=int((~agree).sum()), maxabs_agreeing=float(err[agree].max()),
           over_1e4=int((err > 1e-4).sum()))
    assert lit > 200
    assert int((~agree).sum()) <= 2
    assert float(err[agree].max()) <= 1e-4
