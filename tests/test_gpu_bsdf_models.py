"""Phong, Plastic and Bidirectional on the HIP path, and the standalone eval_and_pdf
(nrt_bsdf_eval), against the float64 restatement in tests/test_bsdf_models_host.py.

Inputs are fixed-seed; wi has |wi.z| >= 0.05 with both signs, and Plastic's lobe draw stays 1e-3
away from p_spec (both by construction, asserted), so no front / back or lobe decision sits on a
rounding edge and no ray is left out.  Where a bar is not the project's FP32 bar (1e-4), it is
4 x the error of the same restatement run in float32 on the CPU against float64 on the same
inputs (floor 1e-6): the device's powf / expf / division differ from libm by a few ulp.  (The
library is built without fp contraction, so the device's multiplies and adds round one by one
like torch's element-wise ops; test 4 relies on that.)
"""
import math

import pytest
import torch
import torch.nn.functional as F

import bench
from oracle import pathtracer_ref as R
from tests.helpers import lib_opt as _lib_opt
from tests.report import report
from tests.test_bsdf_models_host import (BidirectionalRef, PhongRef, PlasticRef, interaction)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (80, 80), (300, 17)]
DIFF, SPEC = [0.6, 0.5, 0.7], [0.8, 0.3, 0.1]
PD, PS = [0.5, 0.4, 0.3], [1.0, 0.9, 0.8]
REFL = [0.25, 0.2, 0.7]


@pytest.fixture(autouse=True)
def _fp32():
    from neural_raytracing_amd import set_precision
    set_precision("fp32")
    yield
    set_precision("fp32")


def _dirs(P, g):
    """Unit vectors with |z| in [0.05, 0.95], the sign alternating."""
    z = (0.05 + 0.9 * torch.rand(P, generator=g)) * torch.where(torch.arange(P) % 2 == 0, 1.0, -1.0)
    phi = 2 * math.pi * torch.rand(P, generator=g)
    r = (1 - z * z).sqrt()
    return torch.stack([r * phi.cos(), r * phi.sin(), z], dim=-1)


def _inputs(P, n_hit, seed):
    """float32 values (the device's inputs); the references read them as float64."""
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(P, 3, generator=g) * 2 - 1) * 0.5
    n = F.normalize(torch.randn(P, 3, generator=g), dim=-1)
    wi, wo = _dirs(P, g), _dirs(P, g)
    if P > 1:
        wi = wi[torch.randperm(P, generator=g)]
    hit = torch.randperm(P, generator=g)[:n_hit]
    active = torch.zeros(P, dtype=torch.bool)
    active[hit] = True
    assert (wi[:, 2].abs() >= 0.05 - 1e-6).all()
    assert P == 1 or ((wi[:, 2] > 0).any() and (wi[:, 2] < 0).any())
    return p, n, wi, wo, active, hit


def _it(p, n, wi, dtype):
    return interaction(p.to(dtype), n.to(dtype), wi.to(dtype))


def _f32(v):
    """The float32 value a parameter holds, as a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


# ---- the models, as (HIP object, restatement factory by dtype) ------------------------------------

def _phong(e):
    from neural_raytracing_amd.pathtracer.bsdf import Phong
    b = Phong(diffuse=DIFF, specular=SPEC, device="cuda")
    if e is not None:
        b.shine = torch.tensor(math.log(e - b.min_spec), device="cuda", requires_grad=True)
    shine = float(b.shine.detach())
    return b, lambda dt: PhongRef([_f32(v) for v in DIFF], [_f32(v) for v in SPEC], shine, dtype=dt)


def _plastic():
    from neural_raytracing_amd.pathtracer.bsdf import Plastic
    b = Plastic(diffuse=PD, specular=PS, device="cuda")
    return b, lambda dt: PlasticRef([_f32(v) for v in PD], [_f32(v) for v in PS], dtype=dt)


def _diffuse():
    from neural_raytracing_amd.pathtracer.bsdf import Diffuse
    b = Diffuse(reflectance=REFL, device="cuda")

    def ref(dt):
        r = R.DiffuseRef()
        r.reflectance = torch.tensor([_f32(v) for v in REFL], dtype=dt)
        return r
    return b, ref


def _neural(seed=3):
    from neural_raytracing_amd.pathtracer.bsdf import NeuralBSDF
    torch.manual_seed(seed)
    b = NeuralBSDF(device="cpu")
    b.mlp.to("cuda")

    def ref(dt):
        r = R.NeuralBSDFRef()
        bench._copy_to_oracle(r.mlp, b.mlp)
        r.to(dt)
        r.mlp.basis_p = r.mlp.basis_p.to(dt)
        return r
    return b, ref


def _two_sided(front, back=None):
    from neural_raytracing_amd.pathtracer.bsdf import Bidirectional
    if back is None:
        return Bidirectional(front[0]), lambda dt: BidirectionalRef(front[1](dt))
    return (Bidirectional(front[0], back[0]),
            lambda dt: BidirectionalRef(front[1](dt), back[1](dt)))


MODELS = {
    "phong2": lambda: _phong(2.0),
    "phong12": lambda: _phong(12.0),
    "plastic": _plastic,
    "bi_phong": lambda: _two_sided(_phong(12.0)),
    "bi_diffuse_plastic": lambda: _two_sided(_diffuse(), _plastic()),
    "bi_neural": lambda: _two_sided(_neural()),
}
# which outputs each class zeroes where ~active (bsdfs.py:108-118, 176-189, 271-291, 434-453)
MASKED = {"bi_phong", "bi_diffuse_plastic", "bi_neural"}


def _err(got, want):
    return float(((got.double() - want).abs() / (1 + want.abs())).max())


def _bar(name, yard):
    bar = max(4 * yard, 1e-6)
    assert bar <= 1e-4, (name, yard)  # else the inputs are badly chosen
    return bar


def _ref_eval(ref, p, n, wi, wo, active, dt, masked):
    f, pdf = ref(dt).eval_and_pdf(_it(p, n, wi, dt), wo.to(dt), active if masked else True)
    return f.detach(), pdf.detach()


# ---- 1. each model alone -------------------------------------------------------------------------

@pytest.mark.parametrize("mask", ["bare", "masked"])
@pytest.mark.parametrize("P,n_hit", SHAPES)
@pytest.mark.parametrize("name", list(MODELS))
def test_model_eval_and_pdf_matches_restatement(name, P, n_hit, mask):
    bsdf, ref = MODELS[name]()
    p, n, wi, wo, active, _ = _inputs(P, n_hit, seed=P + 7)
    if mask == "bare":
        active = torch.ones(P, dtype=torch.bool)
    want = _ref_eval(ref, p, n, wi, wo, active, torch.float64, name in MASKED)
    yard = _ref_eval(ref, p, n, wi, wo, active, torch.float32, name in MASKED)
    from neural_raytracing_amd.pathtracer.interaction import SurfaceInteraction
    it = SurfaceInteraction(p=p.cuda(), wi=wi.cuda())
    it.n = n.cuda()
    with torch.no_grad():
        arg = active.cuda() if mask == "masked" else True
        f, pdf = bsdf.eval_and_pdf(it, wo.cuda(), arg)
    yf, yp = _err(yard[0], want[0]), _err(yard[1], want[1])
    ef, ep = _err(f.cpu(), want[0]), _err(pdf.cpu(), want[1])
    report(f"bsdf_model_eval[{name}-{P}-{n_hit}-{mask}]", yard_f=yf, yard_pdf=yp, err_f=ef,
           err_pdf=ep)
    assert ef <= _bar(name, yf), (ef, yf)
    assert ep <= _bar(name, yp), (ep, yp)
    if name in MASKED and mask == "masked" and (~active).any():
        assert (f.cpu()[~active] == 0).all() and (pdf.cpu()[~active] == 0).all()


def test_phong_default_shine_is_finite_and_diffuse_off_the_lobe():
    """shine = 40: exponent 2.4e17, a degenerate lobe; the result is finite and equals the
    diffuse term wherever R.wo < 1."""
    bsdf, ref = _phong(None)
    p, n, wi, wo, _, _ = _inputs(80, 80, seed=5)
    from neural_raytracing_amd.pathtracer.interaction import SurfaceInteraction
    it = SurfaceInteraction(p=p.cuda(), wi=wi.cuda())
    it.n = n.cuda()
    with torch.no_grad():
        f, pdf = bsdf.eval_and_pdf(it, wo.cuda())
    f = f.cpu()
    assert torch.isfinite(f).all() and torch.isfinite(pdf).all()
    from tests.test_bsdf_models_host import reflect
    rd = (reflect(_it(p, n, wi, torch.float64).frame[..., 2], wi.double()) * wo.double()).sum(-1)
    off = rd < 1 - 1e-6
    assert off.any()
    want = wi[:, 2:3].double() * torch.tensor([_f32(v) for v in DIFF], dtype=torch.float64) / math.pi
    assert _err(f[off], want[off]) <= 1e-6


# ---- the mixture of tests 2, 4, 5 ----------------------------------------------------------------

NC = 6  # components of _mixture


def _mixture(seed=11):
    """NeuralBSDF, Diffuse, Phong, Plastic, Bidirectional(Phong), Bidirectional(NeuralBSDF) under a
    spatial-weights MLP: every kind, and through nrt_shade_direct the flipped-feature kernel
    k_ls_flip."""
    from neural_raytracing_amd.pathtracer.bsdf import ComposeSpatialVarying
    parts = [_neural(seed), _diffuse(), _phong(12.0), _plastic(), _two_sided(_phong(2.0)),
             _two_sided(_neural(seed + 5))]
    torch.manual_seed(seed + 1)
    mix = ComposeSpatialVarying([b for b, _ in parts], device="cpu")
    mix.sp_var_fn.to("cuda")

    def ref(dt):
        m = R.SpatialMixBSDF([r(dt) for _, r in parts])
        bench._copy_to_oracle(m.sp_var_fn, mix.sp_var_fn)
        m.sp_var_fn.to(dt)
        m.sp_var_fn.basis_p = m.sp_var_fn.basis_p.to(dt)
        return m
    return mix, ref


LIGHT = dict(location=[0.3, 1.5, 1.0], scale=4.0)  # Le ~ 1 at the points of the unit ball


def _light():
    from neural_raytracing_amd.pathtracer.lights import PointLights
    return PointLights(device="cuda", **LIGHT), R.PointLightRef(**LIGHT)


def _shade(bsdf, lights, p, n, wi, idx, cnt, prec, ring, nc):
    from neural_raytracing_amd import _lib, set_precision
    from neural_raytracing_amd.pathtracer.integrators.integrators import _bsdf_handle, _light_handle
    set_precision(prec)
    _lib_opt("shade_ring", 1 if ring else 0)
    P = p.shape[0]
    rgb = torch.zeros(P, 3, device="cuda")
    wout = torch.zeros(P, nc, device="cuda")
    _lib.profile_enable(True)
    _lib.profile_reset()
    _lib.call("nrt_shade_direct", _bsdf_handle(bsdf), _light_handle(lights), _lib.ptr(p),
              _lib.ptr(n), _lib.ptr(wi), _lib.ptr(idx), _lib.ptr(cnt), P, _lib.ptr(rgb),
              _lib.ptr(wout), _lib.precision_code(), _lib.stream())
    torch.cuda.synchronize()
    counts = {k: _lib.profile_read(k)[1]
              for k in ("k_bsdf32", "k_bsdf3", "k_bsdf16", "k_shade_direct", "k_ls_flip")}
    _lib.profile_enable(False)
    _lib_opt("shade_ring", 1)
    set_precision("fp32")
    return rgb.cpu(), wout.cpu(), counts


def _hit_list(P, hit):
    idx = torch.zeros(P, dtype=torch.int32)
    idx[:hit.numel()] = hit.to(torch.int32)
    return idx.cuda(), torch.tensor([hit.numel()], dtype=torch.int32).cuda()


# ---- 2. mixture through nrt_shade_direct ---------------------------------------------------------

@pytest.mark.parametrize("P,n_hit", SHAPES)
def test_mixture_shading_ring_per_wave_and_oracle(P, n_hit):
    mix, ref = _mixture()
    lights, lref = _light()
    p, n, wi, _, active, hit = _inputs(P, n_hit, seed=P + 1)
    idx, cnt = _hit_list(P, hit)
    dev = (p.cuda(), n.cuda(), wi.cuda(), idx, cnt)
    want, wwant, c0 = _shade(mix, lights, *dev, "fp32", False, NC)
    assert c0["k_shade_direct"] >= 1 and c0["k_ls_flip"] == 0  # the fused kernel flips inline
    for prec, kern in (("fp32", "k_bsdf32"), ("fp32-split", "k_bsdf3")):
        got, wgot, counts = _shade(mix, lights, *dev, prec, True, NC)
        assert counts[kern] >= 1 and counts["k_ls_flip"] >= 1, counts
        d, dw = (got[hit] - want[hit]).abs().max(), (wgot[hit] - wwant[hit]).abs().max()
        report(f"bsdf_mixture_ring_vs_per_wave[{prec}-{P}-{n_hit}]", rgb_maxabs=float(d),
               weights_maxabs=float(dw), rgb_peak=float(want[hit].abs().max()))
        assert d < 1e-5 and dw < 1e-5, (prec, d, dw)
        miss = ~active
        assert not miss.any() or got[miss].abs().max() == 0  # rays off the hit list: untouched
    # FP32 ring result against the oracle's mixture with the restated components
    got, _, _ = _shade(mix, lights, *dev, "fp32", True, NC)
    with torch.no_grad():
        it = _it(p, n, wi, torch.float32)
        ds, le = lref.sample_direction(it, active)
        f, _ = ref(torch.float32).eval_and_pdf(it, it.to_local(ds.d), active)
        oracle = f * le
    d = (got[hit] - oracle[hit]).abs().max()
    report(f"bsdf_mixture_vs_oracle[{P}-{n_hit}]", rgb_maxabs=float(d),
           rgb_peak=float(oracle[hit].abs().max()))
    assert d < 1e-4, d
    # the per-wave kernel (its two-sided NeuralBSDF branch) against the oracle as well
    d = (want[hit] - oracle[hit]).abs().max()
    report(f"bsdf_mixture_per_wave_vs_oracle[{P}-{n_hit}]", rgb_maxabs=float(d))
    assert d < 1e-4, d


# the project's FP16 bar for shading on the program engine (tests/test_gpu_parity.py
# PSNR_FP16_PROGRAM, dB against the oracle on values in [0, 1])
PSNR_FP16_PROGRAM = 93.0


def test_mixture_shading_fp16_program_engine_matches_restatement():
    """The six-component mixture at fp16: k_bsdf16 (and k_ls_flip before it) must run, and the
    result is held to the project's FP16 program-shading bar against the float64 restatement."""
    mix, ref = _mixture()
    lights, lref = _light()
    P, n_hit = 300, 200
    p, n, wi, _, active, hit = _inputs(P, n_hit, seed=17)
    idx, cnt = _hit_list(P, hit)
    got, wgot, counts = _shade(mix, lights, p.cuda(), n.cuda(), wi.cuda(), idx, cnt, "fp16", True, NC)
    assert counts["k_bsdf16"] >= 1 and counts["k_ls_flip"] >= 1, counts
    assert counts["k_shade_direct"] == 0, counts
    for k in ("scale", "intensity", "location", "const", "linear", "square"):
        setattr(lref, k, getattr(lref, k).double())
    with torch.no_grad():
        it = _it(p, n, wi, torch.float64)
        ds, le = lref.sample_direction(it, active)
        f, _ = ref(torch.float64).eval_and_pdf(it, it.to_local(ds.d), active)
        want = (f * le)[hit]
    mse = float(((got[hit].double() - want) ** 2).mean())
    psnr = -10 * math.log10(max(mse, 1e-12))
    dw = float((wgot[hit].double() - it.normalized_weights[hit]).abs().max())
    report("bsdf_mixture_fp16_vs_restatement", psnr=psnr, rgb_peak=float(want.abs().max()),
           rgb_maxabs=float((got[hit].double() - want).abs().max()), weights_maxabs=dw)
    assert 0.1 < float(want.abs().max()) < 2.0
    assert psnr > PSNR_FP16_PROGRAM, psnr


def test_analytic_components_on_the_program_engine_match_restatement():
    """k_bsdf16's analytic arithmetic alone, at f32 accuracy.  A mixture without a weights MLP
    (every weight 1) of one NeuralBSDF and the analytic kinds runs on the program engine at fp16;
    the NeuralBSDF alone runs the same MLP evaluation on the same features.  The difference of the
    two spectra is the analytic components' sum, and the pdf minus the NeuralBSDF's 1 is theirs;
    both are f32 VALU, so they are held to the yardstick bar of test 1 against float64 (the
    subtraction adds an f32 rounding of values below 2, inside the bar's 1e-6 floor)."""
    from neural_raytracing_amd import _lib, set_precision
    from neural_raytracing_amd.pathtracer.bsdf import ComposeSpatialVarying
    from neural_raytracing_amd.pathtracer.interaction import SurfaceInteraction
    neural = _neural(19)
    parts = [_diffuse(), _phong(12.0), _plastic(), _two_sided(_phong(2.0)),
             _two_sided(_diffuse(), _plastic())]
    mix = ComposeSpatialVarying([neural[0]] + [b for b, _ in parts],
                                spatial_varying_fn=torch.nn.Identity(), device="cpu")
    mix.sp_var_fn = None
    P = 80
    p, n, wi, wo, _, _ = _inputs(P, P, seed=18)
    it = SurfaceInteraction(p=p.cuda(), wi=wi.cuda())
    it.n = n.cuda()
    set_precision("fp16")
    _lib.profile_enable(True)
    _lib.profile_reset()
    with torch.no_grad():
        f_mix, pdf_mix = mix.eval_and_pdf(it, wo.cuda())
        f_n, pdf_n = neural[0].eval_and_pdf(it, wo.cuda())
    torch.cuda.synchronize()
    launches = _lib.profile_read("k_bsdf16")[1]
    _lib.profile_enable(False)
    set_precision("fp32")
    assert launches >= 2, launches
    assert (pdf_n == 1).all()
    got_f, got_pdf = (f_mix - f_n).cpu(), (pdf_mix - pdf_n).cpu()

    def analytic(dt):
        rit = _it(p, n, wi, dt)
        outs = [r(dt).eval_and_pdf(rit, wo.to(dt), torch.ones(P, dtype=torch.bool)) for _, r in parts]
        return sum(o[0] for o in outs), sum(o[1] for o in outs)
    want, yard = analytic(torch.float64), analytic(torch.float32)
    yf, yp = _err(yard[0], want[0]), _err(yard[1], want[1])
    ef, ep = _err(got_f, want[0]), _err(got_pdf, want[1])
    report("bsdf_analytic_on_program_engine", yard_f=yf, yard_pdf=yp, err_f=ef, err_pdf=ep)
    assert ef <= _bar("k_bsdf16 f", yf) and ep <= _bar("k_bsdf16 pdf", yp), (ef, yf, ep, yp)


def test_two_sided_mixture_eval_matches_restatement():
    """Bidirectional(ComposeSpatialVarying([...])) lowers to the mixture of two-sided components;
    its eval_and_pdf against BidirectionalRef(SpatialMixBSDF) in float64, with an active mask."""
    from neural_raytracing_amd.pathtracer.bsdf import Bidirectional, ComposeSpatialVarying
    from neural_raytracing_amd.pathtracer.interaction import SurfaceInteraction
    parts = [_neural(23), _diffuse(), _phong(12.0), _plastic()]
    torch.manual_seed(24)
    mix = ComposeSpatialVarying([b for b, _ in parts], device="cpu")
    mix.sp_var_fn.to("cuda")
    two = Bidirectional(mix)

    def ref(dt):
        m = R.SpatialMixBSDF([r(dt) for _, r in parts])
        bench._copy_to_oracle(m.sp_var_fn, mix.sp_var_fn)
        m.sp_var_fn.to(dt)
        m.sp_var_fn.basis_p = m.sp_var_fn.basis_p.to(dt)
        return BidirectionalRef(m)
    P, n_hit = 300, 170
    p, n, wi, wo, active, _ = _inputs(P, n_hit, seed=25)
    it = SurfaceInteraction(p=p.cuda(), wi=wi.cuda())
    it.n = n.cuda()
    with torch.no_grad():
        f, pdf = two.eval_and_pdf(it, wo.cuda(), active.cuda())
        want = ref(torch.float64).eval_and_pdf(_it(p, n, wi, torch.float64), wo.double(), active)
        yard = ref(torch.float32).eval_and_pdf(_it(p, n, wi, torch.float32), wo, active)
    yf, yp = _err(yard[0], want[0]), _err(yard[1], want[1])
    ef, ep = _err(f.cpu(), want[0]), _err(pdf.cpu(), want[1])
    report("bsdf_two_sided_mixture_eval", yard_f=yf, yard_pdf=yp, err_f=ef, err_pdf=ep)
    assert ef <= _bar("two-sided mixture f", yf) and ep <= _bar("two-sided mixture pdf", yp)
    assert (f.cpu()[~active] == 0).all() and (pdf.cpu()[~active] == 0).all()
    below = active & (wi[:, 2] < 0)
    assert below.any() and f.cpu()[below].abs().max() > 0


def test_mixture_eval_sets_normalized_weights_on_every_ray():
    """ComposeSpatialVarying.eval_and_pdf (bsdfs.py:516-520): it.normalized_weights on every ray,
    inactive ones included, from the kernel's own weights output; the spectrum and pdf are zero
    where inactive."""
    from neural_raytracing_amd.pathtracer.interaction import SurfaceInteraction
    mix, ref = _mixture()
    P, n_hit = 300, 17
    p, n, wi, wo, active, _ = _inputs(P, n_hit, seed=27)
    it = SurfaceInteraction(p=p.cuda(), wi=wi.cuda())
    it.n = n.cuda()
    with torch.no_grad():
        f, pdf = mix.eval_and_pdf(it, wo.cuda(), active.cuda())
        rit = _it(p, n, wi, torch.float64)
        want = ref(torch.float64).eval_and_pdf(rit, wo.double(), active)
    assert it.normalized_weights.shape == (P, NC)
    assert _err(it.normalized_weights.cpu(), rit.normalized_weights) <= 1e-4
    assert _err(f.cpu(), want[0]) <= 1e-4 and _err(pdf.cpu(), want[1]) <= 1e-4
    assert (f.cpu()[~active] == 0).all() and (pdf.cpu()[~active] == 0).all()


# ---- 3. no-MLP mixture at every precision --------------------------------------------------------

def test_analytic_mixture_is_the_same_at_every_precision():
    """Phong + Plastic without a spatial MLP: all analytic arithmetic is f32 VALU, so fp32,
    fp32-split, mixed and fp16 agree to 1e-6 absolute.  A mixture without any MLP has no ring or
    program, so every precision runs the per-wave kernel k_shade_direct (asserted); the program
    engine's analytic code is test_analytic_components_on_the_program_engine_match_restatement."""
    from neural_raytracing_amd.pathtracer.bsdf import ComposeSpatialVarying
    mix = ComposeSpatialVarying([_phong(12.0)[0], _plastic()[0]],
                                spatial_varying_fn=torch.nn.Identity(), device="cpu")
    mix.sp_var_fn = None
    lights, _ = _light()
    p, n, wi, _, active, hit = _inputs(300, 17, seed=2)
    idx, cnt = _hit_list(300, hit)
    dev = (p.cuda(), n.cuda(), wi.cuda(), idx, cnt)
    out = {}
    for prec in ("fp32", "fp32-split", "mixed", "fp16"):
        out[prec], _, counts = _shade(mix, lights, *dev, prec, True, 2)
        assert counts["k_shade_direct"] >= 1 and counts["k_bsdf16"] == 0, (prec, counts)
    assert out["fp32"][hit].abs().max() > 1e-3
    for prec, rgb in out.items():
        d = (rgb - out["fp32"]).abs().max()
        report(f"bsdf_analytic_mixture_precisions[{prec}]", rgb_maxabs=float(d))
        assert d <= 1e-6, (prec, d)


# ---- 4. standalone eval equals shading -----------------------------------------------------------

@pytest.mark.parametrize("prec", ["fp32", "fp32-split", "fp16"])
@pytest.mark.parametrize("P,n_hit", SHAPES)
def test_bsdf_eval_equals_the_shading_stage(P, n_hit, prec):
    from neural_raytracing_amd import _lib, set_precision
    from neural_raytracing_amd.pathtracer.differentiable import light_sample
    from neural_raytracing_amd.pathtracer.integrators.integrators import _bsdf_handle
    from neural_raytracing_amd.pathtracer.interaction import SurfaceInteraction
    mix, ref = _mixture()
    lights, lref = _light()
    p, n, wi, _, active, hit = _inputs(P, n_hit, seed=P + 3)
    idx, cnt = _hit_list(P, hit)
    shaded, _, _ = _shade(mix, lights, p.cuda(), n.cuda(), wi.cuda(), idx, cnt, prec, True, NC)
    dp, dn, dwi = p.cuda(), n.cuda(), wi.cuda()  # held: the library reads raw pointers
    # the wo the light stage produces, bit for bit: its direction in the kernel's operation order
    # (point_light: v / max(sqrt((vx vx + vy vy) + vz vz), 1e-6); separate torch element-wise ops
    # round like the kernel's uncontracted f32 ops), then the library's own to_local (nrt_frames
    # maps the negated ray direction through the frame of n).  Le from the package's restatement.
    it = SurfaceInteraction(p=dp, wi=dwi)
    it.set_normals(dn)
    with torch.no_grad():
        _, le, _, _ = light_sample(lights, it, active.cuda())
        v = lights.location.detach().reshape(1, 3).cuda() - dp
        nrm = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).sqrt().clamp(min=1e-6)
        rays = torch.cat([torch.zeros_like(v), -(v / nrm[:, None])], dim=-1).contiguous()
        wo = torch.empty(P, 3, device="cuda")
        _lib.call("nrt_frames", _lib.ptr(rays), _lib.ptr(dn), P, None, _lib.ptr(wo), _lib.stream())
    set_precision(prec)
    spectrum = torch.full((P, 3), 7.0, device="cuda")
    pdf = torch.full((P,), 7.0, device="cuda")
    wout = torch.zeros(P, NC, device="cuda")
    act = active.to(torch.uint8).cuda()
    _lib.call("nrt_bsdf_eval", _bsdf_handle(mix), _lib.ptr(dp), _lib.ptr(dn),
              _lib.ptr(dwi), _lib.ptr(wo), _lib.ptr(act), P, _lib.ptr(spectrum),
              _lib.ptr(pdf), _lib.ptr(wout), _lib.precision_code(), _lib.stream())
    torch.cuda.synchronize()
    set_precision("fp32")
    got = (spectrum * le).cpu()[hit].double()
    ws = shaded[hit].double()
    # 1e-6 relative, per element (a zero must be a zero)
    e = float(((got - ws).abs() / ws.abs().clamp(min=1e-30)).max()) if (ws != 0).any() else 0.0
    report(f"bsdf_eval_vs_shade[{prec}-{P}-{n_hit}]", rel=e, rgb_peak=float(ws.abs().max()),
           rgb_min=float(ws.abs().min()))
    assert ((got - ws).abs() <= 1e-6 * ws.abs()).all(), e
    assert (spectrum.cpu()[~active] == 0).all() and (pdf.cpu()[~active] == 0).all()
    if prec == "fp32":
        with torch.no_grad():
            rit = _it(p, n, wi, torch.float64)
            m = ref(torch.float64)
            _, want_pdf = m.eval_and_pdf(rit, wo.cpu().double(), active)
        assert _err(pdf.cpu()[hit], want_pdf[hit]) <= 1e-4
        assert _err(wout.cpu()[hit], rit.normalized_weights[hit]) <= 1e-4


# ---- 5. render -----------------------------------------------------------------------------------

def test_render_with_the_mixture_matches_oracle():
    """pathtrace_sample, a 48^2 crop of a 128^2 frame across the silhouette of the unit-sphere SDF
    (no MLP march), Direct, a point light and the five-component mixture, against oracle.render
    with the restated components: <= 1e-4 abs per channel where both marches agree."""
    import random
    import neural_raytracing_amd.pathtracer as pt
    from neural_raytracing_amd.pathtracer.integrators import Direct
    from neural_raytracing_amd.pathtracer.shapes import SDF
    from oracle import recipes
    mix, ref = _mixture()
    lights, lref = _light()
    size, crop, c0 = 128, 48, 0
    c2w = recipes.look_at_c2w((0.0, 1.6, 2.0)).unsqueeze(0)
    focal = recipes.nerf_focal(size)
    oshape = R.MarchedSDF(max_steps=64)
    ocam = R.NeRFCameraRef(c2w, focal)
    random.seed(9)
    with torch.no_grad():
        want = R.render(oshape, lref, ocam, R.DirectRef(), ref(torch.float32), size=size,
                        chunk_size=size, background=0.0, with_noise=0.0, crop=(c0, c0, crop))
    shape = SDF(max_steps=64)
    cam = pt.cameras.NeRFCamera(cam_to_world=c2w.cuda(), focal=focal, device="cuda")
    random.seed(9)
    with torch.no_grad():
        got, _ = pt.pathtrace_sample(shape, lights, cam, Direct(), bsdf=mix, size=size,
                                     chunk_size=size, bundle_size=1, crop_size=crop, uv=(c0, c0),
                                     background=0, with_noise=0.0)
    got = got.cpu().reshape(want.shape)
    rays = ocam.sample_positions(R._tile_positions(c0, c0, crop), size, 0.0, None)
    with torch.no_grad():
        _, ohit = oshape.intersect(rays, primary=False)
        _, hit = shape.intersect(rays.cuda(), primary=False)
    agree = (hit.cpu() == ohit).reshape(crop, crop)
    err = (got - want).abs().amax(-1).reshape(crop, crop)
    lit = int((want.abs().amax(-1) > 1e-3).sum())
    report("bsdf_mixture_render", pixels=err.numel(), lit=lit, hits=int(ohit.sum()),
           disagreeing=int((~agree).sum()), maxabs_agreeing=float(err[agree].max()),
           over_1e4=int((err > 1e-4).sum()), rgb_peak=float(want.max()))
    assert 200 < int(ohit.sum()) < crop * crop - 200  # the crop crosses the silhouette
    assert lit > 100
    assert int((~agree).sum()) <= 2
    assert float(err[agree].max()) <= 1e-4


# ---- 6. path bounce ------------------------------------------------------------------------------

def _bounce_mix():
    from neural_raytracing_amd.pathtracer.bsdf import ComposeSpatialVarying
    parts = [_diffuse(), _phong(12.0), _plastic()]
    mix = ComposeSpatialVarying([b for b, _ in parts], spatial_varying_fn=torch.nn.Identity(),
                                device="cpu")
    mix.sp_var_fn = None
    return mix, parts


def _bounce(fn, mix, lights, p, n, wi, active, u_comp, u_sel, u_lobe):
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.integrators.integrators import _bsdf_handle, _light_handle
    lib = _lib.load(require_device=True)
    P = p.shape[0]
    act = active.to(torch.uint8).cuda()
    thr = torch.ones(P, 3, device="cuda")
    res = torch.zeros(P, 3, device="cuda")
    rays = torch.zeros(P, 6, device="cuda")
    ws = torch.empty(lib.nrt_path_workspace_bytes(P), dtype=torch.uint8, device="cuda")
    dev = [t.cuda().contiguous() for t in (p, n, wi, u_comp, u_sel)]
    args = [_bsdf_handle(mix), _light_handle(lights), None, 0, None, 64, 1e-3, _lib.ptr(dev[0]),
            _lib.ptr(dev[1]), _lib.ptr(dev[2]), P, _lib.ptr(act), _lib.ptr(thr), _lib.ptr(res),
            _lib.ptr(dev[3]), _lib.ptr(dev[4])]
    if fn == "nrt_path_bounce_ex":
        ul = u_lobe.cuda().contiguous() if u_lobe is not None else None
        args.append(_lib.ptr(ul))
    args += [_lib.ptr(rays), _lib.ptr(ws), _lib.precision_code(), _lib.stream()]
    rc = getattr(lib, fn)(*args)
    torch.cuda.synchronize()
    return rc, lib.nrt_last_error().decode(), thr.cpu(), rays.cpu(), act.cpu().bool(), res.cpu()


def _bounce_ref(parts, p, n, wi, active, u_comp, u_sel, u_lobe, dt):
    """ComposeSpatialVarying.sample (bsdfs.py:500-513) over Diffuse / Phong / Plastic.sample with
    the selection rule of oracle.bsdf_sample_ref (weights 1: no spatial MLP)."""
    it = _it(p, n, wi, dt)
    wos, specs = [], []
    for c, (_, ref) in enumerate(parts):
        r = ref(dt)
        u2 = u_comp[:, c].to(dt)
        if isinstance(r, PhongRef):
            wo, _, spec = r.sample(it, u2, active)
        elif isinstance(r, PlasticRef):
            wo, _, spec = r.sample(it, u_lobe[:, c].to(dt), u2, active)
        else:  # Diffuse.sample (bsdfs.py:90-106)
            wo = F.normalize(R.square_to_cos_hemisphere(u2), dim=-1)
            spec = r.preproc(r.reflectance).expand(p.shape).clone()
        wos.append(wo)
        specs.append(spec)
    k = torch.ones(p.shape[0], len(parts), dtype=dt)
    cdf = torch.cumsum(k / k.sum(dim=-1, keepdim=True), dim=-1)
    sel = (u_sel.to(dt).unsqueeze(-1) >= cdf).sum(dim=-1).clamp(max=len(parts) - 1)
    pick = sel[:, None, None].expand(p.shape + (1,))
    wo = F.normalize(torch.stack(wos, dim=-1).gather(-1, pick).squeeze(-1), dim=-1)  # :56
    spec = torch.stack(specs, dim=-1).gather(-1, pick).squeeze(-1)
    thr = spec.clamp(min=1e-10)                      # integrators.py:338, throughput 1 before
    d = it.from_local(wo)
    return thr, d, sel


def test_path_bounce_ex_matches_restated_samples():
    from neural_raytracing_amd import _lib
    mix, parts = _bounce_mix()
    lights, _ = _light()
    P = 80
    p, n, wi, _, _, _ = _inputs(P, P, seed=21)
    active = torch.ones(P, dtype=torch.bool)
    g = torch.Generator().manual_seed(22)
    u_comp = torch.rand(P, 3, 2, generator=g)
    # the selection away from the CDF's steps at 1/3, 2/3
    u_sel = (torch.arange(P) % 3 + 0.1 + 0.8 * torch.rand(P, generator=g)) / 3
    # Plastic's lobe draw 1e-3 away from p_spec (float64), both lobes present where wi.z > 0
    # (below the surface p_spec is within 1e-3 of 1, and the draw goes under it)
    ps = parts[2][1](torch.float64).p_spec(wi[:, 2].double())
    assert (ps > 2e-3).all()
    r = torch.rand(P, generator=g).double()
    under = (torch.arange(P) % 4 < 2) | (ps > 1 - 4e-3)
    lobe = torch.where(under, r * (ps - 1e-3), ps + 1e-3 + r * (1 - ps - 2e-3))
    front = wi[:, 2] > 0
    assert (front & under).any() and (front & ~under).any()
    u_lobe = torch.zeros(P, 3)
    u_lobe[:, 2] = lobe.float()
    assert ((u_lobe[:, 2].double() - ps).abs() >= 1e-3 - 1e-7).all()
    want = _bounce_ref(parts, p, n, wi, active, u_comp, u_sel, u_lobe, torch.float64)
    yard = _bounce_ref(parts, p, n, wi, active, u_comp, u_sel, u_lobe, torch.float32)
    assert torch.equal(want[2], yard[2]) and set(want[2].tolist()) == {0, 1, 2}
    rc, err, thr, rays, act, res = _bounce("nrt_path_bounce_ex", mix, lights, p, n, wi, active,
                                           u_comp, u_sel, u_lobe)
    assert rc == 0, err
    y_t, y_d = _err(yard[0], want[0]), _err(yard[1], want[1])
    e_t, e_d = _err(thr, want[0]), _err(rays[:, 3:], want[1])
    report("path_bounce_ex_vs_restatement", yard_thr=y_t, yard_dir=y_d, err_thr=e_t, err_dir=e_d)
    assert e_t <= _bar("thr", y_t) and e_d <= _bar("dir", y_d), (e_t, y_t, e_d, y_d)
    assert torch.equal(rays[:, :3], p)
    assert torch.equal(act, (want[0] > 0).any(dim=-1))
    # the bounce's emitter term is the shading of the same rays (throughput 1)
    idx, cnt = _hit_list(P, torch.arange(P))
    shaded, _, _ = _shade(mix, lights, p.cuda(), n.cuda(), wi.cuda(), idx, cnt, "fp32", True, 3)
    assert _err(res, shaded.double()) <= 1e-6

    # nrt_path_bounce cannot carry the lobe draw
    rc, err, *_ = _bounce("nrt_path_bounce", mix, lights, p, n, wi, active, u_comp, u_sel, None)
    assert rc == -1 and "u_lobe" in err, (rc, err)
    rc, err, *_ = _bounce("nrt_path_bounce_ex", mix, lights, p, n, wi, active, u_comp, u_sel, None)
    assert rc == -1 and "u_lobe" in err, (rc, err)


def test_path_bounce_refuses_bidirectional_and_keeps_old_mixtures_bit_equal():
    from neural_raytracing_amd.pathtracer.bsdf import ComposeSpatialVarying
    lights, _ = _light()
    P = 80
    p, n, wi, _, _, _ = _inputs(P, P, seed=23)
    active = torch.ones(P, dtype=torch.bool)
    g = torch.Generator().manual_seed(24)
    u_comp, u_sel = torch.rand(P, 2, 2, generator=g), torch.rand(P, generator=g)
    two = ComposeSpatialVarying([_diffuse()[0], _two_sided(_phong(12.0))[0]],
                                spatial_varying_fn=torch.nn.Identity(), device="cpu")
    two.sp_var_fn = None
    rc, err, *_ = _bounce("nrt_path_bounce_ex", two, lights, p, n, wi, active, u_comp, u_sel, None)
    assert rc == -2 and "Bidirectional.sample" in err and "combine" in err, (rc, err)
    torch.manual_seed(25)
    old = ComposeSpatialVarying([_neural(26)[0], _diffuse()[0]], device="cpu")
    old.sp_var_fn.to("cuda")
    a = _bounce("nrt_path_bounce", old, lights, p, n, wi, active, u_comp, u_sel, None)
    b = _bounce("nrt_path_bounce_ex", old, lights, p, n, wi, active, u_comp, u_sel, None)
    assert a[0] == 0 and b[0] == 0, (a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y)


def test_path_integrator_with_plastic_replays_its_recorded_draws():
    """Path.sample end to end with a Plastic component (two bounces on the unit sphere): the run
    that draws from the sampler and the run that gets the same numbers through
    uniforms=[(u_comp, u_sel, u_lobe), ...] give the same bits, so the lobe draw reaches
    nrt_path_bounce_ex in the order it was drawn (component order: Diffuse, Phong, Plastic)."""
    from neural_raytracing_amd.pathtracer.integrators import Path
    from neural_raytracing_amd.pathtracer.shapes import SDF
    mix, _ = _bounce_mix()
    lights, _ = _light()
    g = torch.Generator().manual_seed(41)
    P = 80
    o = torch.tensor([0.0, 1.6, 2.0]).expand(P, 3)
    d = F.normalize((torch.rand(P, 3, generator=g) * 2 - 1) * 0.5 - o, dim=-1)
    rays = torch.cat([o, d], dim=-1).cuda()

    class Recorder:
        def __init__(self):
            self.log = []

        def sample(self, shape, device=None):
            t = torch.rand(tuple(shape), generator=g)
            self.log.append(t)
            return t.cuda()

    rec = Recorder()
    integ = Path(max_depth=2)
    with torch.no_grad():
        a, hit, _ = integ.sample(SDF(max_steps=64), rays, mix, lights=lights, sampler=rec)
    assert hit.float().mean() > 0.9 and len(rec.log) % 5 == 0 and len(rec.log) >= 5
    uniforms = []
    for k in range(0, len(rec.log), 5):
        u_dif, u_ph, lobe, u_pl, u_sel = rec.log[k:k + 5]
        assert lobe.shape == (P,) and u_pl.shape == (P, 2)
        u_lobe = torch.zeros(P, 3)
        u_lobe[:, 2] = lobe
        uniforms.append((torch.stack([u_dif, u_ph, u_pl], dim=1), u_sel, u_lobe))
    with torch.no_grad():
        b, _, _ = integ.sample(SDF(max_steps=64), rays, mix, lights=lights, sampler=None,
                               uniforms=uniforms)
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0
    assert torch.equal(a, b)


# ---- 7. gradients --------------------------------------------------------------------------------

def _gradient_case(shade):
    """Phong + Plastic + Bidirectional(Phong) beside one NeuralBSDF under a weights MLP: shade(mix,
    lights, wgt) runs the package under autograd, backpropagates sum(rgb * wgt) and returns the
    (p, n, wi, active) it shaded; the same functional through the float64 restatement gives the
    expected gradients.  max |a - b| / max |b| < 1e-4 per tensor (tests/test_gpu_train.py's bar);
    a reference gradient that is exactly zero must be zero (or absent) here."""
    from neural_raytracing_amd.pathtracer.bsdf import ComposeSpatialVarying
    parts = [_neural(31), _phong(12.0), _plastic(), _two_sided(_phong(2.0))]
    torch.manual_seed(32)
    mix = ComposeSpatialVarying([b for b, _ in parts], device="cpu")
    mix.sp_var_fn.to("cuda")
    lights, lref = _light()
    P = 80
    wgt = torch.rand(P, 3, generator=torch.Generator().manual_seed(35))
    p, n, wi, active = shade(mix, lights, wgt)
    ph, pl, bi = parts[1][0], parts[2][0], parts[3][0].front
    got = {"phong.diffuse": ph.diffuse.grad, "phong.specular": ph.specular.grad,
           "phong.shine": ph.shine.grad, "plastic.diffuse": pl.diffuse.grad,
           "plastic.specular": pl.specular.grad, "bi.diffuse": bi.diffuse.grad,
           "bi.specular": bi.specular.grad, "bi.shine": bi.shine.grad}
    lin = parts[0][0].mlp._linears()
    got.update({f"mlp.w{i}": l.weight.grad for i, l in enumerate(lin)})
    assert isinstance(pl.eta, float)  # a float in the reference: no gradient exists

    dt = torch.float64
    refs = [r(dt) for _, r in parts]
    leaves = {"phong.diffuse": refs[1].diffuse, "phong.specular": refs[1].specular,
              "phong.shine": refs[1].shine, "plastic.diffuse": refs[2].diffuse,
              "plastic.specular": refs[2].specular, "bi.diffuse": refs[3].front.diffuse,
              "bi.specular": refs[3].front.specular, "bi.shine": refs[3].front.shine}
    for t in leaves.values():
        t.requires_grad_(True)
    m = R.SpatialMixBSDF(refs)
    bench._copy_to_oracle(m.sp_var_fn, mix.sp_var_fn)
    m.sp_var_fn.to(dt)
    m.sp_var_fn.basis_p = m.sp_var_fn.basis_p.to(dt)
    for k in ("scale", "intensity", "location", "const", "linear", "square"):
        setattr(lref, k, getattr(lref, k).to(dt))
    rit = _it(p, n, wi, dt)
    ds, le = lref.sample_direction(rit, active)
    f, _ = m.eval_and_pdf(rit, rit.to_local(ds.d), active)
    ((f * le) * wgt.to(dt)).sum().backward()
    rl = [refs[0].mlp.init, *refs[0].mlp.layers, refs[0].mlp.out]
    want = {k: v.grad for k, v in leaves.items()}
    want.update({f"mlp.w{i}": l.weight.grad for i, l in enumerate(rl)})
    # the inputs light every term: no gradient of the test sits below f32's range
    for k in ("phong.diffuse", "phong.specular", "phong.shine", "plastic.diffuse", "bi.diffuse",
              "bi.specular", "bi.shine", "mlp.w0"):
        assert float(want[k].abs().max()) > 1e-6, (k, float(want[k].abs().max()))
    errs = {}
    for k, w in want.items():
        if float(w.abs().max()) == 0:
            # Plastic's specular reaches only the pdf (bsdfs.py:283-287), never the spectrum: the
            # reference gradient is exactly zero, and so must ours be (or absent)
            assert got[k] is None or float(got[k].abs().max()) == 0, k
            continue
        assert got[k] is not None, k
        errs[k] = float((got[k].cpu().double() - w).abs().max() / w.abs().max())
    return errs


def test_direct_gradients_match_float64_autograd():
    """Direct(...).sample under autograd -- its dispatch through needs_grad, on the unit-sphere
    SDF's intersection of 80 rays from all around the sphere -- against float64 autograd at the
    interaction the integrator returns."""
    from neural_raytracing_amd.pathtracer.integrators import Direct
    from neural_raytracing_amd.pathtracer.shapes import SDF

    def shade(mix, lights, wgt):
        g = torch.Generator().manual_seed(34)
        P = wgt.shape[0]
        o = 2.5 * F.normalize(torch.randn(P, 3, generator=g), dim=-1)
        d = F.normalize((torch.rand(P, 3, generator=g) * 2 - 1) * 0.3 - o, dim=-1)
        rays = torch.cat([o, d], dim=-1).cuda()
        rgb, hit, it = Direct().sample(SDF(max_steps=64), rays, mix, lights=lights)
        assert rgb.requires_grad and hit.all()
        (rgb * wgt.cuda()).sum().backward()
        p, n, wi = (t.detach().cpu().reshape(P, 3) for t in (it.p, it.n, it.wi))
        return p, n, wi, hit.cpu().reshape(P)
    for k, e in _gradient_case(shade).items():
        report(f"bsdf_model_gradients_direct[{k}]", rel=e)
        assert e < 1e-4, (k, e)


def test_shading_gradients_on_both_sides_match_float64_autograd():
    """The same through differentiable.direct_sample on the synthetic interactions of the other
    tests, whose wi lies on both sides of the surface: the back side of Bidirectional under
    autograd."""
    from neural_raytracing_amd.pathtracer.differentiable import direct_sample
    from neural_raytracing_amd.pathtracer.interaction import SurfaceInteraction

    def shade(mix, lights, wgt):
        P = wgt.shape[0]
        p, n, wi, _, _, _ = _inputs(P, P, seed=33)
        active = torch.ones(P, dtype=torch.bool)
        it = SurfaceInteraction(p=p.cuda(), wi=wi.cuda())
        it.set_normals(n.cuda())
        rgb = direct_sample(it, active.cuda(), mix, lights, (P,), "cuda")
        (rgb * wgt.cuda()).sum().backward()
        return p, n, wi, active
    for k, e in _gradient_case(shade).items():
        report(f"bsdf_model_gradients[{k}]", rel=e)
        assert e < 1e-4, (k, e)
