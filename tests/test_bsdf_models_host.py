"""Phong, Plastic and Bidirectional (bsdf/bsdfs.py:121-325, 404-453) restated in torch, and the
host side of their HIP path.

The restatement below is the expected value of the GPU tests (tests/test_gpu_bsdf_models.py): the
three classes line by line, dtype-generic so it runs in float64 (the reference value) and in
float32 (the yardstick for f32 rounding).  Each class has ``joint_eval_pdf(it, wo, active)`` and
so plugs into the oracle's ``SpatialMixBSDF``, ``DirectRef`` and ``render``.  This file checks the
restatement on known answers, then the handle packing, ``nrt_bsdf_create_ex``'s validation and
Path's draw order, none of which needs a device.
"""
import ctypes
import math

import pytest
import torch

from oracle import pathtracer_ref as R


# ---- restatement ---------------------------------------------------------------------------------

def reflect(n, v):
    """bsdfs.py:121-123."""
    return 2 * (n * v).sum(keepdim=True, dim=-1) * n - v


def invert_z(xyz):
    """bsdfs.py:404-406."""
    x, y, z = xyz.split(1, dim=-1)
    return torch.cat([x, y, -z], dim=-1)


def cos_hemisphere_pdf(d):
    """warps.py:52."""
    return d[..., 2] / math.pi


def fresnel(cos_t, eta: float):
    """bsdfs.py:193-218 -> r."""
    def fnma(x, y, z): return -x * y + z          # :194
    def fma(x, y, z): return x * y + z            # :195
    out_mask = cos_t >= 0                         # :196
    inv_eta = 1 / eta                             # :197
    e, ie = torch.tensor(eta, dtype=cos_t.dtype), torch.tensor(inv_eta, dtype=cos_t.dtype)
    eta_it = torch.where(out_mask, e, ie)         # :198
    eta_ti = torch.where(out_mask, ie, e)         # :199
    cos_tt_sqr = fnma(fnma(cos_t, cos_t, 1), eta_ti * eta_ti, 1)  # :200
    cos_t_abs = cos_t.abs()                       # :201
    cos_tt_abs = cos_tt_sqr.clamp(min=1e-10).sqrt()  # :202
    idx_match = eta == 1                          # :204
    special_case = (cos_t_abs == 0) | idx_match   # :205
    a_s = fnma(eta_it, cos_tt_abs, cos_t_abs) / fma(eta_it, cos_tt_abs, cos_t_abs)  # :208-209
    a_p = fnma(eta_it, cos_t_abs, cos_tt_abs) / fma(eta_it, cos_t_abs, cos_tt_abs)  # :210-211
    r = 0.5 * (a_s.square() + a_p.square())       # :213
    r = torch.where(special_case, torch.full_like(r, 0.0 if idx_match else 1.0), r)  # :214
    return r


def fresnel_diff_refl(eta):
    """bsdfs.py:220-235."""
    if eta < 1:
        return -1.4399 * (eta * eta) + 0.7099 * eta + 0.6681 + 0.0636 / eta
    inv_eta = 1 / eta
    inv_eta_2 = inv_eta * inv_eta
    inv_eta_3 = inv_eta_2 * inv_eta
    inv_eta_4 = inv_eta_3 * inv_eta
    inv_eta_5 = inv_eta_4 * inv_eta
    return 0.919317 - 3.4793 * inv_eta + 6.75335 * inv_eta_2 - 7.80989 * inv_eta_3 \
        + 4.98554 * inv_eta_4 - 1.36881 * inv_eta_5


class _Joint:
    def joint_eval_pdf(self, it, wo, active=True):
        """bsdfs.py:68-70."""
        f, pdf = self.eval_and_pdf(it, wo, active)
        return torch.cat([f, pdf.reshape(f.shape[:-1] + (1,))], dim=-1)


class PhongRef(_Joint, torch.nn.Module):
    """bsdfs.py:132-189; diffuse, specular, shine are tensors of the working dtype."""

    def __init__(self, diffuse, specular, shine, min_spec=1, dtype=torch.float64):
        super().__init__()
        self.diffuse = torch.tensor(list(diffuse), dtype=dtype)
        self.specular = torch.tensor(list(specular), dtype=dtype)
        self.shine = torch.tensor(float(shine), dtype=dtype)
        self.min_spec = min_spec

    def eval_and_pdf(self, it, wo, active=True):
        cos_theta_i = it.wi[..., 2]                                           # :177
        R_ = reflect(it.frame[..., 2], it.wi)                                 # :180
        spectral = (R_ * wo).sum(dim=-1).clamp(min=1e-20).pow(self.min_spec + self.shine.exp())
        spectrum = cos_theta_i.unsqueeze(-1) * self.diffuse / math.pi + \
            spectral.unsqueeze(-1) * self.specular / math.pi                  # :182-183
        return spectrum, cos_hemisphere_pdf(wo)                               # :185

    def sample(self, it, u2, active):
        """:155-175 with the (.., 2) draw injected -> (wo, pdf, spectrum)."""
        cos_theta_i = it.wi[..., 2]
        active = (cos_theta_i > 0) & active                                   # :160
        wo = R.square_to_cos_hemisphere(u2)                                   # :163
        pdf = cos_hemisphere_pdf(wo)                                          # :164
        active = (wo[..., 2] > 0) & active                                    # :169
        R_ = reflect(it.frame[..., 2], it.wi)                                 # :170
        spectral = (R_ * wo).sum(dim=-1).clamp(min=1e-20).pow(self.min_spec + self.shine.exp())
        spectrum = cos_theta_i.unsqueeze(-1) * self.diffuse / math.pi + \
            spectral.unsqueeze(-1) * self.specular / math.pi
        spectrum = torch.where(((~active) | (pdf <= 0)).unsqueeze(-1),
                               torch.zeros_like(spectrum), spectrum)          # :174
        return wo, pdf, spectrum


class PlasticRef(_Joint, torch.nn.Module):
    """bsdfs.py:238-325."""

    def __init__(self, diffuse, specular, int_ior=1.49, ext_ior=1.000277, dtype=torch.float64):
        super().__init__()
        self.diffuse = torch.tensor(list(diffuse), dtype=dtype)
        self.specular = torch.tensor(list(specular), dtype=dtype)
        self.eta = int_ior / ext_ior                                          # :254
        self.inv_eta_2 = 1 / (self.eta * self.eta)                            # :256
        self.fdr_int = fresnel_diff_refl(1 / self.eta)                        # :258
        self.fdr_ext = fresnel_diff_refl(self.eta)                            # :259

    def spec_sample_weight(self):
        d, s = self.diffuse.mean(), self.specular.mean()                      # :263-264
        return s / (d + s)

    def lobe_probs(self, cos_theta_i):
        """(prob_specular, prob_diffuse) as eval_and_pdf normalises them (:283-286)."""
        f_i = fresnel(cos_theta_i, self.eta)
        ssw = self.spec_sample_weight()
        prob_specular = ssw * f_i
        prob_diffuse = (1 - f_i) * (1 - ssw)
        tot = prob_specular + prob_diffuse
        return prob_specular / tot, prob_diffuse / tot

    def eval_and_pdf(self, it, wo, active=True):
        f_i = fresnel(it.wi[..., 2], self.eta)                                # :275
        f_o = fresnel(wo[..., 2], self.eta)                                   # :276
        pdf = cos_hemisphere_pdf(wo)                                          # :277
        spectrum = (self.diffuse.expand_as(it.p) / (1 - self.fdr_int)) \
            * self.inv_eta_2 * (pdf * (1 - f_i) * (1 - f_o)).unsqueeze(-1)    # :278-279
        ssw = self.spec_sample_weight()
        prob_specular = ssw * f_i
        prob_diffuse = (1 - f_i) * (1 - ssw)
        prob_diffuse = prob_diffuse / (prob_specular + prob_diffuse)          # :286
        return spectrum, pdf * prob_diffuse

    def p_spec(self, cos_theta_i):
        f_i = fresnel(cos_theta_i, self.eta)
        ssw = self.spec_sample_weight()
        p_spec = f_i * ssw
        p_diff = (1 - f_i) * (1 - ssw)
        return p_spec / (p_spec + p_diff)                                     # :300-302

    def sample(self, it, u_lobe, u2, active):
        """:292-325 with both draws injected -> (wo, pdf, spectrum)."""
        cos_theta_i = it.wi[..., 2]
        active = (cos_theta_i > 0) & active                                   # :297
        f_i = fresnel(cos_theta_i, self.eta)
        p_spec = self.p_spec(cos_theta_i)
        p_diff = 1 - p_spec                                                   # :303
        sample_spec = active & (u_lobe < p_spec)                              # :304
        wo = torch.where(sample_spec.unsqueeze(-1), reflect(it.frame[..., 2], it.wi),
                         R.square_to_cos_hemisphere(u2))                      # :306-310
        pdf = torch.where(sample_spec, p_spec, p_diff * cos_hemisphere_pdf(wo)).clamp(min=1e-10)
        f_o = fresnel(wo[..., 2], self.eta)                                   # :316
        spectrum = torch.where(
            sample_spec.unsqueeze(-1),
            self.specular * (f_i / pdf).unsqueeze(-1),
            self.diffuse.expand_as(it.p) / (1 - self.fdr_int) * pdf.unsqueeze(-1) * self.inv_eta_2
            * (1 - f_i.unsqueeze(-1)) * (1 - f_o.unsqueeze(-1)))              # :317-323
        return wo, pdf, spectrum


class BidirectionalRef(_Joint, torch.nn.Module):
    """bsdfs.py:409-453 (eval_and_pdf; sample fails in the reference, :432)."""

    def __init__(self, front, back=None):
        super().__init__()
        self.front = front
        self.back = front if back is None else back

    def eval_and_pdf(self, it, wo, active=True):
        cos_theta_i = it.wi[..., 2]
        if isinstance(active, bool):
            active = torch.full(cos_theta_i.shape, active)
        front = (cos_theta_i > 0) & active                                    # :437
        back = (cos_theta_i < 0) & active                                     # :438
        front_eval, front_pdf = self.front.eval_and_pdf(it, wo, front)        # :440
        og_wi = it.wi
        it.wi = invert_z(og_wi)                                               # :443
        back_eval, back_pdf = self.back.eval_and_pdf(it, invert_z(wo), back)  # :444
        it.wi = og_wi
        spectrum = torch.where(front.unsqueeze(-1), front_eval,
                               torch.where(back.unsqueeze(-1), back_eval,
                                           torch.zeros_like(back_eval)))      # :447-448
        pdf = torch.where(front, front_pdf,
                          torch.where(back, back_pdf, torch.zeros_like(back_pdf)))
        return spectrum, pdf


def interaction(p, n, wi):
    it = R.Interaction(p)
    it.set_normals(n)
    it.wi = wi
    return it


# ---- known answers -------------------------------------------------------------------------------

def _z(dtype=torch.float64):
    return torch.tensor([[0.0, 0.0, 1.0]], dtype=dtype)


def test_phong_at_normal_incidence():
    """n = wi = wo = z: R = z, R.wo = 1, 1^e = 1 -> f = (diffuse + specular) / pi."""
    d, s = [0.6, 0.5, 0.7], [0.8, 0.3, 0.1]
    for e in (2.0, 12.0):
        ph = PhongRef(d, s, shine=math.log(e - 1))
        f, pdf = ph.eval_and_pdf(interaction(_z() * 0, _z(), _z()), _z())
        want = (torch.tensor(d, dtype=torch.float64) + torch.tensor(s, dtype=torch.float64)) / math.pi
        assert torch.allclose(f[0], want, rtol=0, atol=1e-15)
        assert abs(float(pdf) - 1 / math.pi) < 1e-15


def test_fresnel_known_values():
    eta = 1.49
    one = torch.tensor([1.0], dtype=torch.float64)
    assert abs(float(fresnel(one, eta)) - ((eta - 1) / (eta + 1)) ** 2) < 1e-12
    assert float(fresnel(one * 0, eta)) == 1.0          # grazing
    c = torch.tensor([0.0, 0.3, -0.7, 1.0], dtype=torch.float64)
    assert (fresnel(c, 1.0) == 0).all()                 # index-matched


def test_plastic_lobe_probabilities_sum_to_one():
    pl = PlasticRef([0.5, 0.4, 0.3], [1.0, 0.9, 0.8])
    c = torch.linspace(-1, 1, 41, dtype=torch.float64)
    ps, pd = pl.lobe_probs(c)
    assert (ps + pd - 1).abs().max() < 1e-14


def test_bidirectional_flips_the_back_side_and_is_zero_at_grazing():
    g = torch.Generator().manual_seed(0)
    P = 64
    n = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, dtype=torch.float64), dim=-1)
    wi = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, dtype=torch.float64), dim=-1)
    wo = torch.nn.functional.normalize(torch.randn(P, 3, generator=g, dtype=torch.float64), dim=-1)
    wi[:8, 2] = 0.0
    p = torch.zeros(P, 3, dtype=torch.float64)
    ph = PhongRef([0.6, 0.5, 0.7], [0.8, 0.8, 0.8], shine=math.log(11.0))
    f, pdf = BidirectionalRef(ph).eval_and_pdf(interaction(p, n, wi), wo, torch.ones(P, dtype=torch.bool))
    ff, fp = ph.eval_and_pdf(interaction(p, n, invert_z(wi)), invert_z(wo))
    below = wi[:, 2] < 0
    assert below.any() and (wi[:, 2] > 0).any()
    assert torch.equal(f[below], ff[below]) and torch.equal(pdf[below], fp[below])
    assert (f[:8] == 0).all() and (pdf[:8] == 0).all()


# ---- handle packing ------------------------------------------------------------------------------

def test_phong_component_packs_the_exponent():
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.bsdf import Phong
    ph = Phong(diffuse=[0.1, 0.2, 0.3], specular=[0.4, 0.5, 0.6], min_spec=1, device="cpu")
    ph.shine = torch.tensor(math.log(11.0), requires_grad=True)
    kind, mlp, act, params = ph._component()
    assert kind == _lib.NRT_BSDF_PHONG == 3 and mlp is None and len(params) == _lib.NRT_BSDF_PARAMS
    assert params[:6] == pytest.approx([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], rel=1e-7)
    assert params[6] == float(1 + torch.tensor(math.log(11.0)).exp())
    assert params[7:] == [0.0] * 5
    # the default shine = 40 stays finite in f32 (exp(40) = 2.35e17)
    assert math.isfinite(Phong(device="cpu")._component()[3][6])


def test_plastic_component_packs_the_derived_constants():
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.bsdf import Plastic
    pl = Plastic(diffuse=[0.5, 0.4, 0.3], specular=[1.0, 0.9, 0.8], device="cpu")
    kind, mlp, act, params = pl._component()
    ref = PlasticRef([0.5, 0.4, 0.3], [1.0, 0.9, 0.8])
    assert kind == _lib.NRT_BSDF_PLASTIC == 4 and mlp is None
    eta = 1.49 / 1.000277
    assert params[6] == eta and params[7] == 1 / eta
    assert params[8] == 1 - fresnel_diff_refl(1 / eta) and params[9] == 1 / (eta * eta)
    assert params[10] == pytest.approx(float(ref.spec_sample_weight()), rel=1e-6)
    assert pl.fdr_int == ref.fdr_int and pl.inv_eta_2 == ref.inv_eta_2


def test_bidirectional_component_forms():
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.bsdf import (Bidirectional, ComposeSpatialVarying, Diffuse,
                                                        NeuralBSDF, Phong, Plastic)
    ph, pl, df = Phong(device="cpu"), Plastic(device="cpu"), Diffuse(device="cpu")
    c = Bidirectional(ph)._component()
    assert c[0] == _lib.NRT_BSDF_PHONG and c[4] == (c[0], c[2], c[3])
    c = Bidirectional(df, pl)._component()
    assert c[0] == _lib.NRT_BSDF_DIFFUSE and c[4][0] == _lib.NRT_BSDF_PLASTIC
    assert list(c[4][2]) == list(pl._component()[3])
    with pytest.raises(_lib.NrtError, match="distinct NeuralBSDF"):
        Bidirectional(df, NeuralBSDF(device="cpu"))._component()
    with pytest.raises(_lib.NrtError, match="no HIP implementation"):
        Bidirectional(Bidirectional(ph))._component()
    # a two-sided mixture lowers to the mixture of two-sided components, sharing the weights MLP
    mix = ComposeSpatialVarying([df, ph], device="cpu")
    low = Bidirectional(mix)._lowered()
    assert low.sp_var_fn is mix.sp_var_fn and [b.front for b in low.bsdfs] == [df, ph]
    assert all(isinstance(b, Bidirectional) for b in low.bsdfs)


# ---- nrt_bsdf_create_ex validation (fails before any device call) --------------------------------

NRT_EINVAL = -1


def _create(comps):
    from neural_raytracing_amd import _lib
    lib = _lib.load()
    arr = (_lib.BsdfComponentEx * len(comps))()
    for i, kw in enumerate(comps):
        for k, v in kw.items():
            if k in ("params", "back_params"):
                for q, x in enumerate(v):
                    getattr(arr[i], k)[q] = x
            else:
                setattr(arr[i], k, v)
    out = ctypes.c_void_p()
    rc = lib.nrt_bsdf_create_ex(len(comps), arr, None, ctypes.byref(out))
    return rc, lib.nrt_last_error().decode(), out


PLASTIC = [0.5, 0.5, 0.5, 1, 1, 1, 1.49, 1 / 1.49, 0.4, 0.45, 0.6, 0]


@pytest.mark.parametrize("comp,msg", [
    (dict(kind=7, activation=2), "unknown component kind"),
    (dict(kind=-1, activation=2), "unknown component kind"),
    (dict(kind=0, activation=3), "NeuralBSDF MLP"),                        # missing MLP
    (dict(kind=3, activation=2, params=[0.1] * 6 + [float("nan")]), "non-finite"),
    (dict(kind=3, activation=2, params=[float("inf")]), "non-finite"),
    (dict(kind=3, activation=9), "activation"),
    (dict(kind=4, activation=2, params=[0.5] * 6 + [0.0]), "Plastic needs eta > 0"),
    (dict(kind=4, activation=2, params=PLASTIC[:8] + [0.0]), "Plastic needs eta > 0"),
    (dict(kind=3, activation=2, two_sided=2), "two_sided"),
    (dict(kind=3, activation=2, two_sided=1, back_kind=0, back_activation=2), "back of an analytic"),
    (dict(kind=3, activation=2, two_sided=1, back_kind=9, back_activation=2), "back of an analytic"),
    (dict(kind=3, activation=2, two_sided=1, back_kind=1, back_activation=2,
          back_params=[float("nan")]), "non-finite back"),
    (dict(kind=1, activation=2, two_sided=1, back_kind=4, back_activation=2), "Plastic needs"),
])
def test_bsdf_create_ex_rejects(comp, msg):
    rc, err, out = _create([comp])
    assert rc == NRT_EINVAL and msg in err and not out.value, (rc, err)


def test_bsdf_create_ex_rejects_bad_counts():
    from neural_raytracing_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    arr = (_lib.BsdfComponentEx * 1)()
    assert lib.nrt_bsdf_create_ex(0, arr, None, ctypes.byref(out)) == NRT_EINVAL
    assert lib.nrt_bsdf_create_ex(33, arr, None, ctypes.byref(out)) == NRT_EINVAL
    assert lib.nrt_bsdf_create_ex(1, None, None, ctypes.byref(out)) == NRT_EINVAL
    assert lib.nrt_bsdf_create_ex(1, arr, None, None) == NRT_EINVAL


def test_component_struct_matches_the_header():
    """kind 4 | pad 4 | mlp 8 | activation 4 | params 48 | two_sided, back_kind, back_activation
    12 | back_params 48 -> 128 bytes on LP64."""
    from neural_raytracing_amd import _lib
    assert ctypes.sizeof(_lib.BsdfComponentEx) == 128
    assert _lib.BsdfComponentEx.back_params.offset == 80


# ---- Path's draw order ---------------------------------------------------------------------------

class _Recorder:
    def __init__(self):
        self.shapes = []

    def sample(self, shape, device=None):
        self.shapes.append(tuple(shape))
        return torch.rand(tuple(shape))


def test_path_draws_the_plastic_lobe_before_its_direction():
    """Per component in component order; Plastic: sampler.sample(p_spec.shape) (bsdfs.py:304) then
    its (.., 2) draw (:309); the selection draw last."""
    from neural_raytracing_amd.pathtracer.bsdf import ComposeSpatialVarying, Diffuse, Phong, Plastic
    from neural_raytracing_amd.pathtracer.differentiable import bounce_uniforms
    lead, P = (2, 3, 1), 6
    mix = ComposeSpatialVarying([Diffuse(device="cpu"), Plastic(device="cpu"), Phong(device="cpu")],
                                device="cpu")
    rec = _Recorder()
    u_comp, u_sel, u_lobe = bounce_uniforms(mix, rec, lead, P, "cpu")
    assert rec.shapes == [lead + (2,), lead, lead + (2,), lead + (2,), (P,)]
    assert u_comp.shape == (P, 3, 2) and u_sel.shape == (P,) and u_lobe.shape == (P, 3)
    assert (u_lobe[:, [0, 2]] == 0).all()
    # without a Plastic: today's draws, and no lobe array (nrt_path_bounce, not _ex)
    mix2 = ComposeSpatialVarying([Diffuse(device="cpu"), Phong(device="cpu")], device="cpu")
    rec = _Recorder()
    assert bounce_uniforms(mix2, rec, lead, P, "cpu")[2] is None
    assert rec.shapes == [lead + (2,), lead + (2,), (P,)]
    # injected uniforms need the third array with a Plastic
    from neural_raytracing_amd import _lib
    with pytest.raises(_lib.NrtError, match="u_lobe"):
        bounce_uniforms(mix, rec, lead, P, "cpu", (u_comp, u_sel))


# ---- eval_and_pdf refuses tensors the kernels cannot read ----------------------------------------

@pytest.mark.parametrize("cls", ["Phong", "Plastic", "Diffuse", "Bidirectional"])
def test_eval_and_pdf_refuses_host_tensors(cls):
    """The no-grad eval_and_pdf hands raw pointers to nrt_bsdf_eval: inputs that are not on the
    GPU are refused with NrtError before any library call."""
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer import bsdf as B
    from neural_raytracing_amd.pathtracer.interaction import SurfaceInteraction
    b = B.Bidirectional(B.Phong(device="cpu")) if cls == "Bidirectional" else getattr(B, cls)(device="cpu")
    z = torch.tensor([[0.0, 0.0, 1.0]])
    it = SurfaceInteraction(p=z * 0, wi=z)
    it.n = z
    with torch.no_grad(), pytest.raises(_lib.NrtError, match="must be a tensor on the GPU"):
        b.eval_and_pdf(it, z)
