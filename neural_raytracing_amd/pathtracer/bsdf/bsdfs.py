"""BSDFs on the hot path (bsdf/bsdfs.py).  ``ComposeSpatialVarying`` of ``NeuralBSDF`` /
``Diffuse`` / ``Conductor`` / ``Phong`` / ``Plastic`` components, each optionally wrapped in
``Bidirectional``, evaluates inside the fused shading kernel ``nrt_shade_direct``; ``eval_and_pdf``
of every class is the same BSDF stage at a caller-supplied ``wo`` (``nrt_bsdf_eval``)."""
import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib
from .._handles import _Handle, _cache, mlp_handle
from ..neural_blocks import SkipConnMLP, activation_code


def identity(x):
    return x


def identity_div_pi(x):
    return x / math.pi


class BSDF(nn.Module):
    """General BSDF interface (bsdfs.py:63-72)."""

    def __init__(self):
        super().__init__()

    def sample(self, it, sampler, active=True):
        raise NotImplementedError()

    def eval_and_pdf(self, it, wo, active=True):
        raise NotImplementedError()

    # which outputs eval_and_pdf zeroes where ~active, per class as the reference does
    _mask_spectrum = False
    _mask_pdf = False

    def _eval_hip(self, it, wo, active):
        """eval_and_pdf on the HIP path: nrt_bsdf_eval without gradients, differentiable.bsdf_eval
        when a parameter or an input requires one.  `it`: anything with p, n, wi."""
        from ..differentiable import bsdf_eval, needs_grad
        lead = it.p.shape[:-1]
        if not torch.is_tensor(active):
            active = torch.full(lead, bool(active), dtype=torch.bool, device=it.p.device)
        active = active.expand(lead)
        if needs_grad(self) or (torch.is_grad_enabled() and
                                any(t.requires_grad for t in (it.p, it.wi, wo))):
            return bsdf_eval(self, it, wo, active)
        from ..integrators.integrators import _bsdf_handle
        dev = it.p.device
        names = ("it.p", "it.n", "it.wi", "wo", "active")
        for name, t in zip(names, (it.p, it.n, it.wi, wo, active)):
            # the library reads raw device pointers: nothing from the host or another GPU
            if not torch.is_tensor(t) or not t.is_cuda or t.device != dev:
                raise _lib.NrtError(f"eval_and_pdf: {name} must be a tensor on the GPU of it.p "
                                    f"(got {getattr(t, 'device', type(t).__name__)}, it.p on {dev})")
        P = active.numel()
        flat = [t.detach().expand(lead + (3,)).reshape(P, 3).float().contiguous()
                for t in (it.p, it.n, it.wi, wo)]
        spectrum = torch.empty(P, 3, device=dev)
        pdf = torch.empty(P, device=dev)
        both = self._mask_spectrum and self._mask_pdf
        # a mixture with a weights MLP evaluates every ray and masks afterwards, so that the one
        # evaluation of the MLP also gives it.normalized_weights on every ray (bsdfs.py:516-520)
        weights = None
        if getattr(self, "sp_var_fn", None) is not None:
            weights = torch.empty(P, len(self.bsdfs), device=dev)
        act = active.reshape(P).to(torch.uint8).contiguous() if both and weights is None else None
        _lib.call("nrt_bsdf_eval", _bsdf_handle(self), *[_lib.ptr(t) for t in flat], _lib.ptr(act),
                  P, _lib.ptr(spectrum), _lib.ptr(pdf), _lib.ptr(weights), _lib.precision_code(),
                  _lib.stream())
        spectrum = spectrum.reshape(lead + (3,))
        pdf = pdf.reshape(lead)
        if self._mask_spectrum and act is None:
            spectrum = torch.where(active.unsqueeze(-1), spectrum, torch.zeros_like(spectrum))
        if self._mask_pdf and act is None:
            pdf = torch.where(active, pdf, torch.zeros_like(pdf))
        if weights is not None:
            setattr(it, "normalized_weights", weights.reshape(lead + (len(self.bsdfs),)))
        return spectrum, pdf

    def joint_eval_pdf(self, it, wo, active=True):
        spectrum, pdf = self.eval_and_pdf(it, wo, active)
        return torch.cat([spectrum, pdf.reshape(spectrum.shape[:-1] + (1,))], dim=-1)

    def eval(self, it, wo, active=True):
        return self.eval_and_pdf(it, wo, active)[0]

    def pdf(self, it, wo, active=True):
        return self.eval_and_pdf(it, wo, active)[1]


class Diffuse(BSDF):
    """Diffuse (bsdfs.py:78-118)."""

    def __init__(self, reflectance=[0.25, 0.2, 0.7], preprocess=identity_div_pi, device="cuda"):
        super().__init__()
        if type(reflectance) == list:
            self.reflectance = torch.tensor(reflectance, device=device, requires_grad=True)
        else:
            self.reflectance = reflectance
        self.preproc = preprocess

    def parameters(self):
        return [self.reflectance]

    def random(self):
        self.reflectance = torch.rand_like(self.reflectance, requires_grad=True)
        return self

    def _component(self):
        if self.preproc is identity_div_pi:
            act = _lib.ACT["none"]
        else:
            act = _lib.ACT[activation_code(self.preproc)]
        refl = self.reflectance.detach().float().cpu().tolist()
        return (_lib.NRT_BSDF_DIFFUSE, None, act, refl + [0.0])

    def eval_and_pdf(self, it, wo, active=True):
        """bsdfs.py:108-118 (not masked)."""
        return self._eval_hip(it, wo, active)


class Conductor(BSDF):
    """Conductor (bsdfs.py:345-388)."""

    def __init__(self, specular=[1., 1., 1.], eta: float = 1.3, k: float = 1, device="cuda",
                 activation=torch.sigmoid):
        super().__init__()
        self.eta = torch.tensor(eta, requires_grad=True, dtype=torch.float)
        self.k = torch.tensor(k, requires_grad=True, dtype=torch.float)
        if type(specular) == list:
            self.specular = torch.tensor(specular, device=device, requires_grad=True)
        else:
            self.specular = specular
        self.act = activation

    def parameters(self):
        return [self.eta, self.k, self.specular]

    def random(self):
        self.specular = torch.rand_like(self.specular, requires_grad=True)
        return self

    def _component(self):
        eta = float(F.softplus(self.eta.detach().float()))
        spec = self.specular.detach().float().cpu().tolist()
        return (_lib.NRT_BSDF_CONDUCTOR, None, _lib.ACT[activation_code(self.act)], spec + [eta])

    _mask_spectrum = True

    def eval_and_pdf(self, it, wo, active=True):
        """bsdfs.py:364-388 (the spectrum is masked, the pdf is not)."""
        return self._eval_hip(it, wo, active)


class NeuralBSDF(BSDF):
    """act(SkipConnMLP_6x96,F=64(param_rusin2(it.wi, wo))), pdf 1 (bsdfs.py:613-637)."""

    def __init__(self, activation=torch.sigmoid, device="cuda"):
        super().__init__()
        self.mlp = SkipConnMLP(in_size=3, out=3, num_layers=6, hidden_size=96, freqs=64,
                               device=device).to(device)
        self.act = activation

    def parameters(self):
        return self.mlp.parameters()

    def random(self):
        return self

    def _component(self):
        return (_lib.NRT_BSDF_NEURAL, mlp_handle(self.mlp), _lib.ACT[activation_code(self.act)],
                [0.0, 0.0, 0.0, 0.0])

    def eval_and_pdf(self, it, wo, active=True):
        """bsdfs.py:634-637 (not masked)."""
        return self._eval_hip(it, wo, active)


class ComposeSpatialVarying(BSDF):
    """Spatially varying mixture sum_j sigmoid(sp_var(p))_j f_j (bsdfs.py:482-536)."""

    def __init__(self, bsdfs, spatial_varying_fn=None, device="cuda"):
        super().__init__()
        self.bsdfs = bsdfs
        if spatial_varying_fn is None:
            self.sp_var_fn = SkipConnMLP(num_layers=16, hidden_size=256, freqs=128, sigma=2 << 6,
                                         in_size=3, out=len(bsdfs), device=device,
                                         xavier_init=True).to(device)
        else:
            self.sp_var_fn = spatial_varying_fn
        self.preprocess = identity

    def parameters(self):
        from itertools import chain
        own = self.sp_var_fn.parameters() if self.sp_var_fn is not None else []
        return chain(own, *[b.parameters() for b in self.bsdfs])

    def nrt(self):
        """nrt_bsdf handle (rebuilt when any component's parameters change)."""
        comps = [b._component() for b in self.bsdfs]
        sp = self.sp_var_fn
        sph = mlp_handle(sp) if isinstance(sp, SkipConnMLP) else None
        if sp is not None and sph is None:
            raise _lib.NrtError("spatial_varying_fn must be a SkipConnMLP on the HIP path")
        def build():
            arr = (_lib.BsdfComponentEx * len(comps))()
            for i, comp in enumerate(comps):
                kind, mh, act, params = comp[:4]
                back = comp[4] if len(comp) > 4 else None
                arr[i].kind = kind
                arr[i].mlp = mh.value if mh is not None else None
                arr[i].activation = act
                for q, v in enumerate(params):
                    arr[i].params[q] = float(v)
                if back is not None:  # Bidirectional: (kind, activation, params) of the back side
                    arr[i].two_sided = 1
                    arr[i].back_kind, arr[i].back_activation = back[0], back[1]
                    for q, v in enumerate(back[2]):
                        arr[i].back_params[q] = float(v)
            out = ctypes.c_void_p()
            _lib.check(_lib.load().nrt_bsdf_create_ex(len(comps), arr, sph.value if sph else None,
                                                      ctypes.byref(out)), "nrt_bsdf_create_ex")
            deps = [c[1] for c in comps if c[1] is not None] + ([sph] if sph else [])
            return _Handle(out, "nrt_bsdf_destroy", deps)

        cached = getattr(self, "_nrt_bsdf", None)
        key = tuple((c[0], c[2], tuple(c[3]), id(c[1]),
                     (c[4][0], c[4][1], tuple(c[4][2])) if len(c) > 4 and c[4] else None)
                    for c in comps) + (id(sph),)
        if cached is None or cached[0] != key:
            object.__setattr__(self, "_nrt_bsdf", (key, build()))
        return self._nrt_bsdf[1].value

    _mask_spectrum = True
    _mask_pdf = True

    def eval_and_pdf(self, it, wo, active=True):
        """bsdfs.py:515-528: sum_j k_j [f_j | pdf_j], zero where ~active; sets
        it.normalized_weights on every ray, as the reference does (from the kernel's weights
        output; with gradients, differentiable.bsdf_eval sets it with its graph)."""
        return self._eval_hip(it, wo, active)

    def normalized_weights(self, p, it):
        w = self.sp_var_fn(self.preprocess(p)).reshape(p.shape[:-1] + (len(self.bsdfs),))
        setattr(it, "nonnormalized_weights", w)
        return w.sigmoid()


# ---- the analytic models: Phong, Plastic and the two-sided wrapper ------------------------------

def _pad(params):
    return list(params) + [0.0] * (_lib.NRT_BSDF_PARAMS - len(params))


class Phong(BSDF):
    """bsdfs.py:132-189."""

    def __init__(self, diffuse=[0.6, 0.5, 0.7], specular=[0.8, 0.8, 0.8], min_spec=1, device="cuda"):
        super().__init__()
        self.diffuse = torch.tensor(diffuse, device=device, requires_grad=True) \
            if type(diffuse) == list else diffuse
        self.specular = torch.tensor(specular, device=device, requires_grad=True) \
            if type(specular) == list else specular
        self.shine = torch.tensor(40., dtype=torch.float, device=device, requires_grad=True)
        self.min_spec = min_spec

    def parameters(self):
        return [self.specular, self.diffuse, self.shine]

    def random(self):
        self.shine = torch.rand_like(self.shine, requires_grad=True)
        self.specular = torch.rand_like(self.specular, requires_grad=True)
        self.diffuse = torch.rand_like(self.diffuse, requires_grad=True)
        return self

    def exponent(self):
        """min_spec + exp(shine) (bsdfs.py:181), in float32 as the reference's tensor op."""
        return float(self.min_spec + self.shine.detach().float().exp())

    def _component(self):
        d = self.diffuse.detach().float().cpu().tolist()
        sp = self.specular.detach().float().cpu().tolist()
        return (_lib.NRT_BSDF_PHONG, None, _lib.ACT["none"], _pad(d + sp + [self.exponent()]))

    def eval_and_pdf(self, it, wo, active=True):
        """bsdfs.py:176-189 (not masked)."""
        return self._eval_hip(it, wo, active)


def fresnel_diff_refl(eta):
    """bsdfs.py:220-235 (Mitsuba's diffuse Fresnel reflectance fit)."""
    if eta < 1:
        return -1.4399 * (eta * eta) + 0.7099 * eta + 0.6681 + 0.0636 / eta
    inv = 1 / eta
    return 0.919317 - 3.4793 * inv + 6.75335 * inv ** 2 - 7.80989 * inv ** 3 + \
        4.98554 * inv ** 4 - 1.36881 * inv ** 5


class Plastic(BSDF):
    """bsdfs.py:238-325."""

    def __init__(self, diffuse=[0.5, 0.5, 0.5], specular=[1., 1., 1.], int_ior: float = 1.49,
                 ext_ior: float = 1.000277, device="cuda"):
        super().__init__()
        self.diffuse = torch.tensor(diffuse, device=device, requires_grad=True) \
            if type(diffuse) == list else diffuse
        self.specular = torch.tensor(specular, device=device, requires_grad=True) \
            if type(specular) == list else specular
        assert int_ior > 0 and ext_ior > 0
        self.eta = int_ior / ext_ior
        self.inv_eta_2 = 1 / (self.eta * self.eta)
        self.fdr_int = fresnel_diff_refl(1 / self.eta)
        self.fdr_ext = fresnel_diff_refl(self.eta)

    def spec_sample_weight(self):
        d = self.diffuse.mean()
        s = self.specular.mean()
        return s / (d + s)

    def parameters(self):
        return [self.diffuse, self.specular]

    def random(self):
        self.specular = torch.rand_like(self.specular, requires_grad=True)
        self.diffuse = torch.rand_like(self.diffuse, requires_grad=True)
        return self

    def _component(self):
        """diffuse rgb, specular rgb, eta, 1/eta, 1 - fdr_int, inv_eta_2, spec_sample_weight: the
        constants as the reference holds them, Python doubles (bsdfs.py:197, 254-259, 278)."""
        d = self.diffuse.detach().float().cpu().tolist()
        sp = self.specular.detach().float().cpu().tolist()
        ssw = float(self.spec_sample_weight().detach().float())
        return (_lib.NRT_BSDF_PLASTIC, None, _lib.ACT["none"],
                _pad(d + sp + [self.eta, 1 / self.eta, 1 - self.fdr_int, self.inv_eta_2, ssw]))

    def eval_and_pdf(self, it, wo, active=True):
        """bsdfs.py:271-291 (not masked)."""
        return self._eval_hip(it, wo, active)


class Bidirectional(BSDF):
    """bsdfs.py:409-453: front BSDF for cos(theta_i) > 0, back (default: the front one) with z
    inverted below the surface.  On the HIP path: any leaf on both sides, two different analytic
    leaves, or a ComposeSpatialVarying on both sides (every component two-sided: the weights
    depend on p only, so the spectrum is the same).  A distinct NeuralBSDF behind is refused."""

    _mask_spectrum = True
    _mask_pdf = True

    def __init__(self, front, back=None):
        super().__init__()
        self.front = front
        self.back = front if back is None else back

    def parameters(self):
        from itertools import chain
        return chain(self.front.parameters(), self.back.parameters())

    def _leaf(self, b):
        if isinstance(b, (Bidirectional, ComposeSpatialVarying)) or not hasattr(b, "_component"):
            raise _lib.NrtError(f"Bidirectional({type(b).__name__}) has no HIP implementation "
                                "(supported: a leaf BSDF, or one ComposeSpatialVarying on both "
                                "sides)")
        return b._component()

    def _component(self):
        if self.back is not self.front and (isinstance(self.front, NeuralBSDF) or
                                            isinstance(self.back, NeuralBSDF)):
            raise _lib.NrtError("Bidirectional with a NeuralBSDF needs the same NeuralBSDF on both "
                                "sides on the HIP path (one MLP evaluation per ray); a distinct "
                                "NeuralBSDF behind is not supported")
        kind, mh, act, params = self._leaf(self.front)
        if self.back is self.front:
            return (kind, mh, act, params, (kind, act, params))
        bk, _, bact, bparams = self._leaf(self.back)
        return (kind, mh, act, params, (bk, bact, bparams))

    def _lowered(self):
        """Bidirectional(ComposeSpatialVarying([...])) as the mixture of two-sided components."""
        mix = self.front
        cached = getattr(self, "_nrt_lowered", None)
        if cached is None or cached[0] is not mix or cached[1] != [id(b) for b in mix.bsdfs]:
            w = ComposeSpatialVarying.__new__(ComposeSpatialVarying)
            nn.Module.__init__(w)
            w.bsdfs = [Bidirectional(b) for b in mix.bsdfs]
            w.sp_var_fn = mix.sp_var_fn
            w.preprocess = mix.preprocess
            cached = (mix, [id(b) for b in mix.bsdfs], w)
            object.__setattr__(self, "_nrt_lowered", cached)
        return cached[2]

    def nrt(self):
        if isinstance(self.front, ComposeSpatialVarying):
            if self.back is not self.front:
                raise _lib.NrtError("Bidirectional of a ComposeSpatialVarying needs the same "
                                    "mixture on both sides on the HIP path")
            return self._lowered().nrt()
        wrapper = getattr(self, "_nrt_single", None)
        if wrapper is None:
            wrapper = ComposeSpatialVarying.__new__(ComposeSpatialVarying)
            nn.Module.__init__(wrapper)
            wrapper.bsdfs = [self]
            wrapper.sp_var_fn = None
            object.__setattr__(self, "_nrt_single", wrapper)
        return wrapper.nrt()

    def eval_and_pdf(self, it, wo, active=True):
        """bsdfs.py:434-453 (spectrum and pdf are zero where ~active or wi.z == 0)."""
        return self._eval_hip(it, wo, active)
