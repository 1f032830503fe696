"""Training through the fused path: the differentiable pieces of
``SDF.intersect`` and ``Direct.sample`` for ``loss.backward()``.

Rendering with gradients keeps the reference's split: the march and the 128-step coarse scan
run without gradients (``torch.no_grad`` in sdfs.py:118-131, :239-247) on the fused HIP
kernels; what carries gradients is recomputed at the points they found:

* ``throughput = -1000 * sdf(best_pos)`` (sdfs.py:134-137, :248) -- the SDF MLP forward and
  backward on ``nrt_mlp_forward`` / ``nrt_mlp_backward``;
* ``raw_normals = d sdf / d p`` with ``create_graph=True`` (sdfs.py:184-197) --
  ``nrt_mlp_backward`` for the value, ``nrt_mlp_grad_backward`` for its parameter gradients;
* the shading MLPs (spatial weights, NeuralBSDFs, LightField) -- ``SkipConnMLP`` autograd.

The glue between the MLPs (frames, Rusinkiewicz angles, Fresnel, light falloff, the 128-sphere
smooth-min of ``SphereSDF``) is a few element-wise tensor ops per ray, written here in the
reference's op order so autograd reproduces its gradients.
"""
import math

import torch
import torch.nn.functional as F

from .. import _lib


# ---- interaction frames (interaction.py:9-51) -------------------------------------------------

def coordinate_system(n):
    """Shading frame columns [s, t, n] (interaction.py:9-27), differentiable."""
    n = F.normalize(n, eps=1e-7, dim=-1)
    x, y, z = n.split(1, dim=-1)
    sign = torch.where(z >= 0, 1., -1.)
    s_z = sign + z
    a = -torch.where(s_z.abs() < 1e-6, 1e-6, s_z).reciprocal()
    b = x * y * a
    s = torch.cat([(x * x * a * sign) + 1, b * sign, x * -sign], dim=-1)
    s = F.normalize(s, eps=1e-7, dim=-1)
    t = F.normalize(s.cross(n, dim=-1), eps=1e-7, dim=-1)
    s = F.normalize(n.cross(t, dim=-1), eps=1e-7, dim=-1)
    return torch.stack([s, t, n], dim=-1)


# ---- BSDF helpers (utils.py:43-51, 152-155, 234-258; bsdfs.py:127-129, 327-343) --------------

def nonzero_eps(v, eps: float = 1e-7):
    # a Python scalar branch: no host -> device copy (and no stream sync) per call
    return torch.where(v.abs() < eps, eps, v)


_AXES = {}


def _axis(i, like):
    """Unit axis e_i on like's device, built once per device (no per-call host copy)."""
    key = (like.device, i)
    t = _AXES.get(key)
    if t is None:
        t = torch.zeros(3, device=like.device, dtype=torch.float)
        t[i] = 1.0
        _AXES[key] = t
    return t.expand_as(like)


def rotate_vector(v, axis, c, s):
    return v * c + axis * (v * axis).sum(dim=-1, keepdim=True) * (1 - c) + \
        torch.cross(axis, v, dim=-1) * s


def param_rusin2(wo, wi):
    """[cos phi_d, cos theta_h, cos theta_d] (utils.py:234-258)."""
    wo = F.normalize(wo, dim=-1)
    wi = F.normalize(wi, dim=-1)
    e_1 = _axis(1, wo)
    e_2 = _axis(2, wo)
    H = F.normalize(wo + wi, dim=-1)
    cos_theta_h = H[..., 2]
    r = nonzero_eps(H[..., 1]).hypot(nonzero_eps(H[..., 0])).clamp(min=1e-6)
    c = (H[..., 0] / r).unsqueeze(-1)
    s = -(H[..., 1] / r).unsqueeze(-1)
    tmp = F.normalize(rotate_vector(wi, e_2, c, s), dim=-1)
    c = H[..., 2].unsqueeze(-1)
    s = -(1 - H[..., 2]).clamp(min=1e-6).sqrt().unsqueeze(-1)
    diff = F.normalize(rotate_vector(tmp, e_1, c, s), dim=-1)
    cos_theta_d = diff[..., 2]
    cos_phi_d = torch.atan2(nonzero_eps(diff[..., 1]), nonzero_eps(diff[..., 0])).cos()
    return torch.stack([cos_phi_d, cos_theta_h, cos_theta_d], dim=-1)


def local_reflect(v):
    x, y, z = v.split(1, dim=-1)
    return torch.cat([-x, -y, z], dim=-1)


def fresnel_conductor(cos_t, eta_r: float, eta_i: float):
    ct2 = cos_t * cos_t
    st2 = (1 - ct2).clamp(min=1e-10)
    st4 = st2 * st2
    tmp = eta_r * eta_r - eta_i * eta_i - st2
    a_2_pb_2 = (tmp * tmp + 4 * eta_i * eta_i * eta_r * eta_r).clamp(min=1e-10).sqrt()
    a = (0.5 * (a_2_pb_2 + tmp)).clamp(min=1e-10).sqrt()
    t1 = a_2_pb_2 + ct2
    t2 = 2 * cos_t * a
    r_s = (t1 - t2) / (t1 + t2)
    t3 = a_2_pb_2 * ct2 + st4
    t4 = t2 * st2
    r_p = r_s * (t3 - t4) / (t3 + t4)
    return 0.5 * (r_s + r_p)


# ---- SDF values and gradients with autograd ---------------------------------------------------

def reflect(n, v):
    """bsdfs.py:121-123."""
    return 2 * (n * v).sum(keepdim=True, dim=-1) * n - v


def invert_z(xyz):
    """bsdfs.py:404-406."""
    x, y, z = xyz.split(1, dim=-1)
    return torch.cat([x, y, -z], dim=-1)


def fresnel(cos_t, eta: float):
    """bsdfs.py:193-218, its first result."""
    out_mask = cos_t >= 0
    inv_eta = 1 / eta
    eta_it = torch.where(out_mask, eta, inv_eta)
    eta_ti = torch.where(out_mask, inv_eta, eta)
    cos_tt_sqr = -(-cos_t * cos_t + 1) * (eta_ti * eta_ti) + 1
    cos_t_abs = cos_t.abs()
    cos_tt_abs = cos_tt_sqr.clamp(min=1e-10).sqrt()
    a_s = (-eta_it * cos_tt_abs + cos_t_abs) / (eta_it * cos_tt_abs + cos_t_abs)
    a_p = (-eta_it * cos_t_abs + cos_tt_abs) / (eta_it * cos_t_abs + cos_tt_abs)
    r = 0.5 * (a_s.square() + a_p.square())
    if eta == 1:
        return torch.zeros_like(r)
    return torch.where(cos_t_abs == 0, torch.ones_like(r), r)


def _world_normal(it):
    """it.frame[..., 2]: the last column of [s t n] (interaction.py:9-27)."""
    frame = getattr(it, "frame", None)
    if frame is not None:
        return frame[..., 2]
    return F.normalize(it.n, eps=1e-7, dim=-1)


def needs_grad(*modules):
    """True when autograd is on and any parameter of the given objects requires a gradient."""
    if not torch.is_grad_enabled():
        return False
    for m in modules:
        params = getattr(m, "parameters", None)
        if params is None:
            continue
        try:
            if any(getattr(q, "requires_grad", False) for q in params()):
                return True
        except (TypeError, AttributeError):
            continue
    return False


SMOOTHMIN_K = 32.0  # sdfs.py:43 / utils.py:386-387
# nrt_sphere_smoothmin_* stage the sphere table (13 floats a sphere) in 64 KB of LDS: larger
# SphereSDFs train on the torch restatement (sphere_part under autograd)
SMOOTHMIN_MAX_SPHERES = 64 * 1024 // (13 * 4)


def _fused_smoothmin(sdf, p):
    return p.is_cuda and sdf.centers.shape[0] <= SMOOTHMIN_MAX_SPHERES


class _SphereSmoothMinFn(torch.autograd.Function):
    """(value, d value / d p) of SphereSDF's smooth-min on nrt_sphere_smoothmin_forward, with the
    sphere parameters' gradients of both outputs from nrt_sphere_smoothmin_backward -- for the
    gradient output that is the double backward of SDF.autograd_diff's create_graph=True normal
    (sdfs.py:184-197).  The points carry no gradient (the reference's hit and scan points come
    from the no-grad march)."""

    @staticmethod
    def forward(ctx, p, centers, radii, tfs):
        P, n = p.shape[0], centers.shape[0]
        value = torch.empty(P, device=p.device)
        grad = torch.empty(P, 3, device=p.device)
        c, r, t = (x.detach().float().contiguous() for x in (centers, radii, tfs))
        _lib.call("nrt_sphere_smoothmin_forward", _lib.ptr(p), P, _lib.ptr(c), _lib.ptr(r),
                  _lib.ptr(t), n, SMOOTHMIN_K, _lib.ptr(value), _lib.ptr(grad), _lib.stream())
        ctx.save_for_backward(p, c, r, t)
        return value, grad

    @staticmethod
    def backward(ctx, dvalue, dgrad):
        if torch.is_grad_enabled():
            raise _lib.NrtError("third derivatives of the SphereSDF smooth-min are not on the "
                                "HIP path")
        p, c, r, t = ctx.saved_tensors
        P, n = p.shape[0], c.shape[0]
        lib = _lib.load(require_device=True)
        dc = torch.empty_like(c) if ctx.needs_input_grad[1] else None
        dr = torch.empty_like(r) if ctx.needs_input_grad[2] else None
        dt = torch.empty_like(t) if ctx.needs_input_grad[3] else None
        dv = None if dvalue is None else dvalue.float().contiguous()
        dg = None if dgrad is None else dgrad.float().contiguous()
        ws = torch.empty(lib.nrt_sphere_smoothmin_workspace_bytes(P), dtype=torch.uint8,
                         device=p.device)
        _lib.call("nrt_sphere_smoothmin_backward", _lib.ptr(p), P, _lib.ptr(c), _lib.ptr(r),
                  _lib.ptr(t), n, SMOOTHMIN_K, _lib.ptr(dv), _lib.ptr(dg), _lib.ptr(dc),
                  _lib.ptr(dr), _lib.ptr(dt), _lib.ptr(ws), _lib.stream())
        return None, dc, dr, dt


def sphere_smoothmin(sdf, p):
    """(value, gradient) of the smooth-min part at points p [..., 3] that carry no gradient, on
    the fused kernels; shapes p.shape[:-1] and p.shape."""
    flat = p.detach().reshape(-1, 3).float().contiguous()
    v, g = _SphereSmoothMinFn.apply(flat, sdf.centers, sdf.radii, sdf.tfs)
    return v.reshape(p.shape[:-1]), g.reshape(p.shape)


def sphere_part(sdf, p):
    """The smooth-min of the transformed spheres of SphereSDF (sdfs.py:37-43, utils.py:386-387)."""
    flat = p.reshape(-1, 3).unsqueeze(0)
    tfs = sdf.tfs + torch.eye(3, device=p.device).unsqueeze(0)
    q = torch.einsum("ijk,ibk->ibj", tfs, flat.expand(tfs.shape[0], -1, -1)) - \
        sdf.centers.unsqueeze(1)
    sd = q.norm(p=2, dim=-1) - sdf.radii.unsqueeze(-1)
    return (-(-32. * sd).exp().sum(dim=0).clamp(min=1e-4).log() / 32.).reshape(p.shape[:-1])


# ---- RoundBoxSDF / CapsuleSDF (sdfs.py:46-86): smooth-min of n primitives, no residual MLP ------

PRIM_SMOOTHMIN_K = 16.0  # sdfs.py:68, 86
# nrt_sdf_create_round_boxes / _capsules and nrt_prim_smoothmin_* take at most 1024 primitives:
# larger modules march on the callable path and train on the torch restatements below
PRIM_MAX = 1024
PRIM_ROUND_BOX, PRIM_CAPSULE = 3, 4  # include/nrt.h NRT_PRIM_*


def round_box_part(sdf, p):
    """RoundBoxSDF.forward (sdfs.py:61-68) in torch, in the reference's op order: the CPU path,
    points that carry gradients (a warp around the SDF) and tables over PRIM_MAX.  ``radii`` is
    never read, as in the reference."""
    flat = p.reshape(-1, 3).unsqueeze(0)
    tfs = sdf.tfs + torch.eye(3, device=p.device, dtype=sdf.tfs.dtype).unsqueeze(0)
    q = (torch.einsum("ijk,ibk->ibj", tfs, flat.expand(tfs.shape[0], -1, -1)) -
         sdf.centers.unsqueeze(1)).abs() - sdf.b.unsqueeze(1)
    up = q.clamp(min=1e-7).norm(p=2, dim=-1, keepdim=True)
    x, y, z = q.split(1, dim=-1)
    down = torch.maximum(x, torch.maximum(y, z)).clamp(max=-1e-7)
    sd = up + down
    k = PRIM_SMOOTHMIN_K
    return (-(-k * sd).exp().sum(dim=0).clamp(min=1e-4).log() / k).reshape(p.shape[:-1])


def capsule_part(sdf, p):
    """CapsuleSDF.forward (sdfs.py:78-86) in torch: the clamp binds to the denominator, so h is
    unclamped (infinite cylinders), as the reference."""
    pa = p.reshape(-1, 3).unsqueeze(0) - sdf.a.unsqueeze(1)
    ba = (sdf.b - sdf.a).unsqueeze(1)
    h = (pa * ba).sum(dim=-1, keepdim=True) / \
        (ba * ba).sum(dim=-1, keepdim=True).clamp(min=0, max=1)
    sd = (pa - ba * h).norm(p=2, dim=-1) - sdf.radii.unsqueeze(-1)
    k = PRIM_SMOOTHMIN_K
    return (-(-k * sd).exp().sum(dim=0).clamp(min=1e-4).log() / k).reshape(p.shape[:-1])


def prim_kind(sdf):
    """(NRT_PRIM_* kind, the three parameter tensors in the C ABI's order, torch restatement) of a
    RoundBoxSDF / CapsuleSDF, or None."""
    from .shapes.sdfs import CapsuleSDF, RoundBoxSDF
    if isinstance(sdf, RoundBoxSDF):
        return PRIM_ROUND_BOX, (sdf.centers, sdf.b, sdf.tfs), round_box_part
    if isinstance(sdf, CapsuleSDF):
        return PRIM_CAPSULE, (sdf.a, sdf.b, sdf.radii), capsule_part
    return None


class _PrimSmoothMinFn(torch.autograd.Function):
    """(value, d value / d p) of RoundBoxSDF's / CapsuleSDF's smooth-min on
    nrt_prim_smoothmin_forward, with the primitive parameters' gradients of both outputs from
    nrt_prim_smoothmin_backward (for the gradient output: the double backward of the
    create_graph=True normal, sdfs.py:184-197).  kind: PRIM_ROUND_BOX (A, B, C = centers, b, tfs)
    or PRIM_CAPSULE (a, b, radii).  The points carry no gradient."""

    @staticmethod
    def forward(ctx, p, kind, A, B, C):
        P, n = p.shape[0], A.shape[0]
        value = torch.empty(P, device=p.device)
        grad = torch.empty(P, 3, device=p.device)
        a, b, c = (x.detach().float().contiguous() for x in (A, B, C))
        _lib.call("nrt_prim_smoothmin_forward", kind, _lib.ptr(p), P, _lib.ptr(a), _lib.ptr(b),
                  _lib.ptr(c), n, PRIM_SMOOTHMIN_K, _lib.ptr(value), _lib.ptr(grad), _lib.stream())
        ctx.save_for_backward(p, a, b, c)
        ctx.kind = kind
        return value, grad

    @staticmethod
    def backward(ctx, dvalue, dgrad):
        if torch.is_grad_enabled():
            raise _lib.NrtError("third derivatives of the RoundBoxSDF / CapsuleSDF smooth-min are "
                                "not on the HIP path")
        p, a, b, c = ctx.saved_tensors
        P, n = p.shape[0], a.shape[0]
        lib = _lib.load(require_device=True)
        da = torch.empty_like(a) if ctx.needs_input_grad[2] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[3] else None
        dc = torch.empty_like(c) if ctx.needs_input_grad[4] else None
        dv = None if dvalue is None else dvalue.float().contiguous()
        dg = None if dgrad is None else dgrad.float().contiguous()
        ws = torch.empty(lib.nrt_prim_smoothmin_workspace_bytes(P), dtype=torch.uint8,
                         device=p.device)
        _lib.call("nrt_prim_smoothmin_backward", ctx.kind, _lib.ptr(p), P, _lib.ptr(a), _lib.ptr(b),
                  _lib.ptr(c), n, PRIM_SMOOTHMIN_K, _lib.ptr(dv), _lib.ptr(dg), _lib.ptr(da),
                  _lib.ptr(db), _lib.ptr(dc), _lib.ptr(ws), _lib.stream())
        return None, None, da, db, dc


def _fused_prim(tensors, p):
    return p.is_cuda and all(t.is_cuda for t in tensors) and tensors[0].shape[0] <= PRIM_MAX


def prim_smoothmin(kind, tensors, p):
    """(value, gradient) at points p [..., 3] that carry no gradient, on the fused kernels."""
    flat = p.detach().reshape(-1, 3).float().contiguous()
    v, g = _PrimSmoothMinFn.apply(flat, kind, *tensors)
    return v.reshape(p.shape[:-1]), g.reshape(p.shape)


def sdf_value(sdf, p):
    """sdf(p) with gradients for the SDF's parameters."""
    from .neural_blocks import SkipConnMLP
    from .script_modules import resolve
    from .shapes.sdfs import SPHERE_SDF, _is_sphere_sdf
    sdf = resolve(sdf)
    if sdf is SPHERE_SDF:
        return torch.norm(p, dim=-1) - 1
    if isinstance(sdf, SkipConnMLP):
        return sdf(p).reshape(p.shape[:-1])
    pk = prim_kind(sdf)
    if pk is not None:
        kind, tensors, part = pk
        if _fused_prim(tensors, p) and not p.requires_grad:
            return prim_smoothmin(kind, tensors, p)[0]  # fused forward + parameter backward
        return part(sdf, p)  # points with a gradient, CPU tensors, tables over the limit
    if _is_sphere_sdf(sdf):
        if _fused_smoothmin(sdf, p) and not p.requires_grad:
            out = sphere_smoothmin(sdf, p)[0]  # fused forward + parameter backward
        else:  # points with a gradient (an SDF callable warping them): the torch restatement
            out = sphere_part(sdf, p)
        return out + sdf.shift(p).reshape_as(out)
    raise _lib.NrtError(f"SDF callable {type(sdf).__name__} has no HIP training path")


def sdf_gradient(sdf, p):
    """SDF.autograd_diff (sdfs.py:184-197): d sdf / d p, differentiable with respect to the
    SDF's parameters (create_graph=True).  ``p`` itself is not differentiated (the reference's
    hit points come from the no-grad march)."""
    from .neural_blocks import SkipConnMLP, input_gradient
    from .script_modules import resolve
    from .shapes.sdfs import SPHERE_SDF, _is_sphere_sdf
    sdf = resolve(sdf)
    p = p.detach()
    if sdf is SPHERE_SDF:
        return p / torch.norm(p, dim=-1, keepdim=True)
    if isinstance(sdf, SkipConnMLP):
        return input_gradient(sdf, p)
    pk = prim_kind(sdf)
    if pk is not None:
        kind, tensors, part = pk
        if _fused_prim(tensors, p):
            return prim_smoothmin(kind, tensors, p)[1]  # fused gradient + its double backward
        with torch.enable_grad():
            q = p.clone().requires_grad_(True)
            out = part(sdf, q)
            (g,) = torch.autograd.grad(out, q, torch.ones_like(out), create_graph=True)
        return g
    if _is_sphere_sdf(sdf):
        if _fused_smoothmin(sdf, p):
            g = sphere_smoothmin(sdf, p)[1]  # fused gradient + its double backward
        else:
            with torch.enable_grad():
                q = p.clone().requires_grad_(True)
                out = sphere_part(sdf, q)
                (g,) = torch.autograd.grad(out, q, torch.ones_like(out), create_graph=True)
        return g + input_gradient(sdf.shift, p)
    raise _lib.NrtError(f"SDF callable {type(sdf).__name__} has no HIP training path")


# ---- shading (integrators.py:139-206 with emitter_samples=1, bsdf_samples=0) -----------------

def _per_camera(t, p):
    """A [L, 3] light tensor broadcast like the reference's t[:, None, None, None, :] against
    points p [N, ..., 3]: one row for every camera, or row n for camera n (L == N)."""
    rows = t.reshape(-1, 3).to(p.device)
    if rows.shape[0] == 1 or p.dim() < 2:
        return rows[0]
    if rows.shape[0] != p.shape[0]:
        raise _lib.NrtError(f"PointLights with {rows.shape[0]} locations / intensities for "
                            f"{p.shape[0]} cameras")
    return rows.reshape(rows.shape[0], *([1] * (p.dim() - 2)), 3)


def light_sample(lights, it, active):
    """lights.sample_direction + sample_emitter_dir_wo_isect (scene.py:321-324)
    -> (d, Le, pdf, dist); dist is None for a LightField (lights.py:181-183)."""
    from .lights.lights import LightField, PointLights, RendererPointLights
    p = it.p
    if isinstance(lights, LightField):
        # lights.py:175-195, on the active rows through one integer index (one host sync for
        # its length; the boolean gather and scatters took one each, and their backwards more)
        flat = p.reshape(-1, 3)
        aidx = torch.nonzero(active.reshape(-1)).squeeze(1)
        v = lights.light_field_approx(flat.index_select(0, aidx))
        d = torch.zeros_like(flat).index_put(
            (aidx,), F.normalize(v, eps=1e-6, dim=-1).clamp(min=1e-6, max=1)).reshape(p.shape)
        le = torch.zeros_like(flat).index_put(
            (aidx,), torch.linalg.norm(v, ord=2, dim=-1, keepdim=True) *
            lights.color.sigmoid()).reshape(p.shape)
        pdf = torch.ones(p.shape[:-1], device=p.device)
        dist = None
    elif isinstance(lights, PointLights):
        # lights.py:89-110: location[:, None, None, None, :] against p [N, W, H, B, 3] (one
        # light, or one per camera)
        loc = _per_camera(lights.location, p)
        d = loc - p
        dist = torch.linalg.norm(d, dim=-1, keepdim=True)
        d = F.normalize(d, eps=1e-6, dim=-1)
        fall = lights.const.clamp(min=1e-6).to(p.device) + \
            lights.linear.clamp(min=1e-6).to(p.device) * dist + \
            lights.square.clamp(min=1e-6).to(p.device) * dist.square()
        color = _per_camera(lights.intensity, p)
        le = lights.scale.to(p.device) * F.normalize(color, dim=-1) / fall.clamp(min=1e-6)
        pdf = torch.ones(p.shape[:-1], device=p.device)
    elif isinstance(lights, RendererPointLights):
        # renderer/lighting.py:285-304 (one light): d (loc - p) / (1e-7 + dist), scale I / (..)^2
        lights.single()
        d = lights.location.reshape(-1, 3)[0].to(p.device) - p
        dist = (d * d).sum(dim=-1, keepdim=True).sqrt()
        inv = (1e-7 + dist).reciprocal()
        d = d * inv
        le = lights.scale * lights.intensity.reshape(-1, 3)[0].to(p.device) * inv * inv
        pdf = torch.ones(p.shape[:-1], device=p.device)
    else:
        raise _lib.NrtError(f"light {type(lights).__name__} has no HIP training path")
    le = torch.where(active.unsqueeze(-1), le, torch.zeros_like(le))
    return d, le, pdf, dist


def shadowed_light(shapes, lights, it, active, w_isect):
    """sample_emitter_dir_w_isect / _w_learned_occ (scene.py:290-319) with autograd: the shadow
    march is gradient-free in the reference too (intersect_test runs under no_grad, sdfs.py:
    170-179) and runs on the fused kernel; Le is masked (w_isect=True) or scaled by
    sigmoid(occ([p, dir_to_elev_azim(d)])) where occluded (w_isect=<occlusion MLP>)."""
    from .utils import dir_to_elev_azim
    d, le, pdf, dist = light_sample(lights, it, active)
    if dist is None:
        raise _lib.NrtError("shadow rays need a PointLights (ds.dist, scene.py:296)")
    rays = torch.cat([it.p, d], dim=-1).detach()
    with torch.no_grad():
        visible = shapes.intersect_test(rays, max_t=dist.detach().reshape_as(active)[..., None],
                                        active=active)
    if w_isect is True:
        le = torch.where((~visible | ~active).unsqueeze(-1), torch.zeros_like(le), le)
    else:
        occ_rays = torch.cat([it.p, dir_to_elev_azim(d)], dim=-1)
        le = torch.where((~visible)[..., None], w_isect(occ_rays).sigmoid() * le, le)
        le = active[..., None] * le
    return d, le, pdf


def bsdf_eval(bsdf, it, wo, active, feat=None):
    """eval_and_pdf of the supported BSDFs (bsdfs.py:108-118, 176-189, 271-291, 364-388, 434-453,
    515-536, 634-637).
    `feat`: param_rusin2(it.wi, wo) when the caller already has it."""
    from .bsdf.bsdfs import (Bidirectional, ComposeSpatialVarying, Conductor, Diffuse, NeuralBSDF,
                             Phong, Plastic, identity_div_pi)
    from .neural_blocks import mlp_multi, same_shape
    if isinstance(bsdf, Bidirectional):
        # bsdfs.py:434-453: the back side at (invert_z(wi), invert_z(wo)), the frame unchanged
        import copy
        cos_i = it.wi[..., 2]
        front, back = (cos_i > 0) & active, (cos_i < 0) & active
        f_f, p_f = bsdf_eval(bsdf.front, it, wo, front)
        flipped = copy.copy(it)
        flipped.wi = invert_z(it.wi)
        f_b, p_b = bsdf_eval(bsdf.back, flipped, invert_z(wo), back)
        f = torch.where(front.unsqueeze(-1), f_f,
                        torch.where(back.unsqueeze(-1), f_b, torch.zeros_like(f_b)))
        pdf = torch.where(front, p_f, torch.where(back, p_b, torch.zeros_like(p_b)))
        return f, pdf
    if isinstance(bsdf, Phong):
        # bsdfs.py:176-189: the world normal against the local wi, as written there
        R = reflect(_world_normal(it), it.wi)
        expo = bsdf.min_spec + bsdf.shine.to(wo.device).exp()
        spectral = (R * wo).sum(dim=-1).clamp(min=1e-20).pow(expo)
        f = it.wi[..., 2].unsqueeze(-1) * bsdf.diffuse.to(wo.device) / math.pi + \
            spectral.unsqueeze(-1) * bsdf.specular.to(wo.device) / math.pi
        return f, wo[..., 2] / math.pi
    if isinstance(bsdf, Plastic):
        # bsdfs.py:271-291; eta is a Python float there and carries no gradient
        f_i = fresnel(it.wi[..., 2], bsdf.eta)
        f_o = fresnel(wo[..., 2], bsdf.eta)
        pdf = wo[..., 2] / math.pi
        f = (bsdf.diffuse.to(wo.device).expand_as(it.p) / (1 - bsdf.fdr_int)) * bsdf.inv_eta_2 * \
            (pdf * (1 - f_i) * (1 - f_o)).unsqueeze(-1)
        ssw = bsdf.spec_sample_weight().to(wo.device)
        prob_specular = ssw * f_i
        prob_diffuse = (1 - f_i) * (1 - ssw)
        prob_diffuse = prob_diffuse / (prob_specular + prob_diffuse)
        return f, pdf * prob_diffuse
    if isinstance(bsdf, ComposeSpatialVarying):
        k = bsdf.sp_var_fn(bsdf.preprocess(it.p)).reshape(it.p.shape[:-1] + (len(bsdf.bsdfs),))
        setattr(it, "nonnormalized_weights", k)
        k = k.sigmoid()
        # every NeuralBSDF of the mixture reads the same Rusinkiewicz features of (wi, wo): the
        # reference recomputes them per component (bsdfs.py:634-637); computing them once gives
        # the same values and the same gradient (autograd sums the components' contributions),
        # with ~40 forward and ~80 backward launches per component fewer
        neural = [b for b in bsdf.bsdfs if isinstance(b, NeuralBSDF)]
        pre = {}
        if len(neural) > 1:
            feat = param_rusin2(it.wi, wo)
            mlps = [b.mlp for b in neural]
            if same_shape(mlps) and not any(m.latent_size for m in mlps):
                # the components' MLPs on the shared features: one batched HIP backward
                pre = {id(b): y for b, y in zip(neural, mlp_multi(mlps, feat))}
        parts = []
        for b in bsdf.bsdfs:
            if id(b) in pre:
                f = b.act(pre[id(b)])
                pdf = torch.ones(f.shape[:-1], device=f.device)
            else:
                f, pdf = bsdf_eval(b, it, wo, active, feat if isinstance(b, NeuralBSDF) else None)
            parts.append(torch.cat([f, pdf.reshape(f.shape[:-1] + (1,))], dim=-1))
        spec_pdf = torch.stack(parts, dim=-1)
        setattr(it, "normalized_weights", k)
        spec_pdf = torch.where(active[..., None, None], spec_pdf * k.unsqueeze(-2),
                               torch.zeros_like(spec_pdf))
        f, pdf = spec_pdf.sum(dim=-1).split([3, 1], dim=-1)
        return f, pdf.squeeze(-1)
    if isinstance(bsdf, NeuralBSDF):
        f = bsdf.act(bsdf.mlp(param_rusin2(it.wi, wo) if feat is None else feat))
        return f, torch.ones(f.shape[:-1], device=f.device)
    if isinstance(bsdf, Diffuse):
        refl = bsdf.reflectance.to(wo.device)
        x = wo[..., 2].unsqueeze(-1) * refl
        f = x / math.pi if bsdf.preproc is identity_div_pi else bsdf.preproc(x)
        return f, wo[..., 2] / math.pi
    if isinstance(bsdf, Conductor):
        refl = local_reflect(it.wi)
        thresh = (refl * wo).sum(dim=-1, keepdim=True) > 0.94
        # eta carries no gradient, as in the reference: Conductor.eval_and_pdf passes
        # F.softplus(self.eta) into the @torch.jit.script fresnel_conductor whose eta_r parameter
        # is annotated `float` (bsdfs.py:327-328, 371), so the scripted call receives a plain number
        # and its result has requires_grad=False
        fres = fresnel_conductor(it.wi[..., 2], float(F.softplus(bsdf.eta.detach())), 0.0)
        fres = fres.reshape_as(thresh)
        f = torch.where(thresh, fres * bsdf.act(bsdf.specular.to(wo.device)),
                        torch.zeros_like(it.p))
        pdf = torch.where(thresh.reshape(it.p.shape[:-1]), 1.0, 0.0)
        f = torch.where(active.unsqueeze(-1), f, torch.zeros_like(f))
        return f, pdf
    raise _lib.NrtError(f"BSDF {type(bsdf).__name__} has no HIP training path")


def direct_sample(it, active, bsdf, lights, lead, device, shapes=None, w_isect=False):
    """Direct.sample's shading with autograd (integrators.py:167-189); w_isect as in
    integrators.py:161-166 (True: shadow rays, an MLP: learned occlusion)."""
    from .neural_blocks import SkipConnMLP
    result = torch.zeros(*lead, 3, device=device)
    if not bool(active.any()):
        return result
    if w_isect is True or type(w_isect) is SkipConnMLP:
        d, le, pdf = shadowed_light(shapes, lights, it, active, w_isect)
    else:
        d, le, pdf, _ = light_sample(lights, it, active)
    ae = active & (pdf > 0)
    wo = it.to_local(d)
    f, _ = bsdf_eval(bsdf, it, wo, ae)
    # result[ae] += f[ae] le[ae] without the boolean gathers' host syncs (both are finite and
    # zero outside ae: light_sample / bsdf_eval mask them)
    return torch.where(ae.unsqueeze(-1), result + f * le, result)


def bounce_uniforms(bsdf, sampler, lead, P, dev, injected=None):
    """One bounce's BSDF-sampling randomness -> (u_comp [P, nc, 2], u_sel [P], u_lobe [P, nc] or
    None).  Drawn in the reference's order: per component, in component order, a Plastic's lobe
    draw sampler.sample(p_spec.shape) (bsdfs.py:304) and then the component's (.., 2) draw
    (:98, :163, :309, :628); the selection draw last.  `injected`: (u_comp, u_sel[, u_lobe])."""
    from .bsdf.bsdfs import Plastic
    parts = getattr(bsdf, "bsdfs", [bsdf])
    nc = len(parts)
    plastic = [isinstance(b, Plastic) for b in parts]
    if injected is not None:
        u = [t.to(dev).float().reshape(P, -1).contiguous() for t in injected]
        if any(plastic) and len(u) < 3:
            raise _lib.NrtError("uniforms need (u_comp, u_sel, u_lobe) for a Plastic component")
        return u[0], u[1], (u[2] if any(plastic) else None)
    draws, lobes = [], []
    for is_plastic in plastic:
        if is_plastic:
            lobes.append(sampler.sample(tuple(lead)).to(dev).reshape(P, 1))
        elif any(plastic):
            lobes.append(torch.zeros(P, 1, device=dev))
        draws.append(sampler.sample(tuple(lead) + (2,), device=dev).reshape(P, 1, 2))
    u_comp = torch.cat(draws, dim=1).contiguous()
    u_sel = sampler.sample((P,), device=dev).contiguous()
    return u_comp, u_sel, (torch.cat(lobes, dim=1).contiguous() if any(plastic) else None)


def path_bounce(bh, lh, sh, shadow, occ, max_steps, eps, p, n, wi, P, act, thr, res, u_comp, u_sel,
                u_lobe, rays_out, ws):
    """nrt_path_bounce, or nrt_path_bounce_ex when the mixture has a Plastic lobe draw."""
    if u_lobe is None:
        _lib.call("nrt_path_bounce", bh, lh, sh, shadow, occ, max_steps, eps, p, n, wi, P, act, thr,
                  res, _lib.ptr(u_comp), _lib.ptr(u_sel), rays_out, ws, _lib.precision_code(),
                  _lib.stream())
    else:
        _lib.call("nrt_path_bounce_ex", bh, lh, sh, shadow, occ, max_steps, eps, p, n, wi, P, act,
                  thr, res, _lib.ptr(u_comp), _lib.ptr(u_sel), _lib.ptr(u_lobe), rays_out, ws,
                  _lib.precision_code(), _lib.stream())


def path_sample(shapes, rays, bsdf, lights, max_depth, training, sampler, uniforms=None,
                w_isect=False):
    """Path.sample with autograd (integrators.py:275-354).  Per bounce the emitter term is
    ``direct_sample`` on the current interaction (gradients through its normals and point, the
    BSDF and the light) times the throughput, which the reference detaches after every BSDF
    sample (:335-337).  The BSDF sample itself needs no gradient: ``nrt_path_bounce`` draws it on
    the detached interaction with the same uniforms the no-grad Path uses, and updates the
    (detached) throughput and the active mask.  The spawned rays are then rebuilt with autograd
    -- origin p, direction from_local(wo) through the differentiable frame (:345,
    interaction.py:57) -- so the secondary intersection's points and normals carry gradients as
    in the reference."""
    from .shapes.sdfs import sdf_handle
    from .integrators.integrators import _bsdf_handle, _emitter_mode, _light_handle
    dev = rays.device
    lead = rays.shape[:-1]
    it, active = shapes.intersect(rays, primary=training)
    result = torch.zeros(*lead, 3, device=dev)
    if not bool(active.any()):
        return result, active, it
    original_active = active.clone()
    shadow, occ = _emitter_mode(w_isect)
    P = active.numel()
    act = active.reshape(-1).to(torch.uint8).contiguous()
    thr = torch.ones(P, 3, device=dev)      # detached throughput, updated by the bounce
    scratch = torch.zeros(P, 3, device=dev)  # the bounce's own (gradient-free) emitter sum
    rays_out = torch.empty(P, 6, device=dev)
    lib = _lib.load(require_device=True)
    ws = torch.empty(lib.nrt_path_workspace_bytes(P), dtype=torch.uint8, device=dev)
    sh = sdf_handle(shapes.sdf)
    curr = it
    for depth in range(max_depth):
        cur = act.bool().reshape(lead)
        term = direct_sample(curr, cur, bsdf, lights, lead, dev, shapes, w_isect)
        # a snapshot: autograd keeps this factor for the backward, and the bounce below updates
        # `thr` in place through a raw pointer (no version bump for autograd to catch)
        result = result + thr.clone().reshape(*lead, 3) * term
        u_comp, u_sel, u_lobe = bounce_uniforms(bsdf, sampler, lead, P, dev,
                                                uniforms[depth] if uniforms is not None else None)
        with torch.no_grad():
            cp = curr.p.detach().reshape(P, 3).contiguous()
            cn = curr.n.detach().reshape(P, 3).contiguous()
            cw = curr.wi.detach().reshape(P, 3).contiguous()
            path_bounce(_bsdf_handle(bsdf), _light_handle(lights), sh, shadow, occ,
                        int(shapes.max_steps), float(shapes.epsilon), _lib.ptr(cp), _lib.ptr(cn),
                        _lib.ptr(cw), P, _lib.ptr(act), _lib.ptr(thr), _lib.ptr(scratch),
                        u_comp, u_sel, u_lobe, _lib.ptr(rays_out), _lib.ptr(ws))
        if depth + 1 == max_depth or not bool(act.any()):
            break  # the reference's last spawn is never shaded (:309, :342)
        # the sampled local direction carries no gradient in the reference either: NeuralBSDF /
        # Diffuse sample wo from the cosine hemisphere at the sampler's uniforms (bsdfs.py:90-106,
        # 625-633), independent of the geometry; the Conductor's reflect(it.wi) (:396) would, but
        # Conductor.sample fails in the reference and nrt_path_bounce refuses it.  The world
        # direction is rebuilt through the differentiable frame, as spawn_rays(from_local(wo)).
        with torch.no_grad():
            wo = curr.to_local(rays_out[:, 3:].reshape(*lead, 3))
        d = curr.from_local(wo.detach())
        curr, hits = shapes.intersect(curr.spawn_rays(d), primary=False)
        act &= hits.reshape(-1).to(torch.uint8)
        if not bool(act.any()):
            break
    return result, original_active, it
