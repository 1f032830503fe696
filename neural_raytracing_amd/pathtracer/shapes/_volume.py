"""The reference's volume rendering (nerf.py:46-74 PlainNeRF, :175-214 NeRFLE) as one autograd
Function on the HIP training kernels: sample points, first MLP, input assembly, second MLP and
the rolled-cumprod compositing forward; their backwards and the light / latent reductions in
reverse (csrc/nrt_nerf_train.hip between the MLP kernels of ``_MlpFn``)."""
import torch

from ... import _lib
from .._handles import train_handle
from ..neural_blocks import (_check_versions, _forward_saving, _mlp_forward, _save_versions,
                             mlp_first_order)


class VolumeSpec:
    """What one render needs besides tensors: the model selector, its two MLPs, how many rays
    share a row of ``extra`` (PlainNeRF's latent: one camera's; NeRFLE's light encoding: one
    camera's with one light per camera, else all) and the chunk bound in rays."""

    def __init__(self, model, first, second, steps, rays_per_row, max_rays):
        self.model = model
        self.first, self.second = first, second
        self.steps = steps
        self.rays_per_row = rays_per_row
        self.max_rays = max(1, max_rays)
        self.plain = model == _lib.NRT_NERF_PLAIN
        # PlainNeRF: first_out = [alpha | intermediate (I)]; NeRFLE: [alpha | latent (64)]
        self.inter = first.out.out_features - 1


def chunks(P, per, cmax):
    """(first ray, rays, first latent row, latent rows, rays per latent row) of each call: whole
    cameras while one fits in ``cmax`` rays, else pieces of one camera's rays."""
    r0 = 0
    while r0 < P:
        cam = r0 // per
        if per <= cmax:
            n = min((cmax // per) * per, P - r0)
            rows, rpl = n // per, per
        else:
            n = min(cmax, (cam + 1) * per - r0)
            rows, rpl = 1, n
        yield r0, n, cam, rows, rpl
        r0 += n


def _points(spec, rays, ts, lat, rpl):
    n, S = rays.shape[0], spec.steps
    pts = torch.empty(S * n, 3, device=rays.device)
    lat1 = torch.empty(S * n, lat.shape[1], device=rays.device) if spec.plain else None
    _lib.call("nrt_nerf_points", spec.model, _lib.ptr(rays), n, _lib.ptr(ts), S,
              _lib.ptr(lat) if spec.plain else None, lat.shape[-1], rpl, _lib.ptr(pts),
              _lib.ptr(lat1), _lib.stream())
    return pts, lat1


def _assemble(spec, first_out, rays, extra, rpl, noise):
    n, S, dev = rays.shape[0], spec.steps, rays.device
    dim = extra.shape[-1]
    if spec.plain:
        x2 = torch.empty(S * n, 2, device=dev)
        lat2 = torch.empty(S * n, spec.inter + dim, device=dev)
    else:
        x2, lat2 = torch.empty(S * n, 67 + dim, device=dev), None
    alpha_raw = torch.empty(S, n, device=dev)
    _lib.call("nrt_nerf_assemble", spec.model, _lib.ptr(first_out), _lib.ptr(rays), n, S,
              _lib.ptr(extra), dim, spec.inter, rpl, _lib.ptr(noise), _lib.ptr(x2),
              _lib.ptr(lat2), _lib.ptr(alpha_raw), _lib.stream())
    return x2, lat2, alpha_raw


def _mlp(mlp, handle, x, lat):
    """(y, saved activations or None): the forward _MlpFn would run for this MLP."""
    if lat is None:
        ys, save = _forward_saving([handle], x, [mlp.out.out_features], keep=mlp.training)
        return ys[0], save
    return _mlp_forward(mlp, x, lat, handle), None


def _add(total, part):
    if total is None:
        return part
    return [b if a is None else (a if b is None else a.add_(b)) for a, b in zip(total, part)]


class _VolumeFn(torch.autograd.Function):
    """rgb [P, 3] = volume render of rays [P, 6] with gradients for every nn.Linear weight and
    bias of both MLPs, for ``extra`` (PlainNeRF's latent [N, L]; NeRFLE's light encoding
    [rows, LK], one row or one per camera) and for the rays (learnable cameras: both MLPs' dx
    into ``nrt_nerf_rays_backward``; asked for only when the rays take a gradient).  Per sample
    it keeps first_out and rgb_raw (and what the MLPs' forwards save); the backward computes the
    points and the assembled inputs again."""

    @staticmethod
    def forward(ctx, spec, rays, ts, extra, noise, *params):
        _lib.load(require_device=True)
        h1, h2 = train_handle(spec.first), train_handle(spec.second)  # re-pack after a step
        ex = extra.detach()
        P, S = rays.shape[0], spec.steps
        out = torch.empty(P, 3, device=rays.device)
        kept = []
        with torch.no_grad():
            for r0, n, row0, rows, rpl in chunks(P, spec.rays_per_row, spec.max_rays):
                r = rays[r0:r0 + n]
                e = ex[row0:row0 + rows]
                nz = None if noise is None else noise[:, r0:r0 + n].contiguous()
                pts, lat1 = _points(spec, r, ts, e, rpl)
                first_out, save1 = _mlp(spec.first, h1, pts, lat1)
                del pts, lat1
                x2, lat2, alpha_raw = _assemble(spec, first_out, r, e, rpl, nz)
                rgb_raw, save2 = _mlp(spec.second, h2, x2, lat2)
                del x2, lat2
                _lib.call("nrt_nerf_composite_forward", spec.model, _lib.ptr(alpha_raw),
                          _lib.ptr(rgb_raw), _lib.ptr(ts), n, S, _lib.ptr(out[r0:r0 + n]),
                          _lib.stream())
                kept.append((r0, n, row0, rows, rpl, first_out, rgb_raw, save1, save2))
        ctx.spec, ctx.kept, ctx.handles = spec, kept, (h1, h2)
        ctx.rays, ctx.ts, ctx.extra, ctx.noise = rays, ts, ex, noise
        # the backward reads the latent / light encoding again too (ex shares extra's storage)
        _save_versions(ctx, [*params, extra])
        return out

    @staticmethod
    def backward(ctx, d_out):
        _check_versions(ctx)
        if torch.is_grad_enabled():
            raise _lib.NrtError("second derivatives through the volume render are not on the HIP "
                                "path")
        lib = _lib.load(require_device=True)
        spec, (h1, h2) = ctx.spec, ctx.handles
        rays, ts, ex = ctx.rays, ctx.ts, ctx.extra
        S, dev = spec.steps, rays.device
        dim = ex.shape[-1]
        d_out = d_out.detach().float().reshape(-1, 3).contiguous()
        want_extra, want_rays = ctx.needs_input_grad[3], ctx.needs_input_grad[1]
        d_rays = torch.empty_like(rays) if want_rays else None
        d_extra = torch.zeros_like(ex) if want_extra else None
        g1 = g2 = None
        for r0, n, row0, rows, rpl, first_out, rgb_raw, save1, save2 in ctx.kept:
            r = rays[r0:r0 + n]
            e = ex[row0:row0 + rows]
            nz = None if ctx.noise is None else ctx.noise[:, r0:r0 + n].contiguous()
            # (each intermediate is dropped after its last reader: the MLP backwards' own
            # workspaces set the peak)
            x2, lat2, alpha_raw = _assemble(spec, first_out, r, e, rpl, nz)
            ws = torch.empty(lib.nrt_nerf_volume_workspace_bytes(n, S, dim), dtype=torch.uint8,
                             device=dev)
            d_alpha = torch.empty(S, n, device=dev)
            d_rgb = torch.empty(S * n, 3, device=dev)
            _lib.call("nrt_nerf_composite_backward", spec.model, _lib.ptr(alpha_raw),
                      _lib.ptr(rgb_raw), _lib.ptr(ts), n, S, _lib.ptr(d_out[r0:r0 + n]),
                      _lib.ptr(d_alpha), _lib.ptr(d_rgb), _lib.ptr(ws), _lib.stream())
            del alpha_raw
            # NeRFLE's first MLP reads the second's dx, PlainNeRF's its dlatent
            dx2, dlat2, gr2 = mlp_first_order(spec.second, h2, save2, x2, lat2, d_rgb,
                                              not spec.plain or want_rays, spec.plain)
            d_second = dlat2 if spec.plain else dx2
            d_dir = dx2 if want_rays else None  # the second MLP's dx: the rays' direction term
            del x2, lat2, d_rgb, dx2, dlat2
            d_first_out = torch.empty_like(first_out)
            _lib.call("nrt_nerf_assemble_backward", spec.model, _lib.ptr(d_alpha),
                      _lib.ptr(d_second), n, S, dim, spec.inter, _lib.ptr(d_first_out),
                      _lib.stream())
            del d_alpha
            part = None
            if want_extra:
                part = torch.empty(rows, dim, device=dev)
            if want_extra and not spec.plain:
                _lib.call("nrt_nerf_reduce", spec.model, None, _lib.ptr(d_second), n, S, dim,
                          spec.inter, rpl, _lib.ptr(part), _lib.ptr(ws), _lib.stream())
                d_extra[row0:row0 + rows] += part
            if not spec.plain:
                d_second = None
            pts, lat1 = _points(spec, r, ts, e, rpl)
            d_pts, dlat1, gr1 = mlp_first_order(spec.first, h1, save1, pts, lat1, d_first_out,
                                                want_rays, spec.plain and want_extra)
            del pts, lat1, d_first_out
            if want_rays:
                _lib.call("nrt_nerf_rays_backward", spec.model, _lib.ptr(r), n, _lib.ptr(ts), S,
                          _lib.ptr(d_pts), _lib.ptr(d_dir), d_dir.shape[1],
                          _lib.ptr(d_rays[r0:r0 + n]), _lib.stream())
            del d_pts, d_dir
            if want_extra and spec.plain:
                _lib.call("nrt_nerf_reduce", spec.model, _lib.ptr(dlat1), _lib.ptr(d_second), n, S,
                          dim, spec.inter, rpl, _lib.ptr(part), _lib.ptr(ws), _lib.stream())
                d_extra[row0:row0 + rows] += part
            g1, g2 = _add(g1, gr1), _add(g2, gr2)
        if g1 is None:  # no rays
            g1 = [None] * (2 * len(spec.first._linears()))
            g2 = [None] * (2 * len(spec.second._linears()))
        return (None, d_rays, None, d_extra, None, *g1, *g2)


def render_volume(spec, rays, ts, extra, noise=None):
    """``_VolumeFn`` on rays [P, 6], depths ts [S] and ``extra`` (latent [N, L] or light
    encoding [rows, LK], a plain [LK] being one row; float32 on the rays' device, its graph
    kept)."""
    if extra.dim() == 1:
        extra = extra.reshape(1, -1)
    params = [t for m in (spec.first, spec.second) for lin in m._linears()
              for t in (lin.weight, lin.bias)]
    if any(t.device != rays.device for t in params):
        raise _lib.NrtError("the NeRF's parameters and the rays are on different devices: move "
                            "the module to the GPU (.to(device)) to train it")
    return _VolumeFn.apply(spec, rays, ts, extra.contiguous(), noise, *params)
