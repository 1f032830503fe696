"""Host model of the alpha scan (nrt_march_params.primary = 2, include/nrt.h) on the oracle, and
the ray sets that tests/test_gpu_scan_saturate.py marches; tests/test_scan_saturate_host.py checks
both without a GPU.

The model counts SDF evaluations per ray as the ring marches make them:
  exact      march steps + 129 scan samples + sdf(best)                      (primary = 1)
  in order   the scan stops at its first sample d <= SAT; a ray that has one gets no sdf(best)
  wrap       the same, but a hit ray visits j0, ..., 128, 0, ..., j0 - 1 with
             j0 = min(128, floor(t / step) + 2)
  segments   the 8 segments [0,16], [17,32], ..., [113,128] each stop at their own first
             saturating sample (the tail rays of a launch)
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pathtracer_ref as R
from tests.helpers import blob

SAT = float(np.float32(-0.02))   # the sample test, d <= -0.02f
SAT_THR = 20.0                   # the throughput of a ray that has such a sample
SIGMOID_ONE = 17.33              # f32 sigmoid(x) == 1.0f from here on (see the host test)
EPS, MAX_T, MAX_STEPS, SCAN_MAX_T = 5e-3, 10.0, 64, 2.2   # tests.helpers.intersect_poisoned's
MARGIN = 1e-3        # tests/test_gpu_line_stage.py's: min |d - eps| over a ray's march steps
SAT_MARGIN = 1e-3    # no scan sample this close to SAT: FP16 (7.3e-5) and FP32 agree on the class
J0_MARGIN = 0.02     # a hit's t / step this far from an integer: the device's j0 is the model's
SIZES = [(2061, 1), (6157, 3)]   # (rays, march_blocks), as the line-stage tests: a 13-ray last line
THROUGH, GRAZE, NEAR, FAR = 0, 1, 2, 3
CLASS_NAMES = {THROUGH: "through", GRAZE: "graze", NEAR: "near", FAR: "far"}
SEGMENTS = [(0, 16)] + [(16 * q + 1, 16 * q + 16) for q in range(1, 8)]


def march_live(sdf, rays, max_steps=MAX_STEPS, eps=EPS, max_t=MAX_T):
    """sdfs.py:119-131 on live rays only: (t, hit, evaluations made, min |d - eps| over them)."""
    o, d = rays[:, :3], rays[:, 3:]
    P = rays.shape[0]
    t = torch.zeros(P)
    live = torch.ones(P, dtype=torch.bool)
    hit = torch.zeros(P, dtype=torch.bool)
    steps = torch.zeros(P, dtype=torch.long)
    margin = torch.full((P,), float("inf"))
    with torch.no_grad():
        for _ in range(max_steps):
            live = live & (t < max_t)
            k = live.nonzero().squeeze(-1)
            if k.numel() == 0:
                break
            dv = sdf(o[k] + d[k] * t[k, None]).reshape(-1)
            steps[k] += 1
            margin[k] = torch.minimum(margin[k], (dv - eps).abs())
            now = dv <= eps
            hit[k[now]] = True
            live[k[now]] = False
            t[k[~now]] = t[k[~now]] + dv[~now]
    return t, hit, steps, margin


def scan_samples(sdf, rays, scan_max_t=SCAN_MAX_T):
    """[P, 129] SDF values at the scan's grid (sdfs.py:241-245): sample j at o + (step j) d."""
    o, d = rays[:, :3], rays[:, 3:]
    step = scan_max_t / 128.0
    out = torch.empty(rays.shape[0], 129)
    with torch.no_grad():
        for j in range(129):
            out[:, j] = sdf(o + float(np.float32(step * j)) * d).reshape(-1)
    return out


def scan_thr(sdf, rays, samples, scan_max_t=SCAN_MAX_T):
    """the exact throughput -1000 sdf(o + idx step d) at the first argmin (sdfs.py:137, 246-249)"""
    step = scan_max_t / 128.0
    idx = samples.argmin(dim=1)  # (torch returns the first minimum, as the reference's strict <)
    ts = idx.float() * float(np.float32(step))
    with torch.no_grad():
        return -1000.0 * sdf(rays[:, :3] + ts[:, None] * rays[:, 3:]).reshape(-1), idx


def j0_of(t, hit, scan_max_t=SCAN_MAX_T):
    step = np.float32(scan_max_t / 128.0)
    q = np.floor(np.minimum(t.numpy().astype(np.float32) / step, np.float32(126.0))).astype(np.int64) + 2
    return torch.from_numpy(np.where(hit.numpy(), q, 0))


def _first_sat(vals):
    """per row: samples visited until the first one <= SAT (inclusive), or the row's length"""
    sat = vals <= SAT
    n = vals.shape[1]
    first = torch.where(sat.any(1), sat.float().argmax(1) + 1, torch.full((vals.shape[0],), n))
    return first, sat.any(1)


def scan_costs(samples, t, hit, steps, scan_max_t=SCAN_MAX_T):
    """evaluations per ray under each schedule (module docstring) and the saturation flag"""
    P = samples.shape[0]
    inorder, saturates = _first_sat(samples)
    j0 = j0_of(t, hit, scan_max_t)
    order = (j0[:, None] + torch.arange(129)[None, :]) % 129
    wrap, _ = _first_sat(torch.gather(samples, 1, order))
    segs = torch.zeros(P, dtype=torch.long)
    for a, b in SEGMENTS:
        segs += _first_sat(samples[:, a:b + 1])[0]
    best = (~saturates).long()  # sdf(best) only for a ray without a saturating sample
    return dict(exact=steps + 130, inorder=steps + inorder + best, wrap=steps + wrap + best,
                segments=steps + segs + best, wrap_scan=wrap, saturates=saturates, j0=j0)


# ---------------------------------------------------------------------------------------------
# the ray sets of the GPU tests
# ---------------------------------------------------------------------------------------------
POOL = 64  # rays of each class, at least


def _bisect(ref, u, level):
    lo, hi = torch.zeros(u.shape[0]), torch.ones(u.shape[0])
    with torch.no_grad():
        for _ in range(16):
            mid = 0.5 * (lo + hi)
            under = ref(u * mid[:, None]).reshape(-1) < level
            lo, hi = torch.where(under, mid, lo), torch.where(under, hi, mid)
    return u * hi[:, None]


def _tangents(ref, g, n, level):
    """rays through a point of the given SDF level, at right angles to the gradient there"""
    u = F.normalize(torch.randn(n, 3, generator=g), dim=-1)
    q = _bisect(ref, u, level)
    grad = R.MarchedSDF(sdf=ref).gradient(q)
    d = F.normalize(torch.linalg.cross(grad, torch.randn(n, 3, generator=g)), dim=-1)
    return torch.cat([q - 0.6 * d, d], -1)


@functools.lru_cache(maxsize=None)
def class_rays(hidden):
    """dict(ref, rays [P, 6], cls [P] and the oracle's t, hit, steps, margin, samples [P, 129],
    thr, idx of every ray) for the 8 x `hidden` shift, at the larger of SIZES (the smaller is its
    prefix).  Ray i is of class i % 4, taken in turn from that class's pool."""
    ref, _ = blob(32, hidden, 16, "softplus", seed=21, product=False)
    g = torch.Generator().manual_seed(2000 + hidden)
    n = 400
    u = F.normalize(torch.randn(n, 3, generator=g), dim=-1)
    through = torch.cat([0.9 * u, F.normalize(-u + 0.1 * torch.randn(n, 3, generator=g), dim=-1)], -1)
    # (a tangent ray that hits nears the surface slowly: some 2 % keep MARGIN at every step)
    ng = 30 * n
    graze = _tangents(ref, g, ng, -(0.006 + 0.014 * torch.rand(ng, generator=g)))
    near = _tangents(ref, g, n, 0.008 + 0.035 * torch.rand(n, generator=g))
    v = F.normalize(torch.randn(n // 2, 3, generator=g), dim=-1)
    far = torch.cat([12.0 * v, v], -1)
    cand = torch.cat([through, graze, near, far])
    want = torch.cat([torch.full((c.shape[0],), k) for k, c in
                      ((THROUGH, through), (GRAZE, graze), (NEAR, near), (FAR, far))])
    t, hit, steps, margin = march_live(ref, cand)
    frac = (t / (SCAN_MAX_T / 128.0)) % 1.0
    ok = (margin >= MARGIN) & (~hit | ((frac >= J0_MARGIN) & (frac <= 1 - J0_MARGIN)))
    ok &= hit == ((want == THROUGH) | (want == GRAZE))
    keep = ok.nonzero().squeeze(-1)  # only these are scanned
    cand, want, t, hit, steps, margin = (x[keep] for x in (cand, want, t, hit, steps, margin))
    s = scan_samples(ref, cand)
    smin = s.min(1).values
    ok = (s - SAT).abs().min(1).values >= SAT_MARGIN
    is_cls = {THROUGH: hit & (smin <= SAT), GRAZE: hit & (smin > -0.015) & (smin < 0),
              NEAR: ~hit & (smin > 0) & (smin < 0.05), FAR: ~hit & (smin >= 0.05)}
    pools = {}
    for k in (THROUGH, GRAZE, NEAR, FAR):
        pick = (ok & (want == k) & is_cls[k]).nonzero().squeeze(-1)
        assert pick.numel() >= POOL, f"{pick.numel()} {CLASS_NAMES[k]} rays, {POOL} needed"
        pools[k] = pick[:2 * POOL]
    P = max(p for p, _ in SIZES)
    i = torch.arange(P)
    cls = i % 4
    sel = torch.stack([pools[k][(i // 4) % pools[k].numel()] for k in (THROUGH, GRAZE, NEAR, FAR)])
    sel = sel[cls, i]
    rays = cand[sel].contiguous()
    thr, idx = scan_thr(ref, rays, s[sel])
    return dict(ref=ref, rays=rays, cls=cls, t=t[sel], hit=hit[sel], steps=steps[sel],
                margin=margin[sel], samples=s[sel], thr=thr, idx=idx)
