"""The FP32 ring engine (k_march32, k_scan_best32, k_normal32, k_occl32: nrt_device.h ring32) and the
fp32-split ring engine (k_march3, k_scan_best3, k_normal3, k_occl3, k_sdf_eval3: nrt_ring3.h) across
the descriptor space ring32_supported / ring3_supported (nrt_launch.h) admit, not only at the
F = 16 / 32, 8-layer, skip-3 shapes the scenes use: encodings that leave 1, 2, 3 and 4 live k-steps
in the last encoding quad on both ke = 48 and ke = 80 (seg4's nl branches and the split stream's
slot arithmetic), 1 .. 18 layers, skip periods 1, 2, 3, 4 and past the depth, sphere tables from
none (a bare MLP) to the last count that fits the block's LDS, the first count that does not
(which must run, and meet the same bars, on the per-wave kernels), and an MLP with 16 outputs.

Every comparison observes single SDF evaluations, where float64 is a well-defined reference for
every ray (a whole march is discontinuous at each hit decision):

    march     max_steps = 1, primary = 0: hit = (d(o) <= eps), t = d(o) on the other rays
    scan      primary = 1: throughput / -1000 against the float64 minimum over the 129 scan points
    normals   the hit rays of the one-step march stand at t = 0: raw_n = grad d(o); n; p
    occlusion max_steps = 1: visible = (d(o + 100 eps dir) >= eps)
    eval      nrt_sdf_eval at the origins under fp32-split

The bar, per compared tensor, is the descriptor sweep's (tests/test_gpu_mlp_descriptor_sweep.py):

    err <= max(1e-4 * scale, 4 * e32)

with e32 the error of the same oracle computation in float32 on the CPU and scale the part the
engines compute on the matrix cores -- max|MLP part| over the compared points (values), max
||grad MLP part|| (raw normals) -- so that the sphere term cannot carry an MLP error.  hit and
visible are compared exactly on every ray whose float64 value is further than the value bar from
eps.  tests/test_ring_sweep_host.py holds the table to the engines' gate and the references to the
conditions that make this bar mean what it reads.

What the profile can tell apart: the ring kernels have names of their own; the per-wave ("slab")
march has none (the scope k_intersect wraps every march), its normal pass is k_sdf_grad.  A case
that fits asserts its ring kernels ran and k_sdf_grad did not; the over-size case the reverse.

This module imports without a device (the host test reads its table and references)."""
import collections
import ctypes
import functools
import math
import random

import pytest
import torch
import torch.nn.functional as F

from oracle import pathtracer_ref as R
from tests.helpers import copy_mlp, double_copy, intersect_poisoned, seeded
from tests.report import report

Case = collections.namedtuple("Case", "hidden freqs layers skip activation spheres out gain seed")

P = 333          # ragged against 16-ray tiles, 64-lane waves and 8-wave blocks
EPS = 5e-3
MAX_T = 10.0
BOX = 0.6        # origins uniform in |x| <= BOX
AMP = 0.15       # max |MLP part - its mean| over the origins after the out layer's scaling
HITS = 84        # the out bias puts eps midway between the 84th and 85th smallest d(o)
ENGINES = ("fp32", "fp32-split")
LDS = 160 * 1024 - 1024  # kLdsBytes less kRingLdsReserve (nrt_launch.h)

# gain: every hidden nn.Linear weight of the oracle MLP is multiplied by it before the out layer
# is scaled, so that a deep MLP's output still varies over the box (at the default init an
# 18-layer softplus MLP is a constant to six digits and the scaling would only amplify float32
# noise); seed: of the weights, spheres and rays, picked so that every condition of
# tests/test_ring_sweep_host.py holds (hit counts, scale, e32, leaky kinks).
CASES = {
    #                  H   F   L skip activation  spheres out gain seed
    # ke = 48: nl = 1, 2, 3, 4, and the anchor F = 16
    "f15":       Case(128, 15, 3, 1, "softplus", 1, 1, 1.0, 1),
    "f18":       Case(256, 18, 5, 2, "leaky_relu", 3, 1, 1.5, 23),
    "f20":       Case(128, 20, 8, 3, "leaky_relu", 6, 1, 1.5, 3),
    # skip past the depth: layer 0 is the only skip layer
    "f22":       Case(256, 22, 2, 4, "softplus", 13, 1, 1.0, 4),
    # ke = 80: nl = 1, 2, 3, 4, and the anchor F = 32
    # one hidden layer: no skip layer at all
    "f31":       Case(256, 31, 1, 3, "softplus", 33, 1, 1.0, 5),
    "f34":       Case(128, 34, 12, 4, "softplus", 100, 1, 2.0, 6),
    # kMaxLin; a bare MLP
    "f35":       Case(256, 35, 18, 3, "softplus", 0, 1, 2.2, 7),
    # a bare MLP with 16 outputs, the SDF its row 0
    "f38_out16": Case(128, 38, 3, 1, "leaky_relu", 0, 16, 1.5, 8),
    "f32":       Case(128, 32, 8, 3, "softplus", 64, 1, 1.5, 9),
    # the LDS boundary at the headline's shape (F = 16 anchor): the last sphere count whose table
    # fits beside the FP32 ring's 128 KiB, and the first that does not
    "lds_fit":   Case(256, 16, 8, 3, "softplus", 332, 1, 1.5, 10),
    "lds_over":  Case(256, 16, 8, 3, "softplus", 333, 1, 1.5, 10),
    # ... and at 128 wide, where the ring is 64 KiB (split: 96 KiB) and the gate's other clause
    # binds: the last count whose bias and sphere tables take no more than 48 KiB, and the first
    # past it (the F = 32 shape of the training SDF)
    "lds48_fit":  Case(128, 32, 8, 3, "softplus", 688, 1, 1.5, 11),
    "lds48_over": Case(128, 32, 8, 3, "softplus", 689, 1, 1.5, 11),
}
# {the first entry past a clause of the LDS condition: the last entry that meets it}
OVERSIZE = {"lds_over": "lds_fit", "lds48_over": "lds48_fit"}
FITTING = [n for n in CASES if n not in OVERSIZE]
# the first 1 and the first 17 rays of one nl > 1 case (ke = 48 and ke = 80 between the engines)
RAGGED = {"fp32": "f20", "fp32-split": "f34"}
# nrt_mlp_refresh on these encodings: one nl > 1 case per ke
REFRESH = ("f18", "f34")


# ---------------------------------------------------------------------------------------------
# the engines' gate, restated (nrt_launch.h ring32_supported / ring3_supported)
# ---------------------------------------------------------------------------------------------
def live_ksteps(freqs):
    """nrt_device.h: encoding k-steps (4 slots each) that hold one of the dp = 2 F + 3 slots."""
    return (2 * freqs + 3 + 3) >> 2


def gate(c):
    """{condition: holds} of ring32_supported / ring3_supported for a case, and the figures."""
    dp = 2 * c.freqs + 3
    ke, ke3 = (dp + 15) // 16 * 16, (dp + 31) // 32 * 32
    bias = (c.layers + 2) * max(c.hidden, (c.out + 31) // 32 * 32) * 4  # ring_bias_bytes
    pairs = 4 * (((c.spheres + 3) // 4 + 1) // 2) * 7 * 16 if c.spheres else 0
    sphere = max(64 * c.spheres, pairs)                                  # ring32_sphere_bytes
    basis = 16 * c.freqs
    # ring32::Engine: two slots of the largest chunk (4 sub-blocks x max(H, ke) / 16 KiB), the
    # pieces spread over 8 waves; ring3::Engine: 4 (H + ke3) / 32 KiB a slot, three slots where
    # they fit 128 KiB, else two
    q32 = 4 * max(c.hidden // 16, ke // 16)
    ring32 = 2 * ((q32 + 7) // 8 * 8) * 1024
    q3 = (4 * (c.hidden // 32 + ke3 // 32) + 7) // 8 * 8
    ring3 = (3 if 3 * q3 <= 128 else 2) * q3 * 1024
    tables = basis + bias + sphere
    return {
        "hidden": c.hidden in (128, 256),
        "ke": ke in (48, 80),
        "ke3": ke3 in (64, 96),
        "out": c.out <= 16,
        "activation": c.activation in ("softplus", "leaky_relu"),
        # (ring3_supported has no clause of its own: the host test holds ring3 + tables to LDS)
        "lds": bias + sphere <= 48 * 1024 and ring32 + tables <= LDS,
    }, {"ke": ke, "ke3": ke3, "bias": bias, "sphere": sphere, "ring32": ring32, "ring3": ring3,
        "tables": tables, "cap48": bias + sphere <= 48 * 1024, "total": ring32 + tables <= LDS}


# ---------------------------------------------------------------------------------------------
# the references (CPU, float64 and float32), computed once per case and never modified
# ---------------------------------------------------------------------------------------------
class RefSDF(torch.nn.Module):
    """The oracle SDF of a case: SkipMLP row 0, plus SphereBlobSDF's sphere term where there are
    spheres (blob.shift is the same MLP object, so blob itself is the oracle's SDF when out = 1)."""

    def __init__(self, mlp, blob):
        super().__init__()
        self.mlp = mlp
        self.blob = blob

    def mlp_part(self, p):
        return self.mlp(p)[..., 0]

    def sphere_part(self, p):
        return self.blob.spheres(p) if self.blob is not None else torch.zeros_like(p[..., 0])

    def forward(self, p):
        return self.sphere_part(p) + self.mlp_part(p)


def rays_of(name):
    """[P, 6]: origins uniform in the box, random unit directions."""
    g = torch.Generator().manual_seed(7000 + CASES[name].seed)
    o = (torch.rand(P, 3, generator=g) * 2 - 1) * BOX
    d = F.normalize(torch.randn(P, 3, generator=g), dim=-1)
    return torch.cat([o, d], -1).contiguous()


def scan_max_t(name):
    """dist + random.random() * (2 / 128) (sdfs.py:236) under the case's seed."""
    return 2.2 + random.Random(CASES[name].seed).random() * (2 / 128)


def oracle_sdf(name):
    """The oracle of a case: seeded construction, the blob's usual radii += 0.12 and tfs =
    0.05 randn, the hidden gain, then the out layer's row 0 scaled and shifted so that over the
    origins max|MLP part - mean| = AMP and HITS of the P rays have d(o) < eps."""
    c = CASES[name]
    seeded(c.seed)
    mlp = R.SkipMLP(num_layers=c.layers, hidden_size=c.hidden, in_size=3, out=c.out, skip=c.skip,
                    freqs=c.freqs, activation=c.activation)
    blob = None
    if c.spheres:
        blob = R.SphereBlobSDF(n=c.spheres, shift_layers=1, shift_hidden=8, shift_freqs=1)
        blob.shift = mlp
        with torch.no_grad():
            blob.radii.add_(0.12)
            blob.tfs.copy_(0.05 * torch.randn_like(blob.tfs))
    ref = RefSDF(mlp, blob)
    o = rays_of(name)[:, :3].double()
    with torch.no_grad():
        for lin in mlp.layers:
            lin.weight.mul_(c.gain)
        f64 = double_copy(ref)
        y, s = f64.mlp_part(o), f64.sphere_part(o)
        a = AMP / (y - y.mean()).abs().max()
        v = (s + a * (y - y.mean())).sort().values
        shift = EPS - (v[HITS - 1] + v[HITS]) / 2
        mlp.out.weight[0] *= a.float()
        mlp.out.bias[0] = (a * (mlp.out.bias[0].double() - y.mean()) + shift).float()
    return ref


def _values(ref, pts, dtype):
    """(d, MLP part) of the oracle at float32 points, computed in dtype."""
    m = double_copy(ref) if dtype == torch.float64 else ref
    with torch.no_grad():
        q = pts.to(dtype)
        return m(q), m.mlp_part(q)


def _gradients(ref, pts, dtype):
    """(grad d, grad MLP part) by autograd (sdfs.py:184-197) in dtype."""
    m = double_copy(ref) if dtype == torch.float64 else ref
    out = []
    for fn in (m, m.mlp_part):
        q = pts.to(dtype).requires_grad_(True)
        v = fn(q)
        out.append(torch.autograd.grad(v, q, torch.ones_like(v))[0].detach())
    return out


def _scan(ref, rays, max_t, dtype):
    """The float64 side: min of d over the ray's 129 scan points o + float32(step (j + 1)) dir
    (and o itself), with the MLP part at the minimum.  The float32 side: the oracle's own
    coarse_scan (sdfs.py:232-249), sdf(best_pos) included."""
    if dtype == torch.float32:
        o, d = rays[:, None, :3], rays[:, None, 3:]
        jitter = (max_t - 2.2) / (2 / 128)
        with torch.no_grad():
            v, _ = R.MarchedSDF(sdf=ref, epsilon=EPS).coarse_scan(o, d, jitter=jitter)
        return v.reshape(-1), None
    step = max_t / 128
    ts = torch.tensor([0.0] + [step * (j + 1) for j in range(128)], dtype=torch.float32).double()
    o, d = rays[:, None, :3].double(), rays[:, None, 3:].double()
    pts = o + ts[None, :, None] * d
    m = double_copy(ref)
    with torch.no_grad():
        v, y = m(pts), m.mlp_part(pts)
    best, at = v.min(-1)
    return best, y.gather(-1, at[:, None])[:, 0]


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the tests of a case compare with: {"ref", "rays", "max_t", and per observable
    (float64, float32[, MLP part in float64])}; shared with tests/test_ring_sweep_host.py; nobody
    writes to it."""
    ref = oracle_sdf(name)
    rays = rays_of(name)
    o, d = rays[:, :3], rays[:, 3:]
    t0 = (torch.tensor(1e2) * torch.tensor(EPS)).double()  # the shadow march's start, as float32
    occ_pts64 = o.double() + t0 * d.double()
    out = {"ref": ref, "rays": rays, "max_t": scan_max_t(name)}
    d64, y64 = _values(ref, o, torch.float64)
    out["origin"] = (d64, _values(ref, o, torch.float32)[0], y64)
    with torch.no_grad():
        m = double_copy(ref)
        out["occlusion"] = (m(occ_pts64), ref((o + t0.float() * d)), m.mlp_part(occ_pts64))
    s64, sy64 = _scan(ref, rays, out["max_t"], torch.float64)
    out["scan"] = (s64, _scan(ref, rays, out["max_t"], torch.float32)[0], sy64)
    g64, gy64 = _gradients(ref, o, torch.float64)
    out["grad"] = (g64, _gradients(ref, o, torch.float32)[0], gy64)
    return out


def bar(want64, ref32, scale):
    """(tolerance, the float32 oracle's own error) of one compared tensor (rows of vectors are
    compared by their norm)."""
    diff = ref32.double() - want64
    e32 = (diff.norm(dim=-1) if diff.dim() > 1 else diff.abs()).max().item()
    return max(1e-4 * scale, 4 * e32), e32


def scale_of(part64):
    """max|MLP part| of values, max ||.|| of gradients."""
    return (part64.norm(dim=-1) if part64.dim() > 1 else part64.abs()).max().item()


def value_bar(name, key, rows=None):
    """(bar, e32, scale) of an observable's value tensor over `rows` (default: every ray)."""
    w64, w32, y64 = reference(name)[key]
    rows = slice(None) if rows is None else rows
    scale = scale_of(y64[rows])
    tol, e32 = bar(w64[rows], w32[rows], scale)
    return tol, e32, scale


def decided(name, key, rows=None):
    """The rays whose float64 value is further than the value bar from eps: a binary output is
    compared on these (the others are counted against the 2 % cap)."""
    w64 = reference(name)[key][0][slice(None) if rows is None else rows]
    tol = value_bar(name, key, rows)[0]
    return (w64 - EPS).abs() > tol


# ---------------------------------------------------------------------------------------------
# the product side
# ---------------------------------------------------------------------------------------------
def product_sdf(name, ref=None):
    """SphereSDF + SkipConnMLP shift, or the bare SkipConnMLP, with the oracle's tensors (cuda)."""
    from neural_raytracing_amd.pathtracer.neural_blocks import SkipConnMLP
    from neural_raytracing_amd.pathtracer.shapes import SphereSDF
    c = CASES[name]
    ref = ref or reference(name)["ref"]
    kw = {"activation": F.softplus} if c.activation == "softplus" else {}
    mlp = SkipConnMLP(num_layers=c.layers, hidden_size=c.hidden, in_size=3, out=c.out, skip=c.skip,
                      freqs=c.freqs, device="cpu", **kw)
    copy_mlp(mlp, ref.mlp)
    if not c.spheres:
        return mlp.cuda()
    mine = SphereSDF(n=c.spheres, device="cpu")
    mine.shift = mlp
    with torch.no_grad():
        mine.centers.copy_(ref.blob.centers)
        mine.radii.copy_(ref.blob.radii)
        mine.tfs.copy_(ref.blob.tfs)
    return mine.cuda()


RING = {"fp32": ("k_march32", "k_scan_best32", "k_normal32", "k_occl32"),
        "fp32-split": ("k_march3", "k_scan_best3", "k_normal3", "k_occl3", "k_sdf_eval3")}
COUNTED = sorted({k for v in RING.values() for k in v} | {"k_intersect", "k_sdf_grad", "k_occlusion"})


class _Counted:
    """Launch counts of the ring kernels and of the per-wave scopes over the body."""

    def __enter__(self):
        from neural_raytracing_amd import _lib
        _lib.profile_enable(True)
        _lib.profile_reset()
        self.counts = {}
        return self

    def __exit__(self, *exc):
        from neural_raytracing_amd import _lib
        if exc[0] is None:
            torch.cuda.synchronize()
            self.counts.update({k: _lib.profile_read(k)[1] for k in COUNTED})
        _lib.profile_enable(False)


def _assert_kernels(name, engine, counts, ran):
    """A fitting case: each kernel of `ran` (this engine's: {name: launches}) exactly as often as
    the calls made ask for, no other engine's ring kernel, no k_sdf_grad.  An over-size case: no
    ring kernel at all."""
    print(f"{name} {engine}: launches {counts}")
    ring = {k for v in RING.values() for k in v}
    if name in OVERSIZE:
        assert all(counts[k] == 0 for k in ring), counts
        return
    for k, n in ran.items():
        assert counts[k] == n, (k, n, counts)
    assert all(counts[k] == 0 for k in ring - set(RING[engine])), counts
    assert counts["k_sdf_grad"] == 0, counts


def _code(engine):
    from neural_raytracing_amd import _lib
    return _lib._PRECISIONS[engine]


def _handle(sdf):
    from neural_raytracing_amd.pathtracer.shapes.sdfs import sdf_handle
    return sdf_handle(sdf)


def _intersect(sh, rays, engine, primary, max_t=2.2):
    """The one-step nrt_sdf_intersect into poisoned, guarded outputs."""
    out, broken = intersect_poisoned(sh, rays, 1, _code(engine), eps=EPS, max_t=MAX_T,
                                     scan_max_t=max_t, primary=primary)
    assert not broken, f"guard bands of {broken} overwritten"
    for k in ("t", "p") + (("thr",) if primary else ()):
        assert not torch.isnan(out[k]).any(), f"{k}: words left unwritten"
    assert bool((out["hit"] <= 1).all())
    out["hit"] = out["hit"].bool()
    return out


def _occlusion(sh, rays, engine):
    from neural_raytracing_amd import _lib
    n = rays.shape[0]
    vis = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=rays.device)
    mt = torch.full((n,), 1e6, device=rays.device)  # a light no ray reaches
    _lib.call("nrt_sdf_occlusion", sh, _lib.ptr(rays), n, _lib.ptr(mt), 1, EPS,
              ctypes.c_void_p(vis.data_ptr() + 64), _code(engine), _lib.stream())
    torch.cuda.synchronize()
    v = vis.cpu()
    assert bool((v[:64] == 0xA5).all()) and bool((v[64 + n:] == 0xA5).all()), "guard bands"
    assert bool((v[64:64 + n] <= 1).all()), "visible holds bytes other than 0 and 1"
    return v[64:64 + n].bool()


def _eval(sh, pts, engine):
    from neural_raytracing_amd import _lib
    out = torch.full((pts.shape[0],), float("nan"), device=pts.device)
    _lib.call("nrt_sdf_eval", sh, _lib.ptr(pts), pts.shape[0], _lib.ptr(out), _code(engine),
              _lib.stream())
    torch.cuda.synchronize()
    return out.cpu()


class _Worst:
    """The bar on one tensor; prints each figure before it asserts; keeps the largest err / bar
    per observable for the report."""

    def __init__(self):
        self.by = {}

    def close(self, what, key, got, want64, ref32, scale):
        tol, e32 = bar(want64, ref32, scale)
        diff = got.double() - want64
        err = (diff.norm(dim=-1) if diff.dim() > 1 else diff.abs()).max().item() if diff.numel() else 0.0
        self.by[key] = max(self.by.get(key, 0.0), err / tol)
        print(f"{what} {key}: err {err:.3g}  bar {tol:.3g}  scale {scale:.3g}  e32 {e32:.3g}  "
              f"rows {want64.shape[0]}")
        assert err <= tol, f"{what} {key}: err {err:.3g} > bar {tol:.3g} (scale {scale:.3g}, e32 {e32:.3g})"
        return tol

    def same(self, what, key, got, want, on):
        """A binary output, exactly, on the decided rays; at most 2 % of the rays left out."""
        out = int((~on).sum())
        wrong = int((got[on] != want[on]).sum())
        print(f"{what} {key}: {wrong} wrong of {int(on.sum())} decided rays, {out} left out")
        assert out <= 0.02 * on.numel(), f"{what} {key}: {out} rays within the bar of eps"
        assert wrong == 0, f"{what} {key}: {wrong} rays differ, first {int((got != want)[on].nonzero()[0])}"


@pytest.fixture(autouse=True)
def _fp32(request):
    if "gpu" not in request.keywords:
        yield
        return
    from neural_raytracing_amd import set_precision
    set_precision("fp32")
    yield
    set_precision("fp32")


def _check_case(name, engine, n):
    """Every observable of a case on its first n rays (the references are row-wise, so their
    first n rows are the references of the shorter batch)."""
    r = reference(name)
    rows = slice(0, n)
    mine = product_sdf(name)  # (owns the handle: it lives as long as this module object)
    sh = _handle(mine)
    rays = r["rays"][:n].contiguous().cuda()
    what = f"{name} {engine} P={n}"
    w = _Worst()
    # two intersect calls (each a march and a normal pass, one of them a scan), one shadow march,
    # one point evaluation (split): with the scopes k_intersect and k_occlusion at exactly 2 and
    # 1, every march and shadow march of the case is one of the ring launches counted here
    ks = RING[engine]
    ran = {ks[0]: 2, ks[1]: 1, ks[2]: 2, ks[3]: 1, **({ks[4]: 1} if engine == "fp32-split" else {})}
    rows_of = {}
    try:
        with _Counted() as c:
            m0 = _intersect(sh, rays, engine, primary=0)
            m1 = _intersect(sh, rays, engine, primary=1, max_t=r["max_t"])
            vis = _occlusion(sh, rays, engine)
            if engine == "fp32-split":
                val = _eval(sh, rays[:, :3].contiguous(), engine)
        # 1. the one-step march
        d64, d32, y64 = (x[rows] for x in r["origin"])
        want_hit = d64 <= EPS
        w.same(what, "hit", m0["hit"], want_hit, decided(name, "origin", rows))
        miss = ~m0["hit"] & ~want_hit
        rows_of["t_rows"] = int(miss.sum())
        if miss.any():
            w.close(what, "t", m0["t"][miss], d64[miss], d32[miss], scale_of(y64[miss]))
        else:
            print(f"{what} t: rows 0 (no ray of this batch misses)")
        assert bool((m0["t"][m0["hit"]] == 0).all()), "a ray that hit at its origin has t != 0"
        # 2. the coarse scan (and the march beside it: the same bits as without)
        for k in ("t", "hit", "p", "n", "raw"):
            assert torch.equal(m0[k].view(torch.uint8), m1[k].view(torch.uint8)), f"{k}: primary 0 vs 1"
        s64, s32, sy64 = (x[rows] for x in r["scan"])
        w.close(what, "scan", m1["thr"] / -1000, s64, s32, scale_of(sy64))
        # 3. the normals of the rays that hit (at t = 0: the origin itself)
        h = m0["hit"] & want_hit
        rows_of["raw_n_rows"] = int(h.sum())
        if not h.any():
            print(f"{what} raw_n: rows 0 (no ray of this batch hits)")
        else:
            g64, g32, gy64 = (x[rows][h] for x in r["grad"])
            w.close(what, "raw_n", m0["raw"][h], g64, g32, scale_of(gy64))
            unit = F.normalize(m0["raw"][h], eps=1e-6, dim=-1)
            assert (m0["n"][h] - unit).abs().max().item() <= 1e-6, "n is not normalize(raw_n)"
            p = r["rays"][rows][h][:, :3] + 5 * EPS * m0["n"][h]
            assert (m0["p"][h] - p).abs().max().item() <= 1e-6, "p is not o + 5 eps n"
        assert bool((m0["n"][~m0["hit"]] == 0).all()), "a ray that did not hit has a normal"
        # 4. the shadow march
        o64 = r["occlusion"][0][rows]
        w.same(what, "visible", vis, o64 >= EPS, decided(name, "occlusion", rows))
        # 5. point evaluation on the split engine
        if engine == "fp32-split":
            w.close(what, "eval", val, d64, d32, scale_of(y64))
        _assert_kernels(name, engine, c.counts, ran)
        assert c.counts["k_intersect"] == 2 and c.counts["k_occlusion"] == 1, c.counts
        if name in OVERSIZE:  # the per-wave normal pass of both intersect calls
            assert c.counts["k_sdf_grad"] == 2, c.counts
    finally:
        report("ring_sweep", case=name, engine=engine, P=n, **rows_of,
               **{f"{k}_err_over_bar": round(v, 4) for k, v in w.by.items()})


# ---------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", list(CASES))
def test_ring_engines_against_float64(name, engine):
    _check_case(name, engine, P)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("engine", ENGINES)
def test_ragged_ray_counts(engine, n):
    """One ray (a wave with 15 idle columns, 7 idle waves) and 17 rays (one ray in the second
    tile) of an nl > 1 case: the same bars, the guard bands intact."""
    _check_case(RAGGED[engine], engine, n)


def _exponents(mlp):
    """frexp exponents of max|W|, max|W| log2 e and max|W| ln 2 per linear layer: what the split
    stream's per-layer power-of-two scale is chosen from (nrt_pack.hip)."""
    out = []
    for lin in mlp._linears():
        mx = float(lin.weight.detach().abs().max())
        out.append(tuple(math.frexp(mx * f)[1] for f in (1.0, math.log2(math.e), math.log(2.0))))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", REFRESH)
def test_refreshed_handle_marches_like_a_fresh_pack(name, engine):
    """nrt_mlp_refresh re-gathers stream32 and the split stream through a map built for the
    encoding at hand: after two SGD steps through the training path the one-step march, its
    normals and the scan on train_sdf_handle (refreshed on the device) equal sdf_handle's (packed
    on the host from the same weights) bit for bit.  The split stream keeps its pack-time
    per-layer power-of-two scales across a refresh, so its halves equal a fresh pack's exactly
    while no layer's max|W| has crossed a power of two: the steps are small (the largest entry
    moves by 1e-3) and the test asserts that none has."""
    from neural_raytracing_amd import set_precision
    from neural_raytracing_amd.pathtracer.shapes.sdfs import sdf_handle, train_sdf_handle
    r = reference(name)
    mine = product_sdf(name)
    mlp = getattr(mine, "shift", mine)
    before = [lin.weight.detach().clone() for lin in mlp._linears()]
    exps = _exponents(mlp)
    rays = r["rays"].cuda()
    set_precision(engine)
    first = train_sdf_handle(mine)  # packs the training handle from the weights as they are
    opt = torch.optim.SGD(mlp.parameters(), lr=1.0)
    for _ in range(2):
        opt.zero_grad()
        mlp(rays[:, :3].contiguous()).square().mean().backward()  # the training handle
        opt.param_groups[0]["lr"] = 1e-3 / max(float(q.grad.abs().max()) for q in mlp.parameters())
        opt.step()
    moved = max(float((lin.weight - b).abs().max()) for lin, b in zip(mlp._linears(), before))
    assert moved >= 5e-4, "the SGD steps left the weights where they were"
    assert _exponents(mlp) == exps, "a layer's max|W| crossed a power of two: pick another seed"
    th = train_sdf_handle(mine)
    assert th == first, "the training handle was rebuilt, not refreshed"
    fh = sdf_handle(mine)
    assert fh != th
    outs = []
    with _Counted() as c:
        for sh in (th, fh):
            outs.append(_intersect(sh, rays, engine, primary=1, max_t=r["max_t"]))
    _assert_kernels(name, engine, c.counts, {k: 2 for k in RING[engine][:3]})
    assert outs[0]["hit"].any() and not outs[0]["hit"].all()
    for k in ("t", "hit", "p", "n", "raw", "thr"):
        a, b = outs[0][k], outs[1][k]
        diff = (a.view(torch.uint8) != b.view(torch.uint8)).reshape(a.shape[0], -1).any(-1)
        assert not diff.any(), (f"{name} {engine}: {k} differs on {int(diff.sum())} rays, max|diff| "
                                f"{(a.double() - b.double()).abs().max().item():.3g}")
