"""The launch-queue march's line stages (nrt_kernels.h LineStage) where the 800^2 frame uses them:
slots evicted to make room, evicted lines reopened, and the queue's default threshold.

A ray set built from the oracle makes every 16-ray line of t hold one slow ray (a graze that
marches 40 evaluations or more) at offset 0 and fifteen rays that are over much sooner, so that
a wave's lanes run ahead through many lines while the slow rays keep their lines open: more than
kStageSlots = 8 open lines a wave, hence evictions.  tests/test_line_stage_host.py checks that
precondition on a host model of the slot table, from the oracle's evaluation counts alone.

What "over much sooner" can be is bounded by the SDF: SphereSDF's smooth minimum clamps its sum at
1e-4 (utils.py:385-387), so far from the blob the distance saturates near -log(1e-4)/32 = 0.29
and a ray that leaves needs some 33-37 evaluations to pass max_t = 10.  A miss that ends at its
first evaluation does not exist here.  So fourteen of the fast rays start well inside the surface
(a hit at t == 0: the packed word is -0.0f) and one, at offset 8, starts 12 units out and points
away (a miss, with the oracle's 33-37 evaluations): alternating the two kinds, eight far rays a
line, gives the host model no eviction at all, one far ray a line gives it hundreds.

Every run goes through tests.helpers.intersect_poisoned: outputs poisoned before the launch, with
guard bands.  nrt_profile_staged says whether a march launched with line stages at all (the FP16
march drops them where they would cost a resident block; below its threshold the default options
do not take the queue).  That a staged march on these rays evicts is the host model's word: the
device keeps no count of it (counters in LineStage cost the march kernels scalar registers).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import pathtracer_ref as R
from tests.helpers import (assert_bit_equal, assert_outputs_written, blob, intersect_poisoned,
                           lib_opt)
from tests.report import report

pytestmark = pytest.mark.gpu

EPS, MAX_T, MAX_STEPS = 5e-3, 10.0, 64
SLOW_MIN_STEPS = 40   # a slow ray's evaluations, at least
MARGIN = 1e-3         # min over a slow ray's steps of |d - eps|: far above FP32 error
SIZES = [(2061, 1), (6157, 3)]  # (rays, march_blocks): 128 / 384 full lines and a 13-ray line
FAR_OFFSET = 8        # the far ray's place in its line
SLOW_RAYS = 129       # distinct slow rays (the smaller size's lines)
SLOW, INSIDE, FAR = 0, 1, 2


def oracle_march(sdf, rays, max_steps=MAX_STEPS, eps=EPS, max_t=MAX_T):
    """sdfs.py:119-131 restated on the oracle SDF (as R.MarchedSDF.march, which evaluates every
    ray at every step) with what a ray's march is to the kernel: (t, hit, the evaluations made
    while the ray was live, their min |d - eps|).  Only live rays are evaluated."""
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
            dv = sdf(o[k] + d[k] * t[k, None])
            steps[k] += 1
            margin[k] = torch.minimum(margin[k], (dv - eps).abs())
            now = dv <= eps
            hit[k[now]] = True
            live[k[now]] = False
            t[k[~now]] = t[k[~now]] + dv[~now]
    return t, hit, steps, margin


@functools.lru_cache(maxsize=None)
def eviction_rays(hidden):
    """The ray set for the 8 x `hidden` shift, at the larger of SIZES (the smaller is its prefix):
    dict(ref, rays [P, 6], kind [P], and the oracle's t, hit, steps, margin of every ray)."""
    P = max(p for p, _ in SIZES)
    lines = (P + 15) // 16
    ref, _ = blob(32, hidden, 16, "softplus", seed=21, product=False)
    g = torch.Generator().manual_seed(1000 + hidden)
    # slow: tangent rays.  Along a random direction from the blob's centre, bisect for a point
    # whose distance is a gap a little over eps + MARGIN, and send a ray through it at right
    # angles to the gradient there, from 0.6 before it: it slows down to steps of about the gap
    # and then leaves through the saturated far field.  Keep those that the oracle marches for
    # SLOW_MIN_STEPS evaluations with the margin; a line takes them in turn.
    n = 3 * SLOW_RAYS
    u = F.normalize(torch.randn(n, 3, generator=g), dim=-1)
    gap = EPS + MARGIN + 4e-3 * torch.rand(n, generator=g)
    lo, hi = torch.zeros(n), torch.ones(n)
    with torch.no_grad():
        for _ in range(14):
            mid = 0.5 * (lo + hi)
            under = ref(u * mid[:, None]) < gap
            lo, hi = torch.where(under, mid, lo), torch.where(under, hi, mid)
    q = u * hi[:, None]
    grad = R.MarchedSDF(sdf=ref).gradient(q)
    d = F.normalize(torch.linalg.cross(grad, torch.randn(n, 3, generator=g)), dim=-1)
    cand = torch.cat([q - 0.6 * d, d], -1)
    _, _, steps, margin = oracle_march(ref, cand)
    ok = ((steps >= SLOW_MIN_STEPS) & (margin >= MARGIN)).nonzero().squeeze(-1)
    assert ok.numel() >= SLOW_RAYS, f"{ok.numel()} slow candidates of {n}, {SLOW_RAYS} needed"
    slow = cand[ok[:SLOW_RAYS]][torch.arange(lines) % SLOW_RAYS]
    # inside: origins well under the surface, any direction
    pts = torch.rand(32 * lines, 3, generator=g) * 0.2 - 0.1
    with torch.no_grad():
        deep = (ref(pts) < -0.03).nonzero().squeeze(-1)
    assert deep.numel() >= 15 * lines
    inside = torch.cat([pts[deep[:15 * lines]],
                        F.normalize(torch.randn(15 * lines, 3, generator=g), dim=-1)], -1)
    # far: more than max_t plus the blob's extent out, pointing away
    u = F.normalize(torch.randn(lines, 3, generator=g), dim=-1)
    far = torch.cat([12.0 * u, u], -1)
    rays = inside.reshape(lines, 15, 6)
    rays = torch.cat([slow[:, None], rays], 1)  # [lines, 16, 6]
    rays[:, FAR_OFFSET] = far
    kind = torch.full((lines, 16), INSIDE)
    kind[:, 0] = SLOW
    kind[:, FAR_OFFSET] = FAR
    rays = rays.reshape(-1, 6)[:P].contiguous()
    kind = kind.reshape(-1)[:P].contiguous()
    t, hit, steps, margin = oracle_march(ref, rays)
    return dict(ref=ref, rays=rays, kind=kind, t=t, hit=hit, steps=steps, margin=margin)


# ---------------------------------------------------------------------------------------------
# GPU runs, shared by the tests below
# ---------------------------------------------------------------------------------------------
_KERNEL = {"fp32": "k_march32", "fp16": "k_march16", "fp32-split": "k_march3"}


@functools.lru_cache(maxsize=None)
def _product(hidden):
    from neural_raytracing_amd.pathtracer.shapes.sdfs import sdf_handle
    _, mine = blob(32, hidden, 16, "softplus", seed=21)
    return mine, sdf_handle(mine)  # (the module keeps the handle alive)


def _run(sh, rays, prec, **options):
    """one poisoned nrt_sdf_intersect with the counters on: (outputs, outputs whose guard bands
    changed, march launches with line stages, launches of the precision's march kernel)"""
    from neural_raytracing_amd import _lib
    for k, v in options.items():
        lib_opt(k, v)
    _lib.profile_enable(True, evals=True)
    _lib.profile_reset()
    try:
        out, broken = intersect_poisoned(sh, rays, MAX_STEPS, _lib._PRECISIONS[prec])
        stage = _lib.profile_staged()
        launches = _lib.profile_read(_KERNEL[prec])[1]
    finally:
        _lib.profile_enable(False)
        _lib.profile_reset()
    return out, broken, stage, launches


@functools.lru_cache(maxsize=None)
def _pair(prec, hidden, P, blocks):
    """the eviction rays marched with per-ray stores and with line staging, under the launch queue"""
    rays = eviction_rays(hidden)["rays"][:P].cuda().contiguous()
    _, sh = _product(hidden)
    runs = {}
    try:
        for stage in (0, 1):
            runs[stage] = _run(sh, rays, prec, march_queue=1, march_blocks=blocks, march_stage=stage)
    finally:
        lib_opt("march_stage", 1)
    report(f"line_stage_launches[{prec},{hidden},{P},{blocks}]", staged=runs[1][2])
    return runs


def _staged(prec, hidden, P, blocks):
    return _pair(prec, hidden, P, blocks)[1][2] != 0


@pytest.mark.parametrize("P,blocks", SIZES)
@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32-split"])
def test_evicting_line_stages_match_per_ray_stores(prec, hidden, P, blocks):
    """t, hit, p, n and throughput of the staged march are bit-equal to the march that stores each
    ray's words itself, on rays that force slot evictions and reopened lines; the launch counter
    says that the staged run had its line stages and that the other run had none.
    (blocks = 1: T = 128, so the key stage's limit R - T cuts a line of whole scans too.)  The
    FP16 march drops its stages where they would cost a resident block: such a width is skipped,
    and at least one width has to stage."""
    runs = _pair(prec, hidden, P, blocks)
    (base, _, bstaged, blaunch), (out, _, staged, launch) = runs[0], runs[1]
    assert blaunch == 1 and launch == 1, f"{_KERNEL[prec]} did not run"
    assert bstaged == 0, "march_stage=0 launched with line stages"
    if prec == "fp16" and staged == 0:
        others = [h for h in (128, 256) if h != hidden and _staged(prec, h, P, blocks)]
        assert others, "the FP16 march staged its lines at neither width: find a shape that does"
        pytest.skip(f"the FP16 march at width {hidden} runs without line stages (the launch "
                    "counter reads 0): they would cost a resident block")
    assert staged == 1, "march_stage=1 under the launch queue launched without line stages"
    assert base["hit"].any() and not base["hit"].all()
    assert_bit_equal(out, base, "staged vs per-ray stores")


@pytest.mark.parametrize("P,blocks", SIZES)
@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("prec", ["fp32", "fp16", "fp32-split"])
def test_evicting_line_stages_write_every_word_inside_their_buffers(prec, hidden, P, blocks):
    """The same two runs write into poisoned outputs with guard bands: afterwards no word of t, p
    or the throughput is NaN, hit is 0 or 1, and the guard bands still hold the poison.  The
    per-ray-store run is held to the same, so a failure of the staged run alone is the stages'."""
    runs = _pair(prec, hidden, P, blocks)
    for stage, name in ((0, "per-ray stores"), (1, "line stages")):
        out, broken, _, _ = runs[stage]
        assert not broken, f"{name}: guard bands of {broken} overwritten"
        assert_outputs_written(out, name)


@pytest.mark.parametrize("hidden", [128, 256])
def test_evicting_line_stages_match_oracle(hidden):
    """The staged FP32 march against R.MarchedSDF.intersect on the same rays: every inside-origin
    ray is a hit with t == 0.0 exactly (its packed word is -0.0f: the hit flag is t's sign bit),
    every far ray a miss, the slow rays' hit flags the oracle's (their margin makes that a
    condition), and t within the FP32 bar of 1e-4 where both hit."""
    P, blocks = SIZES[0]
    rs = eviction_rays(hidden)
    kind = rs["kind"][:P]
    with torch.no_grad():
        rit, rhit = R.MarchedSDF(sdf=rs["ref"], epsilon=EPS, max_steps=MAX_STEPS).intersect(
            rs["rays"][:P], max_t=MAX_T, primary=False)
    rt = rit.t.reshape(-1)
    # (the restatement the ray set was chosen with is the oracle's march)
    assert torch.equal(rhit, rs["hit"][:P]) and (rt - rs["t"][:P]).abs().max().item() <= 1e-5
    out, _, staged, _ = _pair("fp32", hidden, P, blocks)[1]
    assert staged == 1
    t, hit = out["t"], out["hit"].bool()
    ins, far, slow = kind == INSIDE, kind == FAR, kind == SLOW
    assert rhit[ins].all() and not rhit[far].any()
    assert hit[ins].all(), f"{int((~hit[ins]).sum())} inside-origin rays lost their hit"
    assert bool((t[ins] == 0.0).all())
    assert not hit[far].any()
    assert torch.equal(hit[slow], rhit[slow])
    assert torch.equal(hit, rhit)
    both = hit & rhit
    t_err = (t[both] - rt[both]).abs().max().item()
    t_err_miss = (t[~both] - rt[~both]).abs().max().item()
    report(f"line_stage_vs_oracle[{hidden}]", rays=P, hits=int(rhit.sum()),
           slow_hits=int(rhit[slow].sum()), t_maxabs=t_err, t_maxabs_miss=t_err_miss)
    assert t_err <= 1e-4


def test_march_queue_default_threshold():
    """At default options the launch queue (and with it the line stages) serves batches of
    64 * 2048 rays or more: 131,071 rays march from per-wave lists without line stages, 131,072
    take the queue with them; both equal march_queue=0 bit for bit."""
    from neural_raytracing_amd import _lib
    _, sh = _product(128)
    g = torch.Generator().manual_seed(29)
    n = 64 * 2048
    d = F.normalize(torch.cat([torch.rand(n, 2, generator=g) * 0.9 - 0.45, -torch.ones(n, 1)], -1),
                    dim=-1)
    rays = torch.cat([torch.tensor([0.0, 0.2, 1.1]).expand(n, 3), d], -1).cuda().contiguous()
    for P in (n - 1, n):
        _lib.load().nrt_reset_options()
        out, broken, staged, launch = _run(sh, rays[:P].contiguous(), "fp32")
        assert launch == 1 and not broken
        assert_outputs_written(out, f"P={P}")
        assert out["hit"].any() and not out["hit"].all()
        base, bbroken, bstaged, _ = _run(sh, rays[:P].contiguous(), "fp32", march_queue=0)
        assert not bbroken and bstaged == 0
        assert_outputs_written(base, f"P={P}, march_queue=0")
        assert_bit_equal(out, base, f"P={P}: defaults vs march_queue=0")
        report(f"march_queue_threshold[{P}]", staged=staged)
        assert staged == (1 if P >= n else 0), f"{P} rays at default options: {staged} staged launches"
