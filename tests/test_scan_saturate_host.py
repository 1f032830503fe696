"""The alpha scan (nrt_march_params.primary = 2) without a GPU: the f32 sigmoid's saturation that
its contract rests on, the host model of its evaluation count on the bench scene, and the ray
sets the GPU tests march (tests/scan_saturate_model.py)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import scan_saturate_model as M
from tests.report import report


def _sigmoid32(x):
    """k_composite's 1.f / (1.f + expf(-thr)), every operation rounded to f32"""
    x = np.asarray(x, dtype=np.float32)
    one = np.float32(1.0)
    return one / (one + np.exp(-x).astype(np.float32))


def test_f32_sigmoid_is_one_from_17_33():
    f = np.float32
    xs = [f(M.SIGMOID_ONE), f(M.SAT_THR)]
    xs += [np.nextafter(x, f(0)) for x in xs[:2]] + [np.nextafter(x, f(1e9)) for x in xs[:2]]
    xs += list(np.arange(17.33, 300.0, 0.37, dtype=np.float32))
    y = _sigmoid32(np.array(xs, dtype=np.float32))
    assert y.dtype == np.float32 and bool((y == f(1.0)).all())
    # the sample test's threshold as a throughput: -1000 * -0.02f is 20 to within an ulp
    thr = f(-1000.0) * f(M.SAT)
    assert thr >= np.nextafter(f(20.0), f(0)) and _sigmoid32(thr) == f(1.0)
    assert _sigmoid32(f(10.0)) < f(1.0)  # (and well below the threshold it is not)


@functools.lru_cache(maxsize=None)
def _bench_model():
    """the host model on a 40 x 40 lattice of the bench's 800^2 view, bench scene weights"""
    import bench
    from oracle import pathtracer_ref as R
    size, n = 800, 40
    scene = bench.build_scene("cpu", 64, light_gain=bench.LIGHT_GAIN)
    osc = bench.oracle_scene(scene)
    shape = osc["shape"]
    focal = float(0.5 * size / math.tan(0.5 * 0.6911))
    cam = R.NeRFCameraRef(bench.view_c2w(0, 1).unsqueeze(0), focal)
    k = torch.arange(n, dtype=torch.float) * (size / n) + size / (2 * n)
    gx, gy = torch.meshgrid(k, k, indexing="ij")
    rays = cam.sample_positions(torch.stack([gy, gx], -1), size).reshape(-1, 6)
    scan_max_t = shape.dist + 0.5 * (2 / 128)
    t, hit, steps, _ = M.march_live(shape.sdf, rays, max_steps=shape.max_steps, eps=shape.epsilon)
    s = M.scan_samples(shape.sdf, rays, scan_max_t)
    thr, _ = M.scan_thr(shape.sdf, rays, s, scan_max_t)
    return dict(costs=M.scan_costs(s, t, hit, steps, scan_max_t), hit=hit, thr=thr, rays=rays.shape[0])


def test_host_model_bench_view():
    m = _bench_model()
    c, hit = m["costs"], m["hit"]
    P = m["rays"]
    per = {k: c[k].sum().item() / P for k in ("exact", "inorder", "wrap")}
    sat = c["saturates"]
    ws = c["wrap_scan"][sat & hit].float()
    report("scan_saturate_host_model", rays=P, hit_fraction=hit.float().mean().item(),
           hits_saturating=(sat & hit).sum().item() / max(int(hit.sum()), 1),
           misses_saturating=int((sat & ~hit).sum()), evals_exact=per["exact"],
           evals_inorder=per["inorder"], evals_wrap=per["wrap"],
           wrap_over_exact=per["wrap"] / per["exact"],
           sat_hit_scan_mean=ws.mean().item() if ws.numel() else 0.0,
           sat_hit_scan_max=ws.max().item() if ws.numel() else 0.0)
    assert per["wrap"] <= per["inorder"] <= per["exact"]
    assert per["wrap"] <= 0.75 * per["exact"]
    # a saturating ray's exact throughput lies 2 logit units or more inside the sigmoid's plateau
    assert sat.any() and bool((m["thr"][sat] >= M.SIGMOID_ONE + 2).all())


@pytest.mark.parametrize("hidden", [128, 256])
def test_gpu_ray_sets(hidden):
    rs = M.class_rays(hidden)
    cls, s, hit = rs["cls"], rs["samples"], rs["hit"]
    smin = s.min(1).values
    for k in (M.THROUGH, M.GRAZE, M.NEAR, M.FAR):
        assert int((cls == k).sum()) >= 64
    for P, _ in M.SIZES:  # every class is in each size's launch-queue tail too
        assert set(cls[P - 128:P].tolist()) == {0, 1, 2, 3}
    assert bool((hit[cls == M.THROUGH]).all()) and bool((smin[cls == M.THROUGH] <= M.SAT).all())
    g = smin[cls == M.GRAZE]
    assert bool(hit[cls == M.GRAZE].all()) and bool(((g > -0.015) & (g < 0)).all())
    n = smin[cls == M.NEAR]
    assert not hit[cls == M.NEAR].any() and bool(((n > 0) & (n < 0.05)).all())
    assert not hit[cls == M.FAR].any() and bool((smin[cls == M.FAR] >= 0.05).all())
    # FP16 and FP32 agree on every sample's class, and on every march step's hit test
    assert (s - M.SAT).abs().min().item() >= M.SAT_MARGIN
    assert rs["margin"].min().item() >= M.MARGIN
    # a grazing hit starts past 0 and wraps all the way around: 129 samples, an exact minimum
    # (its minimum lies past the hit; the index rule across the wrap is the GPU ties test's)
    c = M.scan_costs(s, rs["t"], hit, rs["steps"])
    gz = cls == M.GRAZE
    assert bool((c["j0"][gz] > 0).all()) and bool((c["wrap_scan"][gz] == 129).all())
    # a through hit saturates within a few samples of its start
    th = cls == M.THROUGH
    report(f"scan_saturate_ray_sets[{hidden}]", rays=cls.numel(),
           through_scan_max=c["wrap_scan"][th].max().item(),
           through_scan_mean=c["wrap_scan"][th].float().mean().item(),
           graze_min_lo=g.min().item(), graze_min_hi=g.max().item())
    assert c["wrap_scan"][th].max().item() <= 8
    assert bool((rs["thr"][th] >= M.SIGMOID_ONE + 2).all())
