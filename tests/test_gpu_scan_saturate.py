"""The alpha scan on the GPU (nrt_march_params.primary = 2, include/nrt.h): against the exact scan
(primary = 1) on the ray classes of tests/scan_saturate_model.py, across schedules, on ties under
the wrapped visiting order, by its evaluation count, with option scan_saturate off, and through
RowRenderer.  Every intersect writes into poisoned outputs with guard bands."""
import ctypes
import functools
import math
import random

import pytest
import torch

from tests import scan_saturate_model as M
from tests.helpers import _Guarded, lib_opt
from tests.report import report

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "fp16", "fp32-split"]


def intersect(sh, rays, prec, primary, want_index=False, **options):
    """one nrt_sdf_intersect with the given `primary` into poisoned, guarded outputs, evaluation
    counter on: dict of host outputs (t, hit, p, n, raw, thr, hits = the sorted hit list, index
    if asked for) plus broken (guard bands that changed), staged and evals"""
    from neural_raytracing_amd import _lib
    _lib.load().nrt_reset_options()
    for k, v in options.items():
        lib_opt(k, v)
    P, dev = rays.shape[0], rays.device
    g = {"t": _Guarded(P, torch.float32, dev), "hit": _Guarded(P, torch.uint8, dev),
         "p": _Guarded(3 * P, torch.float32, dev), "n": _Guarded(3 * P, torch.float32, dev),
         "raw": _Guarded(3 * P, torch.float32, dev), "wi": _Guarded(3 * P, torch.float32, dev),
         "thr": _Guarded(P, torch.float32, dev)}
    idx = torch.full((P,), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    sidx = torch.full((P,), -7, dtype=torch.int32, device=dev) if want_index else None
    lib = _lib.load(require_device=True)
    ws = torch.empty(max(lib.nrt_intersect_workspace_bytes(sh, P), 1), dtype=torch.uint8, device=dev)
    mp = _lib.MarchParams(M.MAX_STEPS, M.EPS, M.MAX_T, primary, M.SCAN_MAX_T, _lib._PRECISIONS[prec])
    if sidx is not None:
        mp.scan_index = sidx.data_ptr()
    o = {k: v.out for k, v in g.items()}
    _lib.profile_enable(True, evals=True)
    _lib.profile_reset()
    try:
        _lib.call("nrt_sdf_intersect", sh, _lib.ptr(rays), P, ctypes.byref(mp), _lib.ptr(o["t"]),
                  _lib.ptr(o["hit"]), _lib.ptr(o["p"]), _lib.ptr(o["n"]), _lib.ptr(o["raw"]),
                  _lib.ptr(o["wi"]), _lib.ptr(o["thr"]), _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(ws),
                  _lib.stream())
        torch.cuda.synchronize()
        staged, evals = _lib.profile_staged(), _lib.profile_evals()
    finally:
        _lib.profile_enable(False)
        _lib.profile_reset()
    out = {k: o[k].cpu() for k in ("t", "hit", "thr")}
    out.update({k: o[k].cpu().reshape(P, 3) for k in ("p", "n", "raw")})
    out["hits"] = idx[:int(cnt.item())].sort().values.cpu()
    if sidx is not None:
        out["index"] = sidx.cpu()
    out["alpha"] = alpha_of(o["thr"], o["hit"])
    out.update(broken=[k for k, v in g.items() if not v.guards_intact()], staged=staged, evals=evals)
    return out


def alpha_of(thr, hit):
    """the alpha channel nrt_composite writes from a throughput: [P] floats"""
    from neural_raytracing_amd import _lib
    P = thr.shape[0]
    rgb = torch.zeros(P, 3, device=thr.device)
    img = torch.full((1, P, 1, 4), float("nan"), device=thr.device)
    _lib.call("nrt_composite", _lib.ptr(rgb), _lib.ptr(thr.contiguous()), _lib.ptr(hit.contiguous()),
              1, P, 1, 1, 0, 0.0, _lib.ptr(img), P, 1, 4, 0, 0, _lib.stream())
    torch.cuda.synchronize()
    return img[0, :, 0, 3].cpu()


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def assert_same(a, b, keys, what, rows=None):
    for k in keys:
        x, y = bits(a[k]), bits(b[k])
        if rows is not None:
            x, y = x[rows], y[rows]
        diff = (x != y).reshape(x.shape[0], -1).any(-1) if x.shape == y.shape else None
        assert diff is not None, f"{what}: {k} has {x.shape[0]} entries against {y.shape[0]}"
        assert not diff.any(), f"{what}: {k} differs on {int(diff.sum())} rays, first {int(diff.nonzero()[0])}"


@functools.lru_cache(maxsize=None)
def _product(hidden):
    from neural_raytracing_amd.pathtracer.shapes.sdfs import sdf_handle
    from tests.helpers import blob
    _, mine = blob(32, hidden, 16, "softplus", seed=21)
    return mine, sdf_handle(mine)  # (the module keeps the handle alive)


@functools.lru_cache(maxsize=None)
def _rays(hidden, P):
    return M.class_rays(hidden)["rays"][:P].cuda().contiguous()


@functools.lru_cache(maxsize=None)
def _run(hidden, prec, P, primary, want_index, options):
    _, sh = _product(hidden)
    return intersect(sh, _rays(hidden, P), prec, primary, want_index, **dict(options))


def _opts(blocks, queue=1, stage=1, **more):
    return tuple(sorted(dict(march_blocks=blocks, march_queue=queue, march_stage=stage, **more).items()))


GEOMETRY = ("t", "hit", "p", "n", "raw", "hits")


@pytest.mark.parametrize("P,blocks", M.SIZES)
@pytest.mark.parametrize("hidden", [128, 256])
@pytest.mark.parametrize("prec", PRECS)
def test_alpha_scan_against_exact_scan(prec, hidden, P, blocks):
    """primary = 2 against primary = 1: the march's outputs and the hit list bit-equal; the
    throughput bit-equal on the classes without a saturating sample and exactly 20.0 on the
    through hits; the composite's alpha channel bit-equal everywhere."""
    one = _run(hidden, prec, P, 1, False, _opts(blocks))
    two = _run(hidden, prec, P, 2, False, _opts(blocks))
    cls = M.class_rays(hidden)["cls"][:P]
    assert not one["broken"] and not two["broken"]
    assert one["hit"].any() and not one["hit"].all()
    assert_same(two, one, GEOMETRY, "primary 2 vs 1")
    assert not torch.isnan(two["thr"]).any()
    assert_same(two, one, ("thr",), "primary 2 vs 1, no saturating sample", rows=cls != M.THROUGH)
    th = cls == M.THROUGH
    assert bool((two["thr"][th] == M.SAT_THR).all()), "a through hit's throughput is not 20.0"
    assert bool((one["thr"][th] >= M.SIGMOID_ONE).all())
    assert_same(two, one, ("alpha",), "alpha from primary 2 vs 1")
    assert bool((two["alpha"][th] == 1.0).all()) and bool((two["alpha"][cls == M.FAR] < 1e-9).all())


@pytest.mark.parametrize("prec,hidden", [("fp32", 128), ("fp32", 256), ("fp16", 128), ("fp32-split", 128)])
def test_alpha_scan_schedule_invariance(prec, hidden):
    """the throughput and the scan index of rays without a saturating sample do not depend on the
    grid, on queue or per-wave lists, or on line staging"""
    P = M.SIZES[0][0]
    cls = M.class_rays(hidden)["cls"][:P]
    unsat = cls != M.THROUGH
    base = None
    for blocks in (1, 3, 0):
        for queue in (0, 1):
            for stage in (0, 1):
                out = _run(hidden, prec, P, 2, True, _opts(blocks, queue, stage))
                what = f"blocks={blocks} queue={queue} stage={stage}"
                assert not out["broken"], f"{what}: guard bands of {out['broken']} overwritten"
                if prec != "fp16":  # (the FP16 march drops its stages where they cost a block)
                    assert out["staged"] == (1 if queue and stage else 0), what
                if base is None:
                    base = out
                    continue
                assert_same(out, base, GEOMETRY + ("thr",), what)
                assert_same(out, base, ("index",), what, rows=unsat)
    exact = _run(hidden, prec, P, 1, True, _opts(1))
    assert_same(base, exact, ("index",), "scan index, primary 2 vs 1", rows=unsat)


@functools.lru_cache(maxsize=None)
def _flat_sdf(hidden):
    """a bare MLP SDF that is -0.01 everywhere: every weight zero, output bias -0.01"""
    import torch.nn.functional as F
    from neural_raytracing_amd.pathtracer.neural_blocks import SkipConnMLP
    from neural_raytracing_amd.pathtracer.shapes.sdfs import sdf_handle
    mlp = SkipConnMLP(num_layers=8, hidden_size=hidden, in_size=3, out=1, freqs=16,
                      activation=F.softplus, device="cpu")
    with torch.no_grad():
        for lin in mlp._linears():
            lin.weight.zero_()
            lin.bias.zero_()
        mlp._linears()[-1].bias.fill_(-0.01)
    mlp = mlp.cuda()
    return mlp, sdf_handle(mlp)


@pytest.mark.parametrize("prec", PRECS)
def test_alpha_scan_ties_under_wraparound(prec):
    """every ray hits at t = 0, never saturates, wraps from j0 = 2, and every sample ties: the
    first index wins, as under the exact scan"""
    _, sh = _flat_sdf(128)
    rays = _rays(128, 613)
    outs = {}
    for primary in (1, 2):
        out = outs[primary] = intersect(sh, rays, prec, primary, True, march_blocks=1, march_queue=1)
        assert not out["broken"]
        assert bool(out["hit"].bool().all()) and bool((out["t"] == 0.0).all())
        assert bool((out["index"] == 0).all()), f"primary {primary}: a tie moved the argmin"
        if prec == "fp32":
            assert bool((out["thr"] == 10.0).all())
        else:  # (the FP16 engines round the bias: 10.0 to their accuracy, the same bits in both modes)
            assert (out["thr"] - 10.0).abs().max().item() <= 0.01
    assert_same(outs[2], outs[1], GEOMETRY + ("thr", "index", "alpha"), "ties, primary 2 vs 1")


def test_alpha_scan_evaluation_counts():
    """the device's evaluation counter against the host model (launch queue, one block of 8
    waves: the last 16 x 8 rays are scanned as segments)"""
    hidden, (P, blocks) = 128, M.SIZES[0]
    rs = M.class_rays(hidden)
    steps, hit, t = rs["steps"][:P], rs["hit"][:P], rs["t"][:P]
    c = M.scan_costs(rs["samples"][:P], t, hit, steps)
    one = _run(hidden, "fp32", P, 1, False, _opts(blocks))
    two = _run(hidden, "fp32", P, 2, False, _opts(blocks))
    assert torch.equal(one["hit"].bool(), hit)  # (the margins make the oracle's steps the device's)
    tail = torch.arange(P) >= P - 16 * 8
    lo = int(c["wrap"][~tail].sum() + c["segments"][tail].sum())
    hi = int(c["wrap"][~tail].sum() + (c["exact"] - c["saturates"].long())[tail].sum())
    report("scan_saturate_evals", rays=P, exact=one["evals"], model_exact=int(c["exact"].sum()),
           alpha=two["evals"], model_lo=lo, model_hi=hi)
    assert one["evals"] == int(c["exact"].sum())
    assert lo <= two["evals"] <= hi
    # the saturating class alone: a non-tail ray costs its march steps + at most 8
    th = (rs["cls"][:P] == M.THROUGH).nonzero().squeeze(-1)
    _, sh = _product(hidden)
    out = intersect(sh, _rays(hidden, P)[th.cuda()].contiguous(), "fp32", 2, False,
                    march_blocks=1, march_queue=1)
    n = th.numel()
    assert n > 16 * 8
    st = steps[th]
    report("scan_saturate_evals_through", rays=n, alpha=out["evals"], steps=int(st.sum()))
    assert int(st.sum()) + n <= out["evals"] <= int(st.sum()) + 8 * (n - 128) + 129 * 128
    assert bool((out["thr"] == M.SAT_THR).all())


@pytest.mark.parametrize("prec", PRECS)
def test_scan_saturate_off_is_exact_scan(prec):
    hidden, (P, blocks) = 128, M.SIZES[0]
    one = _run(hidden, prec, P, 1, True, _opts(blocks))
    off = _run(hidden, prec, P, 2, True, _opts(blocks, scan_saturate=0))
    assert not off["broken"]
    assert_same(off, one, GEOMETRY + ("thr", "index", "alpha"), "scan_saturate=0")
    assert off["evals"] == one["evals"]


def test_row_renderer_frames():
    """a 48^2 NeRFIntegrator(Direct) frame is bit-equal with scan_saturate 0 and 1; a plain Direct
    frame (no scan at all) is bit-equal to the one composed after an exact scan; python's RNG
    ends in the same state every time"""
    import bench
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer import render as RR
    from neural_raytracing_amd.pathtracer.integrators import Direct
    _lib.set_precision("fp32")
    dev = torch.device("cuda", 0)
    size = 48
    scene = bench.build_scene(dev, 64, light_gain=bench.LIGHT_GAIN)
    focal = float(0.5 * size / math.tan(0.5 * 0.6911))
    cams = scene["pt"].cameras.NeRFCamera(cam_to_world=bench.view_c2w(0, 1)[None].to(dev),
                                          focal=focal, device=dev)

    def frame(integrator, **options):
        for k, v in options.items():
            lib_opt(k, v)
        rr = RR.RowRenderer(scene["shape"], scene["lights"], cams, integrator, scene["bsdf"], size,
                            list(range(size)), background=0.0, with_noise=1e-3, device=dev)
        torch.manual_seed(5)
        random.seed(5)
        with torch.no_grad():
            img = rr.render().clone()
        return img.cpu(), random.getstate()

    on, s_on = frame(scene["integrator"], scan_saturate=1)
    off, s_off = frame(scene["integrator"], scan_saturate=0)
    assert on.shape[-1] == 4 and not torch.isnan(on).any()
    assert bool((on[..., 3] == 1.0).any()) and bool((on[..., 3] < 0.5).any())
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))
    direct = Direct()
    direct.training = True
    plain, s_plain = frame(direct)
    # the same frame with the exact scan run first (a bare Direct keeps primary = 1)
    torch.manual_seed(5)
    random.seed(5)
    positions = RR.RowRenderer(scene["shape"], scene["lights"], cams, direct, scene["bsdf"], size,
                               list(range(size)), device=dev).positions
    with torch.no_grad():
        rays = cams.rays_tile(0, 0, size, size, size, 1e-3, positions=positions)
        b = RR.direct_kernels(direct, scene["shape"], rays.reshape(-1, 6), scene["bsdf"],
                              scene["lights"])
        want = torch.empty(1, size, size, 3, device=dev)
        RR.composite(b, 1, size, size, False, 0.0, want, 0, 0)
    s_want = random.getstate()
    assert torch.equal(plain.view(torch.int32), want.cpu().view(torch.int32))
    assert s_on == s_off == s_plain == s_want
