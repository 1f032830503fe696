"""NeRFLE with one light per camera (nerf.py:193-197: the light's location rows, or its envmap
rows, broadcast over the camera axis of the rays): nrt_nerfle_forward_lights on the unfused
kernels and on the fused k_nerfle16 (per-lane row lookup; the envmap fold as a one-hot over the
rows), the batched envmap entry, chunked frames, the refusals, the per-row training kernels
called directly, and the NeRF+PT driver's batch shape.

Every comparison against the oracle first proves, on the CPU, that it can tell "row n for camera
n" from "row 0 for every camera": the two oracle frames must differ on cameras 1.. by at least
five times the tolerance applied afterwards, or the test fails on its inputs.  The point-light
gap (a few 1e-3 with these weights) clears the FP32 bar only, so FP16 with a point light is
pinned by the bit-equality with the single-light calls instead."""
import functools
import random

import pytest
import torch
import torch.nn.functional as F

from oracle import pathtracer_ref as R
from tests.helpers import copy_mlp, seeded
from tests.helpers import lib_opt as _lib_opt
from tests.report import report

pytestmark = pytest.mark.gpu

N, W, H = 3, 7, 3  # 21 rays a camera: a camera boundary inside a wave's tiles and inside a block
POINT_LOCS = [[0.3, 1.0, 0.2], [-2.5, 1.5, 2.0], [3.0, -1.0, -2.5]]
ENV_LOCS = [[0.3, 1.0, 0.2], [0.1, 0.9, 0.0], [0.05, -0.95, -0.25]]
ENV_KW = dict(intensity=(0.9, 0.5, 0.3), scale=3.0)  # test_nerfle_envmap_matches_oracle's
FP32_TOL, FP16_TOL = 1e-4, 2e-2  # test_nerfle_matches_oracle's
JITTER_SEED = 6


def _rays(n, w, h, seed):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.0, 0.2, 1.2]) + 0.1 * torch.randn(n, w, h, 1, 3, generator=g)
    d = F.normalize(torch.cat([torch.rand(n, w, h, 1, 2, generator=g) - 0.5,
                               -torch.ones(n, w, h, 1, 1)], -1), dim=-1)
    return torch.cat([o, d], -1)


def _pair(envmap, S, seed):
    from neural_raytracing_amd.pathtracer.shapes import NeRFLE
    seeded(seed)
    ref = R.NeRFLERef(steps=S, envmap=envmap)
    mine = NeRFLE(envmap=envmap, device="cpu", steps=S)
    copy_mlp(mine.first, ref.first)
    copy_mlp(mine.second, ref.second)
    return ref, mine


def _oracle(ref, envmap, rays, locs):
    """The oracle frame of ``rays`` [n, ...] under location rows ``locs`` [n or 1, 3]."""
    random.seed(JITTER_SEED)
    with torch.no_grad():
        if envmap:
            light = R.PointLightRef(location=locs.reshape(-1).tolist(), **ENV_KW)
            return ref(rays, None, jitter=random.random(), light=light)
        return ref(rays, locs, jitter=random.random())


@functools.lru_cache(maxsize=None)
def _case(envmap, S):
    """(ref, mine on the GPU, rays, locs, oracle frame with per-camera rows, gap): computed once
    per (envmap, S) and shared; nothing here is modified afterwards.  gap: how far the oracle
    frame with row 0 for every camera is from it on cameras 1.. (the least over those cameras of
    the largest difference)."""
    ref, mine = _pair(envmap, S, 29 if envmap else 19)
    rays = _rays(N, W, H, 5 if envmap else 4)
    locs = torch.tensor(ENV_LOCS if envmap else POINT_LOCS)
    want = _oracle(ref, envmap, rays, locs)
    row0 = _oracle(ref, envmap, rays, locs[:1].expand(N, 3).contiguous())
    assert torch.equal(want[0], row0[0])
    gap = min((want[n] - row0[n]).abs().max().item() for n in range(1, N))
    return ref, mine.cuda(), rays, locs, want, gap


def _lights(envmap, locs):
    from neural_raytracing_amd.pathtracer.lights import PointLights
    if envmap:
        return PointLights(intensity=list(ENV_KW["intensity"]), location=locs.cuda(),
                           scale=ENV_KW["scale"], device="cuda")
    return PointLights(location=locs.cuda(), device="cuda")


def _mode(mode):
    """"fp32" | "fp16" (fused k_nerfle16) | "fp16-unfused" -> the precision set."""
    from neural_raytracing_amd import set_precision
    _lib_opt("nerf_fused", 0 if mode == "fp16-unfused" else 1)
    set_precision("fp32" if mode == "fp32" else "fp16")


def _render(mine, rays, lights):
    random.seed(JITTER_SEED)
    with torch.no_grad():
        return mine(rays.cuda(), lights).cpu()


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    from neural_raytracing_amd import set_precision
    set_precision("fp32")


MODES = ["fp32", "fp16", "fp16-unfused"]


# ------------------------------------------------------------------------------------------
# 1. parity against the oracle
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [64, 37])
@pytest.mark.parametrize("envmap", [False, True], ids=["point", "envmap"])
def test_per_camera_lights_match_oracle(envmap, S, mode):
    """3 cameras x 7 x 3 rays, each camera under its own light row, against the oracle's
    broadcast.  S = 37: a 32-sample tile straddles two rays, and at every camera boundary two
    cameras.  The gap between the per-camera and the row-0 oracle frames must be five times the
    tolerance (the point light's clears the FP32 bar only: its FP16 cases are asserted against
    the oracle all the same and pinned by test_batched_call_equals_single_light_calls)."""
    _, mine, rays, locs, want, gap = _case(envmap, S)
    tol = FP32_TOL if mode == "fp32" else FP16_TOL
    need = 5 * (tol if envmap else FP32_TOL)
    report(f"nerfle_lights_gap[{'envmap' if envmap else 'point'},S={S}]", gap=gap, need=need)
    assert gap >= need, (gap, need)
    _mode(mode)
    got = _render(mine, rays, _lights(envmap, locs))
    assert got.shape == want.shape == (N, W, H, 1, 3)
    err = (got - want).abs().max().item()
    report(f"nerfle_lights[{'envmap' if envmap else 'point'},S={S},{mode}]", err=err, tol=tol)
    assert err <= tol, err


# ------------------------------------------------------------------------------------------
# 2. the batched call against the single-light calls, camera by camera
# ------------------------------------------------------------------------------------------

def _singles(mine, envmap, rays, locs):
    return [_render(mine, rays[n:n + 1], _lights(envmap, locs[n:n + 1])) for n in range(len(locs))]


def _fused_unfused_bound(mine, rays, locs):
    """The largest difference between the fused and the unfused FP16 frame of the single-light
    envmap call over the cameras' own (rays, light) pairs."""
    _mode("fp16")
    fused = _singles(mine, True, rays, locs)
    _mode("fp16-unfused")
    unfused = _singles(mine, True, rays, locs)
    return max((a - b).abs().max().item() for a, b in zip(fused, unfused))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [64, 37])
@pytest.mark.parametrize("envmap", [False, True], ids=["point", "envmap"])
def test_batched_call_equals_single_light_calls(envmap, S, mode):
    """Camera n of the batched call against the same rays rendered alone under light n: the same
    bits for the point light at every precision and for the unfused envmap.  The fused envmap
    moves the fold's input column (the order of the k-step's sum may differ): bounded by the
    fused-to-unfused FP16 difference of the single-light calls, measured here."""
    _, mine, rays, locs, _, _ = _case(envmap, S)
    _mode(mode)
    for n in range(1, N):  # light n must matter on camera n's rays
        other = _render(mine, rays[n:n + 1], _lights(envmap, locs[:1]))
        own = _render(mine, rays[n:n + 1], _lights(envmap, locs[n:n + 1]))
        assert not torch.equal(own, other)
    got = _render(mine, rays, _lights(envmap, locs))
    singles = _singles(mine, envmap, rays, locs)
    if envmap and mode == "fp16":
        bound = _fused_unfused_bound(mine, rays, locs)
        err = max((got[n:n + 1] - singles[n]).abs().max().item() for n in range(N))
        report(f"nerfle_lights_fold[S={S}]", err=err, bound=bound)
        assert err <= bound, (err, bound)
    else:
        for n in range(N):
            assert torch.equal(got[n:n + 1].view(torch.int32), singles[n].view(torch.int32)), n


# ------------------------------------------------------------------------------------------
# 3. one light row for three cameras
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("envmap", [False, True], ids=["point", "envmap"])
def test_one_row_serves_every_camera(envmap, mode):
    """L = 1 with N = 3 is the single-light frame: equal, bit for bit, to the three
    single-camera calls under that light."""
    _, mine, rays, locs, _, _ = _case(envmap, 37)
    _mode(mode)
    got = _render(mine, rays, _lights(envmap, locs[1:2]))
    for n in range(N):
        alone = _render(mine, rays[n:n + 1], _lights(envmap, locs[1:2]))
        assert torch.equal(got[n:n + 1].view(torch.int32), alone.view(torch.int32)), n


# ------------------------------------------------------------------------------------------
# 4. the fold's capacity
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [4, 14])
def test_envmap_fold_capacity(L):
    """Envmap with L = 4 cameras (the NeRF+LE driver's batch) and with one more camera than a
    folded program holds (13: two groups of cameras), 3 rays a camera: the fused frame against
    the unfused one under the fused-to-unfused difference of the single-light calls."""
    _, mine, _, _, _, _ = _case(True, 37)
    rays = _rays(L, 3, 1, 11)
    g = torch.Generator().manual_seed(12)
    locs = torch.tensor(ENV_LOCS[0]) + 0.8 * torch.randn(L, 3, generator=g)
    bound = _fused_unfused_bound(mine, rays, locs)
    _mode("fp16")
    fused = _render(mine, rays, _lights(True, locs))
    _mode("fp16-unfused")
    unfused = _render(mine, rays, _lights(True, locs))
    assert not torch.equal(unfused[L - 1:], _render(mine, rays[L - 1:], _lights(True, locs[:1])))
    err = (fused - unfused).abs().max().item()
    report(f"nerfle_lights_capacity[L={L}]", err=err, bound=bound)
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------
# 5. chunked frames
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("envmap", [False, True], ids=["point", "envmap"])
@pytest.mark.parametrize("chunk", [25, 8], ids=["whole_cameras", "inside_a_camera"])
def test_chunked_frame_equals_one_call(monkeypatch, chunk, envmap, mode):
    """MAX_WORKSPACE_BYTES for 25 rays a call (one 21-ray camera each) and for 8 (21 = 8 + 8 + 5
    inside every camera): the frame of the one call, bit for bit."""
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.shapes import NeRFLE
    _, mine, rays, locs, _, _ = _case(envmap, 37)
    _mode(mode)
    lights = _lights(envmap, locs)
    whole = _render(mine, rays, lights)
    lib = _lib.load(require_device=True)
    per_ray = lib.nrt_nerfle_workspace_bytes_for(mine.first.nrt(), mine.second.nrt(), 1024, 37,
                                                 48 if envmap else 3,
                                                 _lib.precision_code()) / 1024
    monkeypatch.setattr(NeRFLE, "MAX_WORKSPACE_BYTES", int(per_ray * (chunk + 0.5)))
    calls = []
    real = _lib.call

    def spy(name, *a):
        if name == "nrt_nerfle_forward_lights":
            calls.append(a[3])
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", spy)
    got = _render(mine, rays, lights)
    assert calls == ([21] * 3 if chunk == 25 else [8, 8, 5] * 3), calls
    assert torch.equal(got.view(torch.int32), whole.view(torch.int32))


# ------------------------------------------------------------------------------------------
# 6. refusals and the empty frame
# ------------------------------------------------------------------------------------------

def test_row_count_and_intensity_refusals_and_empty_frame():
    from neural_raytracing_amd import NrtError
    from neural_raytracing_amd.pathtracer.lights import PointLights
    _, mine, rays, locs, _, _ = _case(False, 37)
    _mode("fp32")
    with torch.no_grad():
        with pytest.raises(NrtError, match="one per camera"):
            mine(rays.cuda(), _lights(False, locs[:2]))
        inten = torch.tensor([[1.0, 1.0, 1.0], [0.5, 1.0, 1.0], [1.0, 1.0, 0.2]], device="cuda")
        with pytest.raises(NrtError, match="intensity"):
            mine(rays.cuda(), PointLights(intensity=inten, location=locs.cuda(), device="cuda"))
        empty = mine(rays[:, :0].cuda(), _lights(False, locs))
    assert empty.shape == (N, 0, H, 1, 3)
    # the C entry: rows and rays that do not multiply out
    from neural_raytracing_amd import _lib
    flat = rays.reshape(-1, 6).cuda().contiguous()
    ts = torch.linspace(0, 2, 37).cuda()
    out = torch.empty(flat.shape[0], 3, device="cuda")
    ws = torch.empty(1 << 22, dtype=torch.uint8, device="cuda")
    with pytest.raises(NrtError, match="rows \\* rays_per_light"):
        _lib.call("nrt_nerfle_forward_lights", mine.first.nrt(), mine.second.nrt(), _lib.ptr(flat),
                  flat.shape[0], _lib.ptr(ts), 37, _lib.ptr(locs.cuda()), 3, 3, 20, _lib.ptr(out),
                  _lib.ptr(ws), _lib.precision_code(), _lib.stream())


def test_envmap_rows_entry_equals_the_handle_entry():
    """nrt_light_envmap_rows row r is nrt_light_envmap of a point light at loc[r], bit for bit,
    and follows PointLights.envmap."""
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.lights import PointLights
    from neural_raytracing_amd.pathtracer.utils import elev_azim_to_dir
    _lib.load(require_device=True)
    locs = torch.tensor(ENV_LOCS).cuda()
    bins = 4
    inten = torch.tensor(ENV_KW["intensity"])
    out = torch.full((3, 3 * bins * bins), float("nan"), device="cuda")
    _lib.call("nrt_light_envmap_rows", _lib.ptr(locs), 3, inten.data_ptr(), 1e-8, 1e-8, 1.0,
              ENV_KW["scale"], bins, _lib.ptr(out), _lib.stream())
    points = torch.stack(torch.meshgrid(torch.linspace(0, 180, bins), torch.linspace(0, 45, bins),
                                        indexing="ij"), dim=-1).reshape(-1, 2)
    for r in range(3):
        one = PointLights(intensity=list(ENV_KW["intensity"]), location=locs[r:r + 1],
                          scale=ENV_KW["scale"], device="cuda")
        single = torch.empty(3 * bins * bins, device="cuda")
        _lib.call("nrt_light_envmap", one.nrt(), bins, _lib.ptr(single), _lib.stream())
        assert torch.equal(out[r].view(torch.int32), single.view(torch.int32))
        with torch.no_grad():
            want = one.envmap(elev_azim_to_dir(points.cuda())).reshape(-1)
        assert (out[r] - want).abs().max().item() <= 1e-5 * float(want.abs().max())


# ------------------------------------------------------------------------------------------
# 8. the training kernels with two light rows, called directly
# ------------------------------------------------------------------------------------------

def test_reduce_and_assemble_with_two_light_rows():
    """nrt_nerf_reduce(NERFLE) with rays_per_latent = P / 2: per light row the sum over its
    rays' samples of d_x2[:, 67:] (48 columns, several blocks).  Bound: a float32 sum of m terms
    in any order errs by at most (m - 1) 2^-24 sum|v|; two runs give the same bits.
    nrt_nerf_assemble writes each ray's own row into x2's light columns."""
    from neural_raytracing_amd import _lib
    lib = _lib.load(require_device=True)
    g = torch.Generator().manual_seed(5)
    S, P, dim, rpl = 70, 70, 48, 35
    d2 = torch.randn(S * P, 67 + dim, generator=g)
    terms = d2[:, 67:].double().reshape(S, 2, rpl, dim).permute(1, 0, 2, 3).reshape(2, S * rpl, dim)
    want = terms.sum(1)
    bound = (terms.shape[1] - 1) * 2.0 ** -24 * terms.abs().sum(1) + 1e-12
    d2g = d2.cuda()
    outs = []
    for _ in range(2):
        ws = torch.empty(lib.nrt_nerf_volume_workspace_bytes(P, S, dim), dtype=torch.uint8,
                         device="cuda")
        out = torch.full((2, dim), float("nan"), device="cuda")
        _lib.call("nrt_nerf_reduce", 0, None, _lib.ptr(d2g), P, S, dim, 0, rpl, _lib.ptr(out),
                  _lib.ptr(ws), _lib.stream())
        outs.append(out.cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    err = (outs[0].double() - want).abs()
    report("nerf_reduce[light rows]", err=err.max().item(), bound=bound.min().item())
    assert (err <= bound).all(), (err.max().item(), bound.min().item())
    # assembly: x2 [n, 67 + dim] = [first_out[:, 1:] | r_d | extra[p // rpl]]
    first_out = torch.randn(S * P, 65, generator=g).cuda()
    rays = torch.randn(P, 6, generator=g).cuda()
    extra = torch.randn(2, dim, generator=g).cuda()
    x2 = torch.full((S * P, 67 + dim), float("nan"), device="cuda")
    alpha = torch.full((S, P), float("nan"), device="cuda")
    _lib.call("nrt_nerf_assemble", 0, _lib.ptr(first_out), _lib.ptr(rays), P, S, _lib.ptr(extra),
              dim, 64, rpl, None, _lib.ptr(x2), None, _lib.ptr(alpha), _lib.stream())
    x2 = x2.reshape(S, P, 67 + dim)
    assert torch.equal(x2[..., :64], first_out.reshape(S, P, 65)[..., 1:])
    assert torch.equal(alpha, first_out.reshape(S, P, 65)[..., 0])
    assert torch.equal(x2[..., 64:67], rays[None, :, 3:].expand(S, P, 3))
    row = torch.arange(P, device="cuda") // rpl
    assert torch.equal(x2[..., 67:], extra[row][None].expand(S, P, dim))
    with pytest.raises(_lib.NrtError, match="multiple of rays_per_latent"):
        _lib.call("nrt_nerf_assemble", 0, _lib.ptr(first_out), _lib.ptr(rays), P, S,
                  _lib.ptr(extra), dim, 64, 33, None, _lib.ptr(x2), None, _lib.ptr(alpha),
                  _lib.stream())


# ------------------------------------------------------------------------------------------
# 9. the NeRF+PT / NeRF+LE driver's batch: 4 cameras, one light on each
# ------------------------------------------------------------------------------------------

def _driver_scene(envmap):
    """4 OpenGL cameras around the volume, ``lights.location = cameras.get_camera_center() *
    1.05`` (one location row per camera), NeRFReproduce; the oracle's cameras beside them."""
    from neural_raytracing_amd.pathtracer.cameras import OpenGLPerspectiveCameras
    from neural_raytracing_amd.pathtracer.lights import PointLights
    ref, mine = _pair(envmap, 64, 23)
    cams, Rs, Ts = [], [], []
    for elev, azim in ((0.0, -90.0), (15.0, -30.0), (30.0, 30.0), (45.0, 90.0)):
        Rm, Tm = R.look_at_view_transform_ref(dist=1.0, elev=elev, azim=azim)
        cams.append(R.FoVCameraRef(Rm, Tm, znear=1.0, zfar=100.0))
        Rs.append(Rm)
        Ts.append(Tm)
    cameras = OpenGLPerspectiveCameras(R=torch.cat(Rs), T=torch.cat(Ts), device="cuda")
    lights = PointLights(scale=10, device="cuda")
    lights.location = cameras.get_camera_center() * 1.05
    locs = torch.cat([c.center() * 1.05 for c in cams])
    assert lights.location.shape == (4, 3)
    assert torch.allclose(lights.location.cpu(), locs, atol=1e-5)
    return ref, mine.cuda(), cams, cameras, lights, locs


def test_driver_batch_renders_and_trains():
    """pathtrace_sample as the driver calls it (crop 16, one tile, squeeze_first=False) against
    the oracle on the oracle cameras' rays, camera n under location row n; then one optimiser
    step on the same batch lowers the loss."""
    import neural_raytracing_amd.pathtracer as pt
    from neural_raytracing_amd import set_precision
    from neural_raytracing_amd.pathtracer.integrators import NeRFReproduce
    from tests.test_gpu_configs import _OracleCams
    ref, mine, cams, cameras, lights, locs = _driver_scene(False)
    size, crop, uv = 32, 16, (8, 4)
    rays = _OracleCams(cams).sample_positions(R._tile_positions(uv[0], uv[1], crop), size)
    assert rays.shape == (4, crop, crop, 1, 6)
    want = _oracle(ref, False, rays, locs)[:, :, :, 0]
    row0 = _oracle(ref, False, rays, locs[:1].expand(4, 3).contiguous())[:, :, :, 0]
    gap = min((want[n] - row0[n]).abs().max().item() for n in range(1, 4))
    report("nerfle_lights_driver_gap", gap=gap)
    assert gap >= 5 * FP32_TOL, gap
    set_precision("fp32")

    def sample():
        random.seed(JITTER_SEED)
        return pt.pathtrace_sample(mine, lights, cameras, NeRFReproduce(), size=size,
                                   chunk_size=size, bundle_size=1, crop_size=crop, uv=uv,
                                   background=0, with_noise=0.0, addition=lambda mi: mi,
                                   squeeze_first=False, silent=True)[0]
    with torch.no_grad():
        got = sample()
    assert got.shape == (4, crop, crop, 3)
    err = (got.cpu() - want).abs().max().item()
    report("nerfle_lights_driver", err=err)
    assert err <= FP32_TOL, err
    target = want.cuda() * 0.5
    opt = torch.optim.Adam(mine.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = F.mse_loss(sample(), target)
    loss.backward()
    opt.step()
    with torch.no_grad():
        after = F.mse_loss(sample(), target)
    report("nerfle_lights_driver_step", before=loss.item(), after=after.item())
    assert after.item() < loss.item(), (loss.item(), after.item())


def test_driver_batch_row_shards_assemble_the_frame(monkeypatch):
    """The simulated two-rank row shard of pathtrace (each rank renders [N, its rows, H, B] rays,
    still camera-major) reproduces the unsharded 4-camera frame bit for bit."""
    import neural_raytracing_amd.pathtracer as pt
    from neural_raytracing_amd import set_precision
    from neural_raytracing_amd.pathtracer.integrators import NeRFReproduce
    from tests.test_gpu_rccl import _simulated_shards, _unsharded
    _, mine, _, cameras, lights, _ = _driver_scene(False)
    set_precision("fp32")
    dev = torch.device("cuda", 0)

    def render():
        img, _ = pt.pathtrace(mine, lights, cameras, NeRFReproduce(), size=32, chunk_size=16,
                              bundle_size=1, background=0, silent=True, device=dev)
        return img.clone()
    want, want_state = _unsharded(render)
    assert want.shape == (4, 32, 32, 3)
    got, rows_of, states = _simulated_shards(monkeypatch, 2, render)
    assert sorted(r for rows in rows_of for r in rows) == list(range(32))
    assert all(s == want_state for s in states)
    assert torch.equal(got, want)
    assert float(want.abs().max()) > 0
