"""Training NeRFLE with one light per camera (nerf.py:193-197), through the tensor-op chain of
``_forward_train`` and through the fused volume render (``FUSED_TRAINING``): 3 cameras x 5 x 3
rays, per-camera locations, against float64 autograd of the oracle under the bars and helpers of
tests/test_gpu_nerf_train.py (image 1e-4; per gradient tensor ``err <= max(2e-3 scale, 4 e32) +
1e-9``).  Each case first shows on the CPU that the oracle under row 0 for every camera is five
image tolerances away on cameras 1.., so the comparison tells the two apart."""
import random

import pytest
import torch

from oracle import pathtracer_ref as R
from tests.report import report
from tests.test_gpu_nerf_train import (_check_grads, _names, _nerfle_setup, _oracle_lins,
                                       _to_dtype)
from tests.test_gpu_nerfle_lights import POINT_LOCS

pytestmark = pytest.mark.gpu

SHAPE = (3, 5, 3, 1)
# (the envmap of PointLights' default scale 100 saturates the colour MLP for a light right next
# to a sampled direction: these rows keep every row's location gradient well away from zero)
ENV_LOCS = [[0.3, 1.0, 0.2], [-0.5, 0.7, 0.4], [0.9, -0.4, 1.1]]
LIGHT_ATTRS = ("scale", "intensity", "location", "const", "linear", "square")


def _oracle_run(ref, rays, w, jitter, dtype, envmap, locs):
    """(image, gradients) of the oracle in ``dtype`` under location rows ``locs``."""
    r = _to_dtype(ref, dtype)
    light = None
    if envmap:
        light = R.PointLightRef(location=locs.reshape(-1).tolist())
        for a in LIGHT_ATTRS:
            setattr(light, a, getattr(light, a).to(dtype).requires_grad_())
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        out = r(rays.to(dtype), None if envmap else locs.to(dtype), jitter=jitter, light=light)
        (out * w.to(dtype)).sum().backward()
    finally:
        torch.set_default_dtype(old)
    grads = {k: p.grad.double() for k, p in _names(r.first, r.second, _oracle_lins).items()}
    if envmap:
        for a in LIGHT_ATTRS:
            gr = getattr(light, a).grad
            grads[f"light.{a}"] = torch.zeros_like(getattr(light, a)).double() if gr is None \
                else gr.double()
    return out.detach().double(), grads


def _prove_gap(ref, rays, w, jitter, envmap, locs, want_img):
    row0_img, _ = _oracle_run(ref, rays, w, jitter, torch.float64, envmap,
                              locs[:1].expand(3, 3).contiguous())
    gap = min((want_img[n] - row0_img[n]).abs().max().item() for n in range(1, 3))
    report(f"nerfle_lights_train_gap[{'envmap' if envmap else 'point'}]", gap=gap)
    assert gap >= 5e-4, gap


@pytest.mark.parametrize("fused", [False, True], ids=["tensor_ops", "fused"])
def test_point_lights_per_camera_training(monkeypatch, fused):
    from neural_raytracing_amd import set_precision
    from neural_raytracing_amd.pathtracer.lights import PointLights
    from neural_raytracing_amd.pathtracer.shapes import NeRFLE
    ref, mine, rays, w = _nerfle_setup(False, 8, SHAPE, 0.5)
    locs = torch.tensor(POINT_LOCS)
    random.seed(6)
    jitter = random.random()
    want_img, want = _oracle_run(ref, rays, w, jitter, torch.float64, False, locs)
    _, ref32 = _oracle_run(ref, rays, w, jitter, torch.float32, False, locs)
    _prove_gap(ref, rays, w, jitter, False, locs, want_img)
    assert all(v.abs().max() > 0 for v in want.values())
    set_precision("fp32")
    monkeypatch.setattr(NeRFLE, "FUSED_TRAINING", fused)
    lights = PointLights(location=locs.cuda(), device="cuda")
    random.seed(6)
    img = mine(rays.cuda(), lights)
    assert img.requires_grad and img.shape == SHAPE + (3,)
    ierr = (img.detach().cpu().double() - want_img).abs().max().item()
    report(f"nerfle_lights_train[point,fused={fused}]", image=ierr)
    assert ierr <= 1e-4, ierr
    (img * w.cuda()).sum().backward()
    got = {k: p.grad for k, p in _names(mine.first, mine.second, lambda m: m._linears()).items()}
    _check_grads(f"nerfle_lights_train[point,fused={fused}]", got, want, ref32)
    if fused:  # the fused render's FP32 frame is the no-grad frame, bit for bit
        random.seed(6)
        with torch.no_grad():
            plain = mine(rays.cuda(), lights)
        assert torch.equal(img.detach().view(torch.int32), plain.view(torch.int32))


@pytest.mark.parametrize("fused", [False, True], ids=["tensor_ops", "fused"])
def test_envmap_lights_per_camera_training(monkeypatch, fused):
    """Also the gradients of the light's parameters and of its location [3, 3] through
    lights.envmap and the per-row d_light reduction; row n of location.grad does not move when
    another camera's d_out is zeroed."""
    from neural_raytracing_amd import set_precision
    from neural_raytracing_amd.pathtracer.lights import PointLights
    from neural_raytracing_amd.pathtracer.shapes import NeRFLE
    ref, mine, rays, w = _nerfle_setup(True, 9, SHAPE, 0.5)
    locs = torch.tensor(ENV_LOCS)
    random.seed(4)
    jitter = random.random()
    want_img, want = _oracle_run(ref, rays, w, jitter, torch.float64, True, locs)
    _, ref32 = _oracle_run(ref, rays, w, jitter, torch.float32, True, locs)
    _prove_gap(ref, rays, w, jitter, True, locs, want_img)
    assert want["light.location"].shape == (3, 3)
    assert all(v.abs().max() > 0 for k, v in want.items()
               if k not in ("light.const", "light.linear"))  # those two sit under their clamp
    set_precision("fp32")
    monkeypatch.setattr(NeRFLE, "FUSED_TRAINING", fused)

    def run(weights):
        mine.zero_grad(set_to_none=True)
        lights = PointLights(location=locs.cuda().requires_grad_(), device="cuda")
        random.seed(4)
        img = mine(rays.cuda(), lights)
        assert img.requires_grad
        (img * weights.cuda()).sum().backward()
        return img.detach(), lights
    img, lights = run(w)
    ierr = (img.cpu().double() - want_img).abs().max().item()
    report(f"nerfle_lights_train[envmap,fused={fused}]", image=ierr)
    assert ierr <= 1e-4, ierr
    got = {k: p.grad for k, p in _names(mine.first, mine.second, lambda m: m._linears()).items()}
    for a in LIGHT_ATTRS:
        gr = getattr(lights, a).grad
        got[f"light.{a}"] = torch.zeros_like(getattr(lights, a)) if gr is None else gr
    _check_grads(f"nerfle_lights_train[envmap,fused={fused}]", got, want, ref32)
    loc_grad = lights.location.grad.clone()
    for n in range(3):
        masked = w.clone()
        masked[(n + 1) % 3] = 0
        _, other = run(masked)
        assert torch.equal(other.location.grad[n].view(torch.int32), loc_grad[n].view(torch.int32))
        assert not bool(other.location.grad[(n + 1) % 3].any())
