"""CPU checks of the NeRF-- camera's boundary: the class resolves through the compat package, its
parameters() are the four tensors, CPU tensors are refused, and the new C entries are bound with
the declared argument counts."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nrt.h")

NEW_ENTRIES = {"nrt_raygen_mm": 15, "nrt_raygen_mm_backward_workspace_bytes": 3,
               "nrt_raygen_mm_backward": 20, "nrt_nerf_rays_backward": 10}


def _camera():
    from pytorch3d.pathtracer.cameras import NeRFMMCamera
    return NeRFMMCamera(t=torch.zeros(2, 3), angle=torch.zeros(2, 1),
                        axis=torch.tensor([[0.0, 1.0, 0.0]] * 2), focals=torch.full((2, 2), 20.0),
                        device="cpu")


def test_compat_import_resolves_to_the_product_class():
    from pytorch3d.pathtracer.cameras import NeRFMMCamera
    from neural_raytracing_amd.pathtracer import cameras
    assert NeRFMMCamera is cameras.NeRFMMCamera
    assert issubclass(NeRFMMCamera, cameras.Camera)


def test_parameters_are_the_four_tensors():
    cam = _camera()
    assert len(cam) == 2
    got = cam.parameters()
    assert [id(x) for x in got] == [id(cam.angle), id(cam.axis), id(cam.t), id(cam.focals)]
    torch.optim.Adam(got)  # what train loops hand to an optimiser


def test_cpu_tensors_are_refused():
    from neural_raytracing_amd import NrtError
    cam = _camera()
    with pytest.raises(NrtError, match="HIP path only"):
        cam.rays_tile(0, 0, 4, 4, 16)
    with pytest.raises(NrtError, match="HIP path only"):
        cam.sample_positions(torch.zeros(4, 4, 2), None, size=16)


def test_new_entries_are_declared_and_bound():
    from neural_raytracing_amd import _lib
    assert _lib.NRT_CAM_NERFMM == 3
    raw = open(HEADER).read()
    assert re.search(r"#define\s+NRT_CAM_NERFMM\s+3\b", raw)
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = {name: len(args.split(","))
                for name, args in re.findall(r"\b(nrt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}
    for name, nargs in NEW_ENTRIES.items():
        assert declared.get(name) == nargs, (name, declared.get(name))
        assert len(_lib._SIGNATURES[name][1]) == nargs, name
