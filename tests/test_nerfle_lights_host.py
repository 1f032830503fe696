"""CPU checks of NeRFLE's one-light-per-camera boundary: the two new C entries are bound with the
declared argument counts, the light row count is validated against the rays' camera axis from
shapes alone, and the frame is split into calls of whole cameras or pieces of one camera."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nrt.h")


def _declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["nrt_nerfle_forward_lights", "nrt_light_envmap_rows"])
def test_new_entries_are_bound_as_declared(name):
    import ctypes
    from neural_raytracing_amd import _lib
    args = _declared(name)
    res, sig = _lib._SIGNATURES[name]
    assert res is ctypes.c_int32 and len(sig) == len(args)
    for decl, ct in zip(args, sig):
        want = ctypes.c_void_p if "*" in decl else \
            {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int32,
             "float": ctypes.c_float}[decl.split()[0]]
        assert ct is want, (name, decl)
    # nrt_nerfle_forward_lights is nrt_nerfle_forward with rows and rays_per_light after light_dim
    if name == "nrt_nerfle_forward_lights":
        old = _lib._SIGNATURES["nrt_nerfle_forward"][1]
        assert sig[:8] == old[:8] and sig[10:] == old[8:]
        assert sig[8] is ctypes.c_int64 and sig[9] is ctypes.c_int64


class _Lights:
    def __init__(self, location, intensity=None):
        self.location = location
        self.intensity = torch.ones(1, 3) if intensity is None else intensity


def test_light_rows_are_one_or_one_per_camera():
    from neural_raytracing_amd import NrtError
    from neural_raytracing_amd.pathtracer.shapes import NeRFLE
    nerf = NeRFLE(device="cpu", steps=4)
    lead = (3, 7, 3, 1)
    assert nerf.light_rows(_Lights(torch.zeros(1, 3)), lead) == 1
    assert nerf.light_rows(_Lights(torch.zeros(3)), lead) == 1
    # equal rows are still one per camera: the row count decides, not the values
    assert nerf.light_rows(_Lights(torch.zeros(3, 3)), lead) == 3
    for L in (2, 4):
        with pytest.raises(NrtError, match="one per camera"):
            nerf.light_rows(_Lights(torch.zeros(L, 3)), lead)
    with pytest.raises(NrtError, match="one per camera"):
        nerf.light_rows(_Lights(torch.zeros(3, 3)), (63,))  # no camera axis: one light
    same = torch.tensor([[0.2, 0.4, 0.6]]).expand(3, 3)
    assert nerf.light_rows(_Lights(torch.zeros(3, 3), same), lead) == 3
    rows = torch.tensor([[1.0, 1.0, 1.0], [1.0, 0.5, 1.0], [1.0, 1.0, 1.0]])
    with pytest.raises(NrtError, match="intensity"):
        nerf.light_rows(_Lights(torch.zeros(3, 3), rows), lead)


def test_nerfle_refuses_cpu_rays_before_anything_else():
    from neural_raytracing_amd import NrtError
    from neural_raytracing_amd.pathtracer.shapes import NeRFLE
    with pytest.raises(NrtError, match="HIP path only"):
        NeRFLE(device="cpu", steps=4)(torch.zeros(3, 2, 2, 1, 6), _Lights(torch.zeros(2, 3)))


def test_chunk_plan_of_a_three_camera_frame():
    """The plan NeRFLE.forward follows (_volume.chunks, shared with PlainNeRF): 3 cameras of 21
    rays under 3 light rows, and the same 63 rays under one row."""
    from neural_raytracing_amd.pathtracer.shapes._volume import chunks
    # (first ray, rays, first row, rows, rays per row)
    assert list(chunks(63, 21, 100)) == [(0, 63, 0, 3, 21)]
    assert list(chunks(63, 21, 50)) == [(0, 42, 0, 2, 21), (42, 21, 2, 1, 21)]
    assert list(chunks(63, 21, 25)) == [(21 * c, 21, c, 1, 21) for c in range(3)]
    assert list(chunks(63, 21, 8)) == [(21 * c + o, n, c, 1, n) for c in range(3)
                                       for o, n in ((0, 8), (8, 8), (16, 5))]
    # one light for every camera: the rays are one row's, split anywhere
    assert list(chunks(63, 63, 100)) == [(0, 63, 0, 1, 63)]
    assert list(chunks(63, 63, 25)) == [(0, 25, 0, 1, 25), (25, 25, 0, 1, 25), (50, 13, 0, 1, 13)]
