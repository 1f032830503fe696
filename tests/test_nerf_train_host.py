"""CPU checks of the volume-rendering training path's boundary: the new C entries are bound with
the declared argument counts, PlainNeRF still refuses CPU rays, NeRFLE's fused path is opt-in."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nrt.h")

NEW_ENTRIES = {"nrt_nerf_volume_workspace_bytes", "nrt_nerf_points", "nrt_nerf_assemble",
               "nrt_nerf_assemble_backward", "nrt_nerf_composite_forward",
               "nrt_nerf_composite_backward", "nrt_nerf_reduce"}


def _declared_nerf_entries():
    """{name: argument count} of every nrt_nerf_* prototype in include/nrt.h."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(nrt_nerf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else len(args.split(","))
    return out


def test_every_nerf_entry_has_a_signature_of_the_declared_length():
    from neural_raytracing_amd import _lib
    declared = _declared_nerf_entries()
    assert NEW_ENTRIES <= set(declared), NEW_ENTRIES - set(declared)
    for name, nargs in declared.items():
        assert name in _lib._SIGNATURES, name
        assert len(_lib._SIGNATURES[name][1]) == nargs, (name, nargs)


def test_plain_nerf_refuses_cpu_rays():
    from neural_raytracing_amd import NrtError
    from neural_raytracing_amd.pathtracer.shapes import PlainNeRF
    nerf = PlainNeRF(steps=4, device="cpu")
    nerf.assign_latent(torch.zeros(1, 32, requires_grad=True))
    with pytest.raises(NrtError, match="HIP path only"):
        nerf(torch.zeros(1, 2, 2, 1, 6), None)


def test_nerfle_fused_training_is_opt_in():
    from neural_raytracing_amd.pathtracer.shapes import NeRFLE
    assert NeRFLE.FUSED_TRAINING is False


def test_chunks_cover_every_ray_once():
    """Whole cameras while one fits in the bound, else pieces of one camera with a ragged tail;
    every chunk stays inside the latent rows it names."""
    from neural_raytracing_amd.pathtracer.shapes._volume import chunks
    for P, per, cmax in [(30, 15, 7), (30, 15, 15), (30, 15, 31), (30, 15, 1000), (63, 63, 10)]:
        seen = []
        for r0, n, row0, rows, rpl in chunks(P, per, cmax):
            assert 0 < n <= cmax and rows * rpl == n
            assert row0 == r0 // per and (r0 + n - 1) // per == row0 + rows - 1
            seen.extend(range(r0, r0 + n))
        assert seen == list(range(P)), (P, per, cmax)
