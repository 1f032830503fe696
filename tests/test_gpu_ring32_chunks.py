"""The FP32 ring's chunk schedule and encoding k-steps (nrt_device.h ring32::eval) leave every bit
of the march where it was: SDF.intersect(primary=True) -- k_march32 with its coarse scan,
k_scan_best32 and the forward-mode normals of k_normal_r -- against arrays recorded on an MI355X at
the commit before the encoding's padding k-steps were skipped, stored as uint32 bit patterns in
tests/golden/ring32_chunks/<case>.npz (t, hit, p, n, throughput of 24 x 24 rays, max_steps 64).

The shapes are SphereSDF blobs with a SkipConnMLP shift (seeded on the CPU, so every machine builds
the same weights): the headline's 8x256 F=16, the training / colocate 8x128 F=32, a 3x256 F=32
leaky_relu MLP whose every eligible layer is a skip layer (ke = 80), a 2x128 MLP (two row blocks,
one skip layer) and a 4x256 MLP whose skip period is past its depth.

`python tests/test_gpu_ring32_chunks.py --record` rewrites the arrays from the library in the tree.
"""
import os
import random
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ring32_chunks")
SIDE, STEPS = 24, 64
FIELDS = ("t", "hit", "p", "n", "throughput")

# name: (hidden, freqs, layers, skip, activation, spheres)
CASES = {
    "h256_f16_l8_s3_softplus": (256, 16, 8, 3, "softplus", 128),
    "h128_f32_l8_s3_softplus": (128, 32, 8, 3, "softplus", 64),
    "h256_f32_l3_s1_leaky": (256, 32, 3, 1, "leaky_relu", 32),
    "h128_f16_l2_s3_softplus": (128, 16, 2, 3, "softplus", 32),
    "h256_f16_l4_s5_leaky": (256, 16, 4, 5, "leaky_relu", 16),
}


def _sdf(hidden, freqs, layers, skip, act, spheres, seed=5):
    """SphereSDF(n = spheres) with a visible SkipConnMLP shift, built on the CPU from `seed`."""
    from neural_raytracing_amd.pathtracer.neural_blocks import SkipConnMLP
    from neural_raytracing_amd.pathtracer.shapes import SphereSDF
    torch.manual_seed(seed)
    random.seed(seed)
    sdf = SphereSDF(n=spheres, device="cpu")
    kw = {"activation": F.softplus} if act == "softplus" else {}
    sdf.shift = SkipConnMLP(num_layers=layers, hidden_size=hidden, in_size=3, out=1, skip=skip,
                            freqs=freqs, device="cpu", **kw)
    with torch.no_grad():
        sdf.radii.add_(0.12)
        sdf.tfs.copy_(0.05 * torch.randn_like(sdf.tfs))
        sdf.shift.out.weight.mul_(0.05)
        sdf.shift.out.bias.mul_(0.05)
    return sdf.cuda()


def _rays(n=SIDE, seed=11, eye=(0.0, 0.2, 1.1), spread=0.9):
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor(eye).expand(1, n, n, 1, 3)
    d = F.normalize(torch.cat([torch.rand(1, n, n, 1, 2, generator=g) * spread - spread / 2,
                               -torch.ones(1, n, n, 1, 1)], -1), dim=-1)
    return torch.cat([o, d], -1)


def _march(sdf):
    """{field: uint32 bits on the host} of SDF.intersect(primary=True); asserts k_march32 ran."""
    from neural_raytracing_amd import _lib
    from neural_raytracing_amd.pathtracer.shapes import SDF
    _lib.profile_enable(True)
    _lib.profile_reset()
    random.seed(12)
    with torch.no_grad():
        it, hit = SDF(sdf=sdf, max_steps=STEPS).intersect(_rays().cuda(), primary=True)
    torch.cuda.synchronize()
    n32 = _lib.profile_read("k_march32")[1]
    _lib.profile_enable(False)
    assert n32 >= 1, "the FP32 ring kernel did not run"
    out = {"t": it.t, "hit": hit, "p": it.p, "n": it.n, "throughput": it.throughput}
    return {k: _bits(v) for k, v in out.items()}


def _bits(v):
    v = v.detach().cpu().contiguous()
    if v.dtype == torch.float32:
        return v.numpy().view(np.uint32).reshape(-1)
    return v.to(torch.uint8).numpy().astype(np.uint32).reshape(-1)


@pytest.fixture(autouse=True)
def _fp32():
    from neural_raytracing_amd import set_precision
    set_precision("fp32")
    yield
    set_precision("fp32")


def _assert_same(got, want, what):
    for k in FIELDS:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        diff = got[k] != want[k]
        assert not diff.any(), (f"{what}: {k} differs in {int(diff.sum())} of {diff.size} words, "
                                f"first at {int(np.flatnonzero(diff)[0])}")


@pytest.mark.parametrize("case", list(CASES))
def test_ring32_march_bits_match_recorded(case):
    want = dict(np.load(os.path.join(GOLDEN, case + ".npz")))
    hits = want["hit"].mean()
    assert 0.05 < hits < 0.95, f"the recorded frame is degenerate (hit fraction {hits})"
    _assert_same(_march(_sdf(*CASES[case])), want, case)


def test_ring32_march_bits_independent_of_grid_and_queue():
    """march_blocks 1 / default x march_queue 0 / 1: the same bits (one shape, the 128-wide ring
    with ke = 80, where the padding k-steps and the chunk sizes differ most from the headline)."""
    from neural_raytracing_amd import _lib
    case = "h128_f32_l8_s3_softplus"
    sdf = _sdf(*CASES[case])
    base = _march(sdf)
    for blocks, queue in ((1, 0), (1, 1), (0, 1)):
        _lib.set_option("march_blocks", blocks)
        _lib.set_option("march_queue", queue)
        got = _march(sdf)
        for k in FIELDS:
            assert torch.equal(torch.from_numpy(got[k].astype(np.int64)),
                               torch.from_numpy(base[k].astype(np.int64))), (blocks, queue, k)


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from neural_raytracing_amd import set_precision
    set_precision("fp32")
    out_dir = sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > 2 else GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    for name, cfg in CASES.items():
        arrays = _march(_sdf(*cfg))
        np.savez_compressed(os.path.join(out_dir, name + ".npz"), **arrays)
        print(name, "hit fraction", float(arrays["hit"].mean()),
              {k: v.shape for k, v in arrays.items()}, flush=True)
