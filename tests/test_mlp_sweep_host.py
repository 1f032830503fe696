"""The descriptor sweep's references (tests/test_gpu_mlp_descriptor_sweep.py), checked on the CPU
with the oracle alone: its bar  max(1e-4 * max|want64|, 4 * e32)  means something only if no
reference tensor is numerically dead, and stays as tight as it reads only while the float32
oracle's own error e32 keeps the second clause below the first; a relu / leaky comparison is
well-posed only away from the kinks, where float32 and float64 agree on every unit's side."""
import pytest

from tests.test_gpu_mlp_descriptor_sweep import CASES, KINKED, MS, bar, nearest_kink, reference


def _tensors(name, M):
    """(label, float64 reference, float32 reference) of everything the GPU tests compare."""
    _, _, refs = reference(name, M)
    for key in ("y", "grads", "double"):
        w64, w32 = refs[key]
        for k in w64:
            yield f"{key} {k}", w64[k], w32[k]


def _structural_zeros(c):
    """The double backward's exact zeros: <v, d(sum y)/dx> does not depend on the out layer's
    bias, nor, where the activation is piecewise linear, on any bias at all."""
    n_lin = c.num_layers + 2
    which = range(n_lin) if c.activation in KINKED else [n_lin - 1]
    return {f"double db[{i}]" for i in which}


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("name", list(CASES))
def test_no_reference_tensor_is_dead(name, M):
    """max|.| >= 1e-3 for y, dx, dlatent, every dW and db and their double-backward counterparts
    (the weight gains of the table are there for this), and max|y| <= 1e3.  The only exceptions
    are the double backward's structural zeros, exact in float64 and float32 alike, which the bar
    then holds the kernels to exactly."""
    c = CASES[name]
    zeros = set()
    for label, w64, w32 in _tensors(name, M):
        top = w64.abs().max().item()
        if top == 0.0:
            assert w32.abs().max().item() == 0.0, label
            zeros.add(label)
            continue
        assert top >= 1e-3, f"{name} M={M} {label}: max|want64| {top:.3g}"
    assert zeros == _structural_zeros(c), (sorted(zeros), sorted(_structural_zeros(c)))
    y = reference(name, M)[2]["y"][0]["y"]
    assert y.abs().max().item() <= 1e3


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("name", list(CASES))
def test_the_relative_clause_governs(name, M):
    """4 * e32 <= 1e-4 * max|want64| for every compared tensor: the bar is 1e-4 of the tensor's
    own scale, not something the reference's float32 noise has inflated."""
    for label, w64, w32 in _tensors(name, M):
        tol, e32 = bar(w64, w32)
        scale = w64.abs().max().item()
        assert 4 * e32 <= 1e-4 * scale, \
            f"{name} M={M} {label}: e32 {e32:.3g} = {e32 / max(scale, 1e-300):.3g} of scale {scale:.3g}"
        assert tol == 1e-4 * scale


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.activation in KINKED])
def test_relu_and_leaky_cases_stay_away_from_the_kinks(name, M):
    """No float64 pre-activation within 1e-6 of zero (the per-case seeds of the table are picked
    for this): below that a float32 implementation may land on the other side."""
    ref, (x, lat, _, _), _ = reference(name, M)
    assert nearest_kink(ref, x, lat) >= 1e-6
