"""The generic SkipConnMLP kernels across the descriptor space nrt_mlp_create accepts, not only at
the shapes the bench scenes use: every activation code Python can select, skip periods 1, 2, 3, 4
and >= num_layers, one and eighteen hidden layers, out 1 .. 96 (full and partial 32-row blocks),
in_size on both sides of the register / pointer input switch (4 | 5), no Fourier features, an
encoding width that is, and is one past, a multiple of 16, a latent with and without features, and
the TILE variant of k_mlp_backward32 at NB 1 and NB 2.

Every comparison is against the oracle's SkipMLP in float64 on the CPU.  The bar, per tensor:

    max|got - want64| <= max(1e-4 * max|want64|, 4 * e32)

with e32 the error of the same oracle run in float32: the parity bar of tests/test_gpu_train.py,
but relative to the tensor's own scale instead of max(1, scale), so that a gradient whose true
size is far below 1 cannot pass as all zeros.  tests/test_mlp_sweep_host.py checks, without a GPU,
that under this table no reference tensor is numerically dead, that the relative clause is the one
that governs, and that no relu / leaky pre-activation sits on its kink.

This module imports without a device (the host test reads its table and references)."""
import collections
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import pathtracer_ref as R
from tests.helpers import copy_mlp, seeded
from tests.report import report
from tests.test_gpu_train import _grads

Case = collections.namedtuple(
    "Case", "num_layers hidden in_size out skip freqs latent activation gain sigma seed")

# gain: every nn.Linear weight of the oracle is multiplied by it before the copy, so that no
# gradient tensor is numerically dead (at the default init an 18-layer leaky MLP has
# max|dW[0]| ~ 6e-8); sigma: the Fourier basis' scale (the classes' default 32 throughout: the
# float32 oracle's own error stays below 6e-6 of every tensor's scale even with the 224 features of
# the two freqs = 112 cases, so none needed a lower one); seed: of the weights and, with M, of the
# inputs, picked so that no relu / leaky pre-activation is within 1e-6 of zero.
# tests/test_mlp_sweep_host.py holds the table to all three.
CASES = {
    #                  L   H   in out skip   F lat activation    gain sigma seed
    # no skip layer at all (the only hidden layer is the last); ke 16
    "one_layer":   Case(1, 32, 3, 1, 3, 4, 0, "relu", 2.0, 32, 1),
    # null basis and the packer's stand-in zero row; dp = 2; out = 2
    "no_fourier":  Case(2, 32, 2, 2, 1, 0, 0, "sigmoid", 3.0, 32, 2),
    # every layer but the last skips; dp = 15; out = one full 32-row block
    "skip_every":  Case(5, 64, 3, 32, 1, 6, 0, "leaky_relu", 1.5, 32, 3),
    # pointer input path (in > 4); OB = 2 with one live row in the second block
    "out_33_in5":  Case(4, 96, 5, 33, 2, 8, 0, "relu", 1.5, 32, 4),
    # OB = 3, all rows live; dp = 17 (one past a multiple of 16)
    "out_96_in1":  Case(7, 128, 1, 96, 4, 8, 0, "softplus", 1.5, 32, 5),
    # skip >= L (layer 0 only); dp = 48, no padding slot; latent with a skip period other than 3
    "latent_full": Case(3, 64, 3, 64, 7, 16, 13, "sigmoid", 2.0, 32, 6),
    # kMaxLin; the refresh section table
    "deepest":     Case(18, 32, 3, 3, 3, 2, 0, "leaky_relu", 2.45, 32, 27),
    # in = 4, the last register-path width; OB = 3 partial at NB 8
    "wide_65_in4": Case(6, 256, 4, 65, 2, 10, 0, "softplus", 1.5, 32, 8),
    # latent without Fourier features; dp = 32
    "latent_only": Case(4, 32, 3, 5, 3, 0, 29, "leaky_relu", 1.5, 32, 9),
    # dp = 48; out = 1
    "sdf_in6":     Case(3, 128, 6, 1, 1, 21, 0, "relu", 1.5, 32, 10),
    # TILE backward at NB 1 (ke 240) and at NB 2
    "tile_nb1":    Case(3, 32, 3, 3, 1, 112, 0, "leaky_relu", 1.5, 32, 11),
    "tile_nb2":    Case(3, 64, 3, 3, 2, 112, 0, "sigmoid", 3.0, 32, 12),
}
# one row; one wave plus one row; one four-wave block plus 33 ragged rows
MS = (1, 33, 161)
KINKED = ("relu", "leaky_relu")
NO_LATENT = [n for n, c in CASES.items() if not c.latent]


# ---------------------------------------------------------------------------------------------
# the references (CPU, float64 and float32), computed once per (case, M) and never modified
# ---------------------------------------------------------------------------------------------
def oracle_mlp(name):
    """The oracle's SkipMLP of a case: seeded construction, then the weight gain."""
    c = CASES[name]
    seeded(c.seed)
    ref = R.SkipMLP(num_layers=c.num_layers, hidden_size=c.hidden, in_size=c.in_size, out=c.out,
                    skip=c.skip, freqs=c.freqs, sigma=c.sigma, activation=c.activation,
                    latent_size=c.latent)
    with torch.no_grad():
        for lin in [ref.init, *ref.layers, ref.out]:
            lin.weight.mul_(c.gain)
    return ref


def inputs(name, M):
    """x = rand - 0.5, then latent, dy and v (the double backward's cotangent) = randn."""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 * c.seed + M)
    x = torch.rand(M, c.in_size, generator=g) - 0.5
    lat = torch.randn(M, c.latent, generator=g) if c.latent else None
    dy = torch.randn(M, c.out, generator=g)
    v = torch.randn(M, c.in_size, generator=g)
    return x, lat, dy, v


def _as(ref, dtype):
    m = copy.deepcopy(ref).to(dtype)
    m.basis_p = ref.basis_p.to(dtype)
    return m


def _forward(ref, x, lat, dtype):
    with torch.no_grad():
        return _as(ref, dtype)(x.to(dtype), None if lat is None else lat.to(dtype))


def _double_backward(ref, x, lat, v, dtype):
    """g = d(sum_o y_o)/dx and the parameter gradients of <v, g>, the latent a constant (the
    pattern of tests/test_gpu_train_render.py; a parameter <v, g> does not depend on gets zeros)."""
    m = _as(ref, dtype)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    y = m(xr, None if lat is None else lat.to(dtype))
    (g,) = torch.autograd.grad(y, xr, torch.ones_like(y), create_graph=True)
    (g * v.to(dtype)).sum().backward()
    out = {"g": g.detach()}
    for i, lin in enumerate([m.init, *m.layers, m.out]):
        for k, q in ((f"dW[{i}]", lin.weight), (f"db[{i}]", lin.bias)):
            out[k] = q.grad if q.grad is not None else torch.zeros_like(q)
    return out


def references_of(ref, x, lat, dy, v):
    """{"y" | "grads" | "double": (float64, float32)} of one oracle MLP on one input."""
    out = {}
    for key, fn in (("y", lambda dt: {"y": _forward(ref, x, lat, dt)}),
                    ("grads", lambda dt: _grads(ref, x, lat, dy, dt)),
                    ("double", lambda dt: _double_backward(ref, x, lat, v, dt))):
        out[key] = (fn(torch.float64), fn(torch.float32))
    return out


@functools.lru_cache(maxsize=None)
def reference(name, M):
    """(oracle MLP, (x, lat, dy, v), references_of(...)) of a case at M rows: shared by every
    test of this file and of tests/test_mlp_sweep_host.py; none of them writes to it."""
    ref = oracle_mlp(name)
    inp = inputs(name, M)
    return ref, inp, references_of(ref, *inp)


def preactivations(ref, x, lat=None):
    """The float64 inputs of every activation call of SkipMLP.forward (the hidden units and, on a
    skip layer, the encoding concatenated to them), one tensor per call."""
    m = _as(ref, torch.float64)
    zs = []
    with torch.no_grad():
        enc = R.fourier_encode(x.double().reshape(-1, m.in_size), m.basis_p)
        if lat is not None:
            enc = torch.cat([enc, lat.double().reshape(-1, m.latent_size)], dim=-1)
        h = m.init(enc)
        act = R.ACTIVATIONS[m.act_name]
        for i, lin in enumerate(m.layers):
            if m.is_skip(i):
                h = torch.cat([h, enc], dim=-1)
            zs.append(h)
            h = lin(act(h))
        zs.append(h)
    return zs


def nearest_kink(ref, x, lat=None):
    return min(float(z.abs().min()) for z in preactivations(ref, x, lat))


def off_the_kinks(ref, x, lat, margin=1e-5):
    """(x, lat) with every row that has a float64 pre-activation within `margin` of zero replaced
    by a copy of the first row that has none (M stays what it was).  For weights the table's seed
    could not be picked for -- those an optimiser step on the GPU has produced: the host test's
    condition (1e-6) then holds with room for another implementation's rounding."""
    near = torch.stack([z.abs().min(-1).values for z in preactivations(ref, x, lat)]).min(0).values
    bad = near < margin
    assert int(bad.sum()) <= max(1, x.shape[0] // 20), f"{int(bad.sum())} of {x.shape[0]} rows on a kink"
    if bad.any():
        good = int((~bad).nonzero()[0])
        x = x.clone()
        x[bad] = x[good].clone()
        if lat is not None:
            lat = lat.clone()
            lat[bad] = lat[good].clone()
    assert nearest_kink(ref, x, lat) >= 1e-6
    return x, lat


def bar(want64, ref32):
    """(tolerance, the float32 oracle's own error) of one compared tensor."""
    e32 = (ref32.detach().double() - want64).abs().max().item()
    return max(1e-4 * want64.abs().max().item(), 4 * e32), e32


def _close(got, want64, ref32, what, worst):
    """The bar; prints each figure before it asserts; worst[0] keeps the largest err / bar."""
    tol, e32 = bar(want64, ref32)
    err = (got.detach().cpu().double() - want64).abs().max().item()
    frac = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
    worst[0] = max(worst[0], frac)
    print(f"{what}: max|diff| {err:.3g}  bar {tol:.3g}  scale {want64.abs().max().item():.3g}  "
          f"fp32 ref {e32:.3g}")
    assert err <= tol, (f"{what}: max|diff| {err:.3g} > {tol:.3g} "
                        f"(scale {want64.abs().max().item():.3g}, fp32 ref {e32:.3g})")


def _close_all(got, want, what, worst):
    assert set(got) == set(want[0]), (sorted(got), sorted(want[0]))
    for k in want[0]:
        _close(got[k], want[0][k], want[1][k], f"{what} {k}", worst)


# ---------------------------------------------------------------------------------------------
# the product side
# ---------------------------------------------------------------------------------------------
def product_mlp(name, ref):
    from neural_raytracing_amd.pathtracer.neural_blocks import SkipConnMLP
    c = CASES[name]
    act = {"relu": torch.relu, "softplus": F.softplus, "sigmoid": torch.sigmoid}
    kw = {} if c.activation == "leaky_relu" else {"activation": act[c.activation]}
    mine = SkipConnMLP(num_layers=c.num_layers, hidden_size=c.hidden, in_size=c.in_size,
                       out=c.out, skip=c.skip, freqs=c.freqs, sigma=c.sigma,
                       latent_size=c.latent, device="cpu", **kw)
    return copy_mlp(mine, ref).cuda()


def _dev(t):
    return None if t is None else t.cuda()


def _first_order(mine, x, lat, dy):
    """dx, dlatent and every dW / db of sum(mlp(x, latent) * dy) through autograd (clones)."""
    mine.zero_grad(set_to_none=True)
    xm = x.cuda().requires_grad_(True)
    lm = None if lat is None else lat.cuda().requires_grad_(True)
    (mine(xm, lm) * dy.cuda()).sum().backward()
    got = {"dx": xm.grad.clone()}
    if lm is not None:
        got["dlatent"] = lm.grad.clone()
    for i, a in enumerate(mine._linears()):
        got[f"dW[{i}]"] = a.weight.grad.clone()
        got[f"db[{i}]"] = a.bias.grad.clone()
    return got


def _second_order(mine, x, v):
    """g = input_gradient(mlp, x) and every dW / db of <v, g> (clones)."""
    from neural_raytracing_amd.pathtracer.neural_blocks import input_gradient
    mine.zero_grad(set_to_none=True)
    g = input_gradient(mine, x.cuda())
    (g * v.cuda()).sum().backward()
    got = {"g": g.detach().clone()}
    for i, a in enumerate(mine._linears()):
        got[f"dW[{i}]"] = a.weight.grad.clone()
        got[f"db[{i}]"] = a.bias.grad.clone()
    return got


def _bit_equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        # (through an int32 view: -0.0 and +0.0 differ, NaN equals itself)
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), \
            f"{what} {k}: max|diff| {(a[k] - b[k]).abs().max().item():.3g}"


@pytest.fixture(autouse=True)
def _fp32(request):
    if "gpu" not in request.keywords:
        yield
        return
    from neural_raytracing_amd import set_precision
    set_precision("fp32")
    yield
    set_precision("fp32")


# ---------------------------------------------------------------------------------------------
# the table itself (no GPU work)
# ---------------------------------------------------------------------------------------------
def test_table_holds_a_tile_case_at_nb1_and_nb2_and_no_other():
    """backward_plan / backward_plan_cs (csrc/nrt_api_train.hip) restated: the TILE variant of
    k_mlp_backward32 is selected iff the tiled plan at least doubles the slabs per CU.  Whoever
    changes that rule has to re-pick tile_nb1 and tile_nb2, or the `NB < 4` TILE branch drops out
    of coverage without a test failing.  (The per-wave plan adds one float a row for the output
    staging; both forms are asserted.)"""
    for extra in (0, 1):  # backward_plan_cs | backward_plan
        tile = {}
        for name, c in CASES.items():
            ke = (c.in_size + 2 * c.freqs + c.latent + 15) // 16 * 16
            per_cu = lambda RS: min(8, 160 * 1024 // (32 * (RS + extra) * 4))  # noqa: E731
            tile[name] = per_cu(c.hidden | 1) >= 2 * per_cu((c.hidden + ke) | 1)
        assert {n for n, t in tile.items() if t} == {"tile_nb1", "tile_nb2"}, tile
    assert CASES["tile_nb1"].hidden // 32 == 1 and CASES["tile_nb2"].hidden // 32 == 2


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_fp32(name, M):
    """nrt_mlp_forward (k_mlp_forward<false, NB>) through SkipConnMLP.__call__ under no_grad."""
    ref, (x, lat, _, _), want = reference(name, M)
    mine = product_mlp(name, ref)
    with torch.no_grad():
        got = mine(x.cuda(), _dev(lat))
    worst = [0.0]
    try:
        _close_all({"y": got}, want["y"], f"{name} M={M}", worst)
    finally:
        report("sweep_forward_fp32", case=name, M=M, worst_err_over_bar=worst[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_forward_fp16(name):
    """k_mlp_forward<true, NB> at the bar of test_mlp_forward_fp16_close (tests/test_gpu_parity.py):
    2e-2 * max(1, max|want|)."""
    from neural_raytracing_amd import set_precision
    ref, (x, lat, _, _), want = reference(name, 161)
    mine = product_mlp(name, ref)
    want64 = want["y"][0]["y"]
    set_precision("fp16")
    with torch.no_grad():
        got = mine(x.cuda(), _dev(lat)).cpu().double()
    err = (got - want64).abs().max().item()
    tol = 2e-2 * max(1.0, want64.abs().max().item())
    report("sweep_forward_fp16", case=name, err=err, bar=tol, scale=want64.abs().max().item())
    assert err <= tol, (err, tol)


# ---------------------------------------------------------------------------------------------
# first-order backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("name", list(CASES))
def test_backward(name, M):
    """nrt_mlp_backward through autograd: dx, dlatent and every dW / db against float64 autograd
    of the oracle, with the default weight-gradient kernel and with k_wgrad_tile."""
    from neural_raytracing_amd import _lib
    ref, (x, lat, dy, _), want = reference(name, M)
    mine = product_mlp(name, ref)
    worst = [0.0]
    try:
        for tile in (0, 1):
            with _lib.options(wgrad_tile=tile):
                got = _first_order(mine, x, lat, dy)
            _close_all(got, want["grads"], f"{name} M={M} wgrad_tile={tile}", worst)
    finally:
        report("sweep_backward", case=name, M=M, worst_err_over_bar=worst[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_backward_column_split_bit_equal(name):
    """k_mlp_backward32's column-split variants (option bwd_colsplit 1: TILE where the rule
    selects it, 2: the slab) against the per-wave kernel (0): every gradient bit-equal."""
    from neural_raytracing_amd import _lib
    ref, (x, lat, dy, _), _ = reference(name, 161)
    mine = product_mlp(name, ref)

    def run(opt):
        with _lib.options(bwd_colsplit=opt):
            return _first_order(mine, x, lat, dy)
    base = run(0)
    for mode in (1, 2):
        _bit_equal(base, run(mode), f"{name} bwd_colsplit 0 vs {mode}")


# ---------------------------------------------------------------------------------------------
# double backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("name", NO_LATENT)
def test_double_backward(name, M):
    """input_gradient and the parameter gradients of <v, g> (nrt_mlp_grad_backward) against the
    float64 double backward, under both bwd_colsplit settings, bit-equal to each other.

    tile_nb1 and tile_nb2 are compared, not refused: nrt_mlp_grad_backward's slab row is
    RS = (2 max(H, 32) + 2 max(ke, 16)) | 1 floats and it refuses only when one wave's 32 rows
    exceed 160 KiB; at ke 240 that is 32 * 545 * 4 = 69760 bytes (H 32) and 32 * 609 * 4 = 77952
    bytes (H 64), two waves a block."""
    from neural_raytracing_amd import _lib
    ref, (x, _, _, v), want = reference(name, M)
    mine = product_mlp(name, ref)
    worst = [0.0]
    got = {}
    try:
        for cs in (1, 0):
            with _lib.options(bwd_colsplit=cs):
                got[cs] = _second_order(mine, x, v)
            _close_all(got[cs], want["double"], f"{name} M={M} bwd_colsplit={cs}", worst)
    finally:
        report("sweep_double_backward", case=name, M=M, worst_err_over_bar=worst[0])
    _bit_equal(got[0], got[1], f"{name} M={M} bwd_colsplit 0 vs 1")


@pytest.mark.gpu
def test_grad_backward_with_latent():
    """nrt_mlp_grad_backward documents "latent is held constant" and the Python wrapper refuses a
    latent, so it is called through ctypes here, on a training handle of latent_full at M = 33:
    the parameter gradients of <v, d(sum y)/dx> against the float64 double backward with the
    latent a constant, inside a workspace of exactly the size function's bytes (guard bands)."""
    from tests.test_gpu_backward_entries import _grad_backward, _grad_bufs, _lib as entries_lib
    name, M = "latent_full", 33
    L = entries_lib()
    ref, (x, lat, _, v), want = reference(name, M)
    mine = product_mlp(name, ref)
    want = tuple({k: t for k, t in w.items() if k != "g"} for w in want["double"])
    worst = [0.0]
    got = {}
    try:
        for cs in (1, 0):
            dws, dbs = _grad_bufs(mine)
            with L.options(bwd_colsplit=cs):
                _grad_backward(L, mine, x.cuda(), v.cuda(), dws, dbs, lat=lat.cuda())
            got[cs] = {**{f"dW[{i}]": t for i, t in enumerate(dws)},
                       **{f"db[{i}]": t for i, t in enumerate(dbs)}}
            _close_all(got[cs], want, f"{name} M={M} bwd_colsplit={cs}", worst)
    finally:
        report("sweep_grad_backward_latent", case=name, M=M, worst_err_over_bar=worst[0])
    _bit_equal(got[0], got[1], f"{name} bwd_colsplit 0 vs 1")


# ---------------------------------------------------------------------------------------------
# nrt_mlp_refresh
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_refresh_equals_fresh_pack(name):
    """nrt_mlp_refresh, the device-side second implementation of every fragment layout of
    nrt_pack.hip: after two SGD steps through the autograd path at each precision (training handle
    created, then refreshed in place) mlp(x) through the training handle equals mlp(x) under no_grad (a fresh
    host pack of the same weights) bit for bit, at fp32 and at fp16; the first-order and the
    double-backward gradients through the refreshed handle (its w32, wt32 and bias fragments)
    meet the float64 bar of the weights as they are after the steps (for relu / leaky on rows
    that these weights keep off the kinks: off_the_kinks)."""
    from neural_raytracing_amd import set_precision
    c = CASES[name]
    M = 161
    ref0, (x, lat, dy, v), _ = reference(name, M)
    mine = product_mlp(name, ref0)
    xc, lc = x.cuda(), _dev(lat)
    opt = torch.optim.SGD(mine.parameters(), lr=1.0)
    handle = None
    for prec in ("fp32", "fp16"):
        set_precision(prec)
        for _ in range(2):
            opt.zero_grad()
            y = mine(xc, lc)  # training handle: created on the first call, refreshed after
            y.square().mean().backward()
            # a step that moves the largest weight entry by 0.02, whatever the case's scale
            opt.param_groups[0]["lr"] = 0.02 / max(float(q.grad.abs().max())
                                                   for q in mine.parameters())
            opt.step()
            handle = handle or mine._nrt_train[2]
        y_train = mine(xc, lc).detach()  # refreshed after the last step
        with torch.no_grad():
            y_fresh = mine(xc, lc)  # mlp_handle: packed on the host from the same weights
        assert mine._nrt_train[2] is handle and handle.value != mine.nrt()
        assert torch.equal(y_train.view(torch.int32), y_fresh.view(torch.int32)), \
            f"{name} {prec}: max|diff| {(y_train - y_fresh).abs().max().item():.3g}"
    set_precision("fp32")
    # the oracle with the weights as they are now
    ref = copy.deepcopy(ref0)
    with torch.no_grad():
        for a, b in zip([ref.init, *ref.layers, ref.out], mine._linears()):
            a.weight.copy_(b.weight.cpu())
            a.bias.copy_(b.bias.cpu())
        moved = max(float((a.weight - b.weight).abs().max())
                    for a, b in zip([ref.init, *ref.layers, ref.out],
                                    [ref0.init, *ref0.layers, ref0.out]))
    assert moved >= 0.01, "the SGD steps left the weights where they were"
    if c.activation in KINKED:
        x, lat = off_the_kinks(ref, x, lat)
    want = references_of(ref, x, lat, dy, v)
    worst = [0.0]
    try:
        got = _first_order(mine, x, lat, dy)
        assert mine._nrt_train[2] is handle
        _close_all(got, want["grads"], f"{name} refreshed", worst)
        if not c.latent:
            _close_all(_second_order(mine, x, v), want["double"], f"{name} refreshed double", worst)
    finally:
        report("sweep_refresh", case=name, M=M, worst_err_over_bar=worst[0], weights_moved=moved)
