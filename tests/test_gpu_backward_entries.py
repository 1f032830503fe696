"""The four C entries of the SkipConnMLP backward (nrt_mlp_backward, nrt_mlp_backward_multi,
nrt_mlp_backward_saved, nrt_mlp_grad_backward) called through ctypes on training handles.  They
share one host path (csrc/nrt_api_train.hip backward_core): the single entry is the multi entry
with one MLP, the saved entry the multi entry without its forward part, so their results are
compared bit for bit.  Every workspace is exactly the size function's bytes between two guard
bands, which must come back intact."""
import ctypes
import math

import pytest
import torch

from tests.test_gpu_train import SHAPES, _pair

P = ctypes.c_void_p
GUARD = 4096
SLAB, RING = "8x64_leaky", "neural_bsdf_6x96_F64"
# (bwd_ring, bwd_colsplit): the ring backward where the shape has one, the column-split slab
# kernels, the per-wave slab kernels
PATHS = [(1, 1), (0, 1), (0, 0)]


def _lib():
    from neural_raytracing_amd import _lib as L, set_precision
    set_precision("fp32")
    return L


def _handle(mlp):
    from neural_raytracing_amd.pathtracer._handles import train_handle
    return train_handle(mlp)


def _ptrs(ts):
    return (P * len(ts))(*[0 if t is None else t.data_ptr() for t in ts])


class _Guarded:
    """nbytes of device memory between two GUARD-byte bands of 0xA5."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.ws = self.buf[GUARD:GUARD + self.n]

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == 0xA5).all()), f"{what}: wrote below its workspace"
        assert bool((self.buf[GUARD + self.n:] == 0xA5).all()), f"{what}: wrote past its workspace"


def _grad_bufs(mlp, frozen=False):
    """NaN-filled gradients; frozen: no odd layer's weight and no bias takes one."""
    lins = mlp._linears()
    nan = float("nan")
    dws = [None if frozen and i % 2 else torch.full_like(l.weight, nan) for i, l in enumerate(lins)]
    dbs = [None if frozen else torch.full_like(l.bias, nan) for l in lins]
    return dws, dbs


def _inputs(mlp, M, seed, out):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(M, mlp.in_size, generator=g) - 0.5).cuda()
    dy = torch.randn(M, out, generator=g).cuda()
    return x, dy


def _single(L, mlp, x, dy, lat=None, frozen=False):
    h, M = _handle(mlp), x.shape[0]
    g = _Guarded(L.load(True).nrt_mlp_backward_workspace_bytes(h.value, M))
    dx = torch.full_like(x, float("nan"))
    dlat = None if lat is None else torch.full_like(lat, float("nan"))
    dws, dbs = _grad_bufs(mlp, frozen)
    L.call("nrt_mlp_backward", h.value, L.ptr(x), L.ptr(lat), M, L.ptr(dy), L.ptr(dx), L.ptr(dlat),
           _ptrs(dws), _ptrs(dbs), L.ptr(g.ws), L.stream())
    g.check("nrt_mlp_backward")
    return [dx, dlat] + dws + dbs


def _multi(L, mlps, x, dys, frozen=False, saved=None, rows=None, Ms=None):
    """nrt_mlp_backward_multi, or nrt_mlp_backward_saved on the save buffers `saved`."""
    n, M = len(mlps), x.shape[0]
    hs = (P * n)(*[_handle(m).value for m in mlps])
    g = _Guarded(L.load(True).nrt_mlp_backward_multi_workspace_bytes(hs, n, M))
    dxs = [torch.full_like(x, float("nan")) for _ in mlps]
    bufs = [_grad_bufs(m, frozen) for m in mlps]
    wp = _ptrs([t for dws, _ in bufs for t in dws])
    bp = _ptrs([t for _, dbs in bufs for t in dbs])
    if saved is None:
        L.call("nrt_mlp_backward_multi", hs, n, L.ptr(x), M, _ptrs(dys), _ptrs(dxs), wp, bp,
               L.ptr(g.ws), L.stream())
    else:
        L.call("nrt_mlp_backward_saved", hs, n, L.ptr(x), M, L.ptr(rows), _ptrs(saved), Ms,
               _ptrs(dys), _ptrs(dxs), wp, bp, L.ptr(g.ws), L.stream())
    g.check("nrt_mlp_backward_saved" if saved is not None else "nrt_mlp_backward_multi")
    return [[dx, None] + dws + dbs for dx, (dws, dbs) in zip(dxs, bufs)]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None) == (v is None), f"{what}[{i}]"
        if u is None:
            continue
        assert not bool(torch.isnan(u).any()), f"{what}[{i}]: left unwritten"
        # (through an int32 view: -0.0 and +0.0 differ)
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), \
            f"{what}[{i}]: max|diff| {(u - v).abs().max().item():.3g}"


def _single_equals_multi(name, M, ring, colsplit, frozen):
    L = _lib()
    kw = SHAPES[name]
    _, mlp = _pair(kw, 7)
    x, dy = _inputs(mlp, M, 100 + M, kw["out"])
    with L.options(bwd_ring=ring, bwd_colsplit=colsplit):
        a = _single(L, mlp, x, dy, frozen=frozen)
        b = _multi(L, [mlp], x, [dy], frozen=frozen)[0]
    _assert_same(a, b, f"{name} M={M}")


@pytest.mark.gpu
@pytest.mark.parametrize("ring,colsplit", PATHS)
@pytest.mark.parametrize("M", [1, 33, 3001])  # one row; a ragged second wave; many blocks, > 1 slice
@pytest.mark.parametrize("name", [SLAB, RING])
def test_single_entry_equals_multi_entry_of_one(name, M, ring, colsplit):
    """nrt_mlp_backward(m) and nrt_mlp_backward_multi(&m, 1): dx, every dW and every db bit-equal,
    on the ring backward, the column-split slab kernels and the per-wave slab kernels."""
    _single_equals_multi(name, M, ring, colsplit, frozen=False)


@pytest.mark.gpu
@pytest.mark.parametrize("ring,colsplit", PATHS)
@pytest.mark.parametrize("name", [SLAB, RING])
def test_single_entry_equals_multi_entry_of_one_frozen(name, ring, colsplit):
    """As above with the odd layers' weight pointers and all bias pointers null (a batch with
    fewer jobs than the one the workspace's slice count was planned with)."""
    _single_equals_multi(name, 3001, ring, colsplit, frozen=True)


@pytest.mark.gpu
@pytest.mark.parametrize("live", [1.0, 0.4])
def test_saved_entry_equals_recompute(live):
    """nrt_mlp_backward_saved on the save buffers of nrt_mlp_forward_multi against the recomputing
    nrt_mlp_backward_multi on the same rows: with rows == NULL, and through a 40 % live row index."""
    L = _lib()
    lib = L.load(True)
    kw = SHAPES[RING]
    _, mlp = _pair(kw, 8)
    M = 3001
    x, dy = _inputs(mlp, M, 11, kw["out"])
    h = _handle(mlp)
    nbytes = lib.nrt_mlp_save_bytes(h.value, M)
    assert nbytes > 0
    save = _Guarded(nbytes)
    y = torch.empty(M, kw["out"], device="cuda")
    L.call("nrt_mlp_forward_multi", (P * 1)(h.value), 1, L.ptr(x), M, _ptrs([y]), _ptrs([save.ws]),
           L.precision_code(), L.stream())
    save.check("nrt_mlp_forward_multi")
    rows = None
    xc, dyc = x, dy
    if live < 1.0:
        g = torch.Generator().manual_seed(12)
        idx = torch.nonzero(torch.rand(M, generator=g) < live).reshape(-1).cuda()
        assert 0 < idx.numel() < M
        rows = idx.to(torch.int32)
        xc, dyc = x[idx].contiguous(), dy[idx].contiguous()
    a = _multi(L, [mlp], xc, [dyc], saved=[save.ws], rows=rows, Ms=M)[0]
    b = _multi(L, [mlp], xc, [dyc])[0]
    _assert_same(a, b, f"saved, live {live}")


@pytest.mark.gpu
@pytest.mark.parametrize("ring", [1, 0])
def test_three_mlps_stay_inside_the_workspace(ring):
    """n == 3 at a ragged M: the guard bands (checked in _multi) and each MLP's gradients equal to
    its own single call."""
    L = _lib()
    kw = SHAPES[RING]
    mlps = [_pair(kw, s)[1] for s in (1, 2, 3)]
    M = 33
    x, _ = _inputs(mlps[0], M, 21, kw["out"])
    g = torch.Generator().manual_seed(22)
    dys = [torch.randn(M, kw["out"], generator=g).cuda() for _ in mlps]
    with L.options(bwd_ring=ring):
        got = _multi(L, mlps, x, dys)
        for k, (m, dy) in enumerate(zip(mlps, dys)):
            _assert_same(got[k], _single(L, m, x, dy), f"mlp {k}")


SDF_SHAPE = dict(num_layers=8, hidden_size=64, in_size=3, out=1, freqs=16)


def _grad_backward(L, mlp, x, v, dws, dbs, lat=None):
    h, M = _handle(mlp), x.shape[0]
    g = _Guarded(L.load(True).nrt_mlp_grad_backward_workspace_bytes(h.value, M))
    L.call("nrt_mlp_grad_backward", h.value, L.ptr(x), L.ptr(lat), M, L.ptr(v), _ptrs(dws),
           _ptrs(dbs), None if M == 0 else L.ptr(g.ws), L.stream())
    g.check("nrt_mlp_grad_backward")


@pytest.mark.gpu
@pytest.mark.parametrize("colsplit", [1, 0])
def test_grad_backward_stays_inside_the_workspace(colsplit):
    """nrt_mlp_grad_backward on a one-output SDF shape at a ragged M: guard bands intact, every
    gradient written and finite, the out layer's bias gradient zero."""
    L = _lib()
    _, mlp = _pair(SDF_SHAPE, 9)
    M = 33
    x, v = _inputs(mlp, M, 31, 3)
    dws, dbs = _grad_bufs(mlp)
    with L.options(bwd_colsplit=colsplit):
        _grad_backward(L, mlp, x, v, dws, dbs)
    for t in dws + dbs:
        assert bool(torch.isfinite(t).all())
    assert float(dbs[-1].abs().max()) == 0.0
    assert float(dws[0].abs().max()) > 0.0


@pytest.mark.gpu
def test_zero_rows_zero_every_requested_gradient():
    """M == 0: all four entries return NRT_OK and zero the requested (NaN-filled) gradients."""
    L = _lib()
    kw = SHAPES[RING]
    _, mlp = _pair(kw, 10)
    h = _handle(mlp)
    hs = (P * 1)(h.value)
    x = torch.empty(0, 3, device="cuda")
    dy = torch.empty(0, kw["out"], device="cuda")
    dummy = torch.zeros(256, dtype=torch.uint8, device="cuda")

    def zeroed(call):
        dws, dbs = _grad_bufs(mlp)
        call(_ptrs(dws), _ptrs(dbs))
        torch.cuda.synchronize()
        assert all(float(t.abs().max()) == 0.0 for t in dws + dbs)  # (NaN fails the comparison)

    zeroed(lambda wp, bp: L.call("nrt_mlp_backward", h.value, None, None, 0, None, None, None, wp, bp,
                                 None, L.stream()))
    zeroed(lambda wp, bp: L.call("nrt_mlp_backward_multi", hs, 1, None, 0, _ptrs([dy]), None, wp, bp,
                                 None, L.stream()))
    zeroed(lambda wp, bp: L.call("nrt_mlp_backward_saved", hs, 1, None, 0, None, _ptrs([dummy]), 0,
                                 _ptrs([dy]), None, wp, bp, None, L.stream()))
    _, sdf = _pair(SDF_SHAPE, 9)
    dws, dbs = _grad_bufs(sdf)
    _grad_backward(L, sdf, x, x, dws, dbs)
    assert all(float(t.abs().max()) == 0.0 for t in dws + dbs)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [33, 3001])
@pytest.mark.parametrize("name", [SLAB, RING, "latent_4x32"])
def test_autograd_equals_the_direct_call(name, M):
    """SkipConnMLP.forward + backward (one MLP through neural_blocks._first_order: the saved, the
    multi or, for a latent, the single entry) bit-equal to nrt_mlp_backward called on the same
    handle: dx, dlatent, every dW and db."""
    L = _lib()
    kw = SHAPES[name]
    _, mlp = _pair(kw, 12)
    x, dy = _inputs(mlp, M, 41, kw["out"])
    lat = None
    if kw.get("latent_size"):
        lat = torch.randn(M, kw["latent_size"], generator=torch.Generator().manual_seed(42)).cuda()
    xm = x.clone().requires_grad_(True)
    lm = None if lat is None else lat.clone().requires_grad_(True)
    (mlp(xm, lm) * dy).sum().backward()
    lins = mlp._linears()
    got = [xm.grad, None if lm is None else lm.grad] + [l.weight.grad for l in lins] + \
          [l.bias.grad for l in lins]
    assert not math.isnan(float(xm.grad.sum()))
    _assert_same(got, _single(L, mlp, x, dy, lat=lat), f"{name} M={M}")
