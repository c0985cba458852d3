"""Output pipeline, the part that needs no GPU: the C ABI of the plane packing (argument checks, workspace size), the host-side unpack
against numpy bit for bit, and `pack_reference` -- the packing arithmetic of include/pangu_hip.h restated in numpy with fp32 scalars,
which is the oracle of tests/test_gpu_drain.py and is itself held to the error contract here."""
import os

import numpy as np
import pytest

from pangu_pytorch_amd import _lib

F32 = np.float32
FILL = -32768


def pack_reference(x, mul=None, add=None, levels=0, reciprocal=False):
    """x (planes, plane_elems) float32 in SOURCE plane order; mul / add (planes,) float32 per source plane or None.
    Returns (q int16, scale_offset (planes, 2) float32, nonfinite int32, v float32), all in OUTPUT plane order.
    reciprocal=False divides by the scale, True multiplies by its fp32 reciprocal (what the kernel does)."""
    x = np.ascontiguousarray(x, dtype=F32)
    planes, elems = x.shape
    if mul is not None:
        v = x * np.asarray(mul, F32)[:, None]           # two roundings: the product is stored as fp32 before the sum
        v = v + np.asarray(add, F32)[:, None]
    else:
        v = x.copy()
    if levels:
        assert planes % levels == 0
        v = np.ascontiguousarray(v.reshape(planes // levels, levels, elems)[:, ::-1]).reshape(planes, elems)
    q = np.empty((planes, elems), np.int16)
    so = np.empty((planes, 2), F32)
    nf = np.empty((planes,), np.int32)
    with np.errstate(all="ignore"):
        for p in range(planes):
            fin = np.isfinite(v[p])
            nf[p] = elems - int(fin.sum())
            offset, scale = F32(0), F32(1)
            if nf[p] < elems:
                vf = v[p][fin] if nf[p] else v[p]
                mn, mx = F32(vf.min()), F32(vf.max())
                offset = F32(F32(mx + mn) / F32(2))
                scale = F32(F32(mx - mn) / F32(65534))
                if not scale > 0:
                    scale = F32(1)
            d = (v[p] - offset).astype(F32)
            t = d * F32(F32(1) / scale) if reciprocal else d / scale
            t = np.clip(np.rint(t.astype(F32)), -32767, 32767)
            q[p] = np.where(fin, t, FILL).astype(np.int16)
            so[p] = scale, offset
    return q, so, nf, v


def contract_violations(q, so, v):
    """The error contract, for finite v, evaluated in fp64 with the plane's fp32 scale / offset:
        |q * scale + offset - v| <= 0.5 * scale * (1 + 2^-10) + 4 * 2^-24 * max(|min|, |max|).
    Returns (number of finite values outside it, the largest |error| / bound)."""
    bad, worst = 0, 0.0
    for p in range(v.shape[0]):
        fin = np.isfinite(v[p])
        if not fin.any():
            continue
        vf = v[p][fin].astype(np.float64)
        scale, offset = float(so[p, 0]), float(so[p, 1])
        bound = 0.5 * scale * (1 + 2.0 ** -10) + 4 * 2.0 ** -24 * max(abs(vf.min()), abs(vf.max()))
        err = np.abs(q[p][fin].astype(np.float64) * scale + offset - vf)
        bad += int((err > bound).sum())
        worst = max(worst, float(err.max()) / bound if bound > 0 else float(err.max() > 0))
    return bad, worst


def endpoints_ok(q, v):
    """In every plane with a finite range, min packs to -32767 and max to +32767."""
    for p in range(v.shape[0]):
        fin = np.isfinite(v[p])
        if not fin.any():
            continue
        vf, qf = v[p][fin], q[p][fin]
        if vf.max() > vf.min() and not (qf[vf.argmin()] == -32767 and qf[vf.argmax()] == 32767):
            return False
    return True


def contract_inputs(n=40000, seed=0):
    """The fields the contract was stated for, one plane each."""
    r = np.random.default_rng(seed)
    nan1 = r.standard_normal(n)
    nan1[r.random(n) < 0.01] = np.nan
    ulps = F32(250) + np.spacing(F32(250)) * r.integers(-3, 4, n).astype(F32)
    return np.stack([r.standard_normal(n), 2e5 + 5e3 * r.standard_normal(n), 1e-6 * np.abs(r.standard_normal(n)),
                     101325 + 1500 * r.standard_normal(n), ulps, nan1]).astype(F32)


@pytest.mark.parametrize("reciprocal", [False, True])
def test_reference_meets_the_error_contract(reciprocal):
    x = contract_inputs()
    q, so, nf, v = pack_reference(x, reciprocal=reciprocal)
    bad, worst = contract_violations(q, so, v)
    print(f"reciprocal={reciprocal}: worst |error| / bound = {worst:.3f}")
    assert bad == 0 and worst <= 1.0
    assert endpoints_ok(q, v)
    assert list(nf[:5]) == [0] * 5 and nf[5] == np.isnan(x[5]).sum() > 0
    assert (q[5][np.isnan(x[5])] == FILL).all() and (q[:5] != FILL).all()
    # the affine value and the level reversal: plane (var, l) of the result is source plane (var, L-1-l), de-normalised
    xs = np.random.default_rng(1).standard_normal((6, 50)).astype(F32)
    mul, add = np.linspace(0.5, 3, 6).astype(F32), np.linspace(-200, 900, 6).astype(F32)
    q2, so2, _, v2 = pack_reference(xs, mul, add, levels=3, reciprocal=reciprocal)
    assert np.array_equal(v2[0], xs[2] * mul[2] + add[2]) and np.array_equal(v2[4], xs[4] * mul[4] + add[4])
    assert contract_violations(q2, so2, v2)[0] == 0 and endpoints_ok(q2, v2)


def test_reference_edge_planes():
    x = np.zeros((3, 9), F32)
    x[0] = 271.5                                  # constant: scale 1, offset the value, q = 0
    x[1] = [1, 2, np.nan, 3, np.inf, 4, 5, 6, 7]
    x[2] = [np.nan, np.inf, -np.inf] * 3
    q, so, nf, _ = pack_reference(x)
    assert (q[0] == 0).all() and tuple(so[0]) == (1.0, 271.5) and nf[0] == 0
    assert nf[1] == 2 and q[1][2] == FILL and q[1][4] == FILL and tuple(so[1]) == (F32(6) / F32(65534), 4.0)
    assert q[1][0] == -32767 and q[1][8] == 32767
    assert nf[2] == 9 and (q[2] == FILL).all() and tuple(so[2]) == (1.0, 0.0)


needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libpangu_hip.so not built")


@needs_lib
def test_argument_validation_without_gpu():
    lib = _lib.load()
    P8 = 8          # any non-NULL address: the calls below return before touching memory
    big = 1 << 40
    pack = lib.pangu_pack_planes_i16
    assert pack(None, None, None, None, P8, P8, P8, P8, big, 26, 144, 0) == -2
    assert pack(None, P8, None, None, None, P8, P8, P8, big, 26, 144, 0) == -2
    assert pack(None, P8, None, None, P8, None, P8, P8, big, 26, 144, 0) == -2
    assert pack(None, P8, None, None, P8, P8, None, P8, big, 26, 144, 0) == -2
    assert pack(None, P8, None, None, P8, P8, P8, None, big, 26, 144, 0) == -2
    assert pack(None, P8, P8, None, P8, P8, P8, P8, big, 26, 144, 0) == -2                  # mul without add
    assert pack(None, P8, None, P8, P8, P8, P8, P8, big, 26, 144, 0) == -2                  # add without mul
    assert pack(None, P8, None, None, P8, P8, P8, P8, big, 0, 144, 0) == -1
    assert pack(None, P8, None, None, P8, P8, P8, P8, big, 26, 0, 0) == -1
    assert pack(None, P8, None, None, P8, P8, P8, P8, big, 27, 144, 13) == -1               # planes % levels
    assert pack(None, P8, None, None, P8, P8, P8, P8, big, 26, 144, -1) == -1
    short = lib.pangu_pack_i16_ws_bytes(26, 144) - 1
    assert pack(None, P8, None, None, P8, P8, P8, P8, short, 26, 144, 13) == -4             # the short-workspace code of the ABI
    stage = lib.pangu_stage_planes_f32
    assert stage(None, None, None, None, P8, 26, 144, 0) == -2
    assert stage(None, P8, None, None, None, 26, 144, 0) == -2
    assert stage(None, P8, P8, None, P8, 26, 144, 0) == -2
    assert stage(None, P8, None, None, P8, 0, 144, 0) == -1
    assert stage(None, P8, None, None, P8, 26, 0, 0) == -1
    assert stage(None, P8, None, None, P8, 27, 144, 13) == -1
    unpack = lib.pangu_unpack_i16_host
    assert unpack(None, P8, P8, 1, 1, 1) == -2 and unpack(P8, None, P8, 1, 1, 1) == -2 and unpack(P8, P8, None, 1, 1, 1) == -2
    assert unpack(P8, P8, P8, 0, 1, 1) == -1 and unpack(P8, P8, P8, 1, 0, 1) == -1


@needs_lib
def test_workspace_size():
    ws = _lib.load().pangu_pack_i16_ws_bytes
    sizes = [ws(p, 721 * 1440) for p in (1, 2, 4, 69, 70)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert ws(1, 1) > 0 and ws(69, 721 * 1440) < (1 << 20)        # a few partials per plane, not a second field
    assert ws(3, 0) == -1 and ws(0, 100) == -1 and ws(3, 1 << 31) == -1


@needs_lib
@pytest.mark.parametrize("shape", [(3, 15), (1, 1), (5, 2_100_003)])
def test_unpack_matches_numpy_bit_for_bit(shape):
    lib = _lib.load()
    planes, elems = shape
    r = np.random.default_rng(planes * 1000 + elems % 997)
    q = r.integers(-32768, 32768, size=shape, dtype=np.int64).astype(np.int16)
    q.reshape(-1)[:: max(1, q.size // 11)] = FILL
    q.reshape(-1)[-1] = FILL if elems > 1 else 123              # the ragged tail of the last span carries a fill value
    so = np.stack([r.uniform(1e-4, 3, planes), r.normal(0, 1e4, planes)], axis=1).astype(F32)
    want = q.astype(F32) * so[:, :1] + so[:, 1:]                # fp32 product, then fp32 sum
    want[q == FILL] = np.nan
    for threads in (1, 3, 64):
        got = np.full(shape, 7.0, F32)
        assert lib.pangu_unpack_i16_host(got.ctypes.data, q.ctypes.data, so.ctypes.data, planes, elems, threads) == 0
        assert np.array_equal(np.isnan(got), q == FILL), threads
        ok = q != FILL
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), threads
