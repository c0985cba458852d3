"""The zonal power spectrum without a GPU: the definition restated in numpy float64 (spectrum_ref, what the GPU test compares
against), the fp32 yardstick (spectrum_f32: the kernel's folded, pivot-subtracted transform as two float32 matrix products), the
basis builder, the band weights, SpectrumResult's derived quantities and the argument checks of the C ABI and of score.py."""
import os

import numpy as np
import pytest
import torch

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib


def _d32(x, minus):
    x = np.asarray(x, dtype=np.float32)
    return x if minus is None else (x - np.asarray(minus, dtype=np.float32)[None]).astype(np.float32)


def _ck(W, K):
    c = np.full(K + 1, 2.0)
    c[0] = 1.0
    if K == W // 2:
        c[K] = 1.0
    return c


def spectrum_ref(x, minus, band_weight, K):
    """The definition in float64: x (N, planes, H, W), minus (planes, H, W) or None, band_weight (B, H) -> (N, B, planes, K + 1).
    d = x - minus is taken in fp32 first (the kernel's one rounding); then P_0 = mean(d)^2 and P_k = c_k |X_k|^2 / W^2 with
    np.fft.rfft.  (The pivot of the kernel changes nothing here: pivot + Re X_0(a) / W is the mean of d.)"""
    d = _d32(x, minus).astype(np.float64)
    W = d.shape[-1]
    X = np.fft.rfft(d, axis=-1)[..., :K + 1]
    p = (X.real ** 2 + X.imag ** 2) * _ck(W, K) / float(W) ** 2
    return np.einsum("bh,nphk->nbpk", np.asarray(band_weight, dtype=np.float64), p)


def fold(a):
    """(e, o) (..., M + 1) of rows a (..., W): e[j] = a[j] + a[W - j], o[j] = a[j] - a[W - j]; e[0] = a[0], e[M] = a[M], o = 0
    at both ends."""
    W = a.shape[-1]
    M = W // 2
    back = a[..., :M - 1:-1] if M > 0 else a      # a[W - 1], ..., a[M]
    e = np.empty(a.shape[:-1] + (M + 1,), dtype=a.dtype)
    o = np.zeros_like(e)
    e[..., 0], e[..., M] = a[..., 0], a[..., M]
    e[..., 1:M] = a[..., 1:M] + back[..., :M - 1]
    o[..., 1:M] = a[..., 1:M] - back[..., :M - 1]
    return e, o


def spectrum_f32(x, minus, band_weight, K):
    """The yardstick: the kernel's transform in float32 numpy.  d, pivot = d[0], a = d - pivot, the fold, two float32 matrix
    products against the fp32-rounded basis, the power and the band sum, everything float32."""
    f = np.float32
    d = _d32(x, minus)
    W = d.shape[-1]
    pivot = d[..., :1]
    e, o = fold((d - pivot).astype(f))
    c, s = (t.astype(f) for t in P.score.spectrum_basis(W, K))
    re, im = e @ c, o @ s
    p = ((re * re + im * im) * (_ck(W, K) / float(W) ** 2).astype(f)).astype(f)
    m0 = pivot[..., 0] + re[..., 0] * f(1.0 / W)
    p[..., 0] = m0 * m0
    return np.einsum("bh,nphk->nbpk", np.asarray(band_weight, dtype=f), p).astype(f)


def spectrum_err(p, r):
    """(err over k >= 1, err at k = 0), each (N, B, planes): max_k |P_k - R_k| / sum_{k>=1} R_k and |P_0 - R_0| / (R_0 + that
    sum) -- relative to the band's total power, the size of the white error floor of an fp32 accumulation."""
    p, r = np.asarray(p, dtype=np.float64), np.asarray(r, dtype=np.float64)
    tot = r[..., 1:].sum(-1)
    return np.abs(p[..., 1:] - r[..., 1:]).max(-1) / tot, np.abs(p[..., 0] - r[..., 0]) / (r[..., 0] + tot)


def red_field(shape, seed, offset=300.0):
    """A red-spectrum random field (amplitude ~ k^-1.5, anomaly scale 1) on an offset: zero-mean white noise would hide the
    offset problem the pivot exists for.  float32, shape (..., W)."""
    rng = np.random.default_rng(seed)
    W = shape[-1]
    k = np.arange(1, W // 2 + 1)
    amp = k ** -1.5
    spec = np.zeros(shape[:-1] + (W // 2 + 1,), dtype=np.complex128)
    spec[..., 1:] = amp * (rng.standard_normal(shape[:-1] + (W // 2,)) + 1j * rng.standard_normal(shape[:-1] + (W // 2,)))
    x = np.fft.irfft(spec, n=W, axis=-1)
    x /= x.std()
    return (x + offset).astype(np.float32)


def band_rows(H, B, seed=0):
    """B rows of non-negative weights that sum to 1 each (hand-made, no torch)."""
    rng = np.random.default_rng(seed)
    w = rng.random((B, H)) + 0.1
    return (w / w.sum(1, keepdims=True)).astype(np.float32)


# ---- the restatement and the yardstick -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [8, 72, 100])
def test_fold_identities(W):
    """Re X_k = sum_{j<=M} e[j] cos(2 pi jk / W) and Im X_k = -sum o[j] sin(2 pi jk / W), in float64 against rfft."""
    a = np.random.default_rng(W).standard_normal((5, W))
    e, o = fold(a)
    c, s = P.score.spectrum_basis(W, W // 2)
    X = np.fft.rfft(a, axis=-1)
    scale = np.abs(a).sum(-1, keepdims=True)
    assert np.abs(e @ c - X.real).max() <= 1e-14 * scale.max()
    assert np.abs(-(o @ s) - X.imag).max() <= 1e-14 * scale.max()
    assert (o[:, 0] == 0).all() and (o[:, -1] == 0).all() and (e[:, 0] == a[:, 0]).all() and (e[:, -1] == a[:, W // 2]).all()


@pytest.mark.parametrize("W,k0,want", [(72, 3, 0.5), (72, 36, 1.0), (8, 4, 1.0), (100, 3, 0.5)])
def test_ck_and_the_nyquist_term(W, k0, want):
    """A unit cosine at k0 holds power 1/2 (c_k = 2 collects both signs of k), at the Nyquist wavenumber 1 (c = 1)."""
    n = np.arange(W)
    x = (np.cos(2 * np.pi * k0 * n / W) + 300.0).astype(np.float32)[None, None, None, :]
    one = np.ones((1, 1), dtype=np.float32)
    # the row is rounded to fp32 around 300 (steps of 3e-5): that alone moves X_k0 by about 1.5e-6 of itself
    for fn, tol in ((spectrum_ref, 1e-5), (spectrum_f32, 2e-5)):
        p = fn(x, None, one, W // 2)[0, 0, 0]
        assert abs(p[k0] - want) <= tol and abs(p[0] - 300.0 ** 2) <= 300.0 ** 2 * 1e-6
        rest = np.delete(p, [0, k0])
        assert np.abs(rest).max() <= tol


def test_parseval_and_truncation():
    W, H = 72, 5
    x = red_field((2, 3, H, W), 1)
    bw = band_rows(H, 2)
    full = spectrum_ref(x, None, bw, W // 2)
    ms = np.einsum("bh,nph->nbp", bw.astype(np.float64), (x.astype(np.float64) ** 2).mean(-1))
    assert np.abs(full.sum(-1) - ms).max() <= 1e-12 * ms.max()
    assert np.array_equal(spectrum_ref(x, None, bw, 10), full[..., :11])                   # K < W/2: the first K + 1 columns
    f_full, f_10 = spectrum_f32(x, None, bw, W // 2), spectrum_f32(x, None, bw, 10)
    assert np.allclose(f_10, f_full[..., :11], rtol=1e-5, atol=0)


@pytest.mark.parametrize("W", [8, 72, 100, 1440])
def test_yardstick_against_the_restatement(W):
    """spectrum_f32 against spectrum_ref on the GPU test's kind of input, with and without minus.  The a-priori bound: each X_k is
    a sum of M + 1 fp32 products with |error| <= (M + 1) 2^-24 sum_j |e_j c_jk| <= (M + 1)^1.5 2^-24 |e|_2, and |e|_2^2 is at most
    2 W^2 times the row's anomaly power, so the error of P_k relative to the total power stays below 8 (M + 1)^1.5 2^-24; measured
    values are two to three orders below it (2.5e-7 at W = 72, 1e-6 at W = 1440)."""
    H = 6
    x = red_field((1, 2, H, W), W)
    minus = red_field((2, H, W), W + 1, offset=0.0) * np.float32(0.5)
    bw = band_rows(H, 2, seed=W)
    for m in (None, minus):
        for K in (W // 2, max(1, W // 8)):
            ek, e0 = spectrum_err(spectrum_f32(x, m, bw, K), spectrum_ref(x, m, bw, K))
            print(f"W = {W} K = {K} minus = {m is not None}: err = {ek.max():.3g}, err0 = {e0.max():.3g}")
            assert ek.max() <= 8 * (W // 2 + 1) ** 1.5 * 2.0 ** -24 and e0.max() <= 8 * 2.0 ** -24


def test_pivot_keeps_the_digits_of_an_offset_field():
    """Why the pivot is there: an offset of 5e4 on an anomaly of 1e3, transformed in fp32 with and without it."""
    W = 72
    x = (red_field((1, 1, 4, W), 3, offset=0.0) * np.float32(1e3) + np.float32(5e4)).astype(np.float32)
    bw = band_rows(4, 1)
    ref = spectrum_ref(x, None, bw, W // 2)
    with_pivot = spectrum_err(spectrum_f32(x, None, bw, W // 2), ref)[0].max()
    e, o = fold(x)                                                       # no pivot: the offset rides through every product
    c, s = (t.astype(np.float32) for t in P.score.spectrum_basis(W, W // 2))
    re, im = e @ c, o @ s
    p = (re * re + im * im) * (_ck(W, W // 2) / W ** 2).astype(np.float32)
    without = spectrum_err(np.einsum("bh,nphk->nbpk", bw, p), ref)[0].max()
    assert with_pivot <= 1e-5 and without >= 10 * with_pivot


# ---- the basis builder -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,K", [(8, 4), (72, 36), (100, 7), (1440, 720)])
def test_basis_builder(W, K):
    c, s = P.score.spectrum_basis(W, K)
    assert c.dtype == np.float64 and s.dtype == np.float64 and c.shape == s.shape == (W // 2 + 1, K + 1)
    j, k = np.arange(W // 2 + 1)[:, None], np.arange(K + 1)[None, :]
    r = (j * k) % W
    assert np.abs(c - np.cos(2 * np.pi * r / W)).max() <= 2e-16 and np.abs(s - np.sin(2 * np.pi * r / W)).max() <= 2e-16
    quarter = (4 * r) % W == 0                               # the angle is a multiple of pi / 2: exact values, no 6e-17
    q = (4 * r) // W
    assert np.array_equal(c[quarter], np.array([1.0, 0.0, -1.0, 0.0])[q[quarter]])
    assert np.array_equal(s[quarter], np.array([0.0, 1.0, 0.0, -1.0])[q[quarter]])
    assert (c[0] == 1).all() and (s[0] == 0).all() and (c[:, 0] == 1).all() and (s[:, 0] == 0).all()
    if K == W // 2:
        assert np.array_equal(c[:, K], np.where(np.arange(W // 2 + 1) % 2 == 0, 1.0, -1.0)) and (s[:, K] == 0).all()
    # the argument is reduced in integers: at W = 1440 the largest product j k = 518400 would cost digits as a float angle
    assert np.abs(c * c + s * s - 1).max() <= 4e-16
    for bad in ((6, 3), (10, 2), (8, 0), (8, 5)):
        with pytest.raises(ValueError):
            P.score.spectrum_basis(*bad)


# ---- band weights ----------------------------------------------------------------------------------------------------------------

def test_band_weights():
    H = 37
    w = P.score.latitude_weights(H, "cpu")
    g = P.score.spectrum_band_weights(H)
    assert g.shape == (1, H) and g.dtype == torch.float32
    assert torch.allclose(g[0], w / H, rtol=1e-6, atol=0)
    bands = [(-90, -20), (-20, 20), (20, 90), (-90, 90)]
    b = P.score.spectrum_band_weights(H, bands)
    assert b.shape == (4, H)
    assert torch.allclose(b.double().sum(1), torch.ones(4, dtype=torch.float64), rtol=1e-6, atol=0)
    lat = 90.0 - torch.arange(H) * 180.0 / (H - 1)
    for row, (s, n) in zip(b, bands):
        inside = (lat >= s) & (lat <= n)
        assert (row[~inside] == 0).all()      # (the weight at a pole is -4e-6 cos-units, not 0: latitude_weights keeps 3.1416)
        assert torch.allclose(row[inside] / row[inside].sum(), w[inside] / w[inside].sum(), rtol=1e-5, atol=1e-12)
    assert torch.allclose(b[3], g[0])
    for bad in ([(10.1, 10.2)], [(20, -20)], [(-90, 90)] * 5, [], [(float("nan"), 3.0)], [(1.0,)]):
        with pytest.raises(ValueError):
            P.score.spectrum_band_weights(H, bad)


# ---- SpectrumResult on hand-made tables ------------------------------------------------------------------------------------------

def test_spectrum_result_derived_quantities():
    K = 5
    ref = P.score.SpectrumResult(torch.tensor([[[[9.0, 4.0, 4.0, 4.0, 4.0, 4.0]]]]), torch.arange(K + 1), None)      # (1, 1, 1, 6)
    rows = [[9.0, 4.0, 1.0, 4.0, 1.0, 1.0],      # below from k = 4 on (k = 2 is below, k = 3 is not)
            [9.0, 1.0, 1.0, 1.0, 1.0, 1.0],      # below everywhere: 1
            [9.0, 1.0, 1.0, 1.0, 1.0, 4.0],      # not below at K: K + 1
            [9.0, 4.0, 4.0, 4.0, 4.0, 2.0]]      # exactly at the threshold is not below: K + 1
    res = P.score.SpectrumResult(torch.tensor(rows, dtype=torch.float32).reshape(4, 1, 1, K + 1), torch.arange(K + 1), None)
    er = res.effective_resolution(ref)
    assert er.dtype == torch.int64 and er.shape == (4, 1, 1)
    assert er.reshape(-1).tolist() == [4, 1, K + 1, K + 1]
    assert res.effective_resolution(ref, threshold=0.2).reshape(-1).tolist() == [K + 1] * 4
    r = res.ratio(ref)
    assert r.dtype == torch.float64 and r.shape == (4, 1, 1, K + 1) and r[0, 0, 0].tolist() == [1.0, 1.0, 0.25, 1.0, 0.25, 0.25]
    v = res.variance()
    assert v.dtype == torch.float64 and v.reshape(-1).tolist() == [11.0, 5.0, 8.0, 18.0]
    m = res.mean_over_items()
    assert m.power.shape == (1, 1, 1, K + 1) and m.power.dtype == torch.float64
    assert m.power.reshape(-1).tolist() == [9.0, 2.5, 1.75, 2.5, 1.75, 2.0]
    big = P.score.SpectrumResult(torch.tensor([1.0, 2.0 ** -30, 2.0 ** -30]).reshape(3, 1, 1, 1).expand(3, 1, 1, 2).contiguous(),
                                 torch.arange(2), None)
    assert big.mean_over_items().power[0, 0, 0, 1].item() == (1.0 + 2.0 ** -29) / 3      # added in float64: fp32 would drop the tail


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------------

P16 = 4096          # a 16-B aligned non-NULL address: every call below returns before touching memory


def _call(lib, fields=P16, stride=69 * 721 * 1440, N=1, minus=None, bw=P16, B=1, c=P16, s=P16, K=720, out=P16, ws=P16, ws_bytes=1 << 40,
          planes=69, H=721, W=1440):
    return lib.pangu_zonal_spectrum_f32(None, fields, stride, N, minus, bw, B, c, s, K, out, ws, ws_bytes, planes, H, W)


def test_spectrum_entry_argument_validation_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    NULL, SHAPE, ARG = -2, -1, -4
    for name in ("fields", "bw", "c", "s", "out", "ws"):
        assert _call(lib, **{name: None}) == NULL, name
    item = 69 * 721 * 1440
    shape_cases = [dict(N=0), dict(B=0), dict(B=5), dict(K=0), dict(K=721), dict(W=1442, K=4), dict(W=4, K=2, stride=69 * 721 * 4),
                   dict(W=1 << 15, K=4, H=1, planes=1, stride=1 << 15), dict(planes=0), dict(H=0), dict(W=0), dict(W=-8),
                   dict(H=1 << 20, W=1 << 11, K=4, planes=1, stride=1 << 31),          # H*W = 2^31
                   dict(stride=item - 4), dict(stride=item + 2), dict(N=2, stride=item - 4),
                   dict(N=1 << 14, stride=1 << 27),                                     # (N - 1) * stride + item > 2^40
                   dict(N=3, stride=1 << 39)]
    for kw in shape_cases:
        assert _call(lib, **kw) == SHAPE, kw
    assert _call(lib, N=2, stride=item + 4, ws_bytes=1 << 40, fields=P16 + 4) == ARG      # a longer stride is fine; then alignment
    need = lib.pangu_zonal_spectrum_ws_bytes(1, 69, 721, 1, 720)
    assert need == 69 * 6 * 1 * 721 * 4
    assert _call(lib, ws_bytes=need - 1) == ARG
    for name in ("fields", "minus", "out", "c", "s"):
        assert _call(lib, ws_bytes=need, **{name: P16 + 4}) == ARG, name                # the size passes, the alignment does not
    # NULL before shape before argument
    assert _call(lib, fields=None, N=0, ws_bytes=0) == NULL and _call(lib, N=0, ws_bytes=0) == SHAPE


def test_spectrum_workspace_formula():
    """pangu_zonal_spectrum_ws_bytes is what the entry asks for: one byte less is refused, the exact size passes on to the next
    check (alignment), for every combination; Python keeps a launch under 256 MB by splitting N."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    for N, planes, H, B, K, W in ((1, 69, 721, 1, 720, 1440), (50, 65, 721, 4, 180, 1440), (3, 4, 9, 2, 4, 8), (2, 3, 129, 4, 50, 100)):
        need = lib.pangu_zonal_spectrum_ws_bytes(N, planes, H, B, K)
        assert need == N * planes * ((H + 127) // 128) * B * (K + 1) * 4
        kw = dict(N=N, planes=planes, H=H, B=B, K=K, W=W, stride=planes * H * W)
        assert _call(lib, ws_bytes=need - 1, **kw) == -4
        assert _call(lib, ws_bytes=need, out=P16 + 4, **kw) == -4 and _call(lib, ws_bytes=need, N=0, **{k: v for k, v in kw.items() if k != "N"}) == -1
    for bad in ((0, 69, 721, 1, 720), (1, 0, 721, 1, 720), (1, 69, 0, 1, 720), (1, 69, 721, 0, 720), (1, 69, 721, 5, 720),
                (1, 69, 721, 1, 0), (1 << 30, 1 << 20, 721, 4, 720)):
        assert lib.pangu_zonal_spectrum_ws_bytes(*bad) == -1, bad
    per_item = lib.pangu_zonal_spectrum_ws_bytes(1, 65, 721, 4, 720)
    assert 128 * per_item > P.score.SPECTRUM_WS_LIMIT >= per_item      # E = 128, B = 4 needs the split; one item always fits


def test_spectrum_python_refusals_before_any_launch():
    z = lambda *s: torch.zeros(s)
    up, sf = z(2, 5, 13, 9, 8), z(2, 4, 9, 8)
    zs = P.score.zonal_spectrum
    for args, kw in (((up[0], sf), {}), ((up, sf[:1]), {}), ((up, z(2, 4, 9, 12)), {}), ((z(2, 5, 13, 9, 6), z(2, 4, 9, 6)), {}),
                     ((up, sf), dict(minus_upper=up[:1])), ((up, sf), dict(minus_upper=up, minus_surface=sf)),
                     ((up, sf), dict(kmax=0)), ((up, sf), dict(kmax=5)), ((up, sf), dict(bands=[(20, -20)])),
                     ((up, sf), dict(bands=[(-90, 90)] * 5)), ((up, sf), dict(bands=torch.ones(5, 9))),
                     ((up, sf), dict(bands=torch.ones(2, 8)))):
        with pytest.raises(ValueError):
            zs(*args, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        zs(up, sf)
