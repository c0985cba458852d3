"""The zonal-spectrum kernel on the GPU against the float64 restatement of its definition (test_spectra_cpu.spectrum_ref), with the
error bound taken from the fp32 yardstick (test_spectra_cpu.spectrum_f32) on the same inputs, the exact and structural
properties the definition promises, and the wiring into score.zonal_spectrum and EnsembleRollout.spectra.

Shapes, the smallest at which the kernel can go wrong: (H, W) = (9, 8) (the minimum W: M + 1 = 5 samples, less than one staging
chunk), (37, 72) (one full 32-row sub-tile and a tail of 5; M + 1 = 37 is odd: ragged in j and in k), (33, 100) (W no multiple of
32), all 69 planes each; and (33, 1440) on 3 planes through the C ABI: the real basis, 46 staging chunks of which the last holds
the single sample j = 720, six wavenumber tiles of which the last is ragged (k = 640..720).  H = 129 (one row beyond a 128-row
tile: two row tiles through the second launch) runs on 4 planes at W = 8.

Error measure and bound (per item, band and plane): err = max_{1<=k<=K} |P_k - R_k| / sum_{k>=1} R_k and err0 = |P_0 - R_0| /
(R_0 + sum_{k>=1} R_k), R the restatement with the same arguments; the bound of a case is 4 x the largest err (err0) of
spectrum_f32 on the same inputs (an MFMA accumulates the M + 1 products as one sequential fmaf chain where numpy blocks the sum).

Worst kernel err / bound and err0 / bound measured on an MI355X (also in profiles/spectra.json):
  (9, 8): 0.32, 0.30    (37, 72): 0.24, 0.13    (33, 100): 0.24, 0.14    (33, 1440): 0.23, 0.26    (129, 8): 0.17, 0.07"""
import functools

import numpy as np
import pytest
import torch

import cases
import synth
from pangu_pytorch_amd import _lib
from test_gpu_ensemble import _stats_last
from test_spectra_cpu import band_rows, red_field, spectrum_err, spectrum_f32, spectrum_ref

pytestmark = pytest.mark.gpu

SHAPES = [(9, 8), (37, 72), (33, 100)]
SCORE_RTOL = 1e-5          # the tolerance of tests/test_gpu_quantiles.py for its per-plane scores
FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def _case(H, W, planes=69):
    """Inputs of one shape, made once: x (3, planes, H, W) red fields on an offset of 300, minus (planes, H, W), B = 2 weights."""
    x = red_field((3, planes, H, W), 1000 * H + W)
    minus = (red_field((planes, H, W), 7 * H + W, offset=0.0) * np.float32(0.5) + np.float32(299.0)).astype(np.float32)
    return x, minus, band_rows(H, 2, seed=H)


def _split(a):
    """(.., 69, H, W) numpy -> upper (.., 5, 13, H, W), surface (.., 4, H, W) on the GPU."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lead, (H, W) = tuple(t.shape[:-3]), t.shape[-2:]
    return t[..., :65, :, :].reshape(lead + (5, 13, H, W)).contiguous(), t[..., 65:, :, :].contiguous()


def _joined(ru, rs):
    """(N, B, 69, K + 1) float32 numpy of an (upper, surface) result pair."""
    pu, ps = ru.power, rs.power
    return torch.cat([pu.reshape(pu.shape[0], pu.shape[1], 65, -1), ps], dim=2).cpu().numpy()


def _spectrum(P, x, minus=None, bands=None, kmax=None):
    up, sf = _split(x)
    mu, ms = (None, None) if minus is None else _split(minus)
    return _joined(*P.score.zonal_spectrum(up, sf, mu, ms, bands=bands, kmax=kmax))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(got, x, minus, bw, K, what):
    """got against the restatement within FACTOR x the yardstick's error; returns the two ratios for the record."""
    ref = spectrum_ref(x, minus, bw, K)
    bk, b0 = (FACTOR * e.max() for e in spectrum_err(spectrum_f32(x, minus, bw, K), ref))
    ek, e0 = (e.max() for e in spectrum_err(got, ref))
    print(f"{what}: err = {ek:.3g} (bound {bk:.3g}, ratio {ek / bk:.3f}); err0 = {e0:.3g} (bound {b0:.3g}, ratio {e0 / b0:.3f})")
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert ek <= bk and e0 <= b0, what
    return ek / bk, e0 / b0


@functools.lru_cache(maxsize=None)
def _shape_bound(H, W):
    """(bound, bound0) of a shape: FACTOR x the yardstick's error on the shape's red-field case (K = W/2, no minus)."""
    x, _, bw = _case(H, W)
    return tuple(FACTOR * e.max() for e in spectrum_err(spectrum_f32(x[:1], None, bw, W // 2), spectrum_ref(x[:1], None, bw, W // 2)))


def _abi(x, minus, bw, K):
    """pangu_zonal_spectrum_f32 directly: x (N, planes, H, W), minus (planes, H, W) or None, bw (B, H) numpy -> numpy."""
    import pangu_pytorch_amd as P
    N, planes, H, W = x.shape
    B = bw.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    xt, bt = dev(x), dev(bw)
    mt = None if minus is None else dev(minus)
    c, s = (dev(t) for t in P.score.spectrum_basis(W, K))
    lib = _lib.load()
    need = lib.pangu_zonal_spectrum_ws_bytes(N, planes, H, B, K)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty((N, B, planes, K + 1), dtype=torch.float32, device="cuda")
    _lib.check(lib.pangu_zonal_spectrum_f32(torch.cuda.current_stream().cuda_stream, xt.data_ptr(), planes * H * W, N,
                                            None if mt is None else mt.data_ptr(), bt.data_ptr(), B, c.data_ptr(), s.data_ptr(), K,
                                            out.data_ptr(), ws.data_ptr(), need, planes, H, W), "zonal_spectrum_f32")
    return out.cpu().numpy()


# ---- against the restatement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_against_the_restatement(H, W):
    import pangu_pytorch_amd as P
    x, minus, bw = _case(H, W)
    bands = torch.from_numpy(bw)
    for m in (None, minus):
        for K in (W // 2, max(1, W // 8)):
            got = _spectrum(P, x[:1], m, bands, K)
            _check(got, x[:1], m, bw, K, f"({H}, {W}) K = {K} minus = {m is not None}")


def test_real_basis_through_the_c_abi():
    """W = 1440 with the real basis tables; K = 180 equals the first 181 columns of K = 720 bit for bit (another table stride,
    two wavenumber tiles instead of six)."""
    H, W = 33, 1440
    x, minus, bw = _case(H, W, planes=3)
    full = _abi(x[:1], minus, bw, 720)
    _check(full, x[:1], minus, bw, 720, f"({H}, {W}) K = 720 minus = True")
    part = _abi(x[:1], minus, bw, 180)
    assert np.array_equal(_bits(part), _bits(full[..., :181]))
    _check(_abi(x[:1], None, bw[:1], 720), x[:1], None, bw[:1], 720, f"({H}, {W}) K = 720 minus = False")


def test_two_row_tiles():
    """H = 129: the last row is alone in the second 128-row tile; the second launch adds the two tiles."""
    H, W = 129, 8
    x, minus, bw = _case(H, W, planes=4)
    _check(_abi(x[:2], minus, bw, 4), x[:2], minus, bw, 4, f"({H}, {W}) K = 4 minus = True")


# ---- exact and structural properties ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", SHAPES)
def test_pure_cosines_and_constant_field(H, W):
    import pangu_pytorch_amd as P
    n = np.arange(W)
    bw = band_rows(H, 1, seed=3)
    for k0, want in ((3, 0.5), (W // 2, 1.0)):
        row = (np.cos(2 * np.pi * k0 * n / W) + 300.0).astype(np.float32)
        x = np.broadcast_to(row, (1, 69, H, W)).copy()
        got = _spectrum(P, x, None, torch.from_numpy(bw))
        # The bound is the shape's (that of its red-field case): every row is the same here and the arithmetic nearly exact, so
        # the yardstick's own error on this input is a single draw, at times 0.  err bounds |P_k - R_k| for every k >= 1 by
        # bound * total power (about `want`): the line at k0 and the empty columns.
        ref = spectrum_ref(x, None, bw, W // 2)
        bk, b0 = _shape_bound(H, W)
        ek, e0 = (e.max() for e in spectrum_err(got, ref))
        print(f"({H}, {W}) cosine k0 = {k0}: err / bound = {ek / bk:.3f}, err0 / bound = {e0 / b0:.3f}")
        assert ek <= bk and e0 <= b0
        # the samples are rounded to the fp32 grid at 300 (steps of 2^-15, errors up to 2^-16): that moves the line's amplitude by
        # at most 2^-15 and its power by at most 2^-15 (1 + 2^-16), and puts at most 2 (2^-16)^2 < 1e-9 into an empty column
        grid = 2.0 ** -15 * 1.001
        assert np.abs(ref[..., k0] - want).max() <= grid and np.abs(np.delete(ref, [0, k0], axis=-1)).max() <= 1e-9
        assert np.abs(got[..., k0] - want).max() <= grid + bk * want and np.abs(np.delete(got, [0, k0], axis=-1)).max() <= 1e-9 + bk * want
    c = np.float32(287.15)
    x = np.full((1, 69, H, W), c, dtype=np.float32)
    got = _spectrum(P, x, None, torch.from_numpy(bw))
    assert (got[..., 1:] == 0).all()                                   # a = d - pivot is exactly 0: exact zeros, not small numbers
    # P_0 = sum_h w_h c^2: one rounding of the square, one per product and at most H + 2 additions on the longest chain
    r0 = spectrum_ref(x, None, bw, W // 2)[..., 0]
    assert np.abs(got[..., 0] - r0).max() <= (H + 4) * 2.0 ** -24 * r0.max()


@pytest.mark.parametrize("H,W", SHAPES)
def test_parseval_against_lat_weighted_sums(H, W):
    """Global band, K = W/2: sum_k power is the existing kernel's sum w p^2 / (H W) (weighted_rmse_channels against zero, squared)."""
    import pangu_pytorch_amd as P
    x, _, _ = _case(H, W)
    up, sf = _split(x[:1])
    ru, rs = P.score.zonal_spectrum(up, sf)
    assert ru.power.shape == (1, 1, 5, 13, W // 2 + 1) and rs.power.shape == (1, 1, 4, W // 2 + 1)
    assert ru.k.tolist() == list(range(W // 2 + 1)) and ru.bands is None
    for res, t in ((ru, up), (rs, sf)):
        want = P.score.weighted_rmse_channels(t, torch.zeros_like(t)).double() ** 2
        got = res.power.double().sum(-1)[:, 0]
        assert ((got - want).abs() / want).max().item() <= SCORE_RTOL
    # and without the offset, where the anomaly carries the sum
    a = (x[:1] - np.float32(300.0)).astype(np.float32)
    up, sf = _split(a)
    ru, rs = P.score.zonal_spectrum(up, sf)
    for res, t in ((ru, up), (rs, sf)):
        want = P.score.weighted_rmse_channels(t, torch.zeros_like(t)).double() ** 2
        assert ((res.power.double().sum(-1)[:, 0] - want).abs() / want).max().item() <= SCORE_RTOL


@pytest.mark.parametrize("H,W", SHAPES)
def test_bitwise_identities(H, W, monkeypatch):
    """kmax < W/2 = the first columns; N = 3 strided = three N = 1 calls; minus = the spectrum of the explicit difference; two
    runs agree -- all bit for bit."""
    import pangu_pytorch_amd as P
    x, minus, bw = _case(H, W)
    bands = torch.from_numpy(bw)
    zs = P.score.zonal_spectrum
    up, sf = _split(x)
    mu, ms = _split(minus)
    full = _joined(*zs(up, sf, mu, ms, bands=bands))
    assert np.array_equal(_bits(full), _bits(_joined(*zs(up, sf, mu, ms, bands=bands))))
    kmax = max(1, W // 4)
    assert np.array_equal(_bits(_joined(*zs(up, sf, mu, ms, bands=bands, kmax=kmax))), _bits(full[..., :kmax + 1]))
    # members of a larger buffer: an item stride beyond one item
    big_u = torch.full((3, up[0].numel() + 8), float("nan"), device="cuda")
    big_s = torch.full((3, sf[0].numel() + 4), float("nan"), device="cuda")
    vu, vs = big_u[:, :up[0].numel()].view(up.shape), big_s[:, :sf[0].numel()].view(sf.shape)
    vu.copy_(up)
    vs.copy_(sf)
    assert vu.stride(0) == up[0].numel() + 8 and not vu.is_contiguous()
    strided = _joined(*zs(vu, vs, mu, ms, bands=bands))
    assert np.array_equal(_bits(strided), _bits(full))
    for i in range(3):
        one = _joined(*zs(up[i:i + 1], sf[i:i + 1], mu, ms, bands=bands))
        assert np.array_equal(_bits(one), _bits(full[i:i + 1])), i
    diff = _joined(*zs(up - mu, sf - ms, bands=bands))
    assert np.array_equal(_bits(diff), _bits(full))
    # N split over several launches (what keeps the workspace under SPECTRUM_WS_LIMIT at E = 128, B = 4): here one item each
    monkeypatch.setattr(P.score, "SPECTRUM_WS_LIMIT", 1)
    assert np.array_equal(_bits(_joined(*zs(vu, vs, mu, ms, bands=bands))), _bits(full))


@pytest.mark.parametrize("H,W", SHAPES)
def test_bands(H, W):
    import pangu_pytorch_amd as P
    x, _, _ = _case(H, W)
    g = P.score.spectrum_band_weights(H).numpy()[0]
    cut = H // 3
    south, north = g.copy(), g.copy()
    south[:cut] = 0
    north[cut:] = 0                                                    # two disjoint bands whose weights add to the global row
    bw = np.stack([g, north, np.zeros_like(g), south]).astype(np.float32)
    got = _spectrum(P, x[:1], None, torch.from_numpy(bw))
    assert (got[:, 2] == 0).all()                                      # an all-zero band: exact zeros
    # every P_k is a sum of non-negative terms: each band sum is within (H + 2) roundings of its own value
    assert (np.abs(got[:, 1].astype(np.float64) + got[:, 3] - got[:, 0]) <= (H + 4) * 2.0 ** -24 * got[:, 0]).all()
    # the named bands of spectrum_band_weights
    named = [(-90, 0), (0, 90), (-30, 30)]
    res = P.score.zonal_spectrum(*_split(x[:1]), bands=named)
    assert res[0].bands == tuple((float(s), float(n)) for s, n in named) and res[0].power.shape[1] == 3
    _check(_joined(*res), x[:1], None, P.score.spectrum_band_weights(H, named).numpy(), W // 2, f"({H}, {W}) named bands")


@pytest.mark.parametrize("H,W", SHAPES)
def test_nan_stays_in_its_bands_and_plane(H, W):
    import pangu_pytorch_amd as P
    x, _, _ = _case(H, W)
    x = x[:2].copy()
    x[0, 7, 5, 3] = np.nan                                             # somewhere in a row
    x[1, 66, 2, 0] = np.nan                                            # the pivot of a row (a surface plane)
    bw = band_rows(H, 4, seed=9)
    bw[1, 5] = 0.0                                                     # band 1 does not see row 5, band 2 sees nothing
    bw[2] = 0.0
    bw[3, 2] = 0.0                                                     # band 3 does not see row 2
    got = _spectrum(P, x, None, torch.from_numpy(bw))
    want_nan = np.zeros(got.shape[:3], dtype=bool)                     # (N, B, planes)
    want_nan[0, [0, 3], 7] = True
    want_nan[1, [0, 1], 66] = True
    assert np.array_equal(np.isnan(got).all(-1), want_nan)             # every wavenumber of those entries
    assert np.isfinite(got[~want_nan]).all()                           # and nothing else
    assert (got[:, 2] == 0).all()


# ---- EnsembleRollout.spectra -----------------------------------------------------------------------------------------------------

def test_ensemble_rollout_spectra():
    import pangu_pytorch_amd as P
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    tu, ts = cases.model_targets("cuda")
    sl = _stats_last(stats)
    E, K, bands = 3, 90, [(-90, 90), (-20, 20)]
    ens = P.ensemble.EnsembleRollout(m, inp, inp_s, stats, maps, const_h, sl, members=E, amplitude=0.05, seed=3)
    ens.step()
    assert sorted(ens.spectra(kmax=K)) == ["mean", "members"]
    with pytest.raises(ValueError):
        ens.spectra(target=tu)
    sp = ens.spectra(tu, ts, bands=bands, kmax=K)
    assert sorted(sp) == ["error", "mean", "members", "target"]
    for pair in sp.values():
        assert pair[0].power.shape == (1, 2, 5, 13, K + 1) and pair[1].power.shape == (1, 2, 4, K + 1)
        assert pair[0].bands == ((-90.0, 90.0), (-20.0, 20.0)) and pair[0].k.tolist() == list(range(K + 1))
    up, sf = ens.state()
    (mu, ms), _ = ens.mean_std()
    per_member = P.score.zonal_spectrum(up, sf, bands=bands, kmax=K)
    explicit = P.score.zonal_spectrum((mu - tu[0])[None], (ms - ts[0])[None], bands=bands, kmax=K)
    for i in range(2):
        assert per_member[i].power.shape[0] == E
        assert torch.equal(sp["members"][i].power, per_member[i].power.double().mean(0, keepdim=True))
        assert torch.equal(sp["error"][i].power, explicit[i].power)
        # the mean of the members cannot carry more anomaly power than the members do on average (Jensen, per wavenumber); each
        # side carries at most the kernel's error bound, 4e-6 of its anomaly power at W = 1440
        assert bool((sp["mean"][i].variance() <= sp["members"][i].variance() * (1 + 1e-5)).all())
        er = sp["mean"][i].effective_resolution(sp["members"][i])
        assert er.dtype == torch.int64 and er.shape == sp["mean"][i].power.shape[:-1] and int(er.min()) >= 1 and int(er.max()) <= K + 1
