"""The ensemble quantile kernel on the GPU against the numpy restatement of its definition (test_quantiles_cpu.quantiles_ref):
selections bit for bit, interpolated levels within their fp32 rounding bound, the scores against float64, and the wiring into
EnsembleRollout / ensemble_rollout / HostDrain.

Shapes: H = 9 (a slab tail of one row), W = 24 (narrower than a workgroup) and W = 260 (a slab of 1040 points: 4 passes of 256
threads and a ragged fifth), all 69 planes."""
import numpy as np
import pytest
import torch

import cases
import synth
from test_gpu_ensemble import _stats_last
from test_quantiles_cpu import calibration_case, quantiles_ref

pytestmark = pytest.mark.gpu

H = 9
LEVELS = (0.0, 0.1, 0.5, 0.5, 0.9, 1.0)          # a duplicate; q = 0, q = 1 and (odd E) the median are selections
# an interpolated value is fmaf(frac, b - a, a): one rounding of the difference (|b - a| <= 2 max(|a|, |b|), scaled by frac < 1)
# and one of the fma (a result inside the bracket), each 2^-24 relative: below 3 * 2^-24 * max(|a|, |b|)
INTERP_BOUND = 3 * 2.0 ** -24
SCORE_RTOL = 1e-5                                # the tolerance of tests/test_gpu_ensemble.py for the sibling per-plane scores


def _data(E, W, seed, target=True, step=None):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g, device="cuda")
    up, sf = r(E, 5, 13, H, W), r(E, 4, H, W)
    tu, ts = (r(5, 13, H, W), r(4, H, W)) if target else (None, None)
    if step:                                     # + 0.0: no negative zeros (which zero a selection among equal zeros returns is open)
        up, sf = (torch.round(t / step) * step + 0.0 for t in (up, sf))
    return up.contiguous(), sf.contiguous(), tu, ts


def _weights(P):
    return P.score.latitude_weights(H, "cuda").cpu().numpy()


def _ref(x, q, y=None, w=None):
    E, W = x.shape[0], x.shape[-1]
    return quantiles_ref(x.reshape(E, -1, H, W).cpu().numpy(), q, None if y is None else y.reshape(-1, H, W).cpu().numpy(), w)


def _fields(res):
    """(Q, planes, H, W) float32 numpy of a QuantileResult."""
    f = res.fields
    return f.reshape(f.shape[0], -1, f.shape[-2], f.shape[-1]).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check_fields(got, ref, q, what):
    """Selections bit for bit, interpolations within INTERP_BOUND of the bracket's magnitude, inside the bracket, monotone in q."""
    assert got.dtype == np.float32 and got.shape == ref["fields"].shape
    for l, fr in enumerate(ref["frac"]):
        a, b, want = ref["a"][l], ref["b"][l], ref["fields"][l]
        if fr == 0:
            assert np.array_equal(_bits(got[l]), _bits(want)), (what, l)
        else:
            fin = np.isfinite(want)                  # an infinite bracket end gives an infinite value: equal, not close
            err = np.abs(got[l][fin].astype(np.float64) - want[fin])
            bound = INTERP_BOUND * np.maximum(np.abs(a), np.abs(b))[fin]
            print(f"{what} level {q[l]}: worst interpolation error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert (err <= bound).all(), (what, l)
            assert np.array_equal(got[l][~fin], want[~fin].astype(np.float32)), (what, l)
        assert ((got[l] >= a) & (got[l] <= b)).all(), (what, l)
    for i in range(len(q)):
        for j in range(len(q)):
            if q[i] <= q[j]:
                assert (got[i] <= got[j]).all(), (what, i, j)


def _check_scores(res, ref, what):
    Q = len(res.q)
    assert res.coverage_counts.dtype == torch.int64 and res.pinball.dtype == torch.float32
    cnt = res.coverage_counts.reshape(Q, -1).cpu().numpy()
    for l, fr in enumerate(ref["frac"]):
        if fr == 0:                              # the kernel's field equals the restatement's there, so the counts must too
            assert np.array_equal(cnt[l], ref["coverage_counts"][l]), (what, l)
    for name in ("pinball", "coverage_freq"):
        got, want = getattr(res, name).reshape(Q, -1).double().cpu().numpy(), ref[name]
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(f"{what}: {name} max err / max |ref| = {rel:.3e}")
        assert rel <= SCORE_RTOL, (what, name, rel)


def _same(a, b, fields=True):
    names = ("pinball", "coverage_counts", "coverage_freq", "nonfinite") + (("fields",) if fields else ())
    return a.q == b.q and all(torch.equal(getattr(a, n), getattr(b, n)) for n in names)


@pytest.mark.parametrize("W", [24, 260])
@pytest.mark.parametrize("E", [2, 3, 5, 33, 64, 128])
def test_fields_match_restatement(E, W):
    """E on and off the power-of-two padding of the sorting network, forecast mode (no target)."""
    import pangu_pytorch_amd as P
    up, sf, _, _ = _data(E, W, 1000 * E + W, target=False)
    ru, rs = P.score.ensemble_quantiles(up, sf, LEVELS)
    assert ru.q == LEVELS and ru.fields.shape == (6, 5, 13, H, W) and rs.fields.shape == (6, 4, H, W)
    assert ru.pinball is None and ru.coverage_counts is None and ru.coverage_freq is None
    assert ru.nonfinite.shape == (5, 13) and not ru.nonfinite.any() and not rs.nonfinite.any()
    _check_fields(_fields(ru), _ref(up, LEVELS), LEVELS, f"upper E={E} W={W}")
    _check_fields(_fields(rs), _ref(sf, LEVELS), LEVELS, f"surface E={E} W={W}")


@pytest.mark.parametrize("E", [5, 8, 33])
def test_ties_and_extremes(E):
    """Members on a 0.5 grid (ties are common), a block where all members are equal, and a block with a +inf and a -inf member:
    q = 0, q = 1 and the odd-E median stay bit-exact selections, and nothing becomes NaN."""
    import pangu_pytorch_amd as P
    W = 260
    q = (0.0, 0.1, 0.5, 0.9, 1.0)
    up, sf, _, _ = _data(E, W, E, target=False, step=0.5)
    up[:, :, :, 2:5, 40:120] = up[0, :, :, 2:5, 40:120]
    sf[:, :, 2:5, 40:120] = sf[0, :, 2:5, 40:120]
    up[1, :, :, 5:8, 130:250], up[E - 2, :, :, 5:8, 130:250] = float("inf"), float("-inf")
    sf[1, :, 5:8, 130:250], sf[E - 2, :, 5:8, 130:250] = float("inf"), float("-inf")
    assert ((up[1:] == up[:1]).sum(0) >= 1).float().mean() > 0.3          # ties are common
    for x, res, what in zip((up, sf), P.score.ensemble_quantiles(up, sf, q), ("upper", "surface")):
        got, ref = _fields(res), _ref(x, q)
        assert not np.isnan(got).any() and not res.nonfinite.any()
        exact = [l for l, fr in enumerate(ref["frac"]) if fr == 0]
        assert 0 in exact and 4 in exact and ((E % 2 == 0) or 2 in exact)
        _check_fields(got, ref, q, f"{what} ties E={E}")
        xs = np.sort(x.reshape(E, -1, H, W).cpu().numpy(), axis=0)
        assert np.array_equal(_bits(got[0]), _bits(xs[0])) and np.array_equal(_bits(got[4]), _bits(xs[E - 1]))
        assert np.isneginf(got[0][:, 5:8, 130:250]).all() and np.isposinf(got[4][:, 5:8, 130:250]).all()
        blk = got[:, :, 2:5, 40:120]                                         # all members equal: every level returns that value
        assert all(np.array_equal(_bits(blk[l]), _bits(xs[0][:, 2:5, 40:120])) for l in range(len(q)))


def test_nan_rule():
    """A handful of points NaN in one member: NaN in every field there, counted per plane, left out of the scores."""
    import pangu_pytorch_amd as P
    E, W = 5, 260
    q = (0.0, 0.25, 0.5, 1.0)
    up, sf, tu, ts = _data(E, W, 77)
    pts_u = [(0, 0, 0, 0, 0), (3, 0, 0, 8, 259), (1, 2, 5, 4, 100), (4, 2, 5, 4, 101), (2, 4, 12, 8, 0)]
    pts_s = [(4, 1, 3, 17), (0, 3, 8, 256), (2, 3, 8, 257), (1, 3, 0, 3)]
    for p in pts_u:
        up[p] = float("nan")
    for p in pts_s:
        sf[p] = float("nan")
    up[2, 2, 5, 4, 100] = float("nan")                                       # a second NaN at a point already hit: one point
    w = _weights(P)
    ru, rs = P.score.ensemble_quantiles(up, sf, q, tu, ts)
    want_u = torch.zeros(5, 13, dtype=torch.int64)
    for _, v, z, _, _ in pts_u:
        want_u[v, z] += 1
    assert torch.equal(ru.nonfinite.cpu(), want_u) and rs.nonfinite.tolist() == [0, 1, 0, 3]
    for x, y, res, what in ((up, tu, ru, "upper"), (sf, ts, rs, "surface")):
        got, ref = _fields(res), _ref(x, q, y, w)
        assert np.array_equal(np.isnan(got), np.isnan(ref["fields"]))
        assert np.isnan(got).sum() == len(q) * int(res.nonfinite.sum())
        assert np.array_equal(res.nonfinite.reshape(-1).cpu().numpy(), ref["nonfinite"])
        ok = ~np.isnan(got)
        assert np.array_equal(_bits(got[0][ok[0]]), _bits(ref["fields"][0][ok[0]]))
        _check_scores(res, ref, f"{what} with NaN points")
        own = (y.reshape(-1, H, W)[None] <= res.fields.reshape(len(q), -1, H, W)).sum((-2, -1))      # NaN compares false
        assert torch.equal(res.coverage_counts.reshape(len(q), -1), own)
        assert np.isfinite(res.pinball.cpu().numpy()).all()


@pytest.mark.parametrize("E,W", [(3, 24), (33, 260), (50, 260), (128, 260)])
def test_scores(E, W):
    import pangu_pytorch_amd as P
    q = (0.0, 0.1, 0.5, 0.9, 1.0)
    up, sf, tu, ts = _data(E, W, 31 * E + W)
    w = _weights(P)
    full = P.score.ensemble_quantiles(up, sf, q, tu, ts)
    again = P.score.ensemble_quantiles(up, sf, q, tu, ts)
    bare = P.score.ensemble_quantiles(up, sf, q, tu, ts, want_fields=False)
    for x, y, res, res2, res3, what in zip((up, sf), (tu, ts), full, again, bare, ("upper", "surface")):
        Q = len(q)
        assert res.pinball.shape == res.fields.shape[:-2] == res.coverage_counts.shape == res.coverage_freq.shape
        # coverage against the very fp32 values the kernel wrote
        own = (y.reshape(-1, H, W)[None] <= res.fields.reshape(Q, -1, H, W)).sum((-2, -1))
        assert torch.equal(res.coverage_counts.reshape(Q, -1), own)
        assert int(res.coverage_counts[-1].min()) >= 0 and (res.coverage_counts[0] <= res.coverage_counts[-1]).all()
        ref = _ref(x, q, y, w)
        _check_fields(_fields(res), ref, q, f"{what} E={E} W={W}")
        _check_scores(res, ref, f"{what} E={E} W={W}")
        assert _same(res, res2)                                              # bit-identical from call to call
        assert res3.fields is None and _same(res, res3, fields=False)        # and with or without the fields
        iv = res.interval(1, 3)
        assert torch.equal(iv["coverage"], res.coverage_freq[3].double() - res.coverage_freq[1].double())
        d = (res.fields[3] - res.fields[1]).double() * torch.from_numpy(w).cuda().double()[:, None]
        assert torch.allclose(iv["width"], d.mean((-2, -1)), rtol=1e-12) and (iv["width"] > 0).all()


def test_calibration_sanity():
    """E = 33 members and a target from the same N(0, 1): the median covers half of the 161 460 points (binomial sigma 0.0012; the
    odd-E median is a selection, without the finite-E bias of an interpolated level).  The same draw goes through the restatement
    in test_quantiles_cpu.test_calibration_margin_of_the_gpu_case_on_the_cpu."""
    import pangu_pytorch_amd as P
    x, y, _ = calibration_case()
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    up, sf = x[:, :65].reshape(33, 5, 13, H, 260).contiguous(), x[:, 65:].contiguous()
    ru, rs = P.score.ensemble_quantiles(up, sf, (0.5,), y[:65].reshape(5, 13, H, 260).contiguous(), y[65:].contiguous(),
                                        want_fields=False)
    freq = torch.cat([ru.coverage_freq.reshape(-1), rs.coverage_freq.reshape(-1)]).double().mean().item()
    share = (int(ru.coverage_counts.sum()) + int(rs.coverage_counts.sum())) / (69 * H * 260)
    print(f"pooled median coverage: weighted {freq:.5f}, counted {share:.5f}")
    assert abs(freq - 0.5) < 0.02 and abs(share - 0.5) < 0.02


# ---- wiring --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup():
    import pangu_pytorch_amd as P
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return P, m, cases.model_inputs("cuda")


def _drained(drain, n_fields, last_tag):
    """[(tag, float32 numpy copies of the fields, for the item tagged last_tag only)] of everything a sink-less drain holds, and
    that item's (scale_offset, nonfinite) per field (None in mode "float32")."""
    out, raw = [], None
    for item in drain:
        assert len(item.fields) == n_fields
        if item.tag == last_tag:
            raw = [(None if f.scale_offset is None else f.scale_offset.copy(), None if f.nonfinite is None else f.nonfinite.copy())
                   for f in item.fields]
        out.append((item.tag, item.to_float32() if item.tag == last_tag else None))
    return out, raw


@pytest.mark.timeout(600)
def test_rollout_delivers_products_and_quantile_scores(setup):
    P, m, (inp, inp_s, stats, maps, const_h) = setup
    sl = _stats_last(stats)
    tu, ts = cases.model_targets("cuda")
    targets = [(tu, ts), (inp, inp_s)]
    kw = dict(members=3, amplitude=0.05, steps=2, seed=11, chunk=2)
    q = (0.0, 0.5, 1.0)
    products = dict(mean_std=True, quantiles=q)
    names = P.ensemble.EnsembleRollout.product_names(**products)
    assert names == ["mean_upper", "mean_surface", "std_upper", "std_surface", "quantiles_upper", "quantiles_surface"]
    roll = lambda **extra: P.ensemble.ensemble_rollout(m, inp, inp_s, stats, maps, const_h, sl, **kw, **extra)

    # the parent's call: nothing new in the return value
    up0, sf0, hist0 = roll(targets=targets)
    up0, sf0 = up0.clone(), sf0.clone()
    assert len(hist0) == 2 and all(len(h) == 2 and set(h[0]) == set(P.score.ENSEMBLE_KEYS) == set(h[1]) for h in hist0)
    assert len(roll()) == 2

    # float32 drain + quantile scores in the history
    drain = P.data.HostDrain("cuda", mode="float32", depth=1)
    up, sf, hist = roll(targets=targets, drain=drain, products=products, quantile_levels=(0.1, 0.5, 0.9))
    items, _ = _drained(drain, len(names), 1)
    drain.close()
    assert torch.equal(up, up0) and torch.equal(sf, sf0)
    assert [tag for tag, _ in items] == [0, 1]
    for h, h0 in zip(hist, hist0):
        assert len(h) == 4 and all(torch.equal(h[i][k], h0[i][k]) for i in (0, 1) for k in h0[i])
        assert h[2].q == (0.1, 0.5, 0.9) and h[2].fields is None and h[2].pinball.shape == (3, 5, 13) and h[3].pinball.shape == (3, 4)
    direct = P.score.ensemble_quantiles(up, sf, (0.1, 0.5, 0.9), *targets[1], want_fields=False)
    assert _same(hist[1][2], direct[0], fields=False) and _same(hist[1][3], direct[1], fields=False)
    assert (hist[1][2].pinball > 0).all() and (hist[1][3].pinball > 0).all()

    last = dict(zip(names, (torch.from_numpy(a).cuda() for a in items[1][1])))
    med = P.score.ensemble_quantiles(up, sf, (0.5,))
    assert last["quantiles_upper"].shape == (3, 5, 13, 721, 1440) and last["quantiles_surface"].shape == (3, 4, 721, 1440)
    assert torch.equal(last["quantiles_upper"][1], med[0].fields[0]) and torch.equal(last["quantiles_surface"][1], med[1].fields[0])
    assert torch.equal(last["quantiles_upper"], torch.sort(up, 0).values)    # E = 3: (0, .5, 1) are the three order statistics
    assert torch.equal(last["quantiles_surface"], torch.sort(sf, 0).values)
    su, ss = P.score.ensemble_scores(up, sf, None, None, sl, want_fields=True)
    assert torch.equal(last["mean_upper"], su["mean"]) and torch.equal(last["std_surface"], ss["std"])
    del med, su, ss

    # the same products through the int16 pack: within the pack's documented quantisation step of the float32 delivery
    drain = P.data.HostDrain("cuda", mode="int16", depth=1)
    up2, sf2 = roll(drain=drain, products=products)
    items16, raw = _drained(drain, len(names), 1)
    drain.close()
    assert torch.equal(up2, up0) and torch.equal(sf2, sf0) and [tag for tag, _ in items16] == [0, 1]
    for name, got, (so, nf) in zip(names, items16[1][1], raw):
        want = last[name]
        planes = so.shape[0]
        assert got.shape == tuple(want.shape) and nf.sum() == 0
        v = want.reshape(planes, -1).double()
        s = torch.from_numpy(so[:, 0].astype(np.float64)).cuda().view(-1, 1)
        err = (torch.from_numpy(got).cuda().reshape(planes, -1).double() - v).abs()
        # the pack's contract (include/pangu_hip.h) plus the two fp32 roundings of the host unpack q * scale + offset
        big = torch.maximum(v.min(1, keepdim=True).values.abs(), v.max(1, keepdim=True).values.abs())
        bound = 0.5 * s * (1 + 2.0 ** -10) + 6 * 2.0 ** -24 * big
        print(f"{name}: worst int16 |error| / bound = {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()), name


def test_rollout_object_products_follow_the_names(setup):
    """EnsembleRollout.products on a state set by hand (no model step): the list matches product_names in order and shape, and
    its entries are the tensors of mean_std / quantiles / exceedance."""
    P, m, (inp, inp_s, stats, maps, const_h) = setup
    sl = _stats_last(stats)
    ens = P.ensemble.EnsembleRollout(m, inp, inp_s, stats, maps, const_h, sl, members=3, amplitude=0.05, seed=3)
    thr = (inp[0].mean((-2, -1))[None], inp_s[0].mean((-2, -1))[None])
    args = dict(mean_std=True, quantiles=(0.25, 0.75), thresholds=thr)
    prods, names = ens.products(**args), ens.product_names(**args)
    assert len(prods) == len(names) == 8 and all(t.is_contiguous() and t.dtype == torch.float32 for t in prods)
    (mu, ms), (su, ss) = ens.mean_std()
    qu, qs = ens.quantiles((0.25, 0.75))
    pu, ps = ens.exceedance(thr)
    for got, want in zip(prods, (mu, ms, su, ss, qu, qs, pu, ps)):
        assert torch.equal(got, want)
    assert qu.shape == (2, 5, 13, 721, 1440) and (qu[0] <= qu[1]).all()
    only = ens.products(mean_std=False, quantiles=(0.5,))
    assert len(only) == 2 and only[0].shape == (1, 5, 13, 721, 1440)
    ru, rs = ens.quantile_scores(inp, inp_s, (0.5,))
    assert ru.fields is None and ru.pinball.shape == (1, 5, 13) and rs.coverage_freq.shape == (1, 4)
