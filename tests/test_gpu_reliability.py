"""The ensemble reliability kernel on the GPU against the integer numpy restatement of its definitions
(test_reliability_cpu.reliability_ref): counts for exact equality, the weighted tables and the probability fields within their
fp32 rounding bounds; and the wiring into EnsembleRollout / ensemble_rollout."""
import numpy as np
import pytest
import torch

import cases
import synth
from test_gpu_ensemble import _stats_last
from test_reliability_cpu import reliability_ref

pytestmark = pytest.mark.gpu

# freq against the float64 weighted sum of the reference counts (same fp32 weights), relative to its magnitude.  A 4-row slab
# partial is a chain of 4 fmaf (4 roundings), the slabs are added in double and the result is rounded to fp32 once: below
# 6 * 2^-24 = 3.6e-7 of the sum of the terms' magnitudes.  The terms are >= 0 except in the two pole rows, where the project's
# weights are about -4e-6 of a mid-latitude row's (latitude_weights keeps the reference's 3.1416 for pi, so cos(lat) is just
# below zero there): a bin whose points all lie in a pole row has a small negative frequency, and with the random fields used here a bin
# that mixes a pole row with other rows loses at most parts in a thousand of its sum to cancellation.  The bound asserted is 2e-6.
FREQ_RTOL = 2e-6
PROB_ATOL = 1.2e-7      # a correctly rounded fp32 quotient k / E <= 1: half an ulp, 6e-8


def _data(E, H, W, T, seed, step=None, inf_rows=True):
    """upper (E,5,13,H,W), surface (E,4,H,W), targets, thresholds ((T,5,13), (T,4)) or None, on the device."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g, device="cuda")
    up, sf, tu, ts = r(E, 5, 13, H, W), r(E, 4, H, W), r(5, 13, H, W), r(4, H, W)
    if step:
        up, sf, tu, ts = (torch.round(t / step) * step for t in (up, sf, tu, ts))
    thr = None
    if T:
        thr = (torch.rand((T, 5, 13), generator=g, device="cuda") * 2 - 1, torch.rand((T, 4), generator=g, device="cuda") * 2 - 1)
        if step:
            thr = tuple(torch.round(t / step) * step for t in thr)        # thresholds that members and targets hit exactly
        if inf_rows:
            thr[0][T - 1, 2, 5:] = float("inf")                            # "no event on this plane"
            thr[1][T - 1, 1] = float("inf")
    return up.contiguous(), sf.contiguous(), tu.contiguous(), ts.contiguous(), thr


def _ref(x, y, thr, w, seed, first_plane):
    """reliability_ref on device tensors x (E, *p, H, W), y (*p, H, W) or None, thr (T, *p) or None."""
    E, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    xn = x.reshape(E, -1, H, W).cpu().numpy()
    yn = None if y is None else y.reshape(-1, H, W).cpu().numpy()
    tn = None if thr is None else thr.reshape(thr.shape[0], -1).cpu().numpy()
    return reliability_ref(xn, yn, tn, w, seed, first_plane)


def _raw(tab):
    """(counts, freq) of a ReliabilityTables back in the reference's layout (planes, 1 + 2T, E+1), as numpy."""
    E, T = tab.E, tab.T
    out = []
    for rank, ev, ob in ((tab.rank_counts, tab.event_counts, tab.observed_counts), (tab.rank_freq, tab.event_freq, tab.observed_freq)):
        a = np.zeros((rank.numel() // (E + 1), 1 + 2 * T, E + 1), dtype=np.float64 if rank.is_floating_point() else np.int64)
        a[:, 0] = rank.reshape(-1, E + 1).cpu().numpy()
        if T:
            a[:, 1::2] = ev.reshape(T, -1, E + 1).transpose(0, 1).cpu().numpy()
            a[:, 2::2] = ob.reshape(T, -1, E + 1).transpose(0, 1).cpu().numpy()
        out.append(a)
    return out


def _check(tab, ref, what):
    counts, freq = _raw(tab)
    assert tab.rank_counts.dtype == torch.int64 and tab.rank_freq.dtype == torch.float32
    assert np.array_equal(counts, ref["counts"]), what
    err, mag = np.abs(freq - ref["freq"]), np.abs(ref["freq"])
    rel = (err[mag > 0] / mag[mag > 0]).max()
    print(f"{what}: freq max rel err {rel:.3e}")
    assert (err <= FREQ_RTOL * mag).all(), (what, rel)          # an empty bin is exactly 0
    if tab.prob is not None:
        H, W = tab.prob.shape[-2:]
        perr = np.abs(tab.prob.reshape(tab.T, -1, H, W).double().cpu().numpy() - ref["prob"]).max()
        print(f"{what}: prob max abs err {perr:.3e}")
        assert perr <= PROB_ATOL, (what, perr)


def _weights(P, H):
    return P.score.latitude_weights(H, "cuda").cpu().numpy()


def _same(a, b, prob=True):
    fields = ("rank_counts", "rank_freq", "event_counts", "event_freq", "observed_counts", "observed_freq") + (("prob",) if prob else ())
    return (a.E, a.T) == (b.E, b.T) and all(torch.equal(getattr(a, f), getattr(b, f)) for f in fields)


@pytest.mark.parametrize("W", [24, 260])
@pytest.mark.parametrize("T", [0, 1, 4])
@pytest.mark.parametrize("E", [2, 5, 33, 128])
def test_small_grid_matches_restatement(E, T, W):
    """H = 9: a slab tail of one row; W = 24 is narrower than a workgroup, 4 * 260 / 4 = 260 float4 columns per row pass 256
    threads without being a multiple; all 69 planes; E on and off the member unroll."""
    import pangu_pytorch_amd as P
    H = 9
    up, sf, tu, ts, thr = _data(E, H, W, T, 1000 * E + 10 * T + W)
    ru, rs = P.score.ensemble_reliability(up, sf, tu, ts, thr, seed=17, want_fields=True)
    assert (ru.E, ru.T, rs.E, rs.T) == (E, T, E, T)
    assert ru.rank_counts.shape == (5, 13, E + 1) and rs.event_counts.shape == (T, 4, E + 1)
    assert (ru.prob is None) == (T == 0) and (T == 0 or (ru.prob.shape == (T, 5, 13, H, W) and rs.prob.shape == (T, 4, H, W)))
    w = _weights(P, H)
    _check(ru, _ref(up, tu, thr and thr[0], w, 17, 0), f"upper E={E} T={T} W={W}")
    _check(rs, _ref(sf, ts, thr and thr[1], w, 17, 65), f"surface E={E} T={T} W={W}")


@pytest.mark.parametrize("E", [4, 33])
def test_ties_are_broken_as_restated(E):
    import pangu_pytorch_amd as P
    H, W, T = 9, 260, 2
    up, sf, tu, ts, thr = _data(E, H, W, T, E, step=0.5, inf_rows=False)
    up[:, :, :, 2:6, 40:200] = tu[:, :, 2:6, 40:200]              # a block where every member equals the target
    sf[:, :, 2:6, 40:200] = ts[:, 2:6, 40:200]
    w = _weights(P, H)
    ru, rs = P.score.ensemble_reliability(up, sf, tu, ts, thr, seed=5)
    ref_u, ref_s = _ref(up, tu, thr[0], w, 5, 0), _ref(sf, ts, thr[1], w, 5, 65)
    assert ((up == tu).sum(0) >= 2).any() and (ref_u["counts"][:, 0] > 0).all()       # ties are common, every rank is hit
    _check(ru, ref_u, "upper ties")
    _check(rs, ref_s, "surface ties")
    # another seed: another rank table, the same event tables
    ru2, rs2 = P.score.ensemble_reliability(up, sf, tu, ts, thr, seed=6)
    _check(ru2, _ref(up, tu, thr[0], w, 6, 0), "upper ties, seed 6")
    assert not torch.equal(ru2.rank_counts, ru.rank_counts) and not torch.equal(rs2.rank_counts, rs.rank_counts)
    for f in ("event_counts", "event_freq", "observed_counts", "observed_freq"):
        assert torch.equal(getattr(ru2, f), getattr(ru, f)) and torch.equal(getattr(rs2, f), getattr(rs, f))
    # the surface planes hash as planes 65..68: the low-level call on the same data with first_plane = 65, not 0
    low65 = P.score._reliability(sf, ts, thr[1], T, 5, 65, False, "surface as planes 65..")
    low0 = P.score._reliability(sf, ts, thr[1], T, 5, 0, False, "surface as planes 0..")
    assert _same(low65, rs, prob=False) and not torch.equal(low0.rank_counts, rs.rank_counts)
    assert torch.equal(low0.event_counts, rs.event_counts)
    _check(low0, _ref(sf, ts, thr[1], w, 5, 0), "surface data hashed as planes 0..3")


def test_forecast_mode_keeps_event_tables_and_fields():
    import pangu_pytorch_amd as P
    E, H, W, T = 7, 9, 260, 3
    up, sf, tu, ts, thr = _data(E, H, W, T, 3)
    ver = P.score.ensemble_reliability(up, sf, tu, ts, thr, want_fields=True)
    fc = P.score.ensemble_reliability(up, sf, None, None, thr, want_fields=True)
    w = _weights(P, H)
    _check(fc[0], _ref(up, None, thr[0], w, 0, 0), "upper forecast mode")
    for v, f in zip(ver, fc):
        assert not f.rank_counts.any() and not f.rank_freq.any() and not f.observed_counts.any() and not f.observed_freq.any()
        assert torch.equal(f.event_counts, v.event_counts) and torch.equal(f.event_freq, v.event_freq)
        assert torch.equal(f.prob, v.prob)
        assert v.observed_counts.any()


def test_repeat_launches_are_bit_identical():
    import pangu_pytorch_amd as P
    up, sf, tu, ts, thr = _data(33, 9, 260, 4, 4, step=0.5)
    a = P.score.ensemble_reliability(up, sf, tu, ts, thr, seed=2, want_fields=True)
    b = P.score.ensemble_reliability(up, sf, tu, ts, thr, seed=2, want_fields=True)
    assert _same(a[0], b[0]) and _same(a[1], b[1])


def test_full_grid_surface_exact_counts_and_conservation():
    import pangu_pytorch_amd as P
    E, H, W, T = 4, 721, 1440, 1
    g = torch.Generator(device="cuda").manual_seed(9)
    sf = torch.round(torch.randn((E, 4, H, W), generator=g, device="cuda") * 8) / 8          # ties now and then
    ts = torch.round(torch.randn((4, H, W), generator=g, device="cuda") * 8) / 8
    thr = torch.tensor([[0.25, -0.5, 1.0, float("inf")]], device="cuda")
    tab = P.score._reliability(sf, ts, thr, T, 21, 65, True, "full-grid surface")
    _check(tab, _ref(sf, ts, thr, _weights(P, H), 21, 65), "full-grid surface")
    assert (tab.rank_counts.sum(-1) == 1038240).all() and (tab.event_counts.sum(-1) == 1038240).all()
    assert (tab.event_counts[0, 3, 0] == 1038240) and not tab.observed_counts[0, 3].any()     # +inf: no event on the plane


# ---- wiring --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup():
    import pangu_pytorch_amd as P
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return P, m, cases.model_inputs("cuda")


def test_rollout_fills_the_accumulator_and_leaves_the_state_alone(setup):
    P, m, (inp, inp_s, stats, maps, const_h) = setup
    sl = _stats_last(stats)
    tu, ts = cases.model_targets("cuda")
    targets = [(tu, ts), (inp, inp_s)]
    thr = (torch.stack([tu[0].mean((-2, -1)), inp[0].mean((-2, -1)) + 0.1]),
           torch.stack([ts[0].mean((-2, -1)), inp_s[0].mean((-2, -1)) + 0.1]))
    kw = dict(members=3, amplitude=0.05, steps=2, seed=11, chunk=2)
    acc = P.score.ReliabilityAccumulator(2)
    up, sf, hist = P.ensemble.ensemble_rollout(m, inp, inp_s, stats, maps, const_h, sl, targets=targets, reliability=acc,
                                               thresholds=thr, **kw)
    up, sf = up.clone(), sf.clone()
    up0, sf0, hist0 = P.ensemble.ensemble_rollout(m, inp, inp_s, stats, maps, const_h, sl, targets=targets, **kw)
    assert torch.equal(up, up0) and torch.equal(sf, sf0)
    assert all(torch.equal(a[k], b[k]) for ha, hb in zip(hist, hist0) for a, b in zip(ha, hb) for k in a)
    ens = P.ensemble.EnsembleRollout(m, inp, inp_s, stats, maps, const_h, sl, members=3, amplitude=0.05, seed=11, chunk=2)
    for lead in range(2):
        ens.step()
        u, s = (t.clone() for t in ens.state())
        direct = P.score.ensemble_reliability(u, s, *targets[lead], thresholds=thr, seed=11, want_fields=True)
        assert acc.cases(lead) == 1
        for pooled, d in zip(acc.tables(lead), direct):
            assert (pooled.E, pooled.T) == (3, 2)
            for f in ("rank_counts", "event_counts", "observed_counts"):
                assert torch.equal(getattr(pooled, f), getattr(d, f))
            for f in ("rank_freq", "event_freq", "observed_freq"):
                assert torch.equal(getattr(pooled, f), getattr(d, f).double())
            assert int(d.rank_counts.sum()) == d.rank_counts[..., 0].numel() * 721 * 1440
        via = ens.reliability(*targets[lead], thresholds=thr, seed=11)
        assert _same(via[0], direct[0], prob=False) and _same(via[1], direct[1], prob=False)
        pu, ps = ens.exceedance(thr)
        assert torch.equal(pu, direct[0].prob) and torch.equal(ps, direct[1].prob) and pu.shape == (2, 5, 13, 721, 1440)
    assert torch.equal(ens.state()[0], up) and torch.equal(ens.state()[1], sf)
