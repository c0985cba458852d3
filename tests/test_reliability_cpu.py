"""CPU-side checks of the ensemble reliability surface: the integer numpy restatement of the kernel's definitions
(csrc/reliability.hip pins them; tests/test_gpu_reliability.py checks the kernel against reliability_ref for exact equality), the
derived quantities on CPU tensors, C-entry argument validation and Python refusals."""
import os

import numpy as np
import pytest
import torch

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib
from test_ensemble_cpu import lowbias32


def reliability_ref(x, y, thr, w, seed, first_plane):
    """x (E, planes, H, W) float32, y (planes, H, W) float32 or None, thr (T, planes) float32 or None, w (H,) float32.
    Per grid point of plane p, g = first_plane + p:
      less = #{i: x_i < y}, ties = #{i: x_i == y}, u = lowbias32(lowbias32(lowbias32(seed) ^ g) ^ (h*W + w)),
      rank = less + ((u * (ties + 1)) >> 32)  (uint64 product),  k_t = #{i: x_i > thr[t, p]},  o_t = y > thr[t, p].
    Returns counts (planes, 1 + 2T, E+1) int64 [table 0: rank; 1 + 2t: N_t by k_t; 2 + 2t: O_t by k_t], freq (same shape,
    float64: points weighted by float64(w[h]), divided by H*W), prob (T, planes, H, W) float64 = k_t / E, rank (planes, H, W)
    int64 or None, k (T, planes, H, W) int64.  Comparisons are fp32 comparisons, as on the device."""
    x = np.asarray(x, dtype=np.float32)
    E, planes, H, W = x.shape
    T = 0 if thr is None else thr.shape[0]
    thr = None if thr is None else np.asarray(thr, dtype=np.float32)
    wfull = np.repeat(np.asarray(w, dtype=np.float32).astype(np.float64), W)           # (H*W,)
    counts = np.zeros((planes, 1 + 2 * T, E + 1), dtype=np.int64)
    freq = np.zeros((planes, 1 + 2 * T, E + 1), dtype=np.float64)
    k_all = np.zeros((T, planes, H, W), dtype=np.int64)
    rank_all = None if y is None else np.zeros((planes, H, W), dtype=np.int64)
    idx = np.arange(H * W, dtype=np.uint32)

    def tabulate(p, table, bins, mask=None):
        b = bins.reshape(-1) if mask is None else bins.reshape(-1)[mask.reshape(-1)]
        wt = wfull if mask is None else wfull[mask.reshape(-1)]
        counts[p, table] = np.bincount(b, minlength=E + 1)
        freq[p, table] = np.bincount(b, weights=wt, minlength=E + 1) / (H * W)

    for p in range(planes):
        if y is not None:
            yp = np.asarray(y[p], dtype=np.float32)
            less = (x[:, p] < yp).sum(0).astype(np.uint64)
            ties = (x[:, p] == yp).sum(0).astype(np.uint64)
            hp = lowbias32(lowbias32(seed) ^ np.uint32(first_plane + p))
            u = lowbias32(hp ^ idx).reshape(H, W).astype(np.uint64)
            rank = (less + ((u * (ties + np.uint64(1))) >> np.uint64(32))).astype(np.int64)
            rank_all[p] = rank
            tabulate(p, 0, rank)
        for t in range(T):
            k = (x[:, p] > thr[t, p]).sum(0).astype(np.int64)
            k_all[t, p] = k
            tabulate(p, 1 + 2 * t, k)
            if y is not None:
                tabulate(p, 2 + 2 * t, k, np.asarray(y[p], dtype=np.float32) > thr[t, p])
    return {"counts": counts, "freq": freq, "prob": k_all / float(E), "rank": rank_all, "k": k_all}


def _weights(H):
    return P.score.latitude_weights(H, "cpu").numpy()


def _case(E, planes, H, W, T, seed, step=None):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((E, planes, H, W)).astype(np.float32)
    y = rng.standard_normal((planes, H, W)).astype(np.float32)
    if step:
        x, y = np.round(x / step) * step, np.round(y / step) * step
    thr = rng.uniform(-1.0, 1.0, (T, planes)).astype(np.float32) if T else None
    return x.astype(np.float32), y.astype(np.float32), thr


# ---- the restatement itself ----------------------------------------------------------------------------------------

def test_ref_tables_conserve_points_and_observed_is_bounded():
    E, planes, H, W, T = 7, 3, 9, 24, 2
    x, y, thr = _case(E, planes, H, W, T, 0, step=0.5)
    r = reliability_ref(x, y, thr, _weights(H), 3, 0)
    assert (r["counts"][:, 0].sum(-1) == H * W).all()
    for t in range(T):
        assert (r["counts"][:, 1 + 2 * t].sum(-1) == H * W).all()
        assert (r["counts"][:, 2 + 2 * t] <= r["counts"][:, 1 + 2 * t]).all()
    # the project's weights average to 1 over the rows: the weighted tables sum to about 1
    assert np.allclose(r["freq"][:, 0].sum(-1), 1.0, atol=1e-6) and np.allclose(r["freq"][:, 1].sum(-1), 1.0, atol=1e-6)
    f = reliability_ref(x, None, thr, _weights(H), 3, 0)                     # forecast mode
    assert (f["counts"][:, 0::2] == 0).all() and (f["counts"][:, 1::2] == r["counts"][:, 1::2]).all()
    assert np.array_equal(f["prob"], r["prob"])


def test_ref_rank_equals_less_without_ties():
    E, planes, H, W = 5, 2, 9, 24
    x, y, _ = _case(E, planes, H, W, 0, 1)
    assert not (x == y).any()
    for seed in (0, 99):
        r = reliability_ref(x, y, None, _weights(H), seed, 65)
        assert np.array_equal(r["rank"], (x < y).sum(0))


def test_ref_full_ties_land_in_every_bin_uniformly():
    E, H, W = 4, 40, 100
    x = np.full((E, 1, H, W), 2.5, dtype=np.float32)
    y = np.full((1, H, W), 2.5, dtype=np.float32)
    r = reliability_ref(x, y, None, _weights(H), 7, 0)
    assert r["rank"].min() >= 0 and r["rank"].max() <= E
    c = r["counts"][0, 0]
    assert (c > 0).all() and c.sum() == H * W
    assert np.abs(c - H * W / (E + 1)).max() < 5 * np.sqrt(H * W / (E + 1))          # uniform within 5 sigma
    other = reliability_ref(x, y, None, _weights(H), 8, 0)
    assert not np.array_equal(other["rank"], r["rank"])                              # the seed matters
    plane1 = reliability_ref(x, y, None, _weights(H), 7, 1)
    assert not np.array_equal(plane1["rank"], r["rank"])                             # and so does the plane id


# ---- derived quantities on CPU tensors -----------------------------------------------------------------------------

def _tables(r, E, T, pshape):
    return P.score.ReliabilityTables.from_raw(torch.from_numpy(r["counts"]), torch.from_numpy(r["freq"]), E, T, pshape)


def test_brier_and_curve_from_tables_equal_direct_float64():
    E, H, W, T = 6, 9, 24, 3
    x, y, thr = _case(E, 4, H, W, T, 2, step=0.5)
    w = _weights(H)
    r = reliability_ref(x, y, thr, w, 0, 65)
    tab = _tables(r, E, T, (4,))
    assert tab.rank_counts.shape == (4, E + 1) and tab.event_counts.shape == (T, 4, E + 1) and tab.rank_counts.dtype == torch.int64
    o = (y[None] > thr[:, :, None, None]).astype(np.float64)
    direct = (w.astype(np.float64)[:, None] * (r["prob"] - o) ** 2).sum((-2, -1)) / (H * W)
    assert np.abs(tab.brier().numpy() - direct).max() <= 1e-12
    p, obs, share = tab.reliability_curve()
    assert np.array_equal(p.numpy(), np.arange(E + 1) / E)
    n, ob = r["freq"][:, 1::2].transpose(1, 0, 2), r["freq"][:, 2::2].transpose(1, 0, 2)
    assert np.array_equal(share.numpy(), n)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(obs.numpy(), ob / n, equal_nan=True)
    rf = tab.rank_frequencies().numpy()
    assert np.abs(rf.sum(-1) - 1.0).max() <= 1e-12 and np.allclose(rf, r["freq"][:, 0] / r["freq"][:, 0].sum(-1, keepdims=True))


def test_accumulator_adds_exactly_and_refuses_mixed_shapes():
    E, H, W, T = 5, 9, 24, 2
    w = _weights(H)
    cases = []
    for s in range(3):
        x, y, thr = _case(E, 69, H, W, T, 10 + s, step=0.5)
        ru = _tables(reliability_ref(x[:, :65], y[:65], thr[:, :65], w, s, 0), E, T, (5, 13))
        rs = _tables(reliability_ref(x[:, 65:], y[65:], thr[:, 65:], w, s, 65), E, T, (4,))
        cases.append((ru, rs))
    acc = P.score.ReliabilityAccumulator(2)
    assert acc.cases(0) == 0
    for ru, rs in cases:
        acc.add(0, ru, rs)
    acc.add(1, *cases[1])
    assert acc.cases(0) == 3 and acc.cases(1) == 1
    pu, ps = acc.tables(0)
    for pooled, i in ((pu, 0), (ps, 1)):
        for f in ("rank_counts", "event_counts", "observed_counts"):
            assert getattr(pooled, f).dtype == torch.int64
            assert torch.equal(getattr(pooled, f), sum(getattr(c[i], f) for c in cases))
        for f in ("rank_freq", "event_freq", "observed_freq"):
            assert getattr(pooled, f).dtype == torch.float64
            assert torch.equal(getattr(pooled, f), (getattr(cases[0][i], f) + getattr(cases[1][i], f)) + getattr(cases[2][i], f))
    # the pooled Brier score is the mean of the cases' scores; the pooled rank frequencies still sum to 1
    bu, bs = acc.brier(0)
    assert (bu - sum(c[0].brier() for c in cases) / 3).abs().max().item() <= 1e-12 and bs.shape == (T, 4)
    assert torch.equal(acc.brier(1)[0], cases[1][0].brier())
    assert (acc.rank_frequencies(0)[0].sum(-1) - 1).abs().max().item() <= 1e-12
    assert (acc.reliability_curve(0)[1][2].sum(-1) - 1).abs().max().item() <= 1e-5
    assert not torch.equal(cases[0][0].rank_counts, pu.rank_counts)          # the first case's tables were not adopted
    x, y, thr = _case(E + 1, 4, H, W, T, 0)
    other_e = _tables(reliability_ref(x, y, thr, w, 0, 65), E + 1, T, (4,))
    x, y, thr = _case(E, 4, H, W, T + 1, 0)
    other_t = _tables(reliability_ref(x, y, thr, w, 0, 65), E, T + 1, (4,))
    for bad in (other_e, other_t):
        with pytest.raises(ValueError, match="E = "):
            acc.add(1, cases[0][0], bad)
    with pytest.raises(ValueError, match="nothing added"):
        P.score.ReliabilityAccumulator(1).tables(0)


def test_spread_skill_ratio_formula():
    scores = {"spread": torch.tensor([1.0, 2.0, 0.5]), "rmse_mean": torch.tensor([2.0, 2.0, 0.25])}
    got = P.score.spread_skill_ratio(scores, 10)
    assert torch.allclose(got, (11.0 / 10.0) ** 0.5 * torch.tensor([0.5, 1.0, 2.0]), rtol=1e-7, atol=0)


def test_workspace_formula():
    # per (plane, slab of 4 rows): a uint32 count and a float partial per bin of the 1 + 2T tables
    assert P.score.reliability_workspace_bytes(69, 721, 50, 4) == 69 * 181 * 9 * 51 * 8
    assert P.score.reliability_workspace_bytes(4, 9, 2, 0) == 4 * 3 * 1 * 3 * 8


# ---- C entry and Python refusals -----------------------------------------------------------------------------------

def test_reliability_entry_argument_validation_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    A = 4096          # any non-NULL 16-B aligned address: every call below returns before touching memory
    planes, H, W = 65, 37, 96

    def rel(members=A, stride=planes * H * W, E=3, target=A, thr=A, T=1, w=A, first=0, counts=A, freq=A, prob=None, ws=A,
            ws_bytes=1 << 40, planes=planes, H=H, W=W):
        return lib.pangu_ensemble_reliability_f32(None, members, stride, E, target, thr, T, w, 1, first, counts, freq, prob, ws,
                                                  ws_bytes, planes, H, W)

    for kw in (dict(members=None), dict(w=None), dict(counts=None), dict(freq=None), dict(ws=None)):
        assert rel(**kw) == -2, kw
    assert rel(thr=None) == -2                                  # thresholds required with T > 0
    assert rel(T=0, thr=None, prob=A) == -2                     # prob without thresholds
    assert rel(T=0, thr=None, target=None) == -2                # nothing to compute
    for kw in (dict(E=1), dict(E=129), dict(T=-1), dict(T=5), dict(W=98, stride=planes * H * 98), dict(first=-1),
               dict(planes=0), dict(H=0), dict(W=0), dict(stride=planes * H * W - 4), dict(E=128, stride=1 << 34)):
        assert rel(**kw) == -1, kw
    need = P.score.reliability_workspace_bytes(planes, H, 3, 1)
    assert rel(ws_bytes=need - 1) == -4                         # workspace too small
    for kw in (dict(counts=A + 8), dict(freq=A + 8), dict(prob=A + 8), dict(ws=A + 8)):
        assert rel(ws_bytes=need, **kw) == -4, kw               # outputs not 16-B aligned


def test_reliability_python_refusals_before_any_launch():
    H, W = 8, 96
    up, sf = torch.zeros(3, 5, 13, H, W), torch.zeros(3, 4, H, W)
    thr = lambda T: (torch.zeros(T, 5, 13), torch.zeros(T, 4))
    rel = P.score.ensemble_reliability
    with pytest.raises(ValueError, match="2 <= E"):
        rel(up[:1], sf[:1], up[0], sf[0])
    with pytest.raises(ValueError, match="2 <= E"):
        rel(torch.zeros(129, 5, 13, 1, 4), torch.zeros(129, 4, 1, 4), None, None, thr(1))
    with pytest.raises(ValueError, match="W % 4"):
        rel(torch.zeros(2, 5, 13, H, 102), torch.zeros(2, 4, H, 102), None, None, thr(1))
    with pytest.raises(ValueError, match="both targets"):
        rel(up, sf, up[0], None, thr(1))
    with pytest.raises(ValueError, match="at most 4"):
        rel(up, sf, up[0], sf[0], thr(5))
    with pytest.raises(ValueError, match="nothing to compute"):
        rel(up, sf, None, None)
    with pytest.raises(ValueError, match="nothing to compute"):
        rel(up, sf, None, None, thr(0))
    with pytest.raises(ValueError, match=r"\(T, 5, 13\)"):
        rel(up, sf, up[0], sf[0], (torch.zeros(2, 65), torch.zeros(2, 4)))
    with pytest.raises(ValueError, match=r"\(T, 5, 13\)"):
        rel(up, sf, up[0], sf[0], (torch.zeros(2, 5, 13), torch.zeros(1, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rel(up, sf, up[0], sf[0], thr(1))                       # valid arguments on the CPU: no fallback
    with pytest.raises(ValueError, match="needs targets"):
        P.ensemble.ensemble_rollout(None, up[:1], sf[:1], None, None, None, None, members=3, amplitude=0.1,
                                    reliability=P.score.ReliabilityAccumulator(2))
    with pytest.raises(ValueError, match="only with reliability"):
        P.ensemble.ensemble_rollout(None, up[:1], sf[:1], None, None, None, None, members=3, amplitude=0.1, thresholds=thr(1))
    with pytest.raises(ValueError, match="leads"):
        P.score.ReliabilityAccumulator(0)
