"""Ensemble quantiles without a GPU: the numpy restatement of the definition pinned in csrc/quantile.hip (the reference of
tests/test_gpu_quantiles.py) against numpy.quantile, the argument checks of the C entry, and the Python refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib


def level_params(q, E):
    """(lo, frac) of a level as the entry derives them: h = q (E - 1) in double, lo = floor(h), frac = fp32(h - lo)."""
    h = float(q) * (E - 1)
    lo = int(np.floor(h))
    frac = np.float32(h - lo)
    if lo >= E - 1:
        lo, frac = E - 1, np.float32(0.0)
    return lo, frac


def quantiles_ref(x, q, y=None, w=None):
    """The definition restated: x (E, planes, H, W) float32, q a sequence of levels, y (planes, H, W) float32 or None, w (H,)
    latitude weights.  Sorted in fp32, interpolated in float64 with the fp32 frac, clamped into the bracket; a point with a NaN
    member is NaN in every field, left out of the scores and counted in nonfinite.  Returns a dict: fields (Q, planes, H, W)
    float64, a / b the bracket ends x_(lo), x_(lo+1) (b = a where frac == 0), lo, frac, nonfinite (planes,), and with y pinball /
    coverage_freq (Q, planes) float64 and coverage_counts (Q, planes) int64."""
    x = np.asarray(x, dtype=np.float32)
    E, planes, H, W = x.shape
    bad = np.isnan(x).any(axis=0)
    xs = np.sort(x, axis=0)                  # NaN sorts to the end; those points are overwritten below
    Q = len(q)
    fields, a_all, b_all = (np.empty((Q, planes, H, W), dtype=np.float64) for _ in range(3))
    los, fracs = [], []
    for l, ql in enumerate(q):
        lo, frac = level_params(ql, E)
        a = xs[lo].astype(np.float64)
        if frac == 0:
            f, b = a.copy(), a
        else:
            b = xs[lo + 1].astype(np.float64)
            with np.errstate(invalid="ignore"):
                f = np.fmin(np.fmax(a + np.float64(frac) * (b - a), a), b)      # fmin / fmax: the non-NaN operand
        f[bad] = np.nan
        fields[l], a_all[l], b_all[l] = f, a, b
        los.append(lo)
        fracs.append(frac)
    out = dict(fields=fields, a=a_all, b=b_all, lo=los, frac=fracs, nonfinite=bad.reshape(planes, -1).sum(-1).astype(np.int64))
    if y is not None:
        y = np.asarray(y, dtype=np.float32).astype(np.float64)
        wf = np.where(bad, 0.0, np.asarray(w, dtype=np.float64)[None, :, None])      # (planes, H, W): 0 at left-out points
        pin, cov = np.empty((Q, planes)), np.empty((Q, planes))
        cnt = np.empty((Q, planes), dtype=np.int64)
        for l, ql in enumerate(q):
            f = np.where(bad, 0.0, fields[l])
            u = y - f
            rho = u * (float(ql) - (u < 0))
            c = (y <= f) & ~bad
            pin[l] = (wf * rho).sum((-2, -1)) / (H * W)
            cov[l] = (wf * c).sum((-2, -1)) / (H * W)
            cnt[l] = c.sum((-2, -1))
        out.update(pinball=pin, coverage_freq=cov, coverage_counts=cnt)
    return out


LEVELS = (0.0, 0.1, 0.25, 0.5, 0.9, 1.0)


@pytest.mark.parametrize("E", [2, 3, 5, 33, 128])
def test_restatement_equals_numpy_quantile(E):
    x = np.random.default_rng(E).standard_normal((E, 2, 5, 8)).astype(np.float32)
    ref = quantiles_ref(x, LEVELS)
    want = np.quantile(x.astype(np.float64), LEVELS, axis=0)
    err = np.abs(ref["fields"] - want)
    print(f"E={E}: max rel err vs numpy.quantile {np.max(err / np.maximum(np.abs(want), 1e-30)):.3e}")
    # relative to the bracket's magnitude: the interpolation error is carried by fp32(frac) (6e-8 of the bracket width)
    scale = np.maximum(np.abs(ref["a"]), np.abs(ref["b"]))
    assert (err <= 1e-6 * scale).all()
    assert (ref["fields"] >= ref["a"]).all() and (ref["fields"] <= ref["b"]).all()
    assert not ref["nonfinite"].any()


@pytest.mark.parametrize("E", [2, 3, 5, 33, 128])
def test_restatement_selections_are_exact(E):
    x = np.random.default_rng(100 + E).standard_normal((E, 2, 5, 8)).astype(np.float32)
    ref = quantiles_ref(x, LEVELS)
    xs = np.sort(x, axis=0)
    exact = [l for l, fr in enumerate(ref["frac"]) if fr == 0]
    assert 0 in exact and len(LEVELS) - 1 in exact and ((E % 2 == 0) or 3 in exact)       # q = 0, q = 1, the odd-E median
    for l in exact:
        assert np.array_equal(ref["fields"][l].astype(np.float32).view(np.int32), xs[ref["lo"][l]].view(np.int32))
    assert ref["lo"][0] == 0 and ref["lo"][-1] == E - 1


def test_restatement_nan_rule_and_scores():
    rng = np.random.default_rng(7)
    E, planes, H, W = 5, 3, 4, 8
    x = rng.standard_normal((E, planes, H, W)).astype(np.float32)
    y = rng.standard_normal((planes, H, W)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, H)
    x[2, 1, 0, 3] = x[4, 1, 3, 7] = np.nan
    q = (0.1, 0.5, 1.0)
    ref = quantiles_ref(x, q, y, w)
    assert ref["nonfinite"].tolist() == [0, 2, 0]
    assert np.isnan(ref["fields"][:, 1, 0, 3]).all() and np.isnan(ref["fields"][:, 1, 3, 7]).all()
    assert np.isnan(ref["fields"]).sum() == 2 * len(q)
    # the scores are those of the data with the two points removed: direct float64 evaluation over the kept points
    keep = ~np.isnan(x).any(0)
    for l, ql in enumerate(q):
        f = np.quantile(np.where(np.isnan(x), 0, x).astype(np.float64), ql, axis=0)
        u = y.astype(np.float64) - f
        rho = np.where(u < 0, (ql - 1) * u, ql * u) * w[None, :, None] * keep
        assert np.allclose(ref["pinball"][l], rho.sum((-2, -1)) / (H * W), rtol=1e-6, atol=1e-12)
        assert np.array_equal(ref["coverage_counts"][l], ((y <= ref["fields"][l]) & keep).sum((-2, -1)))


def test_calibration_margin_of_the_gpu_case_on_the_cpu():
    """The draw of tests/test_gpu_quantiles.py::test_calibration_sanity, through the restatement: the pooled median coverage of a
    calibrated N(0, 1) ensemble (E = 33: the median is a selection, no finite-E bias) stays within 0.02 of 0.5."""
    x, y, w = calibration_case()
    ref = quantiles_ref(x, (0.5,), y, w)
    pooled = ref["coverage_freq"][0].mean()
    print(f"pooled median coverage {pooled:.5f}")
    assert abs(pooled - 0.5) < 0.02
    assert abs(ref["coverage_counts"][0].sum() / y.size - 0.5) < 0.02


def calibration_case():
    """E = 33 members and a target from the same N(0, 1), 69 planes of 9 x 260, and the project's latitude weights."""
    g = torch.Generator().manual_seed(33)
    x = torch.randn((33, 69, 9, 260), generator=g)
    y = torch.randn((69, 9, 260), generator=g)
    return x.numpy(), y.numpy(), P.score.latitude_weights(9, "cpu").numpy()


def test_interval_from_the_small_tables():
    q = (0.1, 0.5, 0.9)
    cov = torch.tensor([[0.12, 0.08], [0.5, 0.52], [0.91, 0.88]])
    fields = torch.arange(3 * 2 * 4 * 8, dtype=torch.float32).reshape(3, 2, 4, 8)
    r = P.score.QuantileResult(q, fields, torch.zeros(3, 2), torch.zeros(3, 2, dtype=torch.int64), cov, torch.zeros(2, dtype=torch.int64))
    iv = r.interval(0, 2)
    assert abs(iv["nominal"] - 0.8) < 1e-12
    assert torch.allclose(iv["coverage"], torch.tensor([0.79, 0.80], dtype=torch.float64), atol=1e-6)
    w = P.score.latitude_weights(4, "cpu").double()
    assert torch.allclose(iv["width"], torch.full((2,), 128.0, dtype=torch.float64) * w.mean(), rtol=1e-12)
    bare = P.score.QuantileResult(q, None, None, None, None, torch.zeros(2, dtype=torch.int64)).interval(0, 1)
    assert bare["coverage"] is None and bare["width"] is None
    with pytest.raises(IndexError):
        r.interval(0, 3)
    with pytest.raises(ValueError, match="must not exceed"):
        r.interval(2, 0)


def test_workspace_formula():
    assert P.score.quantiles_workspace_bytes(69, 721, 3) == 69 * 181 * 10 * 4
    assert P.score.quantiles_workspace_bytes(4, 9, 8) == 4 * 3 * 25 * 4
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        assert lib.pangu_ensemble_quantiles_ws_bytes(69, 721, 3) == P.score.quantiles_workspace_bytes(69, 721, 3)
        assert lib.pangu_ensemble_quantiles_ws_bytes(69, 721, 0) == -1 and lib.pangu_ensemble_quantiles_ws_bytes(69, 721, 9) == -1
        assert lib.pangu_ensemble_quantiles_ws_bytes(0, 721, 3) == -1


# ---- C entry and Python refusals -----------------------------------------------------------------------------------

def test_quantiles_entry_argument_validation_without_gpu():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    A = 4096          # any non-NULL aligned address: every call below returns before touching device memory
    planes, H, W = 65, 37, 96
    NOT_GIVEN = object()

    def qt(members=A, stride=planes * H * W, E=3, levels=(0.1, 0.5, 0.9), Q=None, target=A, w=A, fields=A, pin=A, cnt=A, cov=A,
           nonfinite=A, ws=A, ws_bytes=1 << 40, planes=planes, H=H, W=W, levels_ptr=NOT_GIVEN):
        lv = (ctypes.c_double * max(len(levels), 1))(*levels)          # the levels are read on the host: a real array
        lp = ctypes.addressof(lv) if levels_ptr is NOT_GIVEN else levels_ptr
        return lib.pangu_ensemble_quantiles_f32(None, members, stride, E, lp, len(levels) if Q is None else Q, target, w, fields, pin,
                                                cnt, cov, nonfinite, ws, ws_bytes, planes, H, W)

    for kw in (dict(members=None), dict(levels_ptr=None), dict(nonfinite=None), dict(ws=None)):
        assert qt(**kw) == -2, kw
    assert qt(target=None, fields=None) == -2                                   # neither fields nor target
    for kw in (dict(w=None), dict(pin=None), dict(cnt=None), dict(cov=None)):
        assert qt(**kw) == -2, kw                                               # a target without weights / score outputs
    for kw in (dict(E=1), dict(E=129), dict(W=98, stride=planes * H * 98), dict(levels=(), Q=0), dict(levels=(0.5,) * 9),
               dict(planes=0), dict(H=0), dict(W=0), dict(stride=planes * H * W - 4), dict(E=128, stride=1 << 34)):
        assert qt(**kw) == -1, kw
    for kw in (dict(levels=(0.1, 1.5)), dict(levels=(float("nan"),)), dict(levels=(-1e-9, 0.5))):
        assert qt(**kw) == -4, kw                                               # a level outside [0, 1] or NaN
    need = P.score.quantiles_workspace_bytes(planes, H, 3)
    assert qt(ws_bytes=need - 1) == -4                                          # workspace too small
    assert qt(ws_bytes=need, ws=A + 2) == -4                                    # workspace not 4-B aligned


def test_quantiles_python_refusals_before_any_launch():
    H, W = 8, 96
    up, sf = torch.zeros(3, 5, 13, H, W), torch.zeros(3, 4, H, W)
    qf = P.score.ensemble_quantiles
    with pytest.raises(ValueError, match="2 <= E"):
        qf(up[:1], sf[:1], (0.5,))
    with pytest.raises(ValueError, match="2 <= E"):
        qf(torch.zeros(129, 5, 13, 1, 4), torch.zeros(129, 4, 1, 4), (0.5,))
    with pytest.raises(ValueError, match="W % 4"):
        qf(torch.zeros(2, 5, 13, H, 102), torch.zeros(2, 4, H, 102), (0.5,))
    with pytest.raises(ValueError, match="expected upper"):
        qf(up, sf[:2], (0.5,))
    with pytest.raises(ValueError, match="both targets"):
        qf(up, sf, (0.5,), up[0], None)
    with pytest.raises(ValueError, match="1 <= Q <= 8"):
        qf(up, sf, ())
    with pytest.raises(ValueError, match="1 <= Q <= 8"):
        qf(up, sf, (0.5,) * 9)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        qf(up, sf, (0.5, 1.5))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        qf(up, sf, (float("nan"),))
    with pytest.raises(ValueError, match="sequence"):
        qf(up, sf, 0.5)
    with pytest.raises(ValueError, match="nothing to compute"):
        qf(up, sf, (0.5,), want_fields=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        qf(up, sf, (0.5,), up[0], sf[0])                                        # valid arguments on the CPU: no fallback


class _FakeDrain:
    def __init__(self, stats_last=None):
        self.stats_last = stats_last


def test_rollout_refusals_of_the_new_arguments_before_any_device_work():
    up, sf = torch.zeros(1, 5, 13, 8, 96), torch.zeros(1, 4, 8, 96)
    roll = lambda **kw: P.ensemble.ensemble_rollout(None, up, sf, None, None, None, None, members=3, amplitude=0.1, **kw)
    with pytest.raises(ValueError, match="through a drain"):
        roll(products=dict(mean_std=True))
    with pytest.raises(ValueError, match="without stats_last"):
        roll(drain=_FakeDrain(stats_last=(1, 2, 3, 4)))
    with pytest.raises(ValueError, match="quantile_levels needs targets"):
        roll(quantile_levels=(0.5,))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        roll(quantile_levels=(2.0,), targets=[(up, sf)])
    with pytest.raises(ValueError, match="nothing requested"):
        roll(drain=_FakeDrain(), products=dict(mean_std=False))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        roll(drain=_FakeDrain(), products=dict(quantiles=(0.5, -0.1)))


def test_product_names_follow_the_documented_order():
    names = P.ensemble.EnsembleRollout.product_names
    assert names() == ["mean_upper", "mean_surface", "std_upper", "std_surface"]
    assert names(mean_std=False, quantiles=(0.5,)) == ["quantiles_upper", "quantiles_surface"]
    assert names(quantiles=(0.1, 0.9), thresholds=(torch.zeros(1, 5, 13), torch.zeros(1, 4))) == [
        "mean_upper", "mean_surface", "std_upper", "std_surface", "quantiles_upper", "quantiles_surface", "exceedance_upper",
        "exceedance_surface"]
