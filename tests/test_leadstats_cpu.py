"""Lead-window statistics without a GPU: a numpy restatement of pangu_lead_stats_update_f32 that the GPU tests compare the kernel
against (lead_stats_ref), its own sanity on data where the answers are known, the bookkeeping of score.LeadWindowStats and of the
rollout hooks, and the argument checks of the C entry."""
import numpy as np
import pytest
import torch

from pangu_pytorch_amd import _lib, ensemble, rollout, score

F32 = np.float32
U8 = np.uint8


def lead_stats_ref(fields, window, thr=None, mul=None, add=None, levels=0):
    """The statistics of the leads [a, b) = window of fields[lead] (each (planes, E) float32, indexed by ABSOLUTE lead), as
    csrc/leadstats.hip defines them: v = x * mul + add in float32 (multiply, then add; mul / add per SOURCE plane), with levels = L
    output plane v*L + l reads source plane v*L + (L-1-l); thr (T, planes) per OUTPUT plane or None.  float32 arithmetic in lead
    order, the comparison rules verbatim.  Returns a dict: sum, min, max float32 (planes, E); when_min, when_max uint8; count, run,
    longest uint8 (T, planes, E)."""
    a, b = window
    planes = np.asarray(fields[a]).shape[0]
    order = np.arange(planes)
    if levels > 1:
        order = order.reshape(planes // levels, levels)[:, ::-1].reshape(-1)
    T = 0 if thr is None else len(thr)
    thr = np.zeros((0, planes), F32) if thr is None else np.asarray(thr, F32).reshape(T, planes)
    out = {}
    with np.errstate(all="ignore"):
        for lead in range(a, b):
            v = np.asarray(fields[lead], F32).reshape(planes, -1)
            if mul is not None:
                v = (v * np.asarray(mul, F32)[:, None]).astype(F32)
                v = (v + np.asarray(add, F32)[:, None]).astype(F32)
            v = v[order]
            e = (v[None] > thr[:, :, None]).astype(U8)                 # false for NaN and for thr = +inf
            if lead == a:
                out = {"sum": v.copy(), "min": v.copy(), "max": v.copy(), "when_min": np.full(v.shape, lead, U8),
                       "when_max": np.full(v.shape, lead, U8), "count": e.copy(), "run": e.copy(), "longest": e.copy()}
                continue
            out["sum"] = (out["sum"] + v).astype(F32)
            lo = (v < out["min"]) | (v != v)
            hi = (v > out["max"]) | (v != v)
            out["min"] = np.where(lo, v, out["min"])
            out["max"] = np.where(hi, v, out["max"])
            out["when_min"] = np.where(lo, U8(lead), out["when_min"])
            out["when_max"] = np.where(hi, U8(lead), out["when_max"])
            out["count"] = (out["count"] + e).astype(U8)
            out["run"] = np.where(e == 1, out["run"] + U8(1), U8(0)).astype(U8)
            out["longest"] = np.maximum(out["longest"], out["run"])
    return out


def same_bits(a, b):
    """Equal bit for bit: NaN positions and payloads and the sign of zero included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == F32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def longest_run(bits):
    """Brute force: the longest run of ones along axis 0."""
    best = np.zeros(bits.shape[1:], np.int64)
    for idx in np.ndindex(*bits.shape[1:]):
        run = 0
        for k in range(bits.shape[0]):
            run = run + 1 if bits[(k,) + idx] else 0
            best[idx] = max(best[idx], run)
    return best


def test_reference_on_integer_data():
    r = np.random.default_rng(0)
    L, planes, E = 9, 6, 35
    x = r.integers(-20, 21, (L, planes, E)).astype(F32)
    thr = np.stack([r.integers(-10, 11, planes).astype(F32), np.full(planes, np.inf, F32)])
    for a, b in ((0, 9), (2, 3), (3, 8)):
        got = lead_stats_ref(x, (a, b), thr)
        w = x[a:b]
        assert np.array_equal(got["sum"], w.sum(0)) and np.array_equal(got["min"], w.min(0)) and np.array_equal(got["max"], w.max(0))
        assert np.array_equal(got["when_max"], a + w.argmax(0)) and np.array_equal(got["when_min"], a + w.argmin(0))   # the first
        ev = w[:, None] > thr[None, :, :, None]
        assert np.array_equal(got["count"], ev.sum(0)) and np.array_equal(got["longest"], longest_run(ev))
        assert not got["count"][1].any() and not got["longest"][1].any()                # +inf: no event
        assert got["count"].dtype == U8 and got["when_max"].dtype == U8
    # the affine and the level reversal: mul / add by source plane, thresholds by output plane
    mul, add = r.integers(1, 4, planes).astype(F32), r.integers(-5, 6, planes).astype(F32)
    got = lead_stats_ref(x, (1, 6), thr, mul, add, levels=3)
    src = np.array([2, 1, 0, 5, 4, 3])
    v = (x * mul[None, :, None] + add[None, :, None])[1:6][:, src]
    assert np.array_equal(got["sum"], v.sum(0)) and np.array_equal(got["max"], v.max(0))
    assert np.array_equal(got["count"], (v[:, None] > thr[None, :, :, None]).sum(0))


def test_reference_nan_and_signed_zero_rules():
    nan, inf = F32(np.nan), F32(np.inf)
    #               lead 0     1     2     3     4
    cols = np.array([[1.0, nan, 5.0, -7.0, 2.0],          # a NaN takes both extremes at lead 1 and no number takes them back
                     [-0.0, 0.0, -0.0, 0.0, 0.0],         # signed zeros tie: the first lead keeps both extremes, as -0.0
                     [3.0, inf, inf, -inf, 3.0],          # infinities are numbers; ties keep the earlier lead
                     [nan, 1.0, 2.0, 3.0, 4.0],           # a NaN at the first lead
                     [1.0, nan, 2.0, nan, 0.0]], F32).T   # a later NaN takes the extremes again, with its lead
    x = cols.reshape(5, 1, 5).copy()
    got = lead_stats_ref(x, (0, 5), np.array([[1.5]], F32))
    mn, mx, wn, wx = got["min"][0], got["max"][0], got["when_min"][0], got["when_max"][0]
    assert np.isnan(mn[0]) and np.isnan(mx[0]) and wn[0] == 1 and wx[0] == 1
    assert mn[1] == 0 and np.signbit(mn[1]) and np.signbit(mx[1]) and wn[1] == 0 and wx[1] == 0
    assert mx[2] == inf and wx[2] == 1 and mn[2] == -inf and wn[2] == 3
    assert np.isnan(mn[3]) and wn[3] == 0 and wx[3] == 0
    assert np.isnan(mx[4]) and wn[4] == 3 and wx[4] == 3
    assert list(got["count"][0, 0]) == [2, 0, 4, 3, 1]                    # v > thr is false for NaN
    assert list(got["longest"][0, 0]) == [1, 0, 3, 3, 1] and list(got["run"][0, 0]) == [1, 0, 1, 3, 0]
    assert np.isnan(got["sum"][0, 0]) and np.isnan(got["sum"][0, 2])     # inf - inf
    assert got["sum"][0, 1] == 0 and not np.signbit(got["sum"][0, 1])    # -0.0 + 0.0 = +0.0 ...
    one = lead_stats_ref(x, (0, 1))
    assert np.signbit(one["sum"][0, 1]) and one["count"].shape == (0, 1, 5)      # ... and a window of one lead keeps the -0.0


# ---- LeadWindowStats: everything that is refused before a device call ----------------------------------------------------------------

def thresholds(T=1):
    return torch.zeros(T, 5, 13), torch.zeros(T, 4)


def cpu_fields(*lead_dims):
    return torch.zeros(lead_dims + (5, 13, 2, 4)), torch.zeros(lead_dims + (4, 2, 4))


class NoDevice(score.LeadWindowStats):
    """The real checks and bookkeeping; the device side records what it would launch."""

    def _fold(self, lead, upper, surface):
        self.__dict__.setdefault("folded", []).append((lead, [w for w, (a, b) in enumerate(self.windows) if a <= lead < b]))


@pytest.mark.parametrize("windows", [[(3, 3)], [(4, 2)], [(0, 256)], [(-1, 2)], [(0, 1)] * 5, [], [(1,)], 7])
def test_bad_windows(windows):
    with pytest.raises(ValueError):
        score.LeadWindowStats(windows, ("mean",))


def test_statistics_and_thresholds_go_together():
    with pytest.raises(ValueError, match="unknown statistic"):
        score.LeadWindowStats([(0, 2)], ("mean", "median"))
    with pytest.raises(ValueError):
        score.LeadWindowStats([(0, 2)], ())
    for s in ("count", "longest_spell"):
        with pytest.raises(ValueError, match="need thresholds"):
            score.LeadWindowStats([(0, 2)], ("mean", s))
    with pytest.raises(ValueError, match="only by count and longest_spell"):
        score.LeadWindowStats([(0, 2)], ("mean", "max"), thresholds=thresholds())
    with pytest.raises(ValueError):                                                   # _check_thresholds: at most 4, paired shapes
        score.LeadWindowStats([(0, 2)], ("count",), thresholds=thresholds(5))
    with pytest.raises(ValueError):
        score.LeadWindowStats([(0, 2)], ("count",), thresholds=(torch.zeros(2, 5, 13), torch.zeros(1, 4)))
    agg = score.LeadWindowStats([(0, 255)], ("when_min", "longest_spell", "mean"), thresholds=thresholds(4))
    assert agg.stats == ("mean", "when_min", "longest_spell") and agg.T == 4          # the canonical order
    assert agg._kept == ("sum", "min", "when_min", "run", "longest")                   # when_min keeps its extreme
    assert agg.product_names(0) == ["mean_upper", "mean_surface", "when_min_upper", "when_min_surface", "longest_spell_upper",
                                    "longest_spell_surface"]
    assert agg.bytes() == 0 and not agg.complete(0)
    with pytest.raises(IndexError):
        agg.complete(1)


def test_lead_order_and_gaps():
    up, sf = cpu_fields()
    agg = NoDevice([(0, 4), (1, 3), (5, 7)], ("mean",))
    for k in (0, 1, 2):
        agg.update(k, up, sf)
    assert agg.folded == [(0, [0]), (1, [0, 1]), (2, [0, 1])]
    assert agg.complete(1) and not agg.complete(0) and not agg.complete(2)
    with pytest.raises(ValueError, match="strictly increasing"):
        agg.update(2, up, sf)                                                         # repeated
    with pytest.raises(ValueError, match="strictly increasing"):
        agg.update(1, up, sf)                                                         # out of order
    with pytest.raises(ValueError, match="expects lead 3"):
        agg.update(4, up, sf)                                                         # skips lead 3 of (0, 4)
    with pytest.raises(ValueError, match="incomplete"):
        agg.result(0)
    with pytest.raises(ValueError, match="incomplete"):
        agg.products(2)
    agg.update(3, up, sf)
    agg.update(4, up, sf)                                                             # in no window: accepted, nothing to launch
    assert agg.folded[-1] == (4, []) and agg.complete(0)
    with pytest.raises(ValueError, match=r"window \(5, 7\) expects lead 5"):
        agg.update(6, up, sf)                                                         # the first lead of (5, 7) was skipped
    for bad in (-1, 255):
        with pytest.raises(IndexError):
            agg.update(bad, up, sf)
    agg.reset()
    assert not agg.complete(0) and not agg.complete(1)
    agg.update(0, up, sf)                                                             # a new pass starts again from the first lead
    late = NoDevice([(2, 4)], ("max",))
    late.update(0, up, sf)
    with pytest.raises(ValueError, match="expects lead 2"):
        late.update(3, up, sf)


def test_shapes_are_checked_before_the_device():
    up, sf = cpu_fields()
    agg = NoDevice([(0, 3)], ("mean",))
    for bad_up, bad_sf in ((up.double(), sf), (up, sf[:, :, ::2]), (torch.zeros(5, 12, 2, 4), sf), (up, torch.zeros(3, 2, 4)),
                           (up, torch.zeros(4, 2, 8)), (torch.zeros(2, 5, 13, 2, 4), sf), (up.numpy(), sf)):
        with pytest.raises(ValueError):
            agg.update(0, bad_up, bad_sf)
    assert not hasattr(agg, "folded")
    agg.update(0, up, sf)
    up3, sf3 = cpu_fields(3)
    with pytest.raises(ValueError, match="first update"):
        agg.update(1, up3, sf3)
    members = NoDevice([(0, 1)], ("mean",))
    members.update(0, up3, sf3)                                                       # leading dimensions are more planes
    assert members.complete(0)


def test_cpu_tensors_fail_loudly_after_the_bookkeeping_checks():
    up, sf = cpu_fields()
    agg = score.LeadWindowStats([(1, 3)], ("mean", "count"), thresholds=thresholds())
    with pytest.raises(ValueError, match="expects lead 1"):
        agg.update(2, up, sf)                                                         # the bookkeeping error comes first
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):
        agg.update(1, up, sf)
    with pytest.raises(RuntimeError, match="no CPU fallback|MI355X"):
        agg.update(0, up, sf)                                                         # even at a lead in no window
    assert agg._last == -1 and agg.bytes() == 0 and not agg.complete(0)               # a refused update leaves no trace


def test_rollout_hooks_check_the_aggregator_before_the_first_step():
    stats_last = tuple(torch.ones(s) for s in ((1, 4, 1, 1), (1, 4, 1, 1), (1, 5, 13, 1, 1), (1, 5, 13, 1, 1)))
    agg = score.LeadWindowStats([(0, 2), (1, 3)], ("mean",))
    normalised = score.LeadWindowStats([(0, 2)], ("mean",), stats_last=stats_last)
    for steps in (1, 2):
        with pytest.raises(ValueError, match="do not reach the end"):
            rollout.rollout(None, None, None, None, None, None, None, steps=steps, lead_stats=agg)
        with pytest.raises(ValueError, match="do not reach the end"):
            ensemble.ensemble_rollout(None, None, None, None, None, None, None, 2, 0.1, steps=steps, lead_stats=agg)
    with pytest.raises(ValueError, match="without stats_last"):
        rollout.rollout(None, None, None, None, None, None, None, steps=2, lead_stats=normalised)
    with pytest.raises(ValueError, match="without stats_last"):
        ensemble.ensemble_rollout(None, None, None, None, None, None, None, 2, 0.1, steps=2, lead_stats=normalised)
    with pytest.raises(TypeError):                                                    # keyword-only
        rollout.rollout(None, None, None, None, None, None, None, 7, True, False, None, None, None, None, agg)


# ---- the C entry's argument checks ----------------------------------------------------------------------------------------------------

def test_argument_validation_without_gpu():
    lib = _lib.load()
    P8 = 16         # any non-NULL address: the calls below return before touching memory
    fn = lib.pangu_lead_stats_update_f32
    #       stream src mul   add   sum vmin vmax wmin wmax thr T  count run longest planes elems levels lead first
    good = [None, P8, None, None, P8, P8, P8, P8, P8, P8, 2, P8, P8, P8, 26, 63, 13, 3, 0]
    SRC, MUL, ADD, SUM, VMIN, VMAX, WMIN, WMAX, THR, T, COUNT, RUN, LONGEST, PLANES, ELEMS, LEVELS, LEAD = range(1, 18)

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)

    outputs = (SUM, VMIN, VMAX, WMIN, WMAX, COUNT, RUN, LONGEST)
    none = lambda *idx: {f"a{i}": None for i in idx}
    # PANGU_E_NULL
    assert call(**none(SRC)) == -2
    assert call(**{f"a{MUL}": P8}) == -2 and call(**{f"a{ADD}": P8}) == -2             # mul without add, add without mul
    assert call(**none(THR)) == -2                                                     # thr with T > 0
    # PANGU_E_SHAPE
    for i in (PLANES, ELEMS):
        assert call(**{f"a{i}": 0}) == -1 and call(**{f"a{i}": -3}) == -1, i
    assert call(**{f"a{ELEMS}": 1 << 31}) == -1 and call(**{f"a{ELEMS}": 1 << 40}) == -1
    assert call(**{f"a{LEVELS}": -1}) == -1 and call(**{f"a{PLANES}": 27}) == -1       # levels < 0, planes % levels
    assert call(**{f"a{T}": -1}) == -1 and call(**{f"a{T}": 5}) == -1
    assert call(**{f"a{LEAD}": -1}) == -1 and call(**{f"a{LEAD}": 255}) == -1
    assert call(**{f"a{PLANES}": 1 << 30, f"a{LEVELS}": 0, f"a{ELEMS}": 4097}) == -1   # more workgroups than a grid holds
    # PANGU_E_ARG
    assert call(**{f"a{T}": 0}, **none(*outputs, THR)) == -4                           # no output requested
    assert call(**none(VMIN)) == -4 and call(**none(VMAX)) == -4                       # when_* without its extreme
    assert call(**none(RUN)) == -4                                                     # longest without run
    assert call(**none(COUNT, LONGEST)) == -4 and call(**none(COUNT, RUN, LONGEST)) == -4      # T > 0 with neither
    for i in (COUNT, RUN, LONGEST):                                                    # T == 0 with one of them
        assert call(**{f"a{T}": 0}, **none(THR, *(j for j in (COUNT, RUN, LONGEST) if j != i))) == -4, i
    for i in (SRC, SUM, VMIN, VMAX, THR):                                              # fp32 pointers: 4-B aligned
        assert call(**{f"a{i}": P8 + 1}) == -4 and call(**{f"a{i}": P8 + 2}) == -4, i
    assert call(**{f"a{MUL}": P8 + 2, f"a{ADD}": P8}) == -4 and call(**{f"a{MUL}": P8, f"a{ADD}": P8 + 1}) == -4
    # the order of the classes: NULL, then SHAPE, then ARG
    assert call(**none(SRC), **{f"a{PLANES}": 0}) == -2 and call(**none(RUN), **{f"a{LEAD}": 300}) == -1
