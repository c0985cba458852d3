"""Lead-window statistics on the GPU: pangu_lead_stats_update_f32 against the numpy restatement of tests/test_leadstats_cpu.py, the
Python surface (score.LeadWindowStats), the rollout hooks and the composition with deterministic_scores and data.HostDrain.

The kernel's contract is bit for bit, so every comparison is exact (same_bits: NaN positions and the sign of zero included); the one
exception is `mean`, torch's division of the exact sum, checked to 2 ulp of numpy's float32 quotient."""
import numpy as np
import pytest
import torch

from test_leadstats_cpu import lead_stats_ref, same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON_F, POISON_B = -7.25e33, 0xA5
GUARD = 64
FLOAT_KEYS, BYTE_KEYS, EVENT_KEYS = ("sum", "min", "max"), ("when_min", "when_max"), ("count", "run", "longest")
ALL_KEYS = FLOAT_KEYS + BYTE_KEYS + EVENT_KEYS


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    P._lib.load()
    return P


def fields_of(leads, planes, E, seed):
    """(leads, planes, E) float32: per plane an offset plus noise, half of the elements quantised to quarters so that ties between
    leads occur (the earlier lead must win them)."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((leads, planes, E)) * 2.0
    x[..., ::2] = np.round(x[..., ::2] * 2.0) / 4.0
    return (x + np.arange(planes)[None, :, None]).astype(F32)


def thresholds_of(T, x, seed, mul=None, add=None, levels=0):
    """(T, planes) float32 around each OUTPUT plane's mean value at the first lead, so that events come and go; the last threshold of
    the first plane and the whole last row of T = 4 are +inf (no event)."""
    if T == 0:
        return None
    r = np.random.default_rng(seed)
    centre = lead_stats_ref(x, (0, 1), None, mul, add, levels)["sum"].astype(np.float64).mean(1)
    thr = (centre[None, :] + r.uniform(-1.5, 1.5, (T, centre.size))).astype(F32)
    thr[-1, 0] = np.inf
    if T == 4:
        thr[3] = np.inf
    return thr


def affine_of(planes, seed):
    r = np.random.default_rng(seed)
    return r.uniform(0.5, 3.0, planes).astype(F32), r.uniform(-20.0, 90.0, planes).astype(F32)


def abi_window(P, fields, window, thr=None, mul=None, add=None, levels=0, keep=ALL_KEYS, off_f=0, off_b=0, off_src=None):
    """The window [a, b) of fields (leads, planes, E) through the C ABI, one launch per lead on the current stream.  Every output
    lies between two poisoned guard bands of GUARD elements that must come back intact; off_f / off_b shift the fp32 / byte outputs
    by that many elements off their allocation's alignment, off_src (default off_f) the source.  Returns numpy arrays by key."""
    a, b = window
    _, planes, E = fields.shape
    if not any(k in EVENT_KEYS for k in keep):
        thr = None                                   # no event statistic kept: no thresholds either
    T = 0 if thr is None else thr.shape[0]
    keep = tuple(k for k in keep if T or k not in EVENT_KEYS)
    off_src = off_f if off_src is None else off_src
    src = torch.zeros(fields.size + 4, device="cuda")
    src[off_src:off_src + fields.size] = torch.from_numpy(np.ascontiguousarray(fields)).cuda().view(-1)
    dev = lambda t: None if t is None else torch.from_numpy(np.ascontiguousarray(t)).cuda()
    mul, add, thr_d = dev(mul), dev(add), dev(thr)
    bufs = {}
    for k in keep:
        n = planes * E * (T if k in EVENT_KEYS else 1)
        if k in FLOAT_KEYS:
            buf, off = torch.full((n + 2 * GUARD + 4,), POISON_F, device="cuda"), off_f
        else:
            buf, off = torch.full((n + 2 * GUARD + 4,), POISON_B, dtype=torch.uint8, device="cuda"), off_b
        bufs[k] = (buf, GUARD + off, n)
    ptr = lambda k: bufs[k][0][bufs[k][1]:].data_ptr() if k in bufs else None
    lib = P._lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    for lead in range(a, b):
        s = src[off_src + lead * planes * E:]
        P._lib.check(lib.pangu_lead_stats_update_f32(
            stream, s.data_ptr(), None if mul is None else mul.data_ptr(), None if add is None else add.data_ptr(), ptr("sum"),
            ptr("min"), ptr("max"), ptr("when_min"), ptr("when_max"), None if T == 0 else thr_d.data_ptr(), T, ptr("count"), ptr("run"),
            ptr("longest"), planes, E, levels, lead, 1 if lead == a else 0), "lead_stats_update_f32")
    torch.cuda.synchronize()
    out = {}
    for k, (buf, lo, n) in bufs.items():
        poison = POISON_F if k in FLOAT_KEYS else POISON_B
        assert bool((buf[:lo] == poison).all()), f"{k}: wrote before the output"
        assert bool((buf[lo + n:] == poison).all()), f"{k}: wrote behind the output"
        out[k] = buf[lo:lo + n].cpu().numpy().reshape(((T,) if k in EVENT_KEYS else ()) + (planes, E))
    return out


def assert_matches(got, ref, what=""):
    for k, v in got.items():
        assert same_bits(v, ref[k]), f"{what}: {k} differs from the reference in {int((v != ref[k]).sum())} places"


# (id, planes, H, W, levels, affine)
SHAPES = [
    ("3x7x9", 3, 7, 9, 0, False),                    # 63 elements: not a multiple of 4, less than one lane group per lane
    ("6x13x24-levels-affine", 6, 13, 24, 3, True),
    ("3x33x1021", 3, 33, 1021, 0, False),            # several workgroups per plane, ragged tail
]
WINDOWS = [(0, 7), (2, 4), (6, 7)]                   # 7 leads, 2 leads, and 1 lead (first and last coincide)


@pytest.mark.parametrize("T", [0, 1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_kernel_matches_reference(P, shape, T):
    _, planes, H, W, levels, affine = shape
    x = fields_of(7, planes, H * W, seed=planes + T)
    mul, add = affine_of(planes, 5) if affine else (None, None)
    thr = thresholds_of(T, x, 3, mul, add, levels)
    for window in WINDOWS:
        ref = lead_stats_ref(x, window, thr, mul, add, levels)
        got = abi_window(P, x, window, thr, mul, add, levels)
        assert set(got) == set(ALL_KEYS if T else FLOAT_KEYS + BYTE_KEYS)
        assert_matches(got, ref, f"{shape[0]} T={T} window {window}")
        if T:
            assert got["count"].any() and not got["count"][-1, 0].any()              # events happen; +inf: none
    # any subset of the outputs: the statistics do not depend on which others are kept
    subsets = [("sum",), ("min",), ("max", "when_max")] + ([("count",), ("sum", "run", "longest"), ("min", "when_min", "count")] if T else [])
    for keep in subsets:
        got = abi_window(P, x, WINDOWS[0], thr, mul, add, levels, keep=keep)
        assert set(got) == set(keep)
        assert_matches(got, lead_stats_ref(x, WINDOWS[0], thr, mul, add, levels), f"{shape[0]} T={T} keep={keep}")


@pytest.mark.parametrize("offsets", [(1, 1, 1), (1, 0, 0), (0, 0, 1), (0, 1, 0), (3, 3, 2)],
                         ids=["all-one-off", "source-off", "bytes-off", "floats-off", "mixed"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[SHAPES[0][0], SHAPES[2][0]])
def test_misaligned_views_give_the_same_bits(P, shape, offsets):
    """Views one float / one byte off their allocation's alignment: with one common phase the planes go in groups behind a scalar
    head, with different phases one element per lane; the bits are those of the aligned call."""
    _, planes, H, W, levels, _ = shape
    off_src, off_f, off_b = offsets
    x = fields_of(4, planes, H * W, seed=11)
    thr = thresholds_of(2, x, 4)
    ref = lead_stats_ref(x, (0, 4), thr, levels=levels)
    got = abi_window(P, x, (0, 4), thr, levels=levels, off_f=off_f, off_b=off_b, off_src=off_src)
    assert_matches(got, ref, f"{shape[0]} offsets {offsets}")


def test_special_values(P):
    planes, E = 2, 63
    base = fields_of(5, planes, E, seed=21)
    x = base.copy()
    x[1, 0, 5] = np.nan                              # a NaN at one lead
    x[2, 0, 7] = np.inf                              # +inf at another
    x[3, 0, 9] = -np.inf
    x[0, 1, 3], x[1:, 1, 3] = -0.0, 0.0              # -0.0 at the first lead, +0.0 after it
    x[:, 1, 4] = [np.nan, 2.0, np.nan, 3.0, 1.0]     # a NaN at the first lead, and again later
    thr = np.array([[0.5, -1.0]], F32)
    got = abi_window(P, x, (0, 5), thr)
    assert_matches(got, lead_stats_ref(x, (0, 5), thr), "special values")
    # the rules, spelled out
    assert np.isnan(got["min"][0, 5]) and np.isnan(got["max"][0, 5]) and got["when_min"][0, 5] == 1 and got["when_max"][0, 5] == 1
    assert np.isnan(got["sum"][0, 5]) and got["count"][0, 0, 5] == (x[[0, 2, 3, 4], 0, 5] > 0.5).sum()
    assert got["max"][0, 7] == np.inf and got["when_max"][0, 7] == 2 and got["sum"][0, 7] == np.inf
    assert got["min"][0, 9] == -np.inf and got["when_min"][0, 9] == 3
    for k in ("min", "max", "sum"):
        assert got[k][1, 3] == 0
    assert np.signbit(got["min"][1, 3]) and np.signbit(got["max"][1, 3]) and not np.signbit(got["sum"][1, 3])
    assert got["when_min"][1, 3] == 0 and got["when_max"][1, 3] == 0 and got["count"][0, 1, 3] == 5 and got["longest"][0, 1, 3] == 5
    assert np.isnan(got["min"][1, 4]) and got["when_min"][1, 4] == 2 and got["when_max"][1, 4] == 2 and got["count"][0, 1, 4] == 3
    assert got["longest"][0, 1, 4] == 2 and got["run"][0, 1, 4] == 2
    one = abi_window(P, x, (0, 1), thr)              # a window of one lead keeps the -0.0 in its sum
    assert np.signbit(one["sum"][1, 3]) and one["when_max"][1, 3] == 0
    # every other element is what it is without the planted values
    clean = abi_window(P, base, (0, 5), thr)
    touched = np.zeros((planes, E), bool)
    touched[0, [5, 7, 9]] = touched[1, [3, 4]] = True
    for k, v in got.items():
        assert same_bits(v[..., ~touched], clean[k][..., ~touched]), k


def test_long_window_does_not_wrap(P):
    """255 leads, every one above the threshold and above its predecessor: count == longest == 255, when_max == 254."""
    planes, E, L = 2, 63, 255
    r = np.random.default_rng(8)
    x = (np.arange(L)[:, None, None] + r.uniform(0.0, 0.5, (L, planes, E))).astype(F32)
    x[:, 1, ::3] = x[::-1, 1, ::3]                   # falling there: the maximum stays at lead 0, the minimum moves to 254
    thr = np.full((1, planes), -1.0, F32)
    got = abi_window(P, x, (0, L), thr)
    assert_matches(got, lead_stats_ref(x, (0, L), thr), "255 leads")
    assert (got["count"] == 255).all() and (got["longest"] == 255).all() and (got["run"] == 255).all()
    assert (got["when_max"][0] == 254).all() and (got["when_min"][0] == 0).all()
    assert (got["when_max"][1, ::3] == 0).all() and (got["when_min"][1, ::3] == 254).all()


def test_repeatable_and_independent_of_other_planes(P):
    planes, E = 6, 33 * 40
    x = fields_of(3, planes, E, seed=31)
    mul, add = affine_of(planes, 9)
    thr = thresholds_of(2, x, 6, mul, add, 3)
    first = abi_window(P, x, (0, 3), thr, mul, add, levels=3)
    again = abi_window(P, x, (0, 3), thr, mul, add, levels=3)
    for k in first:
        assert same_bits(first[k], again[k]), k
    other = x.copy()
    keep_src = 1                                      # output plane 1 reads source plane 1 of the first variable (levels = 3)
    mask = np.ones(planes, bool)
    mask[keep_src] = False
    other[:, mask] = fields_of(3, planes, E, seed=32)[:, mask] * 3.0
    other[0, 0, 0] = np.nan
    changed = abi_window(P, other, (0, 3), thr, mul, add, levels=3)
    for k in first:
        assert same_bits(first[k][..., 1, :], changed[k][..., 1, :]), k
        assert not same_bits(first[k], changed[k]), k


# ---- score.LeadWindowStats -------------------------------------------------------------------------------------------------------

def _pair_fields(leads, lead_dims, H, W, seed):
    """numpy (leads, *lead_dims, 5, 13, H, W) and (leads, *lead_dims, 4, H, W)."""
    n = int(np.prod(lead_dims, dtype=np.int64)) if lead_dims else 1
    own = lambda x, per: x - (np.arange(x.shape[1]) // per * per).astype(F32)[None, :, None]     # every case: offsets 0..per-1
    up = own(fields_of(leads, n * 65, H * W, seed), 65).reshape((leads,) + lead_dims + (5, 13, H, W))
    sf = own(fields_of(leads, n * 4, H * W, seed + 1), 4).reshape((leads,) + lead_dims + (4, H, W))
    return up, sf


def _thr_pair(T, seed):
    r = np.random.default_rng(seed)
    tu = (np.arange(65).reshape(1, 5, 13) + r.uniform(-1.5, 1.5, (T, 5, 13))).astype(F32)
    ts = (np.arange(4).reshape(1, 4) + r.uniform(-1.5, 1.5, (T, 4))).astype(F32)
    tu[-1, 0, 0] = np.inf
    return tu, ts


def _ref_of(x, window, thr, n_cases, mul=None, add=None, levels=0):
    """lead_stats_ref of x (leads, cases.., planes.., H, W) with thr (T, planes..) shared by the cases, reshaped like a
    LeadWindowResult: byte fields (cases.., T, planes.., H, W)."""
    leads = x.shape[0]
    shape = x.shape[1:]
    H, W = shape[-2:]
    planes = int(np.prod(shape[:-2]))
    t = None
    if thr is not None:
        T = thr.shape[0]
        t = np.broadcast_to(thr.reshape(T, 1, -1), (T, planes // thr[0].size, thr[0].size)).reshape(T, planes)
    ref = lead_stats_ref(x.reshape(leads, planes, H * W), window, t, mul, add, levels)
    out = {k: ref[k].reshape(shape) for k in FLOAT_KEYS + BYTE_KEYS}
    if thr is not None:
        for k in EVENT_KEYS:
            out[k] = np.moveaxis(ref[k].reshape((T,) + shape), 0, n_cases)
    return out


def _check_result(res, ref_u, ref_s, stats, what=""):
    names = {"min": "min", "max": "max", "when_min": "when_min", "when_max": "when_max", "count": "count", "longest_spell": "longest"}
    for stat in stats:
        for got, ref in zip(getattr(res, stat), (ref_u, ref_s)):
            got = got.cpu().numpy()
            if stat == "mean":
                want = ref["sum"] / F32(res.n)
                assert want.dtype == F32 and got.shape == want.shape
                ok = np.abs(got.astype(np.float64) - want) <= 2.0 * np.spacing(np.abs(want))
                assert (ok | (np.isnan(got) & np.isnan(want))).all(), f"{what}: mean off by more than 2 ulp"
            else:
                assert same_bits(got, ref[names[stat]]), f"{what}: {stat}"
    if res.sum is not None:
        for got, ref in zip(res.sum, (ref_u, ref_s)):
            assert same_bits(got.cpu().numpy(), ref["sum"]), f"{what}: sum"


REGIONS = {"global": "global", "tropics": "tropics"}
ALL_STATS = ("mean", "min", "max", "when_min", "when_max", "count", "longest_spell")


def test_python_surface_matches_the_kernel(P):
    E, H, W, T = 3, 5, 9, 2
    windows = [(0, 4), (1, 3), (2, 4)]
    up, sf = _pair_fields(5, (E,), H, W, seed=41)
    tu, ts = _thr_pair(T, seed=42)
    agg = P.score.LeadWindowStats(windows, ALL_STATS, thresholds=(torch.from_numpy(tu), torch.from_numpy(ts)))
    dev = lambda a: torch.from_numpy(a).cuda()

    def one_pass():
        for k in range(5):                            # lead 4 lies in no window: accepted and ignored
            assert not agg.complete(2) or k == 4
            agg.update(k, dev(up[k]), dev(sf[k]))
        return [{s: tuple(t.clone() for t in getattr(agg.result(w), s)) for s in ALL_STATS + ("sum",)} for w in range(3)]

    first = one_pass()
    for w, window in enumerate(windows):
        res = agg.result(w)
        assert res.window == window and res.n == window[1] - window[0]
        assert res.count[0].shape == (E, T, 5, 13, H, W) and res.longest_spell[1].shape == (E, T, 4, H, W)
        assert res.when_max[0].dtype == torch.uint8 and res.count[0].dtype == torch.uint8 and res.mean[0].dtype == torch.float32
        _check_result(res, _ref_of(up, window, tu, 1), _ref_of(sf, window, ts, 1), ALL_STATS, f"window {window}")
    # the same numbers as the C entry called directly on the flattened planes
    t = np.broadcast_to(tu.reshape(T, 1, 65), (T, E, 65)).reshape(T, E * 65)
    abi = abi_window(P, up.reshape(5, E * 65, H * W), (1, 3), t)
    res = agg.result(1)
    assert same_bits(res.max[0].cpu().numpy().reshape(E * 65, -1), abi["max"])
    assert same_bits(res.count[0].movedim(1, 0).contiguous().cpu().numpy().reshape(T, E * 65, -1), abi["count"])
    # bytes(): per window and element 3 x 4 B + 2 x 1 B + T x 3 B
    per_window = E * 69 * H * W * (12 + 2 + 3 * T)
    allocated = sum(t.numel() * t.element_size() for pair in agg._acc for fields in pair for t in fields.values())
    assert agg.bytes() == 3 * per_window == allocated
    # reset() and a second pass over the accumulators as they are: the same bits
    agg.reset()
    assert not agg.complete(0)
    with pytest.raises(ValueError, match="incomplete"):
        agg.result(0)
    second = one_pass()
    for a, b in zip(first, second):
        for s in a:
            assert all(torch.equal(x, y) or same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a[s], b[s])), s
    assert agg.bytes() == allocated


def test_stats_last_and_levels_reversed(P):
    H, W = 5, 8
    up, sf = _pair_fields(3, (2,), H, W, seed=51)
    r = np.random.default_rng(52)
    t = lambda a: torch.from_numpy(a.astype(F32))
    stats_last = (t(r.uniform(-3, 3, (1, 4, 1, 1))), t(r.uniform(0.5, 3, (1, 4, 1, 1))), t(r.uniform(-3, 3, (1, 5, 13, 1, 1))),
                  t(r.uniform(0.5, 3, (1, 5, 13, 1, 1))))
    tu, ts = _thr_pair(1, seed=53)
    stats = ("mean", "max", "when_max", "count")
    agg = P.score.LeadWindowStats([(0, 3)], stats, thresholds=(t(tu), t(ts)), stats_last=stats_last, levels_reversed=True)
    for k in range(3):
        agg.update(k, torch.from_numpy(up[k]).cuda(), torch.from_numpy(sf[k]).cuda())
    # explicit numpy: v = x * std + mean per STORED plane, two roundings; then the level axis of the upper-air tensor reversed
    s_mean, s_std, u_mean, u_std = (a.numpy() for a in stats_last)
    vu = ((up * u_std[None]).astype(F32) + u_mean[None]).astype(F32)[:, :, :, ::-1]
    vs = ((sf * s_std[None]).astype(F32) + s_mean[None]).astype(F32)
    _check_result(agg.result(0), _ref_of(np.ascontiguousarray(vu), (0, 3), tu, 1), _ref_of(vs, (0, 3), ts, 1), stats, "stats_last")


def test_weekly_mean_verification(P):
    """Forecast leads in one aggregator, analysis leads (stored ascending) in another: deterministic_scores of the two window means
    is the weekly-mean scorecard, equal to that of means whose sums numpy built."""
    H, W = 13, 24
    fu, fs = _pair_fields(3, (1,), H, W, seed=61)
    au, as_ = _pair_fields(3, (1,), H, W, seed=63)
    fu, fs, au, as_ = fu + F32(270), fs + F32(270), au + F32(270.5), as_ + F32(270.5)
    forecast = P.score.LeadWindowStats([(0, 3)], ("mean",))
    analysis = P.score.LeadWindowStats([(0, 3)], ("mean",), levels_reversed=True)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for k in range(3):
        forecast.update(k, dev(fu[k]), dev(fs[k]))
        analysis.update(k, dev(au[k, :, :, ::-1]), dev(as_[k]))                     # on disk: ascending levels
    mf, ma = forecast.result(0).mean, analysis.result(0).mean
    got_u, got_s = P.score.deterministic_scores(mf[0], mf[1], ma[0], ma[1], REGIONS)
    sums = lambda x: dev(lead_stats_ref(x.reshape(3, -1, H * W), (0, 3))["sum"].reshape(x.shape[1:]))
    want_u, want_s = P.score.deterministic_scores(sums(fu) / 3.0, sums(fs) / 3.0, sums(au) / 3.0, sums(as_) / 3.0, REGIONS)
    assert torch.equal(got_u.sums, want_u.sums) and torch.equal(got_s.sums, want_s.sums)
    assert bool(torch.isfinite(got_u.rmse).all()) and bool((got_u.rmse > 0).all())
    for got, x in zip(mf + ma, (fu, fs, au, as_)):                                   # and the means themselves: 2 ulp of numpy's
        want = lead_stats_ref(x.reshape(3, -1, H * W), (0, 3))["sum"].reshape(x.shape[1:]) / F32(3)
        assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= 2.0 * np.spacing(np.abs(want))).all()


def test_products_go_through_the_drain(P):
    H, W, T = 5, 8, 2
    up, sf = _pair_fields(2, (2,), H, W, seed=71)
    tu, ts = _thr_pair(T, seed=72)
    stats = ("mean", "max", "when_max", "count", "longest_spell")
    agg = P.score.LeadWindowStats([(0, 2)], stats, thresholds=(torch.from_numpy(tu), torch.from_numpy(ts)))
    for k in range(2):
        agg.update(k, torch.from_numpy(up[k]).cuda(), torch.from_numpy(sf[k]).cuda())
    names, products = agg.product_names(0), agg.products(0)
    assert names == [f"{s}_{part}" for s in stats for part in ("upper", "surface")] and len(products) == len(names)
    assert all(t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda for t in products)
    res = agg.result(0)
    assert torch.equal(products[names.index("when_max_upper")], res.when_max[0].float())
    assert torch.equal(products[names.index("count_surface")], res.count[1].float()) and products[-1].shape == (2, T, 4, H, W)
    drain = P.data.HostDrain("cuda", mode="float32", depth=1)
    drain.submit(products, tag="week1")
    items = [(item.tag, item.to_float32()) for item in drain]
    drain.close()
    assert len(items) == 1 and items[0][0] == "week1" and len(items[0][1]) == len(names)
    for name, got, want in zip(names, items[0][1], products):
        assert same_bits(got, want.cpu().numpy()), name


# ---- the rollout hooks -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup(P):
    import cases
    import synth
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return m, cases.model_inputs("cuda")


def _recording(P, kept, *args, **kw):
    class Recording(P.score.LeadWindowStats):
        def update(self, lead, upper, surface):
            kept.append((lead, upper.clone(), surface.clone()))
            return super().update(lead, upper, surface)

    return Recording(*args, **kw)


def _hook_thresholds(kept_like_upper, kept_like_surface):
    """One threshold per plane: the plane's mean, so that events happen on every plane."""
    return (kept_like_upper.mean((-1, -2)).reshape(1, 5, 13).cpu(), kept_like_surface.mean((-1, -2)).reshape(1, 4).cpu())


@pytest.mark.timeout(300)
@pytest.mark.parametrize("graph", [True, False])
def test_rollout_folds_every_step(P, setup, graph):
    """The model and inputs of tests/test_gpu_scorecard.py::test_rollout_scores_every_step, fp32, 2 steps: the hook leaves the
    returned fields untouched, is handed every step's physical fields, and the windows hold their statistics."""
    from test_gpu_drain import _stats_last as stats_last_of
    m, (inp, inp_s, stats, maps, const_h) = setup
    sl = stats_last_of(stats)
    up0, sf0 = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph)
    thr = _hook_thresholds(up0[0], sf0[0])
    kept = []
    windows = [(0, 2), (1, 2)]
    hook_stats = ("mean", "min", "max", "when_max", "count", "longest_spell")
    agg = _recording(P, kept, windows, hook_stats, thresholds=thr)
    up1, sf1 = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, lead_stats=agg)
    assert torch.equal(up0, up1) and torch.equal(sf0, sf1)
    assert [k for k, _, _ in kept] == [0, 1] and agg.complete(0) and agg.complete(1)
    assert torch.equal(kept[1][1], up1) and torch.equal(kept[1][2], sf1)             # the last step's physical fields
    ku = np.stack([u.cpu().numpy() for _, u, _ in kept])
    ks = np.stack([s.cpu().numpy() for _, _, s in kept])
    tu, ts = thr[0].numpy(), thr[1].numpy()
    for w, window in enumerate(windows):
        _check_result(agg.result(w), _ref_of(ku, window, tu, 1), _ref_of(ks, window, ts, 1), hook_stats, f"graph={graph} {window}")
    last = agg.result(1)                                                              # a window of the last step alone
    for pair in (last.min, last.max, last.sum):
        assert torch.equal(pair[0], up1) and torch.equal(pair[1], sf1)
    assert bool((last.when_max[0] == 1).all()) and bool(last.count[0].any())


@pytest.mark.timeout(300)
def test_ensemble_rollout_folds_every_member(P, setup):
    from test_gpu_drain import _stats_last as stats_last_of
    m, (inp, inp_s, stats, maps, const_h) = setup
    sl = stats_last_of(stats)
    kw = dict(members=2, amplitude=0.05, steps=2, seed=7)
    up0, sf0 = P.ensemble.ensemble_rollout(m, inp, inp_s, stats, maps, const_h, sl, **kw)
    up0, sf0 = up0.clone(), sf0.clone()
    thr = _hook_thresholds(up0[0], sf0[0])
    kept = []
    windows = [(0, 2), (1, 2)]
    hook_stats = ("mean", "max", "when_max", "count")
    agg = _recording(P, kept, windows, hook_stats, thresholds=thr)
    up1, sf1 = P.ensemble.ensemble_rollout(m, inp, inp_s, stats, maps, const_h, sl, lead_stats=agg, **kw)
    assert torch.equal(up0, up1) and torch.equal(sf0, sf1)
    assert [k for k, _, _ in kept] == [0, 1] and tuple(kept[0][1].shape[:3]) == (2, 5, 13)
    assert not torch.equal(kept[1][1][0], kept[1][1][1])                             # the members differ
    ku = np.stack([u.cpu().numpy() for _, u, _ in kept])
    ks = np.stack([s.cpu().numpy() for _, _, s in kept])
    for w, window in enumerate(windows):
        res = agg.result(w)
        assert res.max[0].shape == up1.shape and res.count[1].shape == (2, 1) + tuple(sf1.shape[1:])
        _check_result(res, _ref_of(ku, window, thr[0].numpy(), 1), _ref_of(ks, window, thr[1].numpy(), 1), hook_stats, f"{window}")
    assert torch.equal(agg.result(1).max[0], up1) and torch.equal(agg.result(1).max[1], sf1)
