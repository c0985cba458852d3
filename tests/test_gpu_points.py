"""The observation operator on the GPU: pangu_sample_points_f32 and pangu_point_scores_f32 against the numpy restatements of
tests/test_points_cpu.py, the Python surface (score.sample_points, observation_scores, ObservationAccumulator, PointSeries) and the
rollout hooks.

The sampling contract is bit for bit (same_bits); the sums are checked against the bound derived in csrc/points.hip ('Rounding of
the sums'), restated as point_sums_bound."""
import numpy as np
import pytest
import torch

from test_leadstats_cpu import same_bits
from test_points_cpu import (POINT_CHUNK, POINT_FP32_ADDS, U24, plan_arrays, point_sums_bound, point_sums_ref, point_terms,
                             sample_points_ref)

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON_F, POISON_D = -7.25e33, -3.5e300
GUARD = 64

# (id, planes, H, W, N, levels, affine)
SHAPES = [
    ("3x2x4-1pt", 3, 2, 4, 1, 0, False),                                  # the smallest legal grid, one point
    ("6x7x12-67pt-levels-affine", 6, 7, 12, 67, 3, True),
    ("3x33x1021-3chunks", 3, 33, 1021, 2 * POINT_CHUNK + 452, 0, False),  # W % 4 != 0, two full chunks and a ragged third
]
IDS = [s[0] for s in SHAPES]


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    P._lib.load()
    return P


def points_of(H, W, N, seed):
    """N points: the wrap column first, then the poles, on-node points, the last row and a duplicate, then random ones."""
    r = np.random.default_rng(seed)
    lat_of, lon_of = lambda j: 90.0 - 180.0 * j / (H - 1), lambda i: 360.0 * i / W
    pts = [(lat_of(0.4 * (H - 1)), lon_of(W - 0.25)),          # between the last column and column 0
           (90.0, 12.3), (-90.0, 200.0), (90.0, 0.0),
           (lat_of(1 % H), lon_of(0)), (lat_of(H // 2), lon_of(0)), (lat_of(H - 1), lon_of(0.5)), (lat_of(0.5), lon_of(0)),
           (lat_of(0.4 * (H - 1)), lon_of(W - 0.25)), (lat_of(0.4 * (H - 1)), lon_of(W - 0.25) - 720.0)]
    pts = pts[:N]
    lat = np.array([p[0] for p in pts] + list(r.uniform(-90.0, 90.0, N - len(pts))))
    lon = np.array([p[1] for p in pts] + list(r.uniform(-360.0, 720.0, N - len(pts))))
    return lat, lon


def case_of(P, shape, seed=0):
    """src (planes, H, W), the plan (on the device) and its arrays, mul / add or None, levels."""
    _, planes, H, W, N, levels, affine = shape
    r = np.random.default_rng(seed + planes * 1000 + W)
    src = (r.standard_normal((planes, H, W)) * 3.0 + np.arange(planes)[:, None, None]).astype(F32)
    lat, lon = points_of(H, W, N, seed + 1)
    plan = P.score.point_plan(H, W, lat, lon, device="cuda")
    mul = add = None
    if affine:
        mul, add = r.uniform(0.5, 3.0, planes).astype(F32), r.uniform(-20.0, 90.0, planes).astype(F32)
    return src, plan, plan_arrays(plan), mul, add, levels


def guarded(n, poison, dtype, off=0):
    """(buffer, view of n elements between two poisoned bands of GUARD elements, `off` elements off the allocation's alignment)"""
    buf = torch.full((n + 2 * GUARD + 4,), poison, dtype=dtype, device="cuda")
    return buf, buf[GUARD + off:GUARD + off + n]


def intact(buf, view, poison):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == poison).all()) and bool((buf[lo + view.numel():] == poison).all())


def shifted(a, off):
    """a numpy array on the device, `off` elements behind the start of its allocation"""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = torch.zeros(flat.size + 4, dtype=torch.from_numpy(flat).dtype, device="cuda")
    buf[off:off + flat.size] = torch.from_numpy(flat).cuda()
    return buf[off:off + flat.size]


def dev_plan(arrays, off=0):
    return [shifted(a, off) for a in arrays]


def abi_sample(P, src, arrays, mul=None, add=None, levels=0, off=0):
    planes, H, W = src.shape
    N = arrays[0].size
    s = shifted(src, off)
    row, col, wy, wx = dev_plan(arrays, off)
    m, a = (None, None) if mul is None else (shifted(mul, off), shifted(add, off))
    buf, out = guarded(planes * N, POISON_F, torch.float32, off)
    P._lib.check(P._lib.load().pangu_sample_points_f32(
        torch.cuda.current_stream().cuda_stream, s.data_ptr(), None if m is None else m.data_ptr(), None if a is None else a.data_ptr(),
        row.data_ptr(), col.data_ptr(), wy.data_ptr(), wx.data_ptr(), out.data_ptr(), planes, H, W, N, levels), "sample_points_f32")
    torch.cuda.synchronize()
    assert intact(buf, out, POISON_F), "wrote outside the output"
    return out.cpu().numpy().reshape(planes, N)


def abi_scores(P, src, arrays, obs, clim=None, bits=None, R=1, mul=None, add=None, levels=0, off=0, want_departures=True):
    """(departures (planes, N) or None, sums (planes, R, 10)) through the C ABI, every output between guard bands."""
    planes, H, W = src.shape
    N = arrays[0].size
    lib = P._lib.load()
    s, o = shifted(src, off), shifted(obs, off)
    row, col, wy, wx = dev_plan(arrays, off)
    m, a = (None, None) if mul is None else (shifted(mul, off), shifted(add, off))
    c = None if clim is None else shifted(clim, off)
    b = None if bits is None else shifted(bits, 4 * (off % 2))               # the bytes shifted by 0 or 4
    dbuf, dep = guarded(planes * N, POISON_F, torch.float32, off)
    sbuf, sums = guarded(planes * R * 10, POISON_D, torch.float64, off % 2)
    need = lib.pangu_point_scores_ws_bytes(planes, N, R)
    assert need == planes * ((N + POINT_CHUNK - 1) // POINT_CHUNK) * R * 40
    wbuf, ws = guarded(need // 4, POISON_F, torch.float32, off)
    ptr = lambda t: None if t is None else t.data_ptr()
    P._lib.check(lib.pangu_point_scores_f32(
        torch.cuda.current_stream().cuda_stream, s.data_ptr(), ptr(m), ptr(a), row.data_ptr(), col.data_ptr(), wy.data_ptr(),
        wx.data_ptr(), o.data_ptr(), ptr(c), ptr(b), R, dep.data_ptr() if want_departures else None, sums.data_ptr(), ws.data_ptr(),
        need, planes, H, W, N, levels), "point_scores_f32")
    torch.cuda.synchronize()
    assert intact(sbuf, sums, POISON_D) and intact(wbuf, ws, POISON_F), "wrote outside the sums or the workspace"
    if want_departures:
        assert intact(dbuf, dep, POISON_F), "wrote outside the departures"
    else:
        assert bool((dbuf == POISON_F).all()), "departures were not asked for"
    return (dep.cpu().numpy().reshape(planes, N) if want_departures else None), sums.cpu().numpy().reshape(planes, R, 10)


def obs_of(f, seed, missing_plane=None):
    """Observations around the forecast values f (planes, N): about a third missing (NaN), one plane without any report."""
    r = np.random.default_rng(seed)
    obs = (f + r.standard_normal(f.shape).astype(F32) * F32(1.5)).astype(F32)
    obs[r.random(f.shape) < 1.0 / 3.0] = np.nan
    if missing_plane is not None:
        obs[missing_plane] = np.nan
    return obs


def bits_of(kind, N, seed):
    """(bits or None, R): no region bits; one region under bits; three regions, the last of them empty; eight, region 5 empty."""
    r = np.random.default_rng(seed)
    if kind == "none":
        return None, 1
    if kind == "one":
        return (r.random(N) < 0.6).astype(np.uint8) | np.uint8(0xF0), 1      # bits of regions >= R are ignored
    if kind == "three":
        return (r.integers(0, 4, N)).astype(np.uint8), 3
    return (r.integers(0, 256, N) & ~(1 << 5)).astype(np.uint8), 8


def same_departures(got, ref):
    """bit for bit where a number stands; NaN exactly where the reference has NaN (the payload of a NaN is not pinned)"""
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(got), nan) and same_bits(np.where(nan, F32(0), got), np.where(nan, F32(0), ref))


# ---- sampling ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sample_matches_reference(P, shape):
    src, plan, arrays, mul, add, levels = case_of(P, shape)
    ref = sample_points_ref(src, *arrays, mul, add, levels)
    got = abi_sample(P, src, arrays, mul, add, levels)
    assert same_bits(got, ref), f"{int((got != ref).sum())} of {ref.size} samples differ"
    row, col, wy, wx = arrays
    on_node = (wy == 0) & (wx == 0)
    if mul is None and shape[4] > 1:
        assert on_node.sum() >= 3 and same_bits(got[:, on_node], src[:, row[on_node], col[on_node]])
        assert (col == shape[3] - 1).any() and (row == shape[2] - 1).any() and (row == 0).any()


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shifted_views_give_the_same_bits(P, shape, off):
    src, plan, arrays, mul, add, levels = case_of(P, shape)
    assert same_bits(abi_sample(P, src, arrays, mul, add, levels, off=off), sample_points_ref(src, *arrays, mul, add, levels))
    obs = obs_of(sample_points_ref(src, *arrays, mul, add, levels), 5)
    dep0, sums0 = abi_scores(P, src, arrays, obs, mul=mul, add=add, levels=levels)
    dep1, sums1 = abi_scores(P, src, arrays, obs, mul=mul, add=add, levels=levels, off=off)
    assert same_departures(dep1, dep0) and np.array_equal(sums0, sums1)


def test_special_values(P):
    """A NaN and a +inf planted at nodes reach exactly the points that hold them with a non-zero weight; an on-node neighbour, whose
    weight for the poisoned node is 0, stays clean."""
    H, W = 7, 12
    src = np.arange(2 * H * W, dtype=F32).reshape(2, H, W)
    src[:, 3, 5], src[:, 2, 0] = np.nan, np.inf
    lat_of, lon_of = lambda j: 90.0 - 180.0 * j / (H - 1), lambda i: 360.0 * i / W
    pts = [(lat_of(3), lon_of(4)), (lat_of(2), lon_of(5)), (lat_of(3), lon_of(5)), (lat_of(2.5), lon_of(5)), (lat_of(3), lon_of(4.5)),
           (lat_of(2), lon_of(11)), (lat_of(2), lon_of(11.5)), (lat_of(1.5), lon_of(11.75)), (lat_of(2), lon_of(0)),
           (lat_of(3.5), lon_of(5.5)), (lat_of(4), lon_of(5))]
    plan = P.score.point_plan(H, W, [p[0] for p in pts], [p[1] for p in pts], device="cuda")
    arrays = plan_arrays(plan)
    got = abi_sample(P, src, arrays)
    assert same_bits(np.isnan(got), np.isnan(sample_points_ref(src, *arrays)))
    for p in range(2):
        assert list(np.isnan(got[p])) == [False, False, True, True, True, False, False, False, False, True, False]
        assert list(np.isinf(got[p])) == [False, False, False, False, False, False, True, True, True, False, False]
        assert got[p, 0] == src[p, 3, 4] and got[p, 1] == src[p, 2, 5] and got[p, 5] == src[p, 2, 11] and got[p, 10] == src[p, 4, 5]
    # in the scores a non-finite forecast value reaches the regions that hold its point with a report, and no other
    obs = np.zeros((2, len(pts)), F32)
    obs[1, 2] = np.nan                                                        # plane 1: no report where the NaN is sampled on its node
    bits = np.array([1, 1, 2, 1, 1, 1, 4, 1, 1, 1, 1], np.uint8)               # the on-node NaN alone in region 1, an inf alone in 2
    dep, sums = abi_scores(P, src, arrays, obs, bits=bits, R=3)
    assert np.isnan(sums[0, 1, [1, 2, 3, 4, 6, 7]]).all() and sums[0, 1, 0] == 1      # region 1 of plane 0 holds the NaN: d and a
    assert sums[0, 1, 5] == 0 and sums[0, 1, 8] == 0                          # b = o - c is a number there
    assert not sums[1, 1].any()                                               # plane 1: its only point has no report
    assert np.isinf(sums[:, 2, 2]).all() and np.isnan(sums[:, 0, 1]).all()    # the inf; region 0 holds other NaN samples
    assert sums[0, :, 0].tolist() == [9, 1, 1] and sums[1, :, 9].tolist() == [9, 0, 1]
    assert np.isnan(dep[1, 2]) and np.isnan(dep[0, 2]) and dep[0, 0] == src[0, 3, 4]


# ---- scores -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("regions", ["none", "one", "three", "eight"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scores_match_reference(P, shape, regions):
    src, plan, arrays, mul, add, levels = case_of(P, shape)
    planes, N = shape[1], shape[4]
    f = sample_points_ref(src, *arrays, mul, add, levels)
    obs = obs_of(f, 3, missing_plane=1)
    if N == 1:
        obs[0, 0] = f[0, 0] + F32(0.75)                                        # the one point of plane 0 has a report
    clim = None if shape[6] is False and N > 1 else (np.arange(planes, dtype=F32) + F32(0.5))
    bits, R = bits_of(regions, N, 4)
    dep, sums = abi_scores(P, src, arrays, obs, clim, bits, R, mul, add, levels)
    d_ref, _, valid = point_terms(f, obs, clim)
    assert same_departures(dep, d_ref) and np.array_equal(np.isnan(dep), np.isnan(obs))
    ref, mags = point_sums_ref(f, obs, clim, bits, R)
    assert np.array_equal(sums[..., 0], ref[..., 0]) and np.array_equal(sums[..., 9], ref[..., 9])      # the counts are exact
    masks = np.ones((1, N), bool) if bits is None else np.stack([((bits >> r) & 1) == 1 for r in range(R)])
    assert np.array_equal(sums[..., 0], (valid[:, None, :] & masks[None]).sum(-1))
    bound = point_sums_bound(mags, N)
    err = np.abs(sums - ref)
    worst = float(np.max(err[..., 1:9] / np.where(bound[..., 1:9] > 0, bound[..., 1:9], np.inf), initial=0.0))
    print(f"{shape[0]} regions={regions}: worst error {worst:.3f} of the bound ({POINT_FP32_ADDS} fp32 additions)")
    assert (err <= bound).all()
    assert not sums[1].any()                                                  # a plane without a report: ten zeros per region
    if regions == "three":
        assert not sums[:, 2].any()                                           # an empty region
    if regions == "eight":
        assert not sums[:, 5].any() and (N == 1 or sums[0, 7, 0] > 0)
    if N > 1:
        assert 0.2 < np.isnan(obs[0]).mean() < 0.5
    # the sums do not depend on whether the departures are kept
    _, again = abi_scores(P, src, arrays, obs, clim, bits, R, mul, add, levels, want_departures=False)
    assert np.array_equal(again, sums)


def test_repeatable_and_independent_of_other_planes(P):
    shape = SHAPES[2]
    src, plan, arrays, mul, add, levels = case_of(P, shape)
    f = sample_points_ref(src, *arrays)
    obs = obs_of(f, 8)
    bits, R = bits_of("three", shape[4], 9)
    clim = np.array([0.5, -1.0, 2.0], F32)
    first = abi_scores(P, src, arrays, obs, clim, bits, R)
    s0 = abi_sample(P, src, arrays)
    for _ in range(3):
        dep, sums = abi_scores(P, src, arrays, obs, clim, bits, R)
        assert same_departures(dep, first[0]) and np.array_equal(sums, first[1])
        assert same_bits(abi_sample(P, src, arrays), s0)
    for p in range(3):                                                        # each plane in a launch of its own
        dep, sums = abi_scores(P, src[p:p + 1], arrays, obs[p:p + 1], clim[p:p + 1], bits, R)
        assert same_departures(dep[0], first[0][p]) and np.array_equal(sums[0], first[1][p])
        assert same_bits(abi_sample(P, src[p:p + 1], arrays)[0], s0[p])
    other = src.copy()
    other[0] += F32(1.0)
    dep, sums = abi_scores(P, other, arrays, obs, clim, bits, R)
    assert np.array_equal(sums[1:], first[1][1:]) and not np.array_equal(sums[0], first[1][0])


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------

def _fields(lead_dims, H, W, seed):
    r = np.random.default_rng(seed)
    up = (r.standard_normal(lead_dims + (5, 13, H, W)) * 2.0 + 5.0).astype(F32)
    sf = (r.standard_normal(lead_dims + (4, H, W)) * 2.0 - 1.0).astype(F32)
    return up, sf


def _stats_last(seed):
    r = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a.astype(F32)).cuda()
    return (t(r.uniform(-3, 3, (1, 4, 1, 1))), t(r.uniform(0.5, 2, (1, 4, 1, 1))), t(r.uniform(-3, 3, (1, 5, 13, 1, 1))),
            t(r.uniform(0.5, 2, (1, 5, 13, 1, 1))))


def _small_plan(P, H, W, N, seed, regions=None):
    lat, lon = points_of(H, W, N, seed)
    return P.score.point_plan(H, W, lat, lon, regions, device="cuda")


def test_sample_points_with_stats_last_and_levels_reversed(P):
    H, W, N = 7, 12, 40
    up, sf = _fields((2,), H, W, 21)
    plan = _small_plan(P, H, W, N, 22)
    arrays = plan_arrays(plan)
    sl = _stats_last(23)
    gu, gs = P.score.sample_points(torch.from_numpy(up).cuda(), torch.from_numpy(sf).cuda(), plan, stats_last=sl, levels_reversed=True)
    assert gu.shape == (2, 5, 13, N) and gs.shape == (2, 4, N)
    flat = lambda v, n: np.tile(v.cpu().numpy().reshape(-1), 2).astype(F32)
    mul_u, add_u, mul_s, add_s = flat(sl[3], 65), flat(sl[2], 65), flat(sl[1], 4), flat(sl[0], 4)
    assert same_bits(gu.cpu().numpy().reshape(130, N), abi_sample(P, up.reshape(130, H, W), arrays, mul_u, add_u, 13))
    assert same_bits(gu.cpu().numpy().reshape(130, N), sample_points_ref(up.reshape(130, H, W), *arrays, mul_u, add_u, 13))
    assert same_bits(gs.cpu().numpy().reshape(8, N), sample_points_ref(sf.reshape(8, H, W), *arrays, mul_s, add_s, 0))
    pu, ps = P.score.sample_points(torch.from_numpy(up).cuda(), torch.from_numpy(sf).cuda(), plan)
    assert same_bits(pu.cpu().numpy().reshape(130, N), sample_points_ref(up.reshape(130, H, W), *arrays))
    with pytest.raises(ValueError, match="sample_points"):
        P.score.sample_points(torch.from_numpy(up).cuda(), torch.from_numpy(sf).cuda(), _small_plan(P, H, W + 1, N, 1))
    with pytest.raises(ValueError, match="sample_points"):
        P.score.sample_points(torch.from_numpy(up).cuda()[..., :-1], torch.from_numpy(sf).cuda(), plan)


def _metric_checks(got, ref, mags, N, what):
    """bias, rmse and acc of a ScoreSums against numpy on the reference sums, within what the bound of the sums lets through."""
    bound = point_sums_bound(mags, N)
    g = POINT_FP32_ADDS * U24 / (1.0 - POINT_FP32_ADDS * U24) + 1e-12        # relative error of a sum of one sign
    n = ref[..., 0]
    with np.errstate(all="ignore"):
        bias, rmse = ref[..., 1] / n, np.sqrt(ref[..., 3] / n)
        acc = ref[..., 6] / np.sqrt(ref[..., 7] * ref[..., 8])
        ok = n > 0
        assert np.array_equal(np.isnan(got.bias.cpu().numpy()), ~ok), what
        assert (np.abs(got.bias.cpu().numpy() - bias)[ok] <= (bound[..., 1] / np.maximum(n, 1))[ok] * (1 + 1e-9)).all(), what
        assert (np.abs(got.rmse.cpu().numpy() - rmse)[ok] <= (g * rmse)[ok]).all(), what
        acc_bound = (bound[..., 6] / np.sqrt(ref[..., 7] * ref[..., 8]) + np.abs(acc) * g) / (1.0 - g)
        ok = ok & (ref[..., 7] > 0) & (ref[..., 8] > 0)
        assert (np.abs(got.acc.cpu().numpy() - acc)[ok] <= acc_bound[ok]).all(), what
    assert np.array_equal(got.counts.cpu().numpy(), n.astype(np.int64)), what


def test_observation_scores_against_numpy(P):
    H, W, N = 7, 12, 300
    regions = {"all": "global", "tropics": "tropics", "nowhere": dict(mask=torch.zeros(H, W, dtype=torch.bool))}
    up, sf = _fields((), H, W, 31)
    plan = _small_plan(P, H, W, N, 32, regions)
    arrays, bits = plan_arrays(plan), plan.bits.cpu().numpy()
    sl = _stats_last(33)
    fu, fs = sample_points_ref(up.reshape(65, H, W), *arrays), sample_points_ref(sf, *arrays)
    ou, os_ = obs_of(fu, 34, missing_plane=7), obs_of(fs, 35)
    dev = lambda a, s: torch.from_numpy(a).cuda().reshape(s)
    args = (dev(up, (5, 13, H, W)), dev(sf, (4, H, W)), dev(ou, (5, 13, N)), dev(os_, (4, N)), plan)
    su, ss, du, ds = P.score.observation_scores(*args, clim=sl, want_departures=True)
    assert su.sums.shape == (5, 13, 3, 10) and ss.sums.shape == (4, 3, 10) and su.names == ("all", "tropics", "nowhere")
    cu, cs = sl[2].cpu().numpy().reshape(-1), sl[0].cpu().numpy().reshape(-1)
    assert same_departures(du.cpu().numpy().reshape(65, N), point_terms(fu, ou, cu)[0])
    assert same_departures(ds.cpu().numpy(), point_terms(fs, os_, cs)[0])
    for got, f, o, c, what in ((su, fu, ou, cu, "upper"), (ss, fs, os_, cs, "surface")):
        ref, mags = point_sums_ref(f, o, c, bits, 3)
        shape = tuple(got.sums.shape)
        assert (np.abs(got.sums.cpu().numpy() - ref.reshape(shape)) <= point_sums_bound(mags, N).reshape(shape)).all(), what
        _metric_checks(got, ref.reshape(shape), mags.reshape(shape), N, what)
    assert not su.sums[0, 7].any() and not ss.sums[:, 2].any() and bool(torch.isnan(ss.rmse[:, 2]).all())
    assert bool((ss.counts[:, 1] > 0).all())
    two = P.score.observation_scores(*args)                                   # no climatology, no departures: a pair
    assert len(two) == 2 and bool((two[0].sums[..., 3] == su.sums[..., 3]).all())
    assert two[1].wind_rmse().shape == (3,)
    with pytest.raises(ValueError, match="observation_scores"):
        P.score.observation_scores(args[0], args[1], args[2][..., :-1], args[3], plan)
    with pytest.raises(ValueError, match="observation_scores"):
        P.score.observation_scores(*args, clim=(sl[0], sl[1]))


def test_observation_accumulator_pools_cases(P):
    H, W, N = 7, 12, 150
    plan = _small_plan(P, H, W, N, 41, {"all": "global", "sh": "sh_extratropics"})
    arrays, bits = plan_arrays(plan), plan.bits.cpu().numpy()
    up, sf = _fields((2,), H, W, 42)                                          # two cases
    fu = np.stack([sample_points_ref(up[c].reshape(65, H, W), *arrays) for c in range(2)])
    fs = np.stack([sample_points_ref(sf[c], *arrays) for c in range(2)])
    ou, os_ = obs_of(fu.reshape(130, N), 43).reshape(2, 65, N), obs_of(fs.reshape(8, N), 44).reshape(2, 4, N)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    acc = P.score.ObservationAccumulator(2, plan)
    assert acc.cases(0) == 0
    parts = [acc.score(0, dev(up[c]), dev(sf[c]), dev(ou[c].reshape(5, 13, N)), dev(os_[c]), ) for c in range(2)]
    assert acc.cases(0) == 2 and acc.cases(1) == 0
    pu, ps = acc.result(0)
    assert torch.equal(pu.sums, parts[0][0].sums + parts[1][0].sums) and torch.equal(ps.sums, parts[0][1].sums + parts[1][1].sums)
    # both cases in one call, as leading dimensions, pool to the same table
    acc.score(1, dev(up), dev(sf), dev(ou.reshape(2, 5, 13, N)), dev(os_))
    assert acc.cases(1) == 2 and torch.equal(acc.result(1)[0].sums, pu.sums) and torch.equal(acc.result(1)[1].sums, ps.sums)
    # and equal the scores over the concatenated points
    cat = lambda a: np.concatenate([a[0], a[1]], axis=-1)
    for got, f, o, what in ((pu, cat(fu), cat(ou), "upper"), (ps, cat(fs), cat(os_), "surface")):
        ref, mags = point_sums_ref(f, o, None, np.concatenate([bits, bits]), 2)
        shape = tuple(got.sums.shape)
        assert (np.abs(got.sums.cpu().numpy() - ref.reshape(shape)) <= point_sums_bound(mags, 2 * N).reshape(shape)).all(), what
        _metric_checks(got, ref.reshape(shape), mags.reshape(shape), 2 * N, what)
    with pytest.raises(ValueError, match="ObservationAccumulator"):
        P.score.ObservationAccumulator(0, plan)
    with pytest.raises(IndexError):
        acc.score(2, dev(up[0]), dev(sf[0]), dev(ou[0].reshape(5, 13, N)), dev(os_[0]))
    with pytest.raises(ValueError, match="nothing scored"):
        P.score.ObservationAccumulator(3, plan).result(1)


def test_point_series_and_wind_helpers(P):
    H, W = 7, 12
    lat_of, lon_of = lambda j: 90.0 - 180.0 * j / (H - 1), lambda i: 360.0 * i / W
    nodes = [(1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (1, 7)]
    lat = [lat_of(j) for j, _ in nodes] + [10.0, -47.0, 80.0]
    lon = [lon_of(i) for _, i in nodes] + [33.0, 250.0, 359.0]
    plan = P.score.point_plan(H, W, lat, lon, device="cuda")
    up, sf = _fields((), H, W, 51)
    for (j, i), (u, v) in zip(nodes, ((0.0, 0.0), (0.0, -5.0), (-5.0, 0.0), (0.0, 5.0), (5.0, 0.0), (3.0, 4.0))):
        sf[1, j, i], sf[2, j, i] = u, v                                       # calm, then from north, east, south, west; a 3-4-5
    series = P.score.PointSeries(plan, 3)
    d = lambda a: torch.from_numpy(a).cuda()
    series.record(0, d(up), d(sf))
    series.record(2, d(up + F32(1.0)), d(sf * F32(2.0)))
    assert series.upper.shape == (3, 5, 13, 9) and series.surface.shape == (3, 4, 9)
    arrays = plan_arrays(plan)
    assert same_bits(series.surface[0].cpu().numpy(), sample_points_ref(sf, *arrays))
    assert same_bits(series.upper[2].cpu().numpy().reshape(65, 9), sample_points_ref((up + F32(1.0)).reshape(65, H, W), *arrays))
    assert bool(torch.isnan(series.upper[1]).all()) and bool(torch.isnan(series.surface[1]).all())      # a lead never recorded
    s = series.surface.cpu().numpy()
    u, v = s[:, 1], s[:, 2]
    with np.errstate(all="ignore"):
        speed = np.sqrt(u * u + v * v)
        direction = np.mod(np.degrees(np.arctan2(-u.astype(np.float64), -v.astype(np.float64))), 360.0)
    direction[(u == 0) & (v == 0)] = 0.0
    got_s, got_d = series.wind_speed10().cpu().numpy(), series.wind_direction10().cpu().numpy()
    assert got_s.shape == (3, 9) and np.allclose(got_s, speed, rtol=4 * U24, atol=0, equal_nan=True)
    assert np.allclose(got_d, direction, rtol=0, atol=360.0 * 8 * U24, equal_nan=True)      # an fp32 atan2 and the scaling to degrees
    assert got_s[0, :6].tolist() == [0.0, 5.0, 5.0, 5.0, 5.0, 5.0] and got_s[2, 5] == 10.0
    assert got_d[0, 0] == 0.0 and np.allclose(got_d[0, 1:5], [0.0, 90.0, 180.0, 270.0], rtol=0, atol=360.0 * 8 * U24)
    assert ((got_d[[0, 2]] >= 0) & (got_d[[0, 2]] < 360)).all()
    with pytest.raises(IndexError):
        series.record(3, d(up), d(sf))
    with pytest.raises(ValueError, match="PointSeries"):
        series.record(1, d(np.stack([up, up])), d(np.stack([sf, sf])))
    with pytest.raises(ValueError, match="PointSeries"):
        P.score.PointSeries(plan, 2).wind_speed10()


# ---- the rollout hooks ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup(P):
    import cases
    import synth
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return m, cases.model_inputs("cuda")


@pytest.fixture(scope="module")
def site_plan(P):
    r = np.random.default_rng(61)
    lat = np.concatenate([[90.0, -90.0, 0.0, 51.5], r.uniform(-90, 90, 1196)])
    lon = np.concatenate([[0.0, 180.0, 359.9, -0.1], r.uniform(-180, 360, 1196)])
    return P.score.point_plan(721, 1440, lat, lon, {"global": "global", "europe": "europe"}, device="cuda")


def _recording(P, kept, plan, leads):
    class Recording(P.score.PointSeries):
        def record(self, lead, upper, surface):
            kept.append((lead, upper.clone(), surface.clone()))
            return super().record(lead, upper, surface)

    return Recording(plan, leads)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("graph", [True, False])
def test_rollout_samples_and_scores_every_step(P, setup, site_plan, graph):
    """The model and inputs of tests/test_gpu_leadstats.py::test_rollout_folds_every_step, fp32, 2 steps: the hooks leave the returned
    fields untouched, the series holds every step's fields at the sites and the accumulator their scores."""
    from test_gpu_drain import _stats_last as stats_last_of
    m, (inp, inp_s, stats, maps, const_h) = setup
    sl = stats_last_of(stats)
    N = site_plan.N
    up0, sf0 = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph)
    g = torch.Generator(device="cpu").manual_seed(62)
    obs = []
    for k in range(2):
        ou, os_ = torch.randn(1, 5, 13, N, generator=g), torch.randn(1, 4, N, generator=g)
        ou[torch.rand(ou.shape, generator=g) < 0.3] = float("nan")
        obs.append((ou.cuda(), os_.cuda()))
    kept = []
    series = _recording(P, kept, site_plan, 2)
    acc = P.score.ObservationAccumulator(2, site_plan, clim=sl)
    up1, sf1 = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, sites=series, observations=acc,
                                 obs=obs)
    assert torch.equal(up0, up1) and torch.equal(sf0, sf1)
    assert [k for k, _, _ in kept] == [0, 1] and acc.cases(0) == 1 and acc.cases(1) == 1
    assert torch.equal(kept[1][1], up1) and torch.equal(kept[1][2], sf1)             # the last step's physical fields
    for k, ku, ks in kept:
        su, ss = P.score.sample_points(ku, ks, site_plan)
        assert torch.equal(series.upper[k], su) and torch.equal(series.surface[k], ss)
        want = P.score.observation_scores(ku, ks, *obs[k], site_plan, clim=sl)
        for got, ref in zip(acc.result(k), want):
            assert torch.equal(got.sums, ref.sums.reshape(got.sums.shape))
    arrays = plan_arrays(site_plan)
    assert same_bits(series.surface[1].cpu().numpy().reshape(4, N), sample_points_ref(sf1.cpu().numpy().reshape(4, 721, 1440), *arrays))
    assert bool((acc.result(1)[0].counts[..., 0] > 0).all()) and bool(torch.isfinite(acc.result(1)[1].rmse).all())
    # an entry of None skips that lead
    acc2 = P.score.ObservationAccumulator(2, site_plan)
    P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, observations=acc2, obs=[None, obs[1]])
    assert acc2.cases(0) == 0 and acc2.cases(1) == 1


def test_rollout_checks_the_hooks_before_the_first_step(P, setup, site_plan):
    from test_gpu_drain import _stats_last as stats_last_of
    m, (inp, inp_s, stats, maps, const_h) = setup
    sl = stats_last_of(stats)

    class NeverCalled(torch.nn.Module):
        def forward(self, *a):
            raise AssertionError("the model ran before the arguments were checked")

    run = lambda **kw: P.rollout.rollout(NeverCalled(), inp, inp_s, stats, maps, const_h, sl, steps=2, graph=False, **kw)
    acc, pair = P.score.ObservationAccumulator(2, site_plan), (None, None)
    with pytest.raises(ValueError, match="observations and obs go together"):
        run(observations=acc)
    with pytest.raises(ValueError, match="observations and obs go together"):
        run(obs=[None, None])
    with pytest.raises(ValueError, match="3 obs entries for 2 steps"):
        run(observations=acc, obs=[None, None, None])
    with pytest.raises(ValueError, match="holds 1 leads"):
        run(observations=P.score.ObservationAccumulator(1, site_plan), obs=[None, None])
    with pytest.raises(ValueError, match="holds 1 leads"):
        run(sites=P.score.PointSeries(site_plan, 1))
    with pytest.raises(ValueError, match="a pair"):
        run(observations=acc, obs=[None, (1, 2, 3)])


@pytest.mark.timeout(300)
def test_ensemble_members_are_more_planes(P, setup, site_plan):
    """Ensemble rollouts need no hook: sample_points takes EnsembleRollout's member tensors through the leading dimension."""
    from test_gpu_drain import _stats_last as stats_last_of
    m, (inp, inp_s, stats, maps, const_h) = setup
    ens = P.ensemble.EnsembleRollout(m, inp, inp_s, stats, maps, const_h, stats_last_of(stats), members=2, amplitude=0.05, seed=7)
    ens.step()
    up, sf = ens.state()
    su, ss = P.score.sample_points(up, sf, site_plan)
    assert su.shape == (2, 5, 13, site_plan.N) and ss.shape == (2, 4, site_plan.N)
    for e in range(2):
        mu, ms = P.score.sample_points(up[e].contiguous(), sf[e].contiguous(), site_plan)
        assert torch.equal(su[e], mu) and torch.equal(ss[e], ms)
    assert not torch.equal(su[0], su[1])                                             # the members differ
    series = P.score.PointSeries(site_plan, 1)
    series.record(0, up, sf)
    assert torch.equal(series.surface[0], ss) and series.wind_speed10().shape == (1, 2, site_plan.N)
