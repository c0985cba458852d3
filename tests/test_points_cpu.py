"""The observation operator without a GPU: score.point_plan against a scalar restatement of its recipe, its invariants, region bits
and errors; the numpy restatements of the kernels' pinned arithmetic (tests/test_gpu_points.py compares the kernels with them bit
for bit) and their own accuracy; the host-side argument checks of the two C entries."""
import math
import os

import numpy as np
import pytest
import torch

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib, score

F32 = np.float32
U24 = 2.0 ** -24
GRIDS = [(2, 4), (7, 12), (33, 1021), (721, 1440)]
POINT_CHUNK = 1024                               # csrc/points.hip PT_CHUNK
POINT_FP32_ADDS = 3 + 6 + 3                      # csrc/points.hip PT_FP32_ADDS: in the lane, in the wave, across the four waves


# ---- restatements -------------------------------------------------------------------------------------------------------------------

def point_plan_ref(H, W, lat, lon):
    """row, col (int32) and wy, wx (float32) of the issue's recipe, one point at a time in Python floats (float64)."""
    n = len(lat)
    row, col = np.zeros(n, np.int32), np.zeros(n, np.int32)
    wy, wx = np.zeros(n, F32), np.zeros(n, F32)
    for i in range(n):
        y = (90.0 - float(lat[i])) * (H - 1) / 180.0
        r = min(math.floor(y), H - 1)
        fy = F32(y - r)
        x = (float(lon[i]) % 360.0) * W / 360.0
        c = math.floor(x)
        fx = F32(x - c)
        if c >= W:
            c, fx = 0, F32(0.0)
        if fy == F32(1.0):
            r, fy = r + 1, F32(0.0)
        if fx == F32(1.0):
            c, fx = (c + 1) % W, F32(0.0)
        row[i], col[i], wy[i], wx[i] = r, c, fy, fx
    return row, col, wy, wx


def src_planes(planes, levels):
    """output plane -> source plane (csrc/plane_value.h pk_src_plane)."""
    p = np.arange(planes)
    if levels <= 1:
        return p
    return (p // levels) * levels + (levels - 1 - p % levels)


def sample_points_ref(src, row, col, wy, wx, mul=None, add=None, levels=0):
    """src (planes, H, W) float32 -> (planes, N) float32 in the pinned order of csrc/points.hip, every operation rounded to float32:
    v = src * mul + add per SOURCE plane, the two lines, then the column; a weight of zero selects."""
    planes, H, W = src.shape
    q = src_planes(planes, levels)
    with np.errstate(all="ignore"):
        v = src[q]
        if mul is not None:
            v = v * mul[q][:, None, None].astype(F32) + add[q][:, None, None].astype(F32)
        assert v.dtype == F32
        row, col = row.astype(np.int64), col.astype(np.int64)
        c1, r1 = (col + 1) % W, np.minimum(row + 1, H - 1)
        ux, uy = F32(1.0) - wx, F32(1.0) - wy

        def line(r):
            return np.where(wx == 0, v[:, r, col], v[:, r, col] * ux + v[:, r, c1] * wx)

        l0, l1 = line(row), line(r1)
        f = np.where(wy == 0, l0, l0 * uy + l1 * wy)
    assert f.dtype == F32
    return f


def point_terms(f, obs, clim=None):
    """(d, the eight float32 terms (8, planes, N) of sums[1..8], valid) for f, obs (planes, N) float32 and clim (planes,) or None."""
    c = np.zeros(f.shape[0], F32) if clim is None else clim.astype(F32)
    with np.errstate(all="ignore"):
        d, a, b = f - obs, f - c[:, None], obs - c[:, None]
        terms = np.stack([d, np.abs(d), d * d, a, b, a * b, a * a, b * b])
    assert terms.dtype == F32
    return d, terms, ~np.isnan(obs)


def point_sums_ref(f, obs, clim=None, bits=None, R=1):
    """(sums, abs_sums) float64 (planes, R, 10): the float32 terms of the valid points of each region added in float64 ([0] and [9]
    their number), and the sums of the terms' magnitudes, which scale the error bound."""
    planes, N = f.shape
    _, terms, valid = point_terms(f, obs, clim)
    bits = np.ones(N, np.uint8) if bits is None else bits
    sums, mags = np.zeros((planes, R, 10)), np.zeros((planes, R, 10))
    for r in range(R):
        inside = valid & (((bits >> r) & 1) == 1)[None, :]
        n = inside.sum(1)
        sums[:, r, 0] = sums[:, r, 9] = n
        t = np.where(inside[None], terms.astype(np.float64), 0.0)
        sums[:, r, 1:9] = t.sum(-1).T
        mags[:, r, 1:9] = np.abs(t).sum(-1).T
    return sums, mags


def point_sums_bound(mags, N):
    """|kernel - point_sums_ref| <= this (csrc/points.hip, 'Rounding of the sums'): PT_FP32_ADDS fp32 additions on the longest path,
    one double addition per chunk, and the float64 additions of the reference itself."""
    gamma = lambda n, u: n * u / (1.0 - n * u)
    chunks = (N + POINT_CHUNK - 1) // POINT_CHUNK
    return (gamma(POINT_FP32_ADDS, U24) + gamma(chunks + N, 2.0 ** -53)) * mags


def special_points(H, W, rng, n_random):
    """Random points plus the poles, the longitudes that wrap, points exactly on nodes and a duplicate."""
    lat = list(rng.uniform(-90.0, 90.0, n_random))
    lon = list(rng.uniform(-400.0, 800.0, n_random))
    for la in (90.0, -90.0):
        for lo in (0.0, 123.4):
            lat.append(la), lon.append(lo)
    for lo in (0.0, 360.0, -1e-13, 359.99999999999, -180.0, 540.0):
        lat.append(float(rng.uniform(-80.0, 80.0))), lon.append(lo)
    for j, i in ((0, 0), (H - 1, W - 1), (H // 2, W // 2), (1 % H, W - 1)):
        lat.append(90.0 - 180.0 * j / (H - 1)), lon.append(360.0 * i / W)
    lat.append(lat[0]), lon.append(lon[0])                      # a duplicate
    lat.append(lat[1]), lon.append(lon[1] + 360.0)              # and the same place a turn further
    return np.array(lat), np.array(lon)


def plan_arrays(plan):
    return tuple(t.cpu().numpy() for t in (plan.row, plan.col, plan.wy, plan.wx))


# ---- the plan -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", GRIDS, ids=[f"{h}x{w}" for h, w in GRIDS])
def test_plan_equals_the_restatement_and_keeps_its_invariants(grid):
    H, W = grid
    lat, lon = special_points(H, W, np.random.default_rng(H * 7919 + W), 20000 if H > 100 else 4000)
    plan = score.point_plan(H, W, lat, lon)
    row, col, wy, wx = plan_arrays(plan)
    ref = point_plan_ref(H, W, lat, lon)
    for got, want, name in zip((row, col, wy, wx), ref, ("row", "col", "wy", "wx")):
        assert got.dtype == want.dtype and np.array_equal(got, want), name
    assert (plan.N, plan.H, plan.W, plan.R, plan.names) == (lat.size, H, W, 1, ("global",)) and plan.everywhere
    assert plan.bits.dtype == torch.uint8 and bool((plan.bits == 1).all())
    assert ((wy >= 0) & (wy < 1) & (wx >= 0) & (wx < 1)).all()
    assert ((row >= 0) & (row < H) & (col >= 0) & (col < W)).all()
    assert (wy[row == H - 1] == 0).all()
    n = lat.size
    # the poles, the wrapping longitudes and the nodes sit where they belong
    assert (row[-16:-14] == 0).all() and (row[-14:-12] == H - 1).all() and (wy[-16:-12] == 0).all()
    assert col[-12] == 0 and wx[-12] == 0 and col[-11] == 0 and wx[-11] == 0                  # lon = 0 and 360
    assert col[-10] in (0, W - 1) and col[-9] in (0, W - 1)                                   # lon = -1e-13 and 359.99999999999
    half = 0.0 if W % 2 == 0 else 0.5
    assert col[-8] == W // 2 and wx[-8] == half and col[-7] == W // 2 and wx[-7] == half      # -180 and 540
    for k, (j, i) in zip(range(n - 6, n - 2), ((0, 0), (H - 1, W - 1), (H // 2, W // 2), (1 % H, W - 1))):
        assert (row[k], col[k], wy[k]) == (j, i, 0.0), (k, j, i)
        if (360.0 * i / W) * W / 360.0 == i:                 # the node's longitude is a float64: the point is on it exactly
            assert wx[k] == 0.0, (k, j, i)
        else:
            assert wx[k] < 1e-5, (k, j, i)
    assert (row[-2], col[-2], wy[-2], wx[-2]) == (row[0], col[0], wy[0], wx[0])
    assert (row[-1], col[-1], wy[-1]) == (row[1], col[1], wy[1]) and abs(float(wx[-1]) - float(wx[1])) < 1e-6 * W


def test_plan_keeps_the_callers_order_and_accepts_tensors():
    lat, lon = [10.0, -33.25, 10.0], [5.0, 700.0, 5.0]
    a = score.point_plan(7, 12, lat, lon)
    b = score.point_plan(7, 12, torch.tensor(lat, dtype=torch.float64), torch.tensor(lon, dtype=torch.float64))
    for x, y in zip(plan_arrays(a), plan_arrays(b)):
        assert np.array_equal(x, y)
    assert a.row[0] == a.row[2] and a.col[0] == a.col[2] and a.row[0] != a.row[1]


def test_region_bits_at_the_points():
    H, W = 33, 64
    rng = np.random.default_rng(5)
    mask = torch.from_numpy(rng.random((H, W)) < 0.4)
    regions = {"tropics": "tropics", "europe": "europe", "dateline": dict(lat=(-30.0, 50.0), lon=(170.0, -170.0)),
               "land": dict(mask=mask)}
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    lat = np.concatenate([rng.uniform(-90, 90, 3000), (90.0 - 180.0 * jj / (H - 1)).ravel(), [20.0, -20.0, 35.0, 50.0, 50.0]])
    lon = np.concatenate([rng.uniform(-360, 720, 3000), (360.0 * ii / W).ravel(), [10.0, 10.0, -12.5, 42.5, 170.0]])
    plan = score.point_plan(H, W, lat, lon, regions)
    assert plan.names == ("tropics", "europe", "dateline", "land") and plan.R == 4 and not plan.everywhere
    bits = plan.bits.numpy()
    row, col, wy, wx = plan_arrays(plan)
    l360 = np.mod(lon, 360.0)
    want = [(lat >= -20) & (lat <= 20),
            (lat >= 35) & (lat <= 75) & ((l360 >= 347.5) | (l360 < 42.5)),
            (lat >= -30) & (lat <= 50) & (l360 >= 170.0) & (l360 < 190.0),
            mask.numpy()[row + (wy >= 0.5), (col + (wx >= 0.5)) % W]]
    for r, w in enumerate(want):
        assert np.array_equal((bits >> r) & 1, w.astype(np.uint8)), plan.names[r]
    # points exactly on nodes carry the bits region_bits gives their node (the semantics of _region_box)
    on_grid = score.region_bits(H, W, regions).bits.numpy()
    assert np.array_equal(bits[3000:3000 + H * W].reshape(H, W), on_grid)
    # closed latitude ends, half-open longitude ends
    assert [int(b) & 3 for b in bits[-5:]] == [1, 1, 2, 0, 0] and (bits[-1] >> 2) & 1 == 1
    with pytest.raises(ValueError, match="point_plan"):
        score.point_plan(H, W, lat, lon, {str(i): "global" for i in range(9)})
    with pytest.raises(ValueError, match="point_plan"):
        score.point_plan(H, W, lat, lon, {"a": dict(mask=torch.zeros(3, 3, dtype=torch.bool))})


@pytest.mark.parametrize("lat,lon", [([90.5], [0.0]), ([-90.0001], [0.0]), ([float("nan")], [0.0]), ([0.0], [float("inf")]),
                                     ([0.0], [float("nan")]), ([], []), ([0.0, 1.0], [0.0]), ([[0.0]], [[0.0]])])
def test_plan_rejects_bad_points(lat, lon):
    with pytest.raises(ValueError, match="point_plan"):
        score.point_plan(7, 12, lat, lon)


def test_plan_rejects_bad_grids():
    for H, W in ((1, 4), (0, 4), (4, 0)):
        with pytest.raises(ValueError, match="point_plan"):
            score.point_plan(H, W, [0.0], [0.0])


# ---- the restated sampling ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", GRIDS, ids=[f"{h}x{w}" for h, w in GRIDS])
def test_restated_sample_is_close_to_float64_bilinear(grid):
    """Six roundings lie on the longest path (1 - wx, the product, the line's sum, 1 - wy is beside it, the product, the sum) and the
    weights sum to 1, so the restated sample stays within 6 * 2^-24 * max|corner| of the float64 bilinear value of the same fp32
    weights to first order; 7 leaves room for the second-order terms."""
    H, W = grid
    rng = np.random.default_rng(11 + H)
    lat, lon = special_points(H, W, rng, 5000)
    row, col, wy, wx = plan_arrays(score.point_plan(H, W, lat, lon))
    src = (rng.standard_normal((2, H, W)) * 30.0 + 250.0).astype(F32)
    src[1] = rng.standard_normal((H, W)).astype(F32)                        # a plane around zero
    f = sample_points_ref(src, row, col, wy, wx)
    r, c = row.astype(np.int64), col.astype(np.int64)
    c1, r1 = (c + 1) % W, np.minimum(r + 1, H - 1)
    s = src.astype(np.float64)
    wx64, wy64 = wx.astype(np.float64), wy.astype(np.float64)
    exact = ((s[:, r, c] * (1 - wx64) + s[:, r, c1] * wx64) * (1 - wy64) + (s[:, r1, c] * (1 - wx64) + s[:, r1, c1] * wx64) * wy64)
    corner = np.max(np.abs(np.stack([s[:, r, c], s[:, r, c1], s[:, r1, c], s[:, r1, c1]])), axis=0)
    ratio = np.abs(f.astype(np.float64) - exact) / (U24 * corner)
    print(f"{H}x{W}: worst error {ratio.max():.2f} x 2^-24 max|corner|")
    assert ratio.max() <= 7.0
    on_node = (wx == 0) & (wy == 0)
    assert on_node.sum() >= 3
    assert np.array_equal(f[:, on_node].view(np.uint32), src[:, row[on_node], col[on_node]].view(np.uint32))


def test_restated_sample_selects_zero_weight_taps():
    """A NaN and an infinity at nodes reach exactly the points whose stencil holds them with a non-zero weight."""
    H, W = 7, 12
    src = np.arange(H * W, dtype=F32).reshape(1, H, W)
    src[0, 3, 5], src[0, 2, 0] = np.nan, np.inf
    lat_of, lon_of = lambda j: 90.0 - 180.0 * j / (H - 1), lambda i: 360.0 * i / W
    pts = [(lat_of(3), lon_of(4)), (lat_of(2), lon_of(5)), (lat_of(3), lon_of(5)), (lat_of(2.5), lon_of(5)), (lat_of(3), lon_of(4.5)),
           (lat_of(2), lon_of(11)), (lat_of(2), lon_of(11.5)), (lat_of(1.5), lon_of(11.75)), (lat_of(2), lon_of(0))]
    lat, lon = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    f = sample_points_ref(src, *plan_arrays(score.point_plan(H, W, lat, lon)))[0]
    assert list(np.isnan(f)) == [False, False, True, True, True, False, False, False, False]
    assert list(np.isinf(f)) == [False, False, False, False, False, False, True, True, True]
    assert f[0] == 3 * W + 4 and f[1] == 2 * W + 5 and f[5] == 2 * W + 11


def test_level_reversal_and_affine_follow_the_source_plane():
    rng = np.random.default_rng(3)
    src = rng.standard_normal((6, 5, 8)).astype(F32)
    mul, add = rng.uniform(0.5, 2.0, 6).astype(F32), rng.uniform(-5.0, 5.0, 6).astype(F32)
    row, col, wy, wx = plan_arrays(score.point_plan(5, 8, [90.0 - 180.0 * 2 / 4], [45.0 * 3]))
    f = sample_points_ref(src, row, col, wy, wx, mul, add, levels=3)
    want = np.array([F32(src[q, 2, 3] * mul[q]) + add[q] for q in (2, 1, 0, 5, 4, 3)], F32)
    assert np.array_equal(f[:, 0], want)


def test_sums_restatement_counts_reports_and_regions():
    f = np.array([[1.0, 2.0, 4.0, 8.0]], F32)
    obs = np.array([[0.0, np.nan, 1.0, np.inf]], F32)
    sums, mags = point_sums_ref(f, obs, np.array([1.0], F32), np.array([1, 1, 3, 2], np.uint8), R=3)
    assert sums[0, 0].tolist() == [2.0, 4.0, 4.0, 10.0, 3.0, -1.0, 0.0, 9.0, 1.0, 2.0]
    assert sums[0, 1, 0] == 2 and np.isinf(sums[0, 1, 2]) and not sums[0, 2].any()
    assert mags[0, 0, 5] == 1.0 and point_sums_bound(mags, 4)[0, 0, 3] > 0


# ---- the C entries' host side ---------------------------------------------------------------------------------------------------------

def test_point_entries_validate_their_arguments_without_gpu():
    """Bad arguments are rejected on the host before any launch (no GPU needed)."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built")
    lib = _lib.load()
    P8 = 8                      # any non-NULL aligned address: the calls below return before touching memory
    NULL, SHAPE, ARG = -2, -1, -4
    sample = lambda src=P8, mul=None, add=None, row=P8, col=P8, wy=P8, wx=P8, out=P8, planes=6, H=7, W=12, N=5, levels=0: \
        lib.pangu_sample_points_f32(None, src, mul, add, row, col, wy, wx, out, planes, H, W, N, levels)
    for name in ("src", "row", "col", "wy", "wx", "out"):
        assert sample(**{name: None}) == NULL, name
    assert sample(mul=P8) == NULL and sample(add=P8) == NULL
    for kw in (dict(planes=0), dict(H=1), dict(H=0), dict(W=0), dict(N=0), dict(N=-3), dict(H=65536, W=32768), dict(planes=3, N=1 << 30),
               dict(levels=-1), dict(levels=4)):
        assert sample(**kw) == SHAPE, kw
    for name in ("src", "row", "col", "wy", "wx", "out"):
        assert sample(**{name: 10}) == ARG, name
    assert sample(mul=6, add=P8) == ARG
    scores = lambda src=P8, mul=None, add=None, row=P8, col=P8, wy=P8, wx=P8, obs=P8, clim=None, bits=None, R=1, dep=None, sums=P8, \
        ws=P8, ws_bytes=1 << 40, planes=6, H=7, W=12, N=5, levels=0: \
        lib.pangu_point_scores_f32(None, src, mul, add, row, col, wy, wx, obs, clim, bits, R, dep, sums, ws, ws_bytes, planes, H, W, N,
                                   levels)
    for name in ("src", "row", "col", "wy", "wx", "obs", "sums", "ws"):
        assert scores(**{name: None}) == NULL, name
    assert scores(mul=P8) == NULL and scores(R=2) == NULL                     # no region bits: one region only
    for kw in (dict(planes=0), dict(H=1), dict(W=0), dict(N=0), dict(H=65536, W=32768), dict(planes=3, N=1 << 30), dict(levels=-1),
               dict(levels=4), dict(bits=P8, R=0), dict(bits=P8, R=9)):
        assert scores(**kw) == SHAPE, kw
    need = lib.pangu_point_scores_ws_bytes(6, 5, 1)
    assert need == 6 * 1 * 1 * 40 and scores(ws_bytes=need - 1) == ARG
    assert scores(bits=P8, R=3, ws_bytes=need) == ARG                         # three regions need three times the workspace
    for name in ("src", "row", "col", "wy", "wx", "obs", "clim", "dep", "ws"):
        assert scores(**{name: 10}) == ARG, name
    assert scores(sums=12) == ARG                                             # 8 B for the doubles


def test_point_scores_workspace_size():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built")
    ws = _lib.load().pangu_point_scores_ws_bytes
    assert ws(1, 1, 1) == 40 and ws(1, POINT_CHUNK, 1) == 40 and ws(1, POINT_CHUNK + 1, 1) == 80
    assert ws(69, 10000, 3) == 69 * 10 * 3 * 40 == score.point_scores_workspace_bytes(69, 10000, 3)
    assert score.POINT_CHUNK == POINT_CHUNK
    sizes = [(1, 1, 1), (1, 5000, 1), (2, 5000, 1), (2, 5000, 8), (69, 5000, 8), (69, 1000000, 8), (1, (1 << 31) - 1, 8)]
    got = [ws(*s) for s in sizes]
    assert all(g > 0 for g in got) and got == sorted(got)
    for n0 in (1, 1023, 1024, 4096):
        assert ws(3, n0, 2) <= ws(3, n0 + 1, 2) <= ws(4, n0 + 1, 2) <= ws(4, n0 + 1, 3)
    for bad in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, 5, 0), (5, 5, 9), (2, 1 << 30, 1), (69, 1 << 25, 1)):
        assert ws(*bad) == -1, bad
