"""Conservative regridding without a GPU: the remapping plan (score.regrid_plan), a numpy float64 restatement of the remap that the
GPU tests compare the kernel against (regrid_ref), and the argument checks of pangu_regrid_planes_f32."""
import os

import numpy as np
import pytest

from pangu_pytorch_amd import _lib, score

F32 = np.float32

# (H_in, W_in, H_out, W_out) -> (latitude taps, longitude taps, taps of the polar latitude row)
TAPS = {
    (721, 1440, 121, 240): (7, 7, 4),
    (721, 1440, 181, 360): (5, 5, 3),
    (721, 1440, 73, 144): (11, 11, 6),
    (721, 1440, 241, 480): (3, 3, 2),
    (721, 1440, 361, 720): (3, 3, 2),
    (721, 1440, 100, 250): (9, 7, None),
}
SMALL = [(13, 24, 5, 8), (13, 24, 7, 12), (19, 30, 7, 9), (11, 10, 4, 3), (41, 40, 5, 4)]      # the last: 11 taps per axis
GRIDS = list(TAPS) + SMALL


def regrid_ref(x, plan, mul=None, add=None, levels=0):
    """out = R_lat . v . R_lon^T per plane in float64, from the plan's float64 dense matrices (not from its band tables).  x
    (planes, H_in, W_in) float32; v = x * mul + add in float32, two roundings, mul / add indexed by SOURCE plane; with levels = L
    output plane v*L + l reads source plane v*L + (L-1-l).  Returns (out, bound_scale): the float64 result and |R_lat| . |v| .
    |R_lon|^T, the magnitude the kernel's error bound is relative to."""
    x = np.asarray(x, F32)
    planes = x.shape[0]
    v = x
    if mul is not None:
        v = (x * np.asarray(mul, F32)[:, None, None]).astype(F32)
        v = (v + np.asarray(add, F32)[:, None, None]).astype(F32)
    if levels > 1:
        src = np.arange(planes).reshape(planes // levels, levels)[:, ::-1].reshape(-1)
        v = v[src]
    r_lat, r_lon = plan.dense()
    v = v.astype(np.float64)
    with np.errstate(invalid="ignore"):
        out = np.einsum("Jj,pji,Ii->pJI", r_lat, v, r_lon, optimize=True)
        mag = np.einsum("Jj,pji,Ii->pJI", np.abs(r_lat), np.abs(v), np.abs(r_lon), optimize=True)
    return out, mag


def error_bound(plan, mag):
    """(T_lat + T_lon + 4) * 2^-24 * |R_lat| |v| |R_lon|^T: the forward error of two sequential fp32 fma chains of T_lat and T_lon
    taps with fp32-rounded weights (each tap's product carries the weight's rounding and the chain's roundings after it: at most
    T + 1 factors (1 + d), |d| <= 2^-24, per chain, to first order; + 2 covers the second-order terms)."""
    return (plan.lat_taps + plan.lon_taps + 4) * 2.0 ** -24 * mag


def stencil_nonfinite(x_bad, plan):
    """Where a non-finite input reaches: x_bad (planes, H_in, W_in) bool -> (planes, H_out, W_out) bool."""
    r_lat, r_lon = plan.dense()
    return np.einsum("Jj,pji,Ii->pJI", (r_lat > 0).astype(np.float64), x_bad.astype(np.float64), (r_lon > 0).astype(np.float64)) > 0


def cell_areas(H):
    """Normalised areas of the latitude cells of the H-row grid (sin(latitude) between the cell edges)."""
    edges = np.clip(90.0 - (2.0 * np.arange(H + 1) - 1.0) * 90.0 / (H - 1), -90.0, 90.0)
    s = np.sin(np.deg2rad(edges))
    a = s[:-1] - s[1:]
    return a / a.sum()


def band_to_dense(start, count, weights, n_in):
    out = np.zeros((len(start), n_in), np.float64)
    for r in range(len(start)):
        assert 1 <= count[r] <= weights.shape[1]
        assert (weights[r, count[r]:] == 0).all()
        for t in range(count[r]):
            out[r, (start[r] + t) % n_in] += np.float64(weights[r, t])
    return out


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_plan_properties(grid):
    H_in, W_in, H_out, W_out = grid
    plan = score.regrid_plan(*grid)
    r_lat, r_lon = plan.dense()
    assert r_lat.shape == (H_out, H_in) and r_lon.shape == (W_out, W_in) and r_lat.dtype == r_lon.dtype == np.float64
    for r in (r_lat, r_lon):
        assert (r >= 0).all() and np.abs(r.sum(axis=1) - 1.0).max() <= 1e-12
    # conservation: the area-weighted sum of the output equals that of the input
    assert np.abs(cell_areas(H_out) @ r_lat - cell_areas(H_in)).max() <= 1e-12
    assert np.abs(np.full(W_out, 1.0 / W_out) @ r_lon - 1.0 / W_in).max() <= 1e-12
    # the band tables are the dense matrices, rounded once to float32
    for start, count, w, dense, n_in in ((plan.lat_start, plan.lat_count, plan.lat_weights, r_lat, H_in),
                                         (plan.lon_start, plan.lon_count, plan.lon_weights, r_lon, W_in)):
        assert start.dtype == count.dtype == np.int32 and w.dtype == F32 and w.shape == (len(start), count.max())
        assert np.array_equal(band_to_dense(start, count, w, n_in).astype(F32), dense.astype(F32))
    assert (plan.lat_start >= 0).all() and (plan.lat_start + plan.lat_count <= H_in).all()      # the kernel's contract
    assert (plan.lon_start > -W_in).all() and (plan.lon_start < W_in).all()
    assert 1 <= plan.lat_taps <= 16 and 1 <= plan.lon_taps <= 16
    if grid in TAPS:
        t_lat, t_lon, polar = TAPS[grid]
        assert (plan.lat_taps, plan.lon_taps) == (t_lat, t_lon)
        if polar is not None:
            assert plan.lat_count[0] == plan.lat_count[-1] == polar


def test_product_grid_rows():
    plan = score.regrid_plan(721, 1440, 121, 240)
    want = (np.array([1, 2, 2, 2, 2, 2, 1]) / 12.0).astype(F32)
    assert (plan.lon_count == 7).all() and all(np.array_equal(plan.lon_weights[i], want) for i in range(240))
    assert plan.lon_start[0] == -3 and np.array_equal(plan.lon_start[1:], 6 * np.arange(1, 240) - 3)      # centred on 6 I, wrapped
    r_lon = plan.dense()[1]
    assert r_lon[0, 1437] == 1 / 12 and r_lon[0, 1438] == r_lon[0, 0] == r_lon[0, 2] == 1 / 6 and r_lon[0, 3] == 1 / 12
    assert plan.lat_count[0] == 4 and plan.lat_start[0] == 0 and plan.lat_start[-1] + plan.lat_count[-1] == 721
    assert (plan.lat_count[1:-1] == 7).all() and np.array_equal(plan.lat_start[1:-1], 6 * np.arange(1, 120) - 3)


def test_identity_plan():
    plan = score.regrid_plan(13, 24, 13, 24)
    assert plan.lat_taps == plan.lon_taps == 1
    assert np.array_equal(plan.lat_start, np.arange(13)) and np.array_equal(plan.lon_start, np.arange(24))
    assert (plan.lat_count == 1).all() and (plan.lon_count == 1).all()
    assert (plan.lat_weights == 1).all() and (plan.lon_weights == 1).all()
    assert np.array_equal(plan.dense()[0], np.eye(13)) and np.array_equal(plan.dense()[1], np.eye(24))


@pytest.mark.parametrize("grid, word", [((13, 24, 14, 24), "H_out"), ((13, 24, 1, 24), "H_out"), ((13, 24, 7, 25), "W_out"),
                                        ((13, 24, 7, 0), "W_out"), ((721, 1440, 20, 240), "taps"), ((721, 1440, 121, 60), "taps")])
def test_plan_limits(grid, word):
    with pytest.raises(ValueError, match=word):
        score.regrid_plan(*grid)


def test_reference_constant_and_global_mean():
    for grid in SMALL + [(37, 48, 7, 9)]:
        plan = score.regrid_plan(*grid)
        H_in, W_in, H_out, W_out = grid
        out, mag = regrid_ref(np.full((2, H_in, W_in), 271.5, F32), plan)
        assert np.abs(out - 271.5).max() <= 1e-10 and np.abs(mag - 271.5).max() <= 1e-10
        lat = np.deg2rad(90.0 - np.arange(H_in) * 180.0 / (H_in - 1))
        x = np.repeat(np.cos(lat)[None, :, None], W_in, axis=2).astype(F32)
        out, _ = regrid_ref(x, plan)
        mean_in = (cell_areas(H_in)[:, None] * x[0].astype(np.float64)).sum() / W_in
        mean_out = (cell_areas(H_out)[:, None] * out[0]).sum() / W_out
        assert abs(mean_out - mean_in) <= 1e-12
        assert np.abs(out[0] - out[0][:, :1]).max() <= 1e-12                       # still zonally constant


def test_reference_affine_and_levels():
    plan = score.regrid_plan(13, 24, 7, 12)
    r = np.random.default_rng(3)
    x = r.standard_normal((6, 13, 24)).astype(F32)
    mul, add = np.linspace(0.5, 3, 6).astype(F32), np.linspace(-200, 900, 6).astype(F32)
    out, _ = regrid_ref(x, plan, mul, add, levels=3)
    v2 = ((x[2] * mul[2]).astype(F32) + add[2]).astype(F32)                        # output plane 0 reads source plane 2
    want, _ = regrid_ref(v2[None], plan)
    assert np.array_equal(out[0], want[0])
    bad = np.zeros((6, 13, 24), bool)
    bad[1, 6, 23] = True                                                           # the last column: output columns 11 and 0 (wrap)
    hit = stencil_nonfinite(bad, plan)
    assert hit.sum() == 2 and hit[1, 3, 0] and hit[1, 3, 11]


needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libpangu_hip.so not built")


@needs_lib
def test_argument_validation_without_gpu():
    lib = _lib.load()
    P8 = 16         # any non-NULL address: the calls below return before touching memory
    fn = lib.pangu_regrid_planes_f32
    good = [None, P8, None, None, P8, 26, 13, 24, 7, 12, P8, P8, P8, 3, P8, P8, P8, 3, 13]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)

    for i in (1, 4, 10, 11, 12, 14, 15, 16):                   # src, dst, the six tables
        assert call(**{f"a{i}": None}) == -2, i
    assert call(a2=P8) == -2 and call(a3=P8) == -2             # mul without add, add without mul
    for i in (5, 6, 7, 8, 9):                                  # planes, H_in, W_in, H_out, W_out
        assert call(**{f"a{i}": 0}) == -1 and call(**{f"a{i}": -3}) == -1, i
    assert call(a8=14) == -1 and call(a9=25) == -1             # refinement
    for i in (13, 17):                                         # taps outside 1..16
        assert call(**{f"a{i}": 0}) == -1 and call(**{f"a{i}": 17}) == -1, i
    assert call(a5=27) == -1 and call(a18=-1) == -1            # planes % levels, levels < 0
    assert call(a1=P8 + 2) == -4 and call(a4=P8 + 1) == -4     # alignment
    assert call(a6=1 << 18, a7=1 << 13, a8=2, a9=2) == -1      # H_in * W_in >= 2^31
    assert call(a5=1 << 20, a18=0, a6=1 << 12, a8=1 << 11) == -1      # planes * H_out: more workgroups than a grid holds
    assert call(a7=16388, a9=12) == -1                         # a row longer than the LDS stage
