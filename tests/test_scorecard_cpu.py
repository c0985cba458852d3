"""Regional scorecard, the part that needs no GPU: the float64 restatement of pangu_scorecard_sums_f32 (scorecard_ref, which the
GPU tests import), score.region_bits, the ScoreSums algebra, ScoreAccumulator pooling, the argument checks of both C entries and
the argument checks of rollout(scorecard=, targets=)."""
import os

import numpy as np
import pytest
import torch

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib

S = P.score


def scorecard_ref(pred, target, clim, clim_kind, w, bits, R, target_levels=0):
    """pangu_scorecard_sums_f32 in numpy float64.  pred / target (planes, H, W) fp32; clim None, (planes,) or (planes, H, W); w (H,)
    fp32; bits (H, W) uint8 or None (one region of every point).  Returns (sums, mag), both (planes, R, 10) float64: the ten sums,
    and for the sums 0..8 the sum of |w * term| over the same points (mag[..., 9] = the count), the scale of the error bound."""
    planes, H, W = pred.shape
    order = np.arange(planes)
    if target_levels > 1:
        order = order.reshape(-1, target_levels)[:, ::-1].reshape(-1)
    p, t = pred.astype(np.float64), target[order].astype(np.float64)
    if clim_kind == 0:
        c = np.zeros((planes, 1, 1))
    elif clim_kind == 1:
        c = np.asarray(clim, np.float64).reshape(planes, 1, 1)
    else:
        c = np.asarray(clim, np.float64).reshape(planes, H, W)
    d, a, b = p - t, p - c, t - c
    ww = np.broadcast_to(np.asarray(w, np.float64)[None, :, None], p.shape)
    terms = [np.ones_like(p), d, np.abs(d), d * d, a + 0 * p, b + 0 * p, a * b, a * a, b * b]
    sums, mag = np.zeros((planes, R, 10)), np.zeros((planes, R, 10))
    for r in range(R):
        inside = np.ones((H, W), bool) if bits is None else ((bits >> r) & 1).astype(bool)
        for k, term in enumerate(terms):
            x = (ww * term)[:, inside]
            sums[:, r, k] = x.sum(axis=1)
            mag[:, r, k] = np.abs(x).sum(axis=1)
        sums[:, r, 9] = mag[:, r, 9] = inside.sum()
    return sums, mag


def box(H, W, lat, lon):
    """The region rule, restated directly: closed latitude ends, a half-open longitude range that wraps."""
    rows = np.array([90.0 - 180.0 * j / (H - 1) for j in range(H)])
    cols = np.array([360.0 * i / W for i in range(W)])
    width = lon[1] - lon[0]
    if width <= 0:
        width += 360.0
    in_col = np.array([((x - lon[0]) % 360.0) < width for x in cols])
    return ((rows >= lat[0]) & (rows <= lat[1]))[:, None] & in_col[None, :]


def bit(plan, name):
    return ((plan.bits.numpy() >> plan.names.index(name)) & 1).astype(bool)


# ---- region_bits -------------------------------------------------------------------------------------------------------------

def test_region_bits_small_grid():
    regions = {"tropics": "tropics", "nh": "nh_extratropics", "pacific": "north_pacific", "europe": "europe",
               "own": dict(lat=(-30.0, 15.0), lon=(350.0, 20.0))}
    plan = S.region_bits(13, 24, regions)
    assert plan.names == tuple(regions) and plan.R == 5 and plan.bits.dtype == torch.uint8 and tuple(plan.bits.shape) == (13, 24)
    lat = 90.0 - 15.0 * np.arange(13)
    assert np.array_equal(bit(plan, "tropics"), np.broadcast_to(((lat >= -20) & (lat <= 20))[:, None], (13, 24)))
    assert np.array_equal(bit(plan, "nh"), np.broadcast_to((lat >= 20)[:, None], (13, 24)))
    # the wrapping Pacific box: 145 E .. 130 W = columns 150 .. 225 degrees, rows 60, 45, 30
    want = np.zeros((13, 24), bool)
    want[2:5, 10:16] = True
    assert np.array_equal(bit(plan, "pacific"), want)
    # Europe: -12.5 .. 42.5 holds the columns 0, 15, 30 but not 345
    want = np.zeros((13, 24), bool)
    want[1:4, 0:3] = True
    assert np.array_equal(bit(plan, "europe"), want)
    # a box across the prime meridian, closed latitude ends on grid rows: rows 15 .. -30 = 5 .. 8, columns 350 .. 20 = 0, 15
    want = np.zeros((13, 24), bool)
    want[5:9, 0:2] = True
    assert np.array_equal(bit(plan, "own"), want)
    assert S.region_bits(13, 24, regions) is plan                                   # cached
    glob = S.region_bits(13, 24)
    assert glob.names == ("global",) and bool((glob.bits == 1).all())


def test_region_bits_closed_latitude_ends_at_full_size():
    plan = S.region_bits(721, 1440, {"tropics": "tropics", "nh": "nh_extratropics", "sh": "sh_extratropics"})
    j20 = 280                                                                       # 90 - 180 * 280 / 720 = 20 exactly
    assert bit(plan, "tropics")[j20].all() and bit(plan, "nh")[j20].all() and not bit(plan, "sh")[j20].any()
    assert not bit(plan, "tropics")[j20 - 1].any() and bit(plan, "nh")[j20 - 1].all()
    assert bit(plan, "tropics")[440].all() and bit(plan, "sh")[440].all() and not bit(plan, "tropics")[441].any()


def test_region_presets_point_counts_at_full_size():
    names = list(S.REGION_PRESETS)
    assert len(names) == 12
    for part in (names[:8], names[8:]):
        plan = S.region_bits(721, 1440, {n: n for n in part})
        for n in part:
            lat, lon = S.REGION_PRESETS[n]
            want = box(721, 1440, lat, lon)
            assert np.array_equal(bit(plan, n), want), n
            assert want.sum() > 0
    assert box(721, 1440, *S.REGION_PRESETS["global"]).sum() == 721 * 1440
    assert box(721, 1440, *S.REGION_PRESETS["europe"]).sum() == 161 * 220          # rows 75 .. 35, columns -12.5 .. 42.25
    assert box(721, 1440, *S.REGION_PRESETS["north_pacific"]).sum() == 141 * 340    # rows 60 .. 25, 85 degrees of longitude


def test_region_bits_mask_and_refusals():
    g = torch.Generator().manual_seed(3)
    mask = torch.rand((13, 24), generator=g) > 0.5
    plan = S.region_bits(13, 24, {"land_box": dict(lat=(-45, 60), lon=(30, 200), mask=mask), "land": dict(mask=mask)})
    assert np.array_equal(bit(plan, "land_box"), box(13, 24, (-45, 60), (30, 200)) & mask.numpy())
    assert np.array_equal(bit(plan, "land"), mask.numpy())
    with pytest.raises(ValueError, match="regions"):
        S.region_bits(13, 24, {f"r{i}": "global" for i in range(9)})
    with pytest.raises(ValueError, match="preset"):
        S.region_bits(13, 24, {"x": "atlantis"})
    with pytest.raises(ValueError, match="mask"):
        S.region_bits(13, 24, {"x": dict(mask=torch.ones((13, 25), dtype=torch.bool))})
    with pytest.raises(ValueError, match="lat_lo"):
        S.region_bits(13, 24, {"x": dict(lat=(10, -10))})


# ---- ScoreSums ------------------------------------------------------------------------------------------------------------------

def _points(seed, planes=69, n=40):
    r = np.random.default_rng(seed)
    p = 280.0 + 5.0 * r.standard_normal((planes, n))
    t = p + r.standard_normal((planes, n))
    c = 279.0 + r.standard_normal((planes, n))
    w = r.uniform(0.2, 1.5, n)
    member = r.random((2, n)) > 0.4                                                # two regions
    return p, t, c, w, member


def _sums_of(p, t, c, w, member):
    d, a, b = p - t, p - c, t - c
    terms = [np.ones_like(p), d, np.abs(d), d * d, a, b, a * b, a * a, b * b]
    out = np.zeros((p.shape[0], member.shape[0], 10))
    for r, m in enumerate(member):
        for k, x in enumerate(terms):
            out[:, r, k] = (w * x)[:, m].sum(axis=1)
        out[:, r, 9] = m.sum()
    return out


def _score_sums(raw):
    up = S.ScoreSums(torch.from_numpy(raw[:65].reshape(5, 13, -1, 10)), ("a", "b"))
    sf = S.ScoreSums(torch.from_numpy(raw[65:]), ("a", "b"))
    return up, sf


def test_score_sums_algebra():
    p, t, c, w, member = _points(1)
    up, sf = _score_sums(_sums_of(p, t, c, w, member))
    close = lambda got, want: np.allclose(got.numpy().reshape(want.shape), want, rtol=1e-12, atol=1e-12)
    for r, m in enumerate(member):
        ww = w[m] / w[m].sum()
        d, a, b = (p - t)[:, m], (p - c)[:, m], (t - c)[:, m]
        mean = lambda x: (ww * x).sum(axis=1)
        want = {"bias": mean(d), "mae": mean(np.abs(d)), "mse": mean(d * d), "rmse": np.sqrt(mean(d * d)),
                "acc": mean(a * b) / np.sqrt(mean(a * a) * mean(b * b))}
        ac, bc = a - mean(a)[:, None], b - mean(b)[:, None]
        want["acc_centred"] = mean(ac * bc) / np.sqrt(mean(ac * ac) * mean(bc * bc))
        want["activity_forecast"], want["activity_target"] = np.sqrt(mean(ac * ac)), np.sqrt(mean(bc * bc))
        for name, x in want.items():
            assert close(getattr(up, name)[..., r], x[:65]), name
            assert close(getattr(sf, name)[..., r], x[65:]), name
        assert bool((up.counts[..., r] == int(m.sum())).all()) and up.counts.dtype == torch.int64
        du, dv = d[:65].reshape(5, 13, -1)[3], d[:65].reshape(5, 13, -1)[4]
        assert close(up.wind_rmse()[:, r], np.sqrt((ww * (du * du + dv * dv)).sum(axis=1)))
        assert close(sf.wind_rmse()[r], np.sqrt((ww * (d[66] ** 2 + d[67] ** 2)).sum()))
    assert up.rmse.shape == (5, 13, 2) and up.wind_rmse().shape == (13, 2) and sf.wind_rmse().shape == (2,)
    one = up.region("b")
    assert one.names == ("b",) and torch.equal(one.rmse[..., 0], up.rmse[..., 1])
    with pytest.raises(KeyError):
        up.region("c")


def test_skill_and_centred_acc_invariance():
    p, t, c, w, member = _points(2)
    up, _ = _score_sums(_sums_of(p, t, c, w, member))
    persist, _ = _score_sums(_sums_of(p + 3.0, t, c, w, member))
    want = 1.0 - up.rmse / persist.rmse
    assert torch.equal(up.skill(persist), want) and bool((want > 0).all())
    other = S.ScoreSums(persist.sums, ("a", "x"))
    with pytest.raises(ValueError, match="regions"):
        up.skill(other)
    shifted, _ = _score_sums(_sums_of(p, t, c + 7.5, w, member))
    assert np.allclose(shifted.acc_centred.numpy(), up.acc_centred.numpy(), rtol=0, atol=1e-9)
    assert not np.allclose(shifted.acc.numpy(), up.acc.numpy(), rtol=0, atol=1e-3)     # the uncentred form does depend on it
    assert np.allclose(shifted.activity_forecast.numpy(), up.activity_forecast.numpy(), rtol=1e-9)


# ---- ScoreAccumulator -----------------------------------------------------------------------------------------------------------

def test_accumulator_pools_cases():
    p1, t1, c1, w, member = _points(5)
    p2, t2, c2, _, _ = _points(6)
    acc = S.ScoreAccumulator(3)
    assert acc.cases(1) == 0
    acc.add(1, *_score_sums(_sums_of(p1, t1, c1, w, member)))
    acc.add(1, *_score_sums(_sums_of(p2, t2, c2, w, member)))
    cat = lambda x, y: np.concatenate((x, y), axis=1)
    both = _sums_of(cat(p1, p2), cat(t1, t2), cat(c1, c2), np.concatenate((w, w)), np.concatenate((member, member), axis=1))
    up, sf = acc.sums(1)
    assert acc.cases(1) == 2 and up.cases == 2
    assert np.allclose(up.sums.numpy().reshape(65, 2, 10), both[:65], rtol=1e-13, atol=0)
    assert np.allclose(sf.sums.numpy(), both[65:], rtol=1e-13, atol=0)
    # a stack of cases in one ScoreSums pools the same way
    acc2 = S.ScoreAccumulator(1)
    u1, s1 = _score_sums(_sums_of(p1, t1, c1, w, member))
    u2, s2 = _score_sums(_sums_of(p2, t2, c2, w, member))
    acc2.add(0, S.ScoreSums(torch.stack((u1.sums, u2.sums)), u1.names), S.ScoreSums(torch.stack((s1.sums, s2.sums)), s1.names))
    assert acc2.cases(0) == 2 and torch.equal(acc2.sums(0)[0].sums, up.sums) and torch.equal(acc2.sums(0)[1].sums, sf.sums)
    table = acc.table(1)
    assert table["regions"] == ("a", "b") and table["cases"] == 2
    assert set(S.SCORECARD_METRICS) <= set(table) and table["rmse"].shape == (69, 2)
    assert np.allclose(table["rmse"], np.sqrt(both[..., 3] / both[..., 0]), rtol=1e-12)
    with pytest.raises(IndexError):
        acc.add(3, u1, s1)
    with pytest.raises(IndexError):
        acc.cases(-1)
    with pytest.raises(ValueError, match="nothing scored"):
        acc.sums(0)
    with pytest.raises(ValueError, match="regions"):
        acc.add(0, S.ScoreSums(u1.sums, ("a", "c")), S.ScoreSums(s1.sums, ("a", "c")))
    with pytest.raises(ValueError):
        S.ScoreAccumulator(0)


# ---- the C entries ------------------------------------------------------------------------------------------------------------------

def test_entry_argument_checks_without_gpu():
    """Every refusal returns before a launch: dummy non-NULL addresses, as tests/test_abi.py uses them."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    NULL, SHAPE, ARG = -2, -1, -4
    ws_bytes = lib.pangu_scorecard_ws_bytes
    assert ws_bytes(69, 721, 8) == 69 * 23 * 8 * 40 == S.scorecard_workspace_bytes(69, 721, 8)
    assert ws_bytes(1, 32, 1) == 40 and ws_bytes(1, 33, 1) == 80 and ws_bytes(3, 5, 2) == 3 * 1 * 2 * 40     # planes ceil(H / 32) R 40
    assert ws_bytes(69, 721, 1) == 69 * 23 * 40 == S.scorecard_workspace_bytes(69, 721, 1)
    assert ws_bytes(0, 721, 1) == SHAPE and ws_bytes(1, 0, 1) == SHAPE and ws_bytes(1, 721, 0) == SHAPE and ws_bytes(1, 721, 9) == SHAPE
    assert ws_bytes(1 << 30, 721, 1) == SHAPE                                       # more workgroups than a grid holds
    A = 1 << 20                                                                      # an address aligned for everything
    big = 1 << 40

    def call(pred=A, target=A, levels=0, clim=None, kind=0, w=A, bits=A, R=2, sums=A, ws=A, ws_bytes=big, planes=10, H=13, W=24):
        return lib.pangu_scorecard_sums_f32(None, pred, target, levels, clim, kind, w, bits, R, sums, ws, ws_bytes, planes, H, W)

    for name in ("pred", "target", "w", "sums", "ws"):
        assert call(**{name: None}) == NULL, name
    assert call(kind=1) == NULL and call(kind=2) == NULL                            # a climatology kind without clim
    assert call(bits=None, R=2) == NULL                                             # no mask: one region only
    assert call(W=26) == SHAPE and call(W=0) == SHAPE and call(H=0) == SHAPE and call(planes=0) == SHAPE
    assert call(H=1 << 16, W=1 << 15) == SHAPE                                      # H * W = 2^31
    assert call(R=0) == SHAPE and call(R=9) == SHAPE
    assert call(levels=3) == SHAPE and call(levels=-1) == SHAPE                     # 10 planes are no multiple of 3
    assert call(kind=3, clim=A) == ARG and call(kind=-1, clim=A) == ARG
    assert call(ws_bytes=10 * 1 * 2 * 40 - 1) == ARG                                # one byte short
    for name in ("pred", "target", "ws"):
        assert call(**{name: A + 8}) == ARG, name                                   # 16 B
    assert call(kind=2, clim=A + 8) == ARG and call(kind=1, clim=A + 2) == ARG
    assert call(sums=A + 4) == ARG and call(bits=A + 2) == ARG and call(w=A + 2) == ARG


# ---- rollout(scorecard=, targets=) ------------------------------------------------------------------------------------------------

def test_rollout_refuses_a_scorecard_without_targets():
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("rollout touched the model before it checked its arguments")

        def __call__(self, *a, **k):
            raise AssertionError("rollout called the model before it checked its arguments")

    acc = S.ScoreAccumulator(2)
    x = torch.zeros(1)
    args = (Untouchable(), x, x, None, None, None, None)
    for graph in (True, False):
        with pytest.raises(ValueError, match="go together"):
            P.rollout.rollout(*args, steps=2, graph=graph, scorecard=acc, targets=None)
        with pytest.raises(ValueError, match="go together"):
            P.rollout.rollout(*args, steps=2, graph=graph, targets=[None, None])
        with pytest.raises(ValueError, match="3 targets for 2 steps"):
            P.rollout.rollout(*args, steps=2, graph=graph, scorecard=acc, targets=[None] * 3)
        with pytest.raises(ValueError, match="leads"):
            P.rollout.rollout(*args, steps=3, graph=graph, scorecard=acc, targets=[None] * 3)
    assert acc.cases(0) == 0


def test_reference_restatement_on_a_hand_case():
    """scorecard_ref itself: two points in one region, one in another, level reversal, against sums written out by hand."""
    pred = np.array([[[1.0, 2.0, 4.0, 8.0]], [[0.0, 0.0, 0.0, 0.0]]], np.float32)            # (2, 1, 4)
    target = np.array([[[9.0, 9.0, 9.0, 9.0]], [[0.5, 4.0, 1.0, 8.0]]], np.float32)
    bits = np.array([[1, 3, 0, 2]], np.uint8)
    w = np.array([2.0], np.float32)
    sums, mag = scorecard_ref(pred, target, np.array([1.0, 0.0]), 1, w, bits, 2, target_levels=2)
    # plane 0 reads target plane 1; region 0 = points 0, 1: d = 0.5, -2; a = 0, 1; b = -0.5, 3
    assert np.array_equal(sums[0, 0], [4.0, -3.0, 5.0, 8.5, 2.0, 5.0, 6.0, 2.0, 18.5, 2.0])
    assert np.array_equal(mag[0, 0], [4.0, 5.0, 5.0, 8.5, 2.0, 7.0, 6.0, 2.0, 18.5, 2.0])
    # region 1 = points 1, 3: d = -2, 0; a = 1, 7; b = 3, 7
    assert np.array_equal(sums[0, 1], [4.0, -4.0, 4.0, 8.0, 16.0, 20.0, 104.0, 100.0, 116.0, 2.0])
