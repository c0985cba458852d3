"""Regional scorecard on the GPU: pangu_scorecard_sums_f32 against the float64 restatement of tests/test_scorecard_cpu.py, the
Python surface (score.deterministic_scores, ScoreSums, ScoreAccumulator) and rollout(scorecard=, targets=).

The bound is derived from csrc/scorecard.hip, not measured: |got - ref| <= (n + c) * 2^-24 * sum |w * term| with
  n = 190  the longest chain of fp32 additions a term can pass through for W <= 2048 (one column tile of at most 8 waves): in its
           lane 3 within its word and at most 32 in its class accumulator (one fma per row of the slab), 2 when the two classes join
           the region accumulators, and at most 4 * 32 from the points of deferred words (a lane takes at most 32 of them, four
           points each); then 15 + 2 across the wave, 1 into the per-wave sum over column tiles and 7 across eight waves; the
           slab partials are added in double;
  c = 5    the roundings a term carries apart from additions: one in each of its two factors (d, a, b are fp32 differences), one in
           their product and one in the product with the weight (the deferred points; the words' fma fuses it), and one for the second-order terms and
           the two float64 summations (the kernel's over the slabs and the reference's).
The count (index 9) and every sum of an empty region must be exact.  Worst |error| / bound seen on an MI355X, per case of
test_kernel_matches_reference (which prints them):
    (3, 5, 8) R = 1 without a mask 0.008;  (7, 13, 24) R = 8 boxes and a random mask 0.012;  (4, 19, 36) R = 4 bands, scalar
    climatology 0.013;  (2, 9, 1440) R = 3 0.010;  (2, 721, 16) R = 2 0.004;  (10, 13, 24) level-reversed, climatology field 0.018;
    (4, 721, 1440) R = 8 presets and a land mask 0.007;  the other tests 0.007 .. 0.026 (deterministic_scores, 65 planes)."""
import numpy as np
import pytest
import torch

from test_gpu_regrid import SCORE_RTOL, field
from test_scorecard_cpu import scorecard_ref

pytestmark = pytest.mark.gpu

POISON = -7.25e33
N_ADD, C_TERM = 190, 5
EPS = (N_ADD + C_TERM) * 2.0 ** -24


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    P._lib.load()
    return P


def lat_w(P, H):
    return P.score.latitude_weights(H, "cuda")


def abi_sums(P, pred, target, bits, R, clim=None, kind=0, levels=0, guard=32, ws_extra=256):
    """pred / target (planes, H, W) fp32 numpy (or CUDA tensors), bits (H, W) uint8 numpy or None -> sums (planes, R, 10) float64
    numpy through the C ABI on the current stream.  sums and the workspace are filled with poison first; the guard behind sums and
    the tail of the workspace must come back untouched and no poison may be left in sums."""
    dev = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pred, target = dev(pred), dev(target)
    planes, H, W = pred.shape
    lib = P._lib.load()
    n = planes * R * 10
    sums = torch.full((n + guard,), POISON, dtype=torch.float64, device="cuda")
    need = lib.pangu_scorecard_ws_bytes(planes, H, R)
    assert need == P.score.scorecard_workspace_bytes(planes, H, R)
    ws = torch.full((need + ws_extra,), 0xA5, dtype=torch.uint8, device="cuda")
    c = None if clim is None else dev(np.asarray(clim, np.float32))
    b = None if bits is None else dev(bits)
    w = lat_w(P, H)
    P._lib.check(lib.pangu_scorecard_sums_f32(
        torch.cuda.current_stream().cuda_stream, pred.data_ptr(), target.data_ptr(), levels, None if c is None else c.data_ptr(), kind,
        w.data_ptr(), None if b is None else b.data_ptr(), R, sums.data_ptr(), ws.data_ptr(), need, planes, H, W), "scorecard")
    torch.cuda.synchronize()
    assert bool((sums[n:] == POISON).all()), "wrote behind sums"
    assert bool((ws[need:] == 0xA5).all()), "wrote behind the workspace"
    out = sums[:n].view(planes, R, 10)
    assert not bool((out == POISON).any()), "left part of sums unwritten"
    return out.cpu().numpy()


def check(P, got, pred, target, bits, R, clim=None, kind=0, levels=0, what="", regions=None):
    """got against scorecard_ref within the derived bound, the counts exactly.  Returns the worst |error| / bound."""
    w = lat_w(P, pred.shape[1]).cpu().numpy()
    ref, mag = scorecard_ref(pred, target, clim, kind, w, bits, R, levels)
    rs = list(range(R)) if regions is None else regions
    assert np.array_equal(got[:, rs, 9], ref[:, rs, 9]), f"{what}: counts"
    err = np.abs(got[:, rs, :9] - ref[:, rs, :9])
    bound = EPS * mag[:, rs, :9]
    assert np.array_equal(err[bound == 0], np.zeros_like(err[bound == 0])), f"{what}: an empty sum is not exactly zero"
    worst = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f"scorecard {what} {pred.shape} R={R}: worst |error| / bound = {worst:.4f}")
    assert worst <= 1.0, what
    return worst


def fields(planes, H, W, seed):
    """A forecast and its analysis: the field() of tests/test_gpu_regrid.py and a perturbed copy."""
    p = field(planes, H, W, seed)
    t = (p + 1.5 * np.random.default_rng(seed + 77).standard_normal(p.shape)).astype(np.float32)
    return p, t


def plan_bits(P, H, W, regions):
    return P.score.region_bits(H, W, regions).bits.numpy()


def bits_boxes8(P):
    """13 x 24: overlapping boxes whose edges fall on columns that are no multiple of 4, one wrapping, and a random per-point mask."""
    mask = torch.from_numpy(np.random.default_rng(8).random((13, 24)) > 0.5)
    return plan_bits(P, 13, 24, {
        "global": "global", "a": dict(lat=(-50, 50), lon=(15, 150)), "b": dict(lat=(0, 90), lon=(75, 225)),
        "wrap": dict(lat=(-90, 30), lon=(315, 45)), "random": dict(mask=mask), "random_box": dict(lat=(-60, 60), lon=(30, 300), mask=mask),
        "one_column": dict(lon=(45, 60)), "tropics": "tropics"})


def synthetic_land(H, W):
    lat = np.linspace(0.5 * np.pi, -0.5 * np.pi, H)[:, None]
    lon = (2.0 * np.pi * np.arange(W) / W)[None, :]
    return torch.from_numpy(np.sin(3 * lon + 2 * np.sin(2 * lat)) * np.cos(2 * lat) + 0.3 * np.sin(7 * lon + 5 * lat) > 0.15)


BANDS4 = {"global": "global", "nh": "nh_extratropics", "tropics": "tropics", "sh": "sh_extratropics"}
FULL8 = dict(BANDS4, europe="europe", north_america="north_america", north_pacific="north_pacific")


def case_setup(P, name):
    """-> pred, target, bits, R, clim, kind, levels"""
    r = np.random.default_rng(len(name))
    if name == "one-slab-null-mask":                       # fewer rows than a slab, a row of two float4
        return fields(3, 5, 8, 1) + (None, 1, None, 0, 0)
    if name == "boxes8":                                   # the non-uniform mask word and the region-switch path
        return fields(7, 13, 24, 2) + (bits_boxes8(P), 8, None, 0, 0)
    if name == "bands4-clim-scalar":                       # H no multiple of the slab
        return fields(4, 19, 36, 3) + (plan_bits(P, 19, 36, BANDS4), 4, r.uniform(270, 290, 4).astype(np.float32), 1, 0)
    if name == "full-row":                                 # the full row width: six waves, the last one partly idle
        return fields(2, 9, 1440, 4) + (plan_bits(P, 9, 1440, {"global": "global", "europe": dict(lat=(0, 90), lon=(-12.5, 42.5)),
                                                               "pacific": dict(lon=(145, -130))}), 3, None, 0, 0)
    if name == "full-height":                              # every slab of the full height: the reduce over all slabs
        return fields(2, 721, 16, 5) + (plan_bits(P, 721, 16, {"nh": "nh_extratropics", "tropics": "tropics"}), 2, None, 0, 0)
    if name == "levels-clim-field":                        # level reversal, the third read
        p, t = fields(10, 13, 24, 6)
        return p, t, plan_bits(P, 13, 24, {"global": "global", "a": dict(lat=(-50, 50), lon=(15, 150))}), 2, field(10, 13, 24, 66) - 1.0, 2, 5
    if name == "product":                                  # one full-size case: presets and a synthetic land mask
        land = synthetic_land(721, 1440)
        return fields(4, 721, 1440, 7) + (plan_bits(P, 721, 1440, dict(FULL8, land=dict(mask=land))), 8, None, 0, 0)
    raise KeyError(name)


CASES = ["one-slab-null-mask", "boxes8", "bands4-clim-scalar", "full-row", "full-height", "levels-clim-field", "product"]


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_reference(P, name):
    pred, target, bits, R, clim, kind, levels = case_setup(P, name)
    got = abi_sums(P, pred, target, bits, R, clim, kind, levels)
    check(P, got, pred, target, bits, R, clim, kind, levels, what=name)


def test_masked_single_region_and_clim_kinds(P):
    """R = 1 with a mask (its own kernel variant), and every climatology kind of the variants with 1 and 8 accumulators."""
    pred, target = fields(3, 19, 36, 11)
    cf = field(3, 19, 36, 12) - 2.0
    cs = np.array([279.0, 281.5, 283.0], np.float32)
    for bits, R in ((plan_bits(P, 19, 36, {"box": dict(lat=(-40, 70), lon=(25, 215))}), 1), (None, 1),
                    (np.random.default_rng(4).integers(0, 256, (19, 36)).astype(np.uint8), 8)):
        for clim, kind in ((None, 0), (cs, 1), (cf, 2)):
            got = abi_sums(P, pred, target, bits, R, clim, kind)
            check(P, got, pred, target, bits, R, clim, kind, what=f"R={R} mask={bits is not None} clim_kind={kind}")


def test_bits_of_regions_beyond_R_are_ignored(P):
    pred, target = fields(2, 13, 24, 13)
    bits = np.random.default_rng(5).integers(0, 256, (13, 24)).astype(np.uint8)
    got = abi_sums(P, pred, target, bits, 3)
    assert np.array_equal(got, abi_sums(P, pred, target, bits & 7, 3))
    check(P, got, pred, target, bits, 3, what="high bits")


def test_empty_region_and_single_point(P):
    pred, target = fields(3, 13, 24, 14)
    bits = np.zeros((13, 24), np.uint8)
    bits[:, :] = 1                                          # region 0: everything; region 1: empty; region 2: one point
    bits[7, 10] |= 4
    cs = np.array([280.0, 281.0, 282.0], np.float32)
    got = abi_sums(P, pred, target, bits, 3, cs, 1)
    assert np.array_equal(got[:, 1], np.zeros((3, 10)))
    check(P, got, pred, target, bits, 3, cs, 1, what="empty+single")
    w = np.float64(lat_w(P, 13).cpu().numpy()[7])
    for pl in range(3):
        p, t = pred[pl, 7, 10], target[pl, 7, 10]
        d, a, b = np.float32(p - t), np.float32(p - cs[pl]), np.float32(t - cs[pl])
        want = np.array([1.0, d, abs(d), np.float64(d) * d, a, b, np.float64(a) * b, np.float64(a) * a, np.float64(b) * b]) * w
        assert np.allclose(got[pl, 2, :9], want, rtol=4 * 2.0 ** -24, atol=0) and got[pl, 2, 9] == 1.0


def test_nonfinite_values_stay_in_their_regions(P):
    """A NaN and an infinity in pred at points that lie in regions 0 and 2 only: exactly those regions' sums are non-finite."""
    pred, target = fields(5, 19, 36, 15)
    r = np.random.default_rng(16)
    bits = r.integers(0, 16, (19, 36)).astype(np.uint8)
    spots = ((1, 3, 7), (1, 12, 20), (4, 18, 35))           # (plane, row, column); plane 4: the last row and column
    for _, h, x in spots:
        bits[h, x] = 0b0101
    clean = pred.copy()
    pred[1, 3, 7] = np.nan
    pred[1, 12, 20] = np.inf
    pred[4, 18, 35] = -np.inf
    for clim, kind in ((None, 0), (field(5, 19, 36, 17), 2)):
        got = abi_sums(P, pred, target, bits, 4, clim, kind)
        for pl in (1, 4):
            for reg in (0, 2):
                assert not np.isfinite(got[pl, reg, 1:4]).any() and np.isfinite(got[pl, reg, [0, 9]]).all(), (pl, reg)
        finite = np.isfinite(got).all(axis=2)
        want = np.ones((5, 4), bool)
        want[[1, 1, 4, 4], [0, 2, 0, 2]] = False
        assert np.array_equal(finite, want)
        # the other regions never read those points: the reference with them replaced serves
        check(P, got, clean, target, bits, 4, clim, kind, what=f"nan+inf clim_kind={kind}", regions=[1, 3])
        check(P, got[[0, 2, 3]], clean[[0, 2, 3]], target[[0, 2, 3]], bits, 4, None if clim is None else clim[[0, 2, 3]], kind,
              what="nan+inf, the clean planes")


def test_bit_identical_and_independent_of_the_other_planes(P):
    pred, target = fields(7, 37, 1440, 18)
    bits = plan_bits(P, 37, 1440, dict(FULL8, land=dict(mask=synthetic_land(37, 1440))))
    cf = field(7, 37, 1440, 19)
    for clim, kind in ((None, 0), (cf, 2)):
        a = abi_sums(P, pred, target, bits, 8, clim, kind)
        b = abi_sums(P, pred, target, bits, 8, clim, kind)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "not bit-identical from run to run"
        for pl in (0, 3, 6):
            one = abi_sums(P, pred[pl:pl + 1], target[pl:pl + 1], bits, 8, None if clim is None else clim[pl:pl + 1], kind)
            assert np.array_equal(one[0].view(np.uint64), a[pl].view(np.uint64)), f"plane {pl} depends on its neighbours"


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def _state(B, H, W, seed):
    x = field(B * 69, H, W, seed).reshape(B, 69, H, W)
    up = torch.from_numpy(np.ascontiguousarray(x[:, :65])).cuda().view(B, 5, 13, H, W)
    sf = torch.from_numpy(np.ascontiguousarray(x[:, 65:])).cuda()
    return up, sf


def _stats_last(seed):
    r = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    return (t(r.uniform(275, 285, (1, 4, 1, 1))), t(r.uniform(0.5, 3, (1, 4, 1, 1))),
            t(r.uniform(275, 285, (1, 5, 13, 1, 1))), t(r.uniform(0.5, 3, (1, 5, 13, 1, 1))))


def test_deterministic_scores_against_the_existing_scores(P):
    H, W = 19, 36
    up, sf = _state(2, H, W, 21)
    tu, ts = _state(2, H, W, 22)
    su, ss = P.score.deterministic_scores(up, sf, tu, ts)
    assert su.names == ("global",) and su.sums.shape == (2, 5, 13, 1, 10) and ss.sums.shape == (2, 4, 1, 10)
    assert su.sums.dtype == torch.float64 and su.sums.is_cuda
    close = lambda got, want: bool(((got - want.double()).abs() <= SCORE_RTOL * want.double().abs()).all())
    for s, p, t in ((su, up, tu), (ss, sf, ts)):
        assert close(s.rmse[..., 0], P.score.weighted_rmse_channels(p, t))
        assert close(s.acc[..., 0], P.score.weighted_acc_channels(p, t))
        assert bool((s.counts == H * W).all())
    # stats_last as the climatology: the ACC of ensemble_scores for an ensemble of two identical members
    sl = _stats_last(23)
    cu, cs = P.score.deterministic_scores(up[0], sf[0], tu[0], ts[0], clim=sl)
    eu, es = P.score.ensemble_scores(torch.stack((up[0], up[0])), torch.stack((sf[0], sf[0])), tu[:1], ts[:1], sl)
    assert cu.sums.shape == (5, 13, 1, 10) and close(cu.acc[..., 0], eu["acc_mean"]) and close(cs.acc[..., 0], es["acc_mean"])
    assert close(cu.rmse[..., 0], eu["rmse_mean"]) and close(cs.rmse[..., 0], es["rmse_mean"])


def test_deterministic_scores_cases_levels_regions_and_wind(P):
    H, W = 13, 24
    up, sf = _state(6, H, W, 31)
    tu, ts = _state(6, H, W, 32)
    plan = P.score.region_bits(H, W, {"global": "global", "box": dict(lat=(-50, 50), lon=(15, 150)), "tropics": "tropics"}, "cuda")
    sl = _stats_last(33)
    clim_fields = _state(1, H, W, 34)
    clim_fields = (clim_fields[0][0], clim_fields[1][0])
    eq = lambda a, b: np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
    for clim in (None, sl, clim_fields):
        # leading case dimensions (2, 3): case for case what a call on that case gives
        shaped = lambda t: t.view((2, 3) + tuple(t.shape[1:]))
        su, ss = P.score.deterministic_scores(shaped(up), shaped(sf), shaped(tu), shaped(ts), plan, clim)
        assert su.sums.shape == (2, 3, 5, 13, 3, 10) and ss.sums.shape == (2, 3, 4, 3, 10) and su.names == plan.names
        for i in range(6):
            ou, os_ = P.score.deterministic_scores(up[i], sf[i], tu[i], ts[i], plan, clim)
            assert eq(ou.sums, su.sums[i // 3, i % 3]) and eq(os_.sums, ss.sums[i // 3, i % 3])
        # a target stored with its level axis reversed
        ru, rs = P.score.deterministic_scores(up, sf, tu.flip(2).contiguous(), ts, plan, clim, target_levels_reversed=True)
        assert eq(ru.sums, su.sums.view(ru.sums.shape)) and eq(rs.sums, ss.sums.view(rs.sums.shape))
    # the same through a mapping and against the reference, wind_rmse against numpy
    su, ss = P.score.deterministic_scores(up[0], sf[0], tu[0], ts[0], {"global": "global", "box": dict(lat=(-50, 50), lon=(15, 150)),
                                                                      "tropics": "tropics"})
    bits = plan.bits.cpu().numpy()
    flat = lambda t: t.reshape(-1, H, W).cpu().numpy()
    check(P, su.sums.reshape(65, 3, 10).cpu().numpy(), flat(up[0]), flat(tu[0]), bits, 3, what="deterministic_scores upper")
    check(P, ss.sums.reshape(4, 3, 10).cpu().numpy(), flat(sf[0]), flat(ts[0]), bits, 3, what="deterministic_scores surface")
    w = lat_w(P, H).double().cpu().numpy()[None, :, None]
    for r in range(3):
        m = ((bits >> r) & 1).astype(bool)
        d = (up[0].double() - tu[0].double()).cpu().numpy()
        want = np.sqrt(((w * (d[3] ** 2 + d[4] ** 2))[:, m]).sum(axis=1) / np.broadcast_to(w, (13, H, W))[:, m].sum(axis=1))
        assert np.allclose(su.wind_rmse()[:, r].cpu().numpy(), want, rtol=1e-5)
        d = (sf[0].double() - ts[0].double()).cpu().numpy()
        want = np.sqrt((w[0] * (d[1] ** 2 + d[2] ** 2))[m].sum() / np.broadcast_to(w[0], (H, W))[m].sum())
        assert np.allclose(ss.wind_rmse()[r].cpu().numpy(), want, rtol=1e-5)
    # an accumulator pools what it scores
    acc = P.score.ScoreAccumulator(2, plan, sl)
    acc.score(1, up[:2], sf[:2], tu[:2], ts[:2])
    acc.score(1, up[2], sf[2], tu[2], ts[2])
    assert acc.cases(1) == 3 and acc.cases(0) == 0
    want_u, want_s = P.score.deterministic_scores(up[:3], sf[:3], tu[:3], ts[:3], plan, sl)
    assert torch.allclose(acc.sums(1)[0].sums, want_u.sums.sum(0), rtol=1e-14, atol=0)
    assert torch.allclose(acc.sums(1)[1].sums, want_s.sums.sum(0), rtol=1e-14, atol=0)
    assert acc.table(1)["rmse"].shape == (69, 3)
    # mismatches raise
    with pytest.raises(ValueError, match="region plan"):
        P.score.deterministic_scores(up[..., :12, :].contiguous(), sf[..., :12, :].contiguous(), tu[..., :12, :].contiguous(),
                                     ts[..., :12, :].contiguous(), plan)
    with pytest.raises(RuntimeError, match="float32"):
        P.score.deterministic_scores(up.double(), sf, tu, ts)
    with pytest.raises(ValueError, match="target"):
        P.score.deterministic_scores(up, sf, tu[:2], ts)
    with pytest.raises(ValueError, match="clim"):
        P.score.deterministic_scores(up, sf, tu, ts, clim=(tu,))


# ---- rollout(scorecard=, targets=) ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup(P):
    import cases
    import synth
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return m, cases.model_inputs("cuda")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("graph", [True, False])
def test_rollout_scores_every_step(P, setup, graph):
    """The model and inputs of tests/test_gpu_drain.py::test_rollout_drains_every_step, fp32, 2 steps: the hook leaves the returned
    fields untouched, is handed every step's physical fields, and pools per lead exactly what deterministic_scores gives."""
    from test_gpu_drain import _stats_last as stats_last_of
    m, (inp, inp_s, stats, maps, const_h) = setup
    sl = stats_last_of(stats)
    up0, sf0, hist = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, keep=True)
    g = torch.Generator(device="cuda").manual_seed(5)
    targets = [(inp + torch.randn(inp.shape, generator=g, device="cuda"), inp_s + torch.randn(inp_s.shape, generator=g, device="cuda"))
               for _ in range(2)]
    regions = {"global": "global", "nh": "nh_extratropics", "europe": "europe"}
    kept = []

    class Recording(P.score.ScoreAccumulator):
        def score(self, lead, upper, surface, target_upper, target_surface):
            kept.append((lead, upper.clone(), surface.clone()))
            return super().score(lead, upper, surface, target_upper, target_surface)

    acc = Recording(2, regions, sl)
    up1, sf1 = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, scorecard=acc, targets=targets)
    assert torch.equal(up0, up1) and torch.equal(sf0, sf1)
    assert [k for k, _, _ in kept] == [0, 1]
    assert torch.equal(kept[1][1], up1) and torch.equal(kept[1][2], sf1)           # the last step's physical fields
    for (k, up, sf), (out, out_s) in zip(kept, hist):
        for got, want in zip((up, sf), P.rollout.norm_back(out, out_s, sl)):
            assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-5, atol=1e-3)
        want_u, want_s = P.score.deterministic_scores(up, sf, *targets[k], regions, sl)
        got_u, got_s = acc.sums(k)
        assert acc.cases(k) == 1 and got_u.names == ("global", "nh", "europe")
        assert torch.equal(got_u.sums, want_u.sums[0]) and torch.equal(got_s.sums, want_s.sums[0])
        assert bool(torch.isfinite(got_u.rmse).all()) and bool((got_u.rmse > 0).all())
    if not graph:                                                                    # a None target leaves its lead empty
        empty = P.score.ScoreAccumulator(2, regions, sl)
        P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=False, scorecard=empty, targets=[None, targets[1]])
        assert empty.cases(0) == 0 and empty.cases(1) == 1
        assert torch.equal(empty.sums(1)[0].sums, acc.sums(1)[0].sums) and torch.equal(empty.sums(1)[1].sums, acc.sums(1)[1].sums)
