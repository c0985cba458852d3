"""Event verification, the part that needs no GPU: the int64 / float64 restatement of pangu_event_scores_f32 (events_ref, which
the GPU tests import), the identities of the Fractions Skill Score, the EventScores algebra, EventAccumulator pooling and the
argument checks of score.event_scores, score.EventAccumulator and rollout(events=, targets=)."""
import numpy as np
import pytest
import torch

import pangu_pytorch_amd as P

S = P.score


def box_counts(ev, r):
    """ev (.., H, W) of 0 / 1 -> int64 (.., H, W): the events in the (2r+1) x (2r+1) box around every point, as a sum of shifted
    copies: rows outside the grid are absent, columns wrap."""
    ev = ev.astype(np.int64)
    H = ev.shape[-2]
    vert = np.zeros_like(ev)
    for dr in range(-r, r + 1):
        lo, hi = max(0, -dr), min(H, H - dr)                       # rows h with 0 <= h + dr < H
        if lo < hi:
            vert[..., lo:hi, :] += ev[..., lo + dr:hi + dr, :]
    out = np.zeros_like(ev)
    for dc in range(-r, r + 1):
        out += np.roll(vert, -dc, axis=-1)                         # out[w] += vert[(w + dc) mod W]
    return out


def events_ref(pred, target, thr, radii, lat_w, domain, target_levels=0):
    """pangu_event_scores_f32 restated.  pred / target (planes, H, W) fp32, thr (T, planes) fp32, radii a sequence of ints, lat_w (H,)
    fp32, domain (H, W) bool or None (every point).  Returns counts int64 (T, planes, 4), wsums float64 (T, planes, 4) and fss
    float64 (T, planes, N, 2); the weighted sums are added in row order."""
    planes, H, W = pred.shape
    order = np.arange(planes)
    if target_levels > 1:
        order = order.reshape(-1, target_levels)[:, ::-1].reshape(-1)
    thr = np.asarray(thr, np.float32)
    T = thr.shape[0]
    with np.errstate(invalid="ignore"):
        f = pred[None] > thr[:, :, None, None]                     # (T, planes, H, W); a comparison with NaN is False
        o = target[order][None] > thr[:, :, None, None]
    dom = np.ones((H, W), bool) if domain is None else np.asarray(domain, bool)
    w = np.asarray(lat_w, np.float32).astype(np.float64)
    rows = lambda x: (x & dom).sum(axis=-1).astype(np.int64)       # (T, planes, H): exact integer row sums
    table = np.stack([rows(f & o), rows(f & ~o), rows(~f & o), rows(~f & ~o)], axis=-1)      # (T, planes, H, 4)
    counts = table.sum(axis=2)
    wsums = np.zeros((T, planes, 4))
    for h in range(H):
        wsums += w[h] * table[:, :, h, :].astype(np.float64)
    fss = np.zeros((T, planes, len(radii), 2))
    for i, r in enumerate(radii):
        cf, co = box_counts(f, r), box_counts(o, r)
        A = np.where(dom, (cf - co) ** 2, 0).sum(axis=-1)          # int64 (T, planes, H)
        B = np.where(dom, cf ** 2 + co ** 2, 0).sum(axis=-1)
        for h in range(H):
            n = float((min(h + r, H - 1) - max(h - r, 0) + 1) * (2 * r + 1))
            s = w[h] / (n * n)
            fss[:, :, i, 0] += s * A[:, :, h].astype(np.float64)
            fss[:, :, i, 1] += s * B[:, :, h].astype(np.float64)
    return counts, wsums, fss


def blobs(planes, H, W, seed):
    """Smooth fp32 fields (planes, H, W): white noise under two passes of a 5 x 5 box mean, so that events come in patches."""
    x = np.random.default_rng(seed).standard_normal((planes, H, W))
    for _ in range(2):
        x = sum(np.roll(np.roll(x, a, axis=-2), b, axis=-1) for a in range(-2, 3) for b in range(-2, 3)) / 25.0
    return (x / x.std()).astype(np.float32)


def weights(H):
    return S.latitude_weights(H, "cpu").numpy()


def as_scores(ref, radii, cases=1):
    counts, wsums, fss = ref
    return S.EventScores(torch.from_numpy(counts), torch.from_numpy(wsums), torch.from_numpy(fss), radii, cases)


# ---- the reference itself and the identities ----------------------------------------------------------------------------------

def test_reference_on_a_hand_case():
    """One 3 x 4 plane written out by hand: f at (0,0) and (1,1), o at (0,0) and (2,3)."""
    pred = np.zeros((1, 3, 4), np.float32)
    target = np.zeros((1, 3, 4), np.float32)
    pred[0, 0, 0] = pred[0, 1, 1] = 2.0
    target[0, 0, 0] = target[0, 2, 3] = 2.0
    w = np.array([1.0, 2.0, 4.0], np.float32)
    counts, wsums, fss = events_ref(pred, target, np.array([[1.0]], np.float32), (0, 1), w, None)
    assert counts.tolist() == [[[1, 1, 1, 9]]]
    assert wsums.tolist() == [[[1.0, 2.0, 4.0, 3.0 + 6.0 + 12.0]]]
    assert fss[0, 0, 0].tolist() == [2.0 + 4.0, 2.0 * 1.0 + 2.0 + 4.0]              # r = 0: FA + misses, 2 hits + FA + misses, weighted
    # r = 1 (W = 4: three of four columns), row 0 holds rows 0..1 (n = 6), row 1 rows 0..2 (n = 9), row 2 rows 1..2 (n = 6)
    cf = np.array([[2, 2, 1, 1], [2, 2, 1, 1], [1, 1, 1, 0]])
    co = np.array([[1, 1, 0, 1], [2, 1, 1, 2], [1, 0, 1, 1]])
    n = np.array([6.0, 9.0, 6.0])
    num = sum(w[h] / n[h] ** 2 * ((cf[h] - co[h]) ** 2).sum() for h in range(3))
    den = sum(w[h] / n[h] ** 2 * (cf[h] ** 2 + co[h] ** 2).sum() for h in range(3))
    assert np.allclose(fss[0, 0, 1], [num, den], rtol=1e-15)
    # a domain of one point: the neighbourhood still sees the events outside it
    dom = np.zeros((3, 4), bool)
    dom[2, 0] = True
    c1, _, f1 = events_ref(pred, target, np.array([[1.0]], np.float32), (1,), w, dom)
    assert c1.tolist() == [[[0, 0, 0, 1]]] and np.allclose(f1[0, 0, 0], [0.0, 4.0 / 36.0 * 2.0], rtol=1e-15)


def test_identities_at_radius_zero_and_level_reversal():
    H, W = 11, 16
    pred, target = blobs(6, H, W, 1), blobs(6, H, W, 2)
    thr = np.array([[0.0] * 6, [0.8] * 6], np.float32)
    dom = np.random.default_rng(3).random((H, W)) > 0.3
    for domain in (None, dom):
        counts, wsums, fss = events_ref(pred, target, thr, (0, 2), weights(H), domain)
        assert np.array_equal(counts.sum(-1), np.full((2, 6), H * W if domain is None else dom.sum()))
        assert np.allclose(fss[..., 0, 0], wsums[..., 1] + wsums[..., 2], rtol=1e-13)
        assert np.allclose(fss[..., 0, 1], 2 * wsums[..., 0] + wsums[..., 1] + wsums[..., 2], rtol=1e-13)
        e = as_scores((counts, wsums, fss), (0, 2))
        assert torch.allclose(e.fss()[..., 0], 1.0 - (e.wsums[..., 1] + e.wsums[..., 2]) / (2 * e.wsums[..., 0] + e.wsums[..., 1] + e.wsums[..., 2]))
    rev = target.reshape(2, 3, H, W)[:, ::-1].reshape(6, H, W)
    for a, b in zip(events_ref(pred, rev, thr, (0, 2), weights(H), None, target_levels=3), events_ref(pred, target, thr, (0, 2), weights(H), None)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("H,W", [(37, 72), (33, 100)])
def test_fss_grows_with_the_radius_for_a_displaced_field(H, W):
    """The double penalty: a forecast that is the truth three columns off scores badly point by point and well from the scale of
    the displacement on."""
    target = blobs(2, H, W, 7)
    pred = np.roll(target, 3, axis=-1)
    thr = np.full((1, 2), 1.0, np.float32)
    radii = (0, 2, 8, 16)
    e = as_scores(events_ref(pred, target, thr, radii, weights(H), None), radii)
    fss = e.fss().numpy()[0]
    assert (np.diff(fss, axis=-1) > 0).all(), fss
    assert (fss[:, 0] < 0.6).all() and (fss[:, 2] > 0.9).all() and (fss[:, 3] > 0.97).all(), fss
    useful = e.useful_radius().numpy()[0]
    assert set(useful.tolist()) <= {2, 8}, useful                                   # not at r = 0, reached by r = 8


def test_fss_is_one_for_identical_fields():
    H, W = 9, 12
    x = blobs(3, H, W, 9)
    radii = (0, 1, 4)
    e = as_scores(events_ref(x, x.copy(), np.zeros((1, 3), np.float32), radii, weights(H), None), radii)
    assert np.array_equal(e.fss_sums[..., 0].numpy(), np.zeros((1, 3, 3)))
    assert np.array_equal(e.fss().numpy(), np.ones((1, 3, 3)))
    assert np.array_equal(e.useful_radius().numpy(), np.zeros((1, 3), np.int64))
    assert np.array_equal(e.counts[..., 1:3].numpy(), np.zeros((1, 3, 2), np.int64))


# ---- EventScores and EventAccumulator -----------------------------------------------------------------------------------------

def test_derived_scores_on_a_hand_table():
    """hits 30, false alarms 20, misses 10, correct negatives 40."""
    counts = torch.tensor([[30, 20, 10, 40], [0, 0, 0, 100], [0, 0, 0, 0]])
    fss = torch.tensor([[[1.0, 4.0], [0.5, 4.0]], [[0.0, 0.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]]], dtype=torch.float64)
    e = S.EventScores(counts, counts.double(), fss, (0, 3))
    row = lambda t: t.tolist()[0]
    assert row(e.pod()) == 30 / 40 and row(e.far()) == 20 / 50 and row(e.csi()) == 30 / 60 and row(e.frequency_bias()) == 50 / 40
    assert row(e.ets()) == (30 - 20) / (60 - 20)                                     # random hits 50 * 40 / 100
    assert row(e.base_rate()) == 0.4 and row(e.fss_useful()) == 0.7
    assert e.fss()[0].tolist() == [0.75, 0.875] and e.useful_radius().tolist() == [0, -1, -1]
    for name in ("pod", "far", "csi", "frequency_bias", "ets"):                      # no events at all: every denominator is 0
        assert torch.isnan(getattr(e, name)()[1:]).all(), name
    assert e.base_rate()[1].item() == 0.0 and torch.isnan(e.base_rate()[2])          # an empty domain has no base rate either
    assert torch.isnan(e.fss()[1:]).all()
    with pytest.raises(ValueError, match="fss_sums"):
        S.EventScores(counts, counts.double(), fss, (0, 3, 5))
    with pytest.raises(ValueError, match="counts and wsums"):
        S.EventScores(counts, counts.double()[:2], fss, (0, 3))


def _case(seed, H=9, W=12):
    pred, target = blobs(69, H, W, seed), blobs(69, H, W, seed + 100)
    return pred, target


def _split(ref, T, radii, cases=1):
    counts, wsums, fss = ref
    N = len(radii)
    up = S.EventScores(torch.from_numpy(counts[:, :65].reshape(T, 5, 13, 4).copy()), torch.from_numpy(wsums[:, :65].reshape(T, 5, 13, 4).copy()),
                       torch.from_numpy(fss[:, :65].reshape(T, 5, 13, N, 2).copy()), radii, cases)
    sf = S.EventScores(torch.from_numpy(counts[:, 65:].copy()), torch.from_numpy(wsums[:, 65:].copy()), torch.from_numpy(fss[:, 65:].copy()),
                       radii, cases)
    return up, sf


def test_accumulator_pools_cases():
    H, W, T, radii = 9, 12, 2, (0, 2)
    thr = np.stack([np.zeros(69, np.float32), np.full(69, 0.7, np.float32)])
    thresholds = (torch.from_numpy(thr[:, :65].reshape(T, 5, 13).copy()), torch.from_numpy(thr[:, 65:].copy()))
    (p1, t1), (p2, t2) = _case(1), _case(2)
    w = weights(H)
    r1, r2 = events_ref(p1, t1, thr, radii, w, None), events_ref(p2, t2, thr, radii, w, None)
    acc = S.EventAccumulator(3, thresholds, radii)
    acc.add(1, *_split(r1, T, radii))
    acc.add(1, *_split(r2, T, radii))
    assert acc.cases(1) == 2 and acc.cases(0) == 0
    # the reference on both cases' points at once: the cases as further planes, added per plane
    both = events_ref(np.concatenate((p1, p2)), np.concatenate((t1, t2)), np.tile(thr, (1, 2)), radii, w, None)
    want = [x.reshape(T, 2, 69, *x.shape[2:]).sum(axis=1) for x in both]
    up, sf = acc.sums(1)
    got = [np.concatenate((a.numpy().reshape(T, 65, *a.shape[3:]), b.numpy()), axis=1) for a, b in
           ((up.counts, sf.counts), (up.wsums, sf.wsums), (up.fss_sums, sf.fss_sums))]
    assert np.array_equal(got[0], want[0]) and got[0].dtype == np.int64
    assert np.allclose(got[1], want[1], rtol=1e-15, atol=0) and np.allclose(got[2], want[2], rtol=1e-15, atol=0)
    assert np.allclose(up.fss().numpy().reshape(T, 65, 2), (1.0 - want[2][..., 0] / want[2][..., 1])[:, :65], rtol=1e-14, equal_nan=True)
    # a batch of cases in one EventScores pools like its cases one by one
    stacked = [S.EventScores(torch.stack((a.counts, b.counts)), torch.stack((a.wsums, b.wsums)), torch.stack((a.fss_sums, b.fss_sums)), radii)
               for a, b in zip(_split(r1, T, radii), _split(r2, T, radii))]
    acc.add(2, *stacked)
    assert acc.cases(2) == 2 and torch.equal(acc.sums(2)[0].counts, up.counts) and torch.equal(acc.sums(2)[1].fss_sums, sf.fss_sums)
    table = acc.table(1)
    assert table["cases"] == 2 and table["radii"] == radii and table["pod"].shape == (T, 69) and table["fss"].shape == (T, 69, 2)
    assert table["useful_radius"].dtype == np.int64 and np.array_equal(table["fss"][:, :65], up.fss().numpy().reshape(T, 65, 2), equal_nan=True)
    assert np.array_equal(table["ets"][:, 65:], sf.ets().numpy(), equal_nan=True)
    with pytest.raises(ValueError, match="nothing scored"):
        acc.sums(0)
    with pytest.raises(IndexError):
        acc.add(3, *stacked)
    with pytest.raises(ValueError, match="radii"):
        acc.add(0, *_split(events_ref(p1, t1, thr, (0, 1), w, None), T, (0, 1)))
    with pytest.raises(ValueError, match="expected counts"):
        acc.add(0, stacked[1], stacked[1])


# ---- argument checks ------------------------------------------------------------------------------------------------------------

def test_event_scores_argument_checks():
    H, W = 9, 12
    up, sf = torch.zeros(5, 13, H, W), torch.zeros(4, H, W)
    thr = (torch.zeros(2, 5, 13), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="expected upper"):
        S.event_scores(up[0], sf, up[0], sf, thr)
    with pytest.raises(ValueError, match="disagree"):
        S.event_scores(up, sf[..., :8], up, sf[..., :8], thr)
    with pytest.raises(ValueError, match="W % 4"):
        S.event_scores(up[..., :10], sf[..., :10], up[..., :10], sf[..., :10], thr)
    with pytest.raises(ValueError, match="both targets"):
        S.event_scores(up, sf, up, None, thr)
    with pytest.raises(ValueError, match="one value per forecast value"):
        S.event_scores(up, sf, up[:4], sf, thr)
    with pytest.raises(ValueError, match="thresholds are required"):
        S.event_scores(up, sf, up, sf, None)
    with pytest.raises(ValueError, match="thresholds must be a pair"):
        S.event_scores(up, sf, up, sf, (torch.zeros(2, 5, 13), torch.zeros(3, 4)))
    with pytest.raises(ValueError, match="at most 4 thresholds"):
        S.event_scores(up, sf, up, sf, (torch.zeros(5, 5, 13), torch.zeros(5, 4)))
    for radii, match in (((), "radii"), ((0, 1, 2, 3, 4), "radii"), ((2, 2), "strictly increasing"), ((3, 1), "strictly increasing"),
                         ((-1,), "radius"), ((33,), "radius"), ((6,), "wider"), (1.5, "sequence"), (("a",), "sequence")):
        with pytest.raises(ValueError, match=match):
            S.event_scores(up, sf, up, sf, thr, radii=radii)
    with pytest.raises(ValueError, match="without regions"):
        S.event_scores(up, sf, up, sf, thr, region="tropics")
    with pytest.raises(ValueError, match="one region to score"):
        S.event_scores(up, sf, up, sf, thr, regions={"tropics": "tropics"})
    with pytest.raises(ValueError, match="one region to score"):
        S.event_scores(up, sf, up, sf, thr, regions={"tropics": "tropics"}, region="europe")
    with pytest.raises(ValueError, match="region plan"):
        S.event_scores(up, sf, up, sf, thr, regions=S.region_bits(H + 1, W, {"tropics": "tropics"}), region="tropics")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                       # every check passed: the launch needs the device
        S.event_scores(up, sf, up, sf, thr, radii=(0, 5), regions={"tropics": "tropics"}, region="tropics")
    assert S.event_scores_workspace_bytes(69, 721, 4, 4) == 69 * 721 * 45 * 8


def test_accumulator_argument_checks():
    thr = (torch.zeros(1, 5, 13), torch.zeros(1, 4))
    with pytest.raises(ValueError, match="leads"):
        S.EventAccumulator(0, thr, (0,))
    with pytest.raises(ValueError, match="thresholds are required"):
        S.EventAccumulator(1, None, (0,))
    with pytest.raises(ValueError, match="strictly increasing"):
        S.EventAccumulator(1, thr, (4, 2))
    with pytest.raises(ValueError, match="without regions"):
        S.EventAccumulator(1, thr, (0,), region="tropics")
    acc = S.EventAccumulator(2, thr, [0, 4])
    assert acc.radii == (0, 4) and acc.T == 1 and acc.leads == 2
    with pytest.raises(IndexError):
        acc.cases(2)


def test_rollout_checks_events_and_targets_before_the_model():
    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("rollout touched the model before it checked its arguments")

        def __call__(self, *a, **k):
            raise AssertionError("rollout called the model before it checked its arguments")

    thr = (torch.zeros(1, 5, 13), torch.zeros(1, 4))
    ev, card = S.EventAccumulator(2, thr, (0, 2)), S.ScoreAccumulator(2)
    x = torch.zeros(1)
    args = (Untouchable(), x, x, None, None, None, None)
    for graph in (True, False):
        with pytest.raises(ValueError, match="events needs targets"):
            P.rollout.rollout(*args, steps=2, graph=graph, events=ev)
        with pytest.raises(ValueError, match="scorecard and targets go together"):           # the earlier texts stay
            P.rollout.rollout(*args, steps=2, graph=graph, scorecard=card, events=ev)
        with pytest.raises(ValueError, match="scorecard and targets go together"):
            P.rollout.rollout(*args, steps=2, graph=graph, targets=[None, None])
        with pytest.raises(ValueError, match="3 targets for 2 steps"):
            P.rollout.rollout(*args, steps=2, graph=graph, events=ev, targets=[None] * 3)
        with pytest.raises(ValueError, match="event accumulator holds 2 leads"):
            P.rollout.rollout(*args, steps=3, graph=graph, events=ev, targets=[None] * 3)
        with pytest.raises(ValueError, match="a pair"):
            P.rollout.rollout(*args, steps=2, graph=graph, events=ev, targets=[None, (x,)])
    assert ev.cases(0) == 0
