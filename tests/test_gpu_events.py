"""pangu_event_scores_f32 (csrc/events.hip) on the device against events_ref (tests/test_events_cpu.py), at the shapes where the
kernel can go wrong, and the Python surface on top of it: score.event_scores, score.EventAccumulator, rollout(events=).

Exactness.  Counts are integers and always compared with ==.  With lat_weight[h] = n_h^2 (a float where that is exact in fp32: every
row for r <= 16 and all but rows_h = 65 at r = 32, which get weight 0; full boxes of 65 rows have a test of their own, with real
weights) s_h = 1 and both FSS sums are sums of exact integers below 2^53: they must EQUAL the reference.  With real weights every output is a sum of H non-negative double terms s_h * integer, each
rounded once, added in some fixed order: |got - ref| <= (H + 4) 2^-52 ref."""
import ctypes

import numpy as np
import pytest
import torch

from test_events_cpu import blobs, events_ref

pytestmark = pytest.mark.gpu

POISON_BYTE = 0xA5
NULL, SHAPE, ARG = -2, -1, -4


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    P._lib.load()
    return P


def abi_events(P, pred, target, thr, radii, w, domain=None, bit=0, levels=0, bits=None, guard=64, ws_extra=256):
    """pred / target (planes, H, W) fp32 numpy, thr (T, planes), w (H,) fp32, domain (H, W) bool or None (or `bits`, the uint8 mask
    itself) -> counts int64 (T, planes, 4), wsums, fss (T, planes, N, 2) float64 numpy through the C ABI.  Outputs and workspace are
    filled with a byte pattern first: the guards behind every output and behind the workspace must come back untouched."""
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    pred, target, thr, w = dev(pred, np.float32), dev(target, np.float32), dev(thr, np.float32), dev(w, np.float32)
    planes, H, W = pred.shape
    T, N = thr.shape[0], len(radii)
    if bits is None and domain is not None:
        bits = (np.asarray(domain, bool).astype(np.uint8) << bit).astype(np.uint8)
    b = None if bits is None else dev(bits, np.uint8)
    lib = P._lib.load()
    need = lib.pangu_event_scores_ws_bytes(planes, H, T, N)
    assert need == P.score.event_scores_workspace_bytes(planes, H, T, N)
    sizes = (T * planes * 4 * 8, T * planes * 4 * 8, T * planes * N * 2 * 8)
    outs = [torch.full((n + guard,), POISON_BYTE, dtype=torch.uint8, device="cuda") for n in sizes]
    ws = torch.full((need + ws_extra,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    host_radii = (ctypes.c_int * N)(*radii)
    P._lib.check(lib.pangu_event_scores_f32(
        torch.cuda.current_stream().cuda_stream, pred.data_ptr(), target.data_ptr(), levels, thr.data_ptr(), T, host_radii, N,
        w.data_ptr(), None if b is None else b.data_ptr(), bit, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
        ws.data_ptr(), need, planes, H, W), "event_scores")
    torch.cuda.synchronize()
    for o, n in zip(outs, sizes):
        assert bool((o[n:] == POISON_BYTE).all()), "wrote behind an output"
    assert bool((ws[need:] == POISON_BYTE).all()), "wrote behind the workspace"
    counts = outs[0][:sizes[0]].cpu().numpy().view(np.int64).reshape(T, planes, 4)
    wsums = outs[1][:sizes[1]].cpu().numpy().view(np.float64).reshape(T, planes, 4)
    fss = outs[2][:sizes[2]].cpu().numpy().view(np.float64).reshape(T, planes, N, 2)
    return counts, wsums, fss


def exact_weights(H, r):
    """n_h^2 as fp32 where that is exact, else 0."""
    n = np.array([(min(h + r, H - 1) - max(h - r, 0) + 1) * (2 * r + 1) for h in range(H)], np.float64)
    w = (n * n).astype(np.float32)
    return np.where(w.astype(np.float64) == n * n, w, np.float32(0.0)).astype(np.float32)


def fields(planes, H, W, seed):
    return blobs(planes, H, W, seed), blobs(planes, H, W, seed + 1000)


def thresholds(T, planes, seed):
    return np.random.default_rng(seed).uniform(-0.5, 1.2, (T, planes)).astype(np.float32)


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)) for x, y in zip(a, b))


def lat_w(P, H):
    return P.score.latitude_weights(H, "cpu").numpy()


def assert_close(got, ref, H, what=""):
    """Counts ==, the weighted sums within (H + 4) 2^-52 relative.  Prints the worst error in units of the bound."""
    assert np.array_equal(got[0], ref[0]), what
    tol = (H + 4) * 2.0 ** -52
    worst = 0.0
    for g, r in zip(got[1:], ref[1:]):
        err = np.abs(g - r)
        worst = max(worst, float((err / np.maximum(tol * np.abs(r), 1e-300)).max()))
        assert (err <= tol * np.abs(r)).all(), (what, worst)
    print(f"{what}: worst error {worst:.3f} of the bound")


# ---- exactness at the ABI -----------------------------------------------------------------------------------------------------

S_ROWS = 32      # the kernel's slab height (score.EVENT_SLAB_ROWS, checked below)
EXACT = [(5, 8, (0, 1, 3)), (3, 72, (8,)), (37, 72, (0, 2, 8, 16)), (33, 100, (0, 2, 8, 16)),
         (S_ROWS - 1, 72, (1, 32)), (S_ROWS, 72, (1, 32)), (S_ROWS + 1, 72, (1, 32)), (2 * S_ROWS + 1, 72, (1, 32))]


@pytest.mark.parametrize("H,W,radii", EXACT, ids=[f"{h}x{w}" for h, w, _ in EXACT])
def test_integer_sums_equal_the_reference(P, H, W, radii):
    assert P.score.EVENT_SLAB_ROWS == S_ROWS
    planes, T = 3, 2
    pred, target = fields(planes, H, W, H * W)
    thr = thresholds(T, planes, H)
    for r in radii:
        w = exact_weights(H, r)
        assert (w > 0).sum() >= H - 1
        for domain in (None, np.random.default_rng(r).random((H, W)) > 0.4):
            got = abi_events(P, pred, target, thr, (r,), w, domain, bit=3)
            ref = events_ref(pred, target, thr, (r,), w, domain)
            assert np.array_equal(got[0], ref[0]), (r, "counts")
            assert np.array_equal(got[1], ref[1]), (r, "weighted counts")             # integers times integers here
            assert np.array_equal(got[2], ref[2]), (r, "fss sums")
            assert got[2][..., 1].max() > 0
            if r == 0:
                assert np.array_equal(got[2][..., 0, 0], got[1][..., 1] + got[1][..., 2])
                assert np.array_equal(got[2][..., 0, 1], 2 * got[1][..., 0] + got[1][..., 1] + got[1][..., 2])


REAL = [(70, 72, (0, 2, 8, 32)), (2 * S_ROWS + 1, 72, (1, 32)), (37, 72, (0, 2, 8, 16)), (33, 100, (2, 8, 16))]


@pytest.mark.parametrize("H,W,radii", REAL, ids=[f"{h}x{w}" for h, w, _ in REAL])
def test_real_weights_all_radii_in_one_call(P, H, W, radii):
    planes, T = 5, 4
    pred, target = fields(planes, H, W, 3 * H + W)
    thr = thresholds(T, planes, W)
    w = lat_w(P, H)
    domain = np.random.default_rng(H).random((H, W)) > 0.25
    for dom in (None, domain):
        got = abi_events(P, pred, target, thr, radii, w, dom, bit=7)
        assert_close(got, events_ref(pred, target, thr, radii, w, dom), H, f"{H}x{W} {'masked' if dom is not None else 'global'}")


def test_wide_row_and_a_sum_beyond_32_bits(P):
    """W = 1440 (six waves, 360 of 384 lanes), r = 32, nearly every point an event: a row's B_h, about 2 * 1440 * 2600^2, passes 2^32."""
    H, W, r = 40, 1440, 32
    pred, target = np.ones((1, H, W), np.float32), np.ones((1, H, W), np.float32)
    target[0, :, ::7] = -1.0
    w = exact_weights(H, r)
    got = abi_events(P, pred, target, np.zeros((1, 1), np.float32), (r,), w)
    ref = events_ref(pred, target, np.zeros((1, 1), np.float32), (r,), w, None)
    assert ref[2][0, 0, 0, 1] > H * 2.0 ** 32 / 2
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])


@pytest.mark.parametrize("H,W", [(70, 72), (66, 1440)], ids=["70x72", "66x1440"])
def test_full_boxes_of_65_rows(P, H, W):
    """r = 32 with dense events: a lane's four columns hold 65 events each, 260 in all, more than a byte; a column's box 4225.  Every
    point an event in both fields, every point an event in one field only, and a full block next to an empty one."""
    r, w = 32, lat_w(P, H)
    ones, zeros = np.ones((1, H, W), np.float32), np.zeros((1, H, W), np.float32)
    block, shifted = zeros.copy(), zeros.copy()
    block[0, :, :W // 2] = 1.0                                                       # full columns 0 .. W/2-1, empty beyond
    shifted[0, 2:, 6:W // 2 + 6] = 1.0
    thr = np.array([[0.5], [2.0]], np.float32)                                       # the second threshold: no event at all
    dom = np.random.default_rng(H).random((H, W)) > 0.3
    for name, pred, target in (("all / all", ones, ones), ("all / none", ones, zeros), ("block / all", block, ones),
                               ("block / shifted block", block, shifted)):
        for radii, domain in (((r,), None), ((0, 8, r), dom)):
            got = abi_events(P, pred, target, thr, radii, w, domain, bit=4)
            ref = events_ref(pred, target, thr, radii, w, domain)
            assert_close(got, ref, H, f"{H}x{W} {name} {radii}")
            assert not got[2][1].any()
    full = abi_events(P, ones, zeros, thr[:1], (r,), np.ones(H, np.float32))          # cf = n_h, co = 0: both sums are W per row
    assert np.abs(full[2][0, 0, 0] - W * H).max() <= (H + 4) * 2.0 ** -52 * W * H


@pytest.mark.parametrize("H,W,T,radii", [(40, 1440, 4, (0, 2, 16)), (34, 4096, 3, (1, 32))], ids=["thresholds-split", "one-threshold-100KB"])
def test_wide_rows_at_the_lds_limits(P, H, W, T, radii):
    """At 1440 columns four thresholds do not fit a workgroup's share of LDS and are split over the grid; at 4096 columns (16 waves)
    and r = 32 a single threshold needs about 100 KB, more than the 64 KB a kernel gets without asking."""
    pred, target = fields(1, H, W, W + T)
    thr = thresholds(T, 1, W)
    w = lat_w(P, H)
    dom = np.random.default_rng(W).random((H, W)) > 0.2
    assert_close(abi_events(P, pred, target, thr, radii, w, dom, bit=1), events_ref(pred, target, thr, radii, w, dom), H, f"{H}x{W}")


# ---- independence and determinism ---------------------------------------------------------------------------------------------

def test_outputs_do_not_depend_on_the_rest_of_the_call(P):
    H, W, planes, T, radii = 37, 72, 4, 3, (0, 2, 8)
    pred, target = fields(planes, H, W, 11)
    thr = thresholds(T, planes, 12)
    w = lat_w(P, H)
    domain = np.random.default_rng(13).random((H, W)) > 0.3
    full = abi_events(P, pred, target, thr, radii, w, domain)
    assert same_bits(full, abi_events(P, pred, target, thr, radii, w, domain)), "two runs differ"
    for t in range(T):
        for p in range(planes):
            for i, r in enumerate(radii):
                one = abi_events(P, pred[p:p + 1], target[p:p + 1], thr[t:t + 1, p:p + 1], (r,), w, domain)
                assert same_bits(one, (full[0][t:t + 1, p:p + 1], full[1][t:t + 1, p:p + 1], full[2][t:t + 1, p:p + 1, i:i + 1])), (t, p, r)


# ---- wrap, domain, thresholds, levels -------------------------------------------------------------------------------------------

def test_columns_wrap_and_rows_do_not(P):
    H, W, r = 6, 16, 1
    w = exact_weights(H, r)
    zero = np.zeros((1, H, W), np.float32)
    thr = np.full((1, 1), 0.5, np.float32)

    def seen(event, centre):
        pred = zero.copy()
        pred[0][event] = 1.0
        dom = np.zeros((H, W), bool)
        dom[centre] = True
        counts, _, fss = abi_events(P, pred, zero, thr, (r,), w, dom)
        assert np.array_equal(fss, events_ref(pred, zero, thr, (r,), w, dom)[2])
        assert counts.sum() == 1
        return fss[0, 0, 0].tolist()

    assert seen((2, 0), (2, W - 1)) == [1.0, 1.0] and seen((2, W - 1), (3, 0)) == [1.0, 1.0]      # across the seam, both ways
    assert seen((2, 0), (2, W - 2)) == [0.0, 0.0]
    assert seen((0, 5), (H - 1, 5)) == [0.0, 0.0] and seen((H - 1, 5), (0, 5)) == [0.0, 0.0]      # the poles are ends
    assert seen((0, 5), (1, 4)) == [1.0, 1.0]


def test_domain_selects_centres_only(P):
    H, W, planes, radii = 37, 72, 2, (0, 2, 8)
    pred, target = fields(planes, H, W, 21)
    thr = thresholds(2, planes, 22)
    w = lat_w(P, H)
    dom = np.random.default_rng(23).random((H, W)) > 0.5
    dom[9] = False                                                                   # an empty row
    ref = events_ref(pred, target, thr, radii, w, dom)
    assert_close(abi_events(P, pred, target, thr, radii, w, dom, bit=2), ref, H, "empty row")
    # every other bit set everywhere changes nothing
    bits = ((dom.astype(np.uint8) << 2) | np.uint8(0xFB)).astype(np.uint8)
    assert same_bits(abi_events(P, pred, target, thr, radii, w, bit=2, bits=bits), abi_events(P, pred, target, thr, radii, w, dom, bit=2))
    # a single point, with an event just outside the mask that its neighbourhood must see
    one = np.zeros((H, W), bool)
    one[20, 30] = True
    p1, t1 = np.zeros((1, H, W), np.float32), np.zeros((1, H, W), np.float32)
    p1[0, 20, 31] = 1.0
    half = np.full((1, 1), 0.5, np.float32)
    got = abi_events(P, p1, t1, half, (0, 2), exact_weights(H, 2), one)
    assert got[0].tolist() == [[[0, 0, 0, 1]]] and got[2][0, 0].tolist() == [[0.0, 0.0], [1.0, 1.0]]
    assert np.array_equal(got[2], events_ref(p1, t1, half, (0, 2), exact_weights(H, 2), one)[2])
    # an empty domain: all zeros, and no score
    empty = abi_events(P, pred, target, thr, radii, w, np.zeros((H, W), bool))
    assert not empty[0].any() and not empty[1].any() and not empty[2].any()
    e = P.score.EventScores(torch.from_numpy(empty[0]), torch.from_numpy(empty[1]), torch.from_numpy(empty[2]), radii)
    assert torch.isnan(e.fss()).all() and torch.isnan(e.pod()).all() and bool((e.useful_radius() == -1).all())


def test_infinite_threshold_nan_and_level_reversal(P):
    H, W, radii = 13, 24, (0, 3)
    w = lat_w(P, H)
    pred, target = fields(26, H, W, 31)
    thr = thresholds(2, 26, 32)
    thr[1, 5] = np.inf                                                               # an event that never happens
    pred[7, 3, 4] = np.nan                                                           # a non-event, as every comparison with NaN
    pred[7, 6, :] = np.inf
    target[8, 2, 2] = np.nan
    got = abi_events(P, pred, target, thr, radii, w)
    assert_close(got, events_ref(pred, target, thr, radii, w, None), H, "inf / NaN")
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    assert got[0][1, 5].tolist() == [0, 0, 0, H * W] and not got[2][1, 5].any()
    rev = abi_events(P, pred, target, thr, radii, w, levels=13)
    assert_close(rev, events_ref(pred, target, thr, radii, w, None, target_levels=13), H, "levels")
    flipped = target.reshape(2, 13, H, W)[:, ::-1].reshape(26, H, W)
    assert same_bits(rev, abi_events(P, pred, flipped, thr, radii, w))
    assert not same_bits(rev, got)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_every_error_code(P):
    """Every refusal returns before a launch: dummy aligned addresses, and a real host array for the radii."""
    lib = P._lib.load()
    ws_bytes = lib.pangu_event_scores_ws_bytes
    assert ws_bytes(69, 721, 4, 4) == 69 * 721 * 45 * 8 and ws_bytes(1, 1, 1, 1) == 6 * 8
    for bad in ((0, 5, 1, 1), (1, 0, 1, 1), (1, 5, 0, 1), (1, 5, 5, 1), (1, 5, 1, 0), (1, 5, 1, 5), (1 << 30, 721, 1, 1)):
        assert ws_bytes(*bad) == SHAPE, bad
    A, big = 1 << 20, 1 << 40

    def call(pred=A, target=A, levels=0, thr=A, T=2, radii=(0, 2), N=None, w=A, bits=A, bit=0, counts=A, wsums=A, fss=A, ws=A,
             ws_bytes=big, planes=10, H=13, W=24):
        n = len(radii) if N is None and radii is not None else N
        host = None if radii is None else (ctypes.c_int * max(len(radii), 1))(*radii)
        return lib.pangu_event_scores_f32(None, pred, target, levels, thr, T, host, n, w, bits, bit, counts, wsums, fss, ws, ws_bytes,
                                          planes, H, W)

    for name in ("pred", "target", "thr", "w", "counts", "wsums", "fss", "ws"):
        assert call(**{name: None}) == NULL, name
    assert call(radii=None, N=1) == NULL
    assert call(W=26) == SHAPE and call(W=0) == SHAPE and call(H=0) == SHAPE and call(planes=0) == SHAPE and call(W=4100) == SHAPE
    assert call(H=1 << 20, W=2048) == SHAPE                                           # H * W = 2^31
    assert call(T=0) == SHAPE and call(T=5) == SHAPE
    assert call(radii=(), N=0) == SHAPE and call(radii=(0, 1, 2, 3, 4)) == SHAPE
    assert call(radii=(2, 2)) == SHAPE and call(radii=(3, 1)) == SHAPE and call(radii=(-1,)) == SHAPE and call(radii=(33,)) == SHAPE
    assert call(radii=(12,)) == SHAPE                                                 # 2r+1 = 25 > W
    assert call(levels=3) == SHAPE and call(levels=-1) == SHAPE                       # 10 planes are no multiple of 3
    assert call(bit=-1) == ARG and call(bit=8) == ARG
    assert call(ws_bytes=10 * 13 * (1 + 6 + 8) * 8 - 1) == ARG                        # one byte short
    for name in ("pred", "target", "ws"):
        assert call(**{name: A + 8}) == ARG, name                                     # 16 B
    for name in ("counts", "wsums", "fss"):
        assert call(**{name: A + 4}) == ARG, name                                     # 8 B
    for name in ("thr", "w", "bits"):
        assert call(**{name: A + 2}) == ARG, name                                     # 4 B


def test_a_workspace_one_byte_short_launches_nothing(P):
    lib = P._lib.load()
    H, W = 5, 8
    x = torch.zeros((1, H, W), device="cuda")
    thr, w = torch.zeros((1, 1), device="cuda"), torch.ones(H, device="cuda")
    outs = [torch.full((16,), POISON_BYTE, dtype=torch.uint8, device="cuda").repeat(4) for _ in range(3)]
    need = lib.pangu_event_scores_ws_bytes(1, H, 1, 1)
    ws = torch.full((need,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    rc = lib.pangu_event_scores_f32(torch.cuda.current_stream().cuda_stream, x.data_ptr(), x.data_ptr(), 0, thr.data_ptr(), 1,
                                    (ctypes.c_int * 1)(0), 1, w.data_ptr(), None, 0, outs[0].data_ptr(), outs[1].data_ptr(),
                                    outs[2].data_ptr(), ws.data_ptr(), need - 1, 1, H, W)
    torch.cuda.synchronize()
    assert rc == ARG and all(bool((o == POISON_BYTE).all()) for o in outs) and bool((ws == POISON_BYTE).all())


# ---- the Python surface ---------------------------------------------------------------------------------------------------------

def _state(B, H, W, seed):
    x = blobs(B * 69, H, W, seed).reshape(B, 69, H, W)
    up = torch.from_numpy(np.ascontiguousarray(x[:, :65])).cuda().view(B, 5, 13, H, W)
    sf = torch.from_numpy(np.ascontiguousarray(x[:, 65:])).cuda()
    return up, sf


def _thresholds(T, seed):
    thr = thresholds(T, 69, seed)
    return (torch.from_numpy(thr[:, :65].reshape(T, 5, 13).copy()).cuda(), torch.from_numpy(thr[:, 65:].copy()).cuda()), thr


def test_event_scores_and_accumulator(P):
    H, W, T, radii = 33, 72, 2, (0, 2, 8)
    up, sf = _state(2, H, W, 41)
    tu, ts = _state(2, H, W, 42)
    thr_pair, thr = _thresholds(T, 43)
    eu, es = P.score.event_scores(up, sf, tu, ts, thr_pair, (0,))
    assert eu.counts.shape == (2, T, 5, 13, 4) and es.counts.shape == (2, T, 4, 4) and eu.counts.dtype == torch.int64 and eu.counts.is_cuda
    assert eu.wsums.dtype == torch.float64 and eu.fss_sums.shape == (2, T, 5, 13, 1, 2) and es.fss_sums.shape == (2, T, 4, 1, 2)
    # r = 0: the counts restated with torch
    for e, x, t, th in ((eu, up, tu, thr_pair[0]), (es, sf, ts, thr_pair[1])):
        f, o = x.unsqueeze(1) > th[None, ..., None, None], t.unsqueeze(1) > th[None, ..., None, None]
        want = torch.stack([(f & o).sum((-2, -1)), (f & ~o).sum((-2, -1)), (~f & o).sum((-2, -1)), (~f & ~o).sum((-2, -1))], -1)
        assert torch.equal(e.counts, want)
        assert bool((e.counts.sum(-1) == H * W).all())
    # all radii, a region, a level-reversed target: case for case against the reference
    plan = P.score.region_bits(H, W, {"tropics": "tropics", "box": dict(lat=(-50, 60), lon=(300, 100))}, "cuda")
    dom = ((plan.bits.cpu().numpy() >> 1) & 1).astype(bool)
    w = P.score.latitude_weights(H, "cuda").cpu().numpy()                            # the weights event_scores uses, to the bit
    eu, es = P.score.event_scores(up, sf, tu.flip(2).contiguous(), ts, thr_pair, radii, plan, "box", target_levels_reversed=True)
    flat = lambda a, b: np.concatenate((a.reshape(65, H, W).cpu().numpy(), b.cpu().numpy()))
    refs = []
    for c in range(2):
        ref = events_ref(flat(up[c], sf[c]), flat(tu[c], ts[c]), thr, radii, w, dom)
        refs.append(ref)
        got = [np.concatenate((a[c].reshape(T, 65, *a.shape[4:]).cpu().numpy(), b[c].cpu().numpy()), axis=1)
               for a, b in ((eu.counts, es.counts), (eu.wsums, es.wsums), (eu.fss_sums, es.fss_sums))]
        assert_close(got, ref, H, f"event_scores case {c}")
    # the same through a mapping of regions
    mu, _ = P.score.event_scores(up, sf, tu.flip(2).contiguous(), ts, thr_pair, radii, {"tropics": "tropics", "box": dict(lat=(-50, 60), lon=(300, 100))},
                                 "box", target_levels_reversed=True)
    assert torch.equal(mu.counts, eu.counts) and torch.equal(mu.wsums, eu.wsums) and torch.equal(mu.fss_sums, eu.fss_sums)
    fss = eu.fss()
    assert fss.shape == (2, T, 5, 13, 3) and fss.is_cuda and eu.useful_radius().shape == (2, T, 5, 13)
    # pooled over the cases
    acc = P.score.EventAccumulator(2, thr_pair, radii, plan, "box")
    acc.score(1, up[0], sf[0], tu[0], ts[0])
    acc.score(1, up[1:], sf[1:], tu[1:], ts[1:])
    assert acc.cases(1) == 2 and acc.cases(0) == 0
    pu, ps = acc.sums(1)
    pooled = [np.concatenate((a.reshape(T, 65, *a.shape[3:]).cpu().numpy(), b.cpu().numpy()), axis=1)
              for a, b in ((pu.counts, ps.counts), (pu.wsums, ps.wsums), (pu.fss_sums, ps.fss_sums))]
    want = [refs[0][k] + refs[1][k] for k in range(3)]
    assert_close(pooled, want, H + 1, "pooled")                                      # one more addition
    table = acc.table(1)
    want_fss = 1.0 - want[2][..., 0] / want[2][..., 1]
    assert table["fss"].shape == (T, 69, 3) and np.allclose(table["fss"], want_fss, rtol=1e-12, equal_nan=True)
    with pytest.raises(RuntimeError, match="float32"):
        P.score.event_scores(up.double(), sf, tu, ts, thr_pair)


# ---- rollout(events=, targets=) -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup(P):
    import cases
    import synth
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return m, cases.model_inputs("cuda")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("graph", [True, False])
def test_rollout_scores_events_every_step(P, setup, graph):
    """The model and inputs of tests/test_gpu_scorecard.py::test_rollout_scores_every_step, 2 steps, one None target: the hook
    leaves the returned fields untouched, is handed the step's physical fields, and pools per lead exactly what event_scores gives
    on the kept history."""
    from test_gpu_drain import _stats_last as stats_last_of
    m, (inp, inp_s, stats, maps, const_h) = setup
    sl = stats_last_of(stats)
    up0, sf0, hist = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, keep=True)
    g = torch.Generator(device="cuda").manual_seed(5)
    target = (inp + torch.randn(inp.shape, generator=g, device="cuda"), inp_s + torch.randn(inp_s.shape, generator=g, device="cuda"))
    mean_u, mean_s = target[0][0].mean((-2, -1)), target[1][0].mean((-2, -1))
    thr = (torch.stack((mean_u, mean_u + 0.5)), torch.stack((mean_s, mean_s + 0.5)))
    radii, regions = (0, 2, 8), {"tropics": "tropics", "nh": "nh_extratropics"}
    kept = []

    class Recording(P.score.EventAccumulator):
        def score(self, lead, upper, surface, target_upper, target_surface):
            kept.append((lead, upper.clone(), surface.clone()))
            return super().score(lead, upper, surface, target_upper, target_surface)

    acc = Recording(2, thr, radii, regions, "nh")
    card = P.score.ScoreAccumulator(2)
    up1, sf1 = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, events=acc, scorecard=card,
                                 targets=[None, target])
    assert torch.equal(up0, up1) and torch.equal(sf0, sf1)
    assert [k for k, _, _ in kept] == [1] and acc.cases(0) == 0 and acc.cases(1) == 1 and card.cases(0) == 0 and card.cases(1) == 1
    _, up, sf = kept[0]
    assert torch.equal(up, up1) and torch.equal(sf, sf1)                            # the last step's physical fields
    for got, want in zip((up, sf), P.rollout.norm_back(*hist[1], sl)):
        assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-5, atol=1e-3)
    want_u, want_s = P.score.event_scores(up, sf, *target, thr, radii, regions, "nh")
    got_u, got_s = acc.sums(1)
    for got, want in ((got_u, want_u), (got_s, want_s)):
        assert torch.equal(got.counts, want.counts[0]) and torch.equal(got.wsums, want.wsums[0]) and torch.equal(got.fss_sums, want.fss_sums[0])
    nh = int(((P.score.region_bits(721, 1440, regions).bits >> 1) & 1).sum())
    assert bool((got_u.counts.sum(-1) == nh).all()) and int(got_u.counts[..., 0].sum()) > 0
    fss = got_u.fss()
    assert bool(torch.isfinite(fss).all()) and bool((fss[..., 1:] >= fss[..., :-1]).all())      # noise on the truth: smoother is better
    # events alone, without a scorecard
    alone = P.score.EventAccumulator(2, thr, radii, regions, "nh")
    up2, sf2 = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=graph, events=alone, targets=[None, target])
    assert torch.equal(up0, up2) and torch.equal(sf0, sf2) and alone.cases(0) == 0
    assert torch.equal(alone.sums(1)[0].fss_sums, got_u.fss_sums) and torch.equal(alone.sums(1)[1].counts, got_s.counts)
