"""Fair-CRPS ensemble fine-tuning, host side: the torch form of the loss (train._fair_crps_loss_torch, the reference of
tests/test_gpu_crps_train.py) against the closed-form gradient and against the weighted L1 loss, the C entry points' argument
checks, and ensemble_train_step's refusals.  No GPU needed."""
import ctypes
import os

import pytest
import torch

from pangu_pytorch_amd import _lib, dist, train
from pangu_pytorch_amd.rollout import norm_back

L, H, W = 2, 5, 8


def _members(E, seed, dtype=torch.float64):
    """x (E,5,L,H,W), x_s (E,4,H,W), t (1,5,L,H,W), t_s (1,4,H,W) with planted ties: member 1 == member 0 on one row, member 0 ==
    target on another, every member == target at one point (and with E > 2, three members tied on a third row)."""
    g = torch.Generator().manual_seed(seed)
    x, x_s = torch.randn(E, 5, L, H, W, generator=g, dtype=dtype), torch.randn(E, 4, H, W, generator=g, dtype=dtype)
    t, t_s = torch.randn(1, 5, L, H, W, generator=g, dtype=dtype), torch.randn(1, 4, H, W, generator=g, dtype=dtype)
    x[1, :, :, 1] = x[0, :, :, 1]
    x_s[1, :, 1] = x_s[0, :, 1]
    x[0, :, :, 2] = t[0, :, :, 2]
    x_s[0, :, 2] = t_s[0, :, 2]
    x[:, 1, 0, 3, 4] = t[0, 1, 0, 3, 4]
    x_s[:, 2, 3, 4] = t_s[0, 2, 3, 4]
    if E > 2:
        x[2, :, :, 4] = x[1, :, :, 4] = x[0, :, :, 4]
        x_s[2, :, 4] = x_s[1, :, 4] = x_s[0, :, 4]
    return x, x_s, t, t_s


def _closed_form(x, t, w, a, k, g=1.0):
    """d x_e = g k w[v] a[h] (sign(x_e - t)/E - sum_f sign(x_e - x_f) / (E(E-1)))."""
    E = x.shape[0]
    pair = torch.sign(x.unsqueeze(1) - x.unsqueeze(0)).sum(1)             # [e] = sum_f sign(x_e - x_f)
    return g * k * w * a * (torch.sign(x - t) / E - pair / (E * (E - 1)))


def _lat(dtype):
    return train._crps_lat_weights(H, torch.device("cpu")).to(dtype).view(H, 1)


@pytest.mark.parametrize("lat_weighted", [True, False])
@pytest.mark.parametrize("E", [2, 3, 5, 16])
def test_torch_form_has_the_closed_form_gradient(E, lat_weighted):
    x, x_s, t, t_s = _members(E, 10 + E)
    xs = [x[e:e + 1].clone().requires_grad_(True) for e in range(E)]
    xs_s = [x_s[e:e + 1].clone().requires_grad_(True) for e in range(E)]
    loss = train._fair_crps_loss_torch(xs, xs_s, t, t_s, lat_weighted=lat_weighted)
    g = 0.37
    (loss * g).backward()
    wu = torch.tensor(train.UPPER_WEIGHTS, dtype=torch.float64).view(1, 5, 1, 1, 1)
    ws = torch.tensor(train.SURFACE_WEIGHTS, dtype=torch.float64).view(1, 4, 1, 1)
    a = _lat(torch.float64) if lat_weighted else torch.ones(H, 1, dtype=torch.float64)
    assert float(a.min()) >= 0.0
    want = _closed_form(x, t, wu, a, 1.0 / t.numel(), g)
    want_s = _closed_form(x_s, t_s, ws, a, 0.25 / t_s.numel(), g)
    got, got_s = torch.cat([v.grad for v in xs]), torch.cat([v.grad for v in xs_s])
    assert float((got - want).abs().max()) <= 1e-12 and float((got_s - want_s).abs().max()) <= 1e-12
    assert float(want.abs().max()) > 1e-4
    if E == 2:          # member 1 where member 0 is tied with the target: the two signs cancel, an exact zero
        assert float(got[1, :, :, 2].abs().max()) == 0.0 and float(got[0, :, :, 2].abs().min()) > 0.0
    # the loss itself, from the definition point by point
    c = (x - t).abs().mean(0) - (x.unsqueeze(1) - x.unsqueeze(0)).abs().sum((0, 1)) / (2 * E * (E - 1))
    c_s = (x_s - t_s).abs().mean(0) - (x_s.unsqueeze(1) - x_s.unsqueeze(0)).abs().sum((0, 1)) / (2 * E * (E - 1))
    ref = (c * wu[0] * a).mean() + 0.25 * (c_s * ws[0] * a).mean()
    assert abs(float(loss.detach()) - float(ref)) <= 1e-12 * abs(float(ref))


@pytest.mark.parametrize("E", [2, 5])
def test_identical_members_give_the_weighted_l1_loss(E):
    x, x_s, t, t_s = _members(E, 3)
    o, o_s = x[:1].clone().requires_grad_(True), x_s[:1].clone().requires_grad_(True)
    ref = train._weighted_l1_loss_torch(o, o_s, t, t_s)
    d_ref, d_ref_s = torch.autograd.grad(ref, (o, o_s))
    xs = [x[:1].clone().requires_grad_(True) for _ in range(E)]
    xs_s = [x_s[:1].clone().requires_grad_(True) for _ in range(E)]
    got = train.fair_crps_loss(xs, xs_s, t, t_s, lat_weighted=False)          # (CPU tensors: the torch form)
    assert abs(float(got.detach()) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
    got.backward()
    for v, v_s in zip(xs, xs_s):                    # each member carries 1/E of the L1 gradient
        assert float((v.grad * E - d_ref).abs().max()) <= 1e-12 and float((v_s.grad * E - d_ref_s).abs().max()) <= 1e-12


def test_target_statistics_and_level_reversal():
    E = 3
    x, x_s, t, t_s = _members(E, 4)
    g = torch.Generator().manual_seed(7)
    sl = (torch.randn(1, 4, 1, 1, generator=g, dtype=torch.float64) * 10, torch.rand(1, 4, 1, 1, generator=g, dtype=torch.float64) * 5 + 0.5,
          torch.randn(1, 5, L, 1, 1, generator=g, dtype=torch.float64) * 10, torch.rand(1, 5, L, 1, 1, generator=g, dtype=torch.float64) * 5 + 0.5)
    phys, phys_s = norm_back(t, t_s, sl)
    stored = phys.flip(-3).contiguous()                                     # as on disk: ascending levels
    xs, xs_s = [x[e:e + 1] for e in range(E)], [x_s[e:e + 1] for e in range(E)]
    got = train._fair_crps_loss_torch(xs, xs_s, stored, phys_s, True, sl)
    tn, tn_s = train.norm_data(stored.flip(-3), phys_s, sl)                   # the explicit flip and normData
    want = train._fair_crps_loss_torch(xs, xs_s, tn, tn_s)
    assert float(got) == float(want)
    assert float(got) != float(train._fair_crps_loss_torch(xs, xs_s, tn.flip(-3), tn_s))       # the reversal matters


def test_member_count_is_checked():
    x, x_s, t, t_s = _members(2, 5)
    for E in (1, 17):
        with pytest.raises(ValueError, match="members"):
            train.fair_crps_loss([x[:1]] * E, [x_s[:1]] * E, t, t_s)
    with pytest.raises(ValueError, match="surface member fields"):
        train.fair_crps_loss([x[:1]] * 2, [x_s[:1]] * 3, t, t_s)


# ---- the C entry points ----------------------------------------------------------------------------------------------------------

P8 = 8          # any non-NULL address: the calls below return before touching memory
GEOM = (1, 5, 13, 4, 37, 96)


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _arr(E, null_at=None):
    return (ctypes.c_void_p * max(E, 1))(*[None if e == null_at else P8 for e in range(max(E, 1))])


def test_entries_are_declared_and_bound():
    names = ("pangu_fair_crps_loss_blocks", "pangu_fair_crps_loss_fwd", "pangu_fair_crps_loss_bwd")
    assert all(n in _lib.header_functions() and n in _lib.SIGNATURES for n in names)
    assert [len(_lib.SIGNATURES[n]) for n in names] == [7, 22, 23]


def test_entry_argument_validation_without_gpu():
    lib = _lib_or_skip()

    def fwd(E=3, ptrs=None, members=None, members_s=None, geom=GEOM, stats=(None,) * 4):
        p = [P8] * 7 if ptrs is None else ptrs          # target, target_surface, w_upper, w_surface, lat_weight, partial, loss
        return lib.pangu_fair_crps_loss_fwd(None, _arr(E) if members is None else members, _arr(E) if members_s is None else members_s,
                                            E, *p, *geom, 0, *stats)

    def bwd(E=3, ptrs=None, members=None, d_members=None, d_members_s=None, geom=GEOM, stats=(None,) * 4):
        p = [P8] * 6 if ptrs is None else ptrs          # target, target_surface, w_upper, w_surface, lat_weight, grad
        return lib.pangu_fair_crps_loss_bwd(None, _arr(E) if members is None else members, _arr(E), E, *p,
                                            _arr(E) if d_members is None else d_members, _arr(E) if d_members_s is None else d_members_s,
                                            *geom, 0, *stats)

    # blocks: E = 2 keeps 8 vectors per thread (8192-element chunks), E >= 9 one (1024)
    assert lib.pangu_fair_crps_loss_blocks(2, 1, 5, 13, 4, 721, 1440) == 69 * 127
    assert lib.pangu_fair_crps_loss_blocks(16, 1, 5, 13, 4, 721, 1440) == 69 * 1014
    assert lib.pangu_fair_crps_loss_blocks(3, *GEOM) == 69 * 1
    for E in (1, 17, 0, -3):
        assert lib.pangu_fair_crps_loss_blocks(E, *GEOM) == -4
        assert fwd(E=E) == -4 and bwd(E=E) == -4
    # null pointers: every required slot, the member arrays and their entries; lat_weight alone may be NULL
    for slot in (0, 1, 2, 3, 5, 6):
        p = [P8] * 7
        p[slot] = None
        assert fwd(ptrs=p) == -2, slot
    for slot in (0, 1, 2, 3, 5):
        p = [P8] * 6
        p[slot] = None
        assert bwd(ptrs=p) == -2, slot
    assert lib.pangu_fair_crps_loss_fwd(None, None, _arr(3), 3, *[P8] * 7, *GEOM, 0, *(None,) * 4) == -2
    assert lib.pangu_fair_crps_loss_fwd(None, _arr(3), None, 3, *[P8] * 7, *GEOM, 0, *(None,) * 4) == -2
    assert lib.pangu_fair_crps_loss_bwd(None, _arr(3), _arr(3), 3, *[P8] * 6, None, _arr(3), *GEOM, 0, *(None,) * 4) == -2
    assert lib.pangu_fair_crps_loss_bwd(None, _arr(3), _arr(3), 3, *[P8] * 6, _arr(3), None, *GEOM, 0, *(None,) * 4) == -2
    for e in range(3):
        assert fwd(members=_arr(3, null_at=e)) == -2 and fwd(members_s=_arr(3, null_at=e)) == -2
        assert bwd(members=_arr(3, null_at=e)) == -2 and bwd(d_members=_arr(3, null_at=e)) == -2
        assert bwd(d_members_s=_arr(3, null_at=e)) == -2
    # statistics: all four or none
    for n in (1, 2, 3):
        for first in range(4):
            st = [None] * 4
            for i in range(n):
                st[(first + i) % 4] = P8
            assert fwd(stats=st) == -2 and bwd(stats=st) == -2
    # sizes: non-positive, or overflowing (H * W beyond 32-bit in-plane indices; more blocks than a grid holds)
    for i in range(6):
        for bad in (0, -1):
            geom = list(GEOM)
            geom[i] = bad
            assert fwd(geom=geom) == -1 and bwd(geom=geom) == -1 and lib.pangu_fair_crps_loss_blocks(3, *geom) == -1
    for geom in ((1, 5, 13, 4, 1 << 16, 1 << 15), (1, 5, 13, 4, (1 << 31) - 1, (1 << 31) - 1), (1 << 20, 1 << 20, 13, 4, 37, 96),
                 ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, 37, 96), (1 << 12, 1 << 12, 1, 4, 721, 1440)):
        assert fwd(geom=geom) == -1 and bwd(geom=geom) == -1 and lib.pangu_fair_crps_loss_blocks(3, *geom) == -1


# ---- ensemble_train_step's refusals (before any launch) ------------------------------------------------------------------------

STATS = (torch.zeros(1, 4, 1, 1), torch.ones(1, 4, 1, 1), torch.zeros(1, 5, 13, 1, 1), torch.ones(1, 5, 13, 1, 1))


def _cpu_batch(B=1, lon=96):
    f, s = (lambda: torch.zeros(B, 5, 13, 8, lon)), (lambda: torch.zeros(B, 4, 8, lon))
    return f(), s(), f(), s()


def _call(batch, stats_last=STATS, members=4, amplitude=0.1, seed=0, **kw):
    return train.ensemble_train_step(None, None, batch, None, None, None, stats_last, members=members, amplitude=amplitude,
                                     seed=seed, **kw)


def test_ensemble_train_step_refusals():
    for members in (1, 17, 0):
        with pytest.raises(ValueError, match="members"):
            _call(_cpu_batch(), members=members)
    with pytest.raises(ValueError, match="amplitude"):
        _call(_cpu_batch(), amplitude=None)
    with pytest.raises(ValueError, match="9 values"):
        _call(_cpu_batch(), amplitude=[0.1] * 4)
    with pytest.raises(TypeError):                      # members, amplitude and seed are required keywords
        train.ensemble_train_step(None, None, _cpu_batch(), None, None, None, STATS, members=4, seed=0)
    with pytest.raises(TypeError):
        train.ensemble_train_step(None, None, _cpu_batch(), None, None, None, STATS, 4, 0.1, 0)
    with pytest.raises(ValueError, match="one sample"):
        _call(_cpu_batch(B=2))
    with pytest.raises(ValueError, match="stats_last"):
        _call(_cpu_batch(), stats_last=None)
    with pytest.raises(ValueError, match="got 3 tensors"):
        _call(_cpu_batch()[:3])
    bad = list(_cpu_batch())
    bad[2] = torch.zeros(1, 5, 13, 8, 48)
    with pytest.raises(ValueError, match="the target is"):
        _call(bad)
    with pytest.raises(ValueError, match="W % L"):      # the perturbation lattice must divide the longitude circle
        _call(_cpu_batch(lon=120))
    with pytest.raises(RuntimeError, match="CPU tensors"):
        _call(_cpu_batch())
    with pytest.raises(RuntimeError, match="CPU tensors"):
        _call(_cpu_batch(), checkpoint=False)
    sync = dist.FlatGradSync(torch.nn.Linear(4, 4))
    try:
        with pytest.raises(RuntimeError, match="FlatGradSync"):
            _call(_cpu_batch(), grad_sync=sync.finish)                      # checkpoint=True is the default
        with pytest.raises(RuntimeError, match="FlatGradSync"):
            _call(_cpu_batch(), grad_sync=sync.finish, checkpoint=True)
        with pytest.raises(RuntimeError, match="CPU tensors"):              # ... while checkpoint=False takes it
            _call(_cpu_batch(), grad_sync=sync.finish, checkpoint=False)
    finally:
        sync.remove()
