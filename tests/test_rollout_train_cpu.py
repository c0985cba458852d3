"""Multi-step (rollout) fine-tuning, host side: the C entry point's argument checks, the torch form of the fused feed-back seed
against plain autograd through `norm_back`, and rollout_train_step's argument errors.  No GPU needed."""
import os

import pytest
import torch

from pangu_pytorch_amd import _lib, train
from pangu_pytorch_amd.rollout import norm_back

P8 = 8          # any non-NULL address: the calls below return before touching memory
GEOM = (1, 5, 13 * 100, 4, 100, 13, 0)


def _seed(lib, ptrs, geom=GEOM, stats=(None,) * 4):
    return lib.pangu_rollout_l1_seed_bwd(None, *ptrs, *geom, *stats)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_seed_entry_point_is_declared_and_bound():
    assert "pangu_rollout_l1_seed_bwd" in _lib.header_functions()
    assert len(_lib.SIGNATURES["pangu_rollout_l1_seed_bwd"]) == 25


# slots after the stream: out, target, out_surface, target_surface, w_upper, w_surface, grad, d_next, d_next_surface, std_upper,
# std_surface, d_out, d_out_surface
REQUIRED = (0, 1, 2, 3, 4, 5, 6, 11, 12)


@pytest.mark.parametrize("slot", REQUIRED)
def test_seed_null_in_a_required_slot(lib, slot):
    ptrs = [P8] * 13
    ptrs[slot] = None
    assert _seed(lib, ptrs) == -2
    ptrs[7:11] = [None] * 4                     # ... and in the last step's form (no d_next)
    assert _seed(lib, ptrs) == -2


def test_seed_d_next_needs_its_partner_and_the_stds(lib):
    base = [P8] * 13
    for missing in (7, 8, 9, 10):               # d_next, d_next_surface, std_upper, std_surface
        ptrs = list(base)
        ptrs[missing] = None
        assert _seed(lib, ptrs) == -2, missing
    ptrs = list(base)
    ptrs[9] = ptrs[10] = None                   # d_next without stds
    assert _seed(lib, ptrs) == -2
    assert _seed(lib, base, stats=(P8, None, None, None)) == -2          # target statistics: all four or none


def test_seed_shape_errors(lib):
    ptrs = [P8] * 13
    assert _seed(lib, ptrs, geom=(1, 5, 13 * 100, 4, 100, 11, 0)) == -1          # plane_u % levels != 0
    assert _seed(lib, ptrs, geom=(0, 5, 13 * 100, 4, 100, 13, 0)) == -1          # B = 0
    ptrs[7:11] = [None] * 4
    assert _seed(lib, ptrs, geom=(0, 5, 13 * 100, 4, 100, 13, 0)) == -1


# ---- the torch form of the seed == autograd through norm_back ------------------------------------------------------------------

B, V, L, H, W = 2, 5, 3, 6, 8


def _fields(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, V, L, H, W, generator=g), torch.randn(B, 4, H, W, generator=g)


@pytest.fixture(scope="module")
def stats_last():
    g = torch.Generator().manual_seed(7)
    return (torch.randn(1, 4, 1, 1, generator=g) * 10, torch.rand(1, 4, 1, 1, generator=g) * 5 + 0.5,
            torch.randn(1, V, L, 1, 1, generator=g) * 10, torch.rand(1, V, L, 1, 1, generator=g) * 5 + 0.5)


def _phys_targets(seed, stats_last, rev):
    t, t_s = norm_back(*_fields(seed), stats_last)
    return (t.flip(-3).contiguous() if rev else t), t_s


def _stand_in_model(up, sf, stats_last):
    """A differentiable map from physical input fields to normalised output fields (what the model is to the chain)."""
    s_mean, s_std, u_mean, u_std = stats_last
    x, x_s = (up - u_mean) / u_std, (sf - s_mean) / s_std
    return torch.tanh(x.roll(1, -1)) * 0.9 + 0.1 * x, torch.sin(x_s.roll(2, -2)) + 0.2 * x_s


@pytest.mark.parametrize("rev", [False, True])
def test_seed_reference_is_autograd_through_norm_back(stats_last, rev):
    lam = (0.3, 0.7)
    out, out_s = (t.requires_grad_(True) for t in _fields(1))
    tgt1, tgt2 = _phys_targets(2, stats_last, rev), _phys_targets(3, stats_last, rev)
    # plain autograd over the whole chain
    up, sf = norm_back(out, out_s, stats_last)
    out2, out2_s = _stand_in_model(up, sf, stats_last)
    total = lam[0] * train._weighted_l1_loss_torch(out, out_s, *tgt1, rev, stats_last) \
        + lam[1] * train._weighted_l1_loss_torch(out2, out2_s, *tgt2, rev, stats_last)
    ref, ref_s = torch.autograd.grad(total, (out, out_s))
    # the same chain cut at the fed-back state: d_next from step 2 alone, then the seed formula
    up2, sf2 = (t.detach().requires_grad_(True) for t in (up, sf))
    o2, o2_s = _stand_in_model(up2, sf2, stats_last)
    d_next, d_next_s = torch.autograd.grad(lam[1] * train._weighted_l1_loss_torch(o2, o2_s, *tgt2, rev, stats_last), (up2, sf2))
    got, got_s = train._rollout_seed_torch(out.detach(), out_s.detach(), *tgt1, torch.tensor(lam[0]), d_next, d_next_s, stats_last, rev)
    assert torch.equal(got, ref) and torch.equal(got_s, ref_s)
    assert d_next.abs().max() > 0 and not torch.equal(got, got - d_next * stats_last[3])       # the chain term is really there
    # without d_next: the loss gradient alone
    a, a_s = train._rollout_seed_torch(out.detach(), out_s.detach(), *tgt1, torch.tensor(lam[0]), None, None, stats_last, rev)
    la = lam[0] * train._weighted_l1_loss_torch(out, out_s, *tgt1, rev, stats_last)
    ra, ra_s = torch.autograd.grad(la, (out, out_s))
    assert torch.equal(a, ra) and torch.equal(a_s, ra_s)


@pytest.mark.parametrize("rev", [False, True])
def test_step_function_chain_is_autograd_through_norm_back(stats_last, rev):
    """RolloutStepFn (its torch arm: CPU tensors) chained over three steps, with the fed-back fields handed in as buffers the way
    the forward's last kernel writes them, gives the gradients of the plain torch composition."""
    lam = (0.2, 0.5, 0.3)
    x0, x0_s = norm_back(*_fields(11), stats_last)
    w = torch.nn.Parameter(torch.tensor(0.8))          # a "model parameter" shared by all steps
    tg = [_phys_targets(20 + k, stats_last, rev) for k in range(3)]

    def model(up, sf):
        o, o_s = _stand_in_model(up, sf, stats_last)
        return o * w, o_s * w

    cur, cur_s, losses = x0, x0_s, []
    for k in range(3):
        o, o_s = model(cur, cur_s)
        losses.append(train._weighted_l1_loss_torch(o, o_s, *tg[k], rev, stats_last))
        cur, cur_s = norm_back(o, o_s, stats_last)
    ref_total = train._weighted_total(losses, lam)
    ref_w, = torch.autograd.grad(ref_total, (w,))

    cur, cur_s, got = x0, x0_s, []
    for k in range(3):
        o, o_s = model(cur, cur_s)
        nxt = nxt_s = None
        if k < 2:
            with torch.no_grad():                       # stands for ops.scatter_denorm: plain buffers holding norm_back(out)
                nxt, nxt_s = norm_back(o, o_s, stats_last)
        loss_k, cur, cur_s = train.RolloutStepFn.apply(o, o_s, *tg[k], nxt, nxt_s, rev, stats_last)
        got.append(loss_k)
    assert cur is None and cur_s is None
    total = train._weighted_total(got, lam)
    got_w, = torch.autograd.grad(total, (w,))
    assert torch.equal(total, ref_total) and all(torch.equal(a, b) for a, b in zip(got, losses))
    torch.testing.assert_close(got_w, ref_w, rtol=1e-5, atol=0)      # (the sum over a field's elements runs in another order)


# ---- argument errors -----------------------------------------------------------------------------------------------------------

def _cpu_batch(K, B_=1):
    f = lambda: torch.zeros(B_, 5, 13, 8, 16)
    s = lambda: torch.zeros(B_, 4, 8, 16)
    return (f(), s()) + tuple(t for _ in range(K) for t in (f(), s()))


STATS = (torch.zeros(1, 4, 1, 1), torch.ones(1, 4, 1, 1), torch.zeros(1, 5, 13, 1, 1), torch.ones(1, 5, 13, 1, 1))


def _call(batch, stats_last=STATS, **kw):
    return train.rollout_train_step(None, None, batch, None, None, None, stats_last, **kw)


def test_rollout_train_step_argument_errors():
    with pytest.raises(ValueError, match="empty or odd"):
        _call(_cpu_batch(2)[:5])                        # odd target list
    with pytest.raises(ValueError, match="empty or odd"):
        _call(_cpu_batch(1)[:2])                        # no target at all
    with pytest.raises(ValueError, match="lead_weights"):
        _call(_cpu_batch(2), lead_weights=[1.0])
    with pytest.raises(ValueError, match="stats_last"):
        _call(_cpu_batch(2), stats_last=None)
    with pytest.raises(ValueError, match="one sample"):
        _call(_cpu_batch(2, B_=2))
    bad = list(_cpu_batch(2))
    bad[4] = torch.zeros(1, 5, 13, 8, 12)
    with pytest.raises(ValueError, match="target 2"):
        _call(bad)
    bad = list(_cpu_batch(2))
    bad[3] = torch.zeros(1, 3, 8, 16)
    with pytest.raises(ValueError, match="target 1"):
        _call(bad)
    with pytest.raises(RuntimeError, match="CPU tensors"):
        _call(_cpu_batch(2))
    with pytest.raises(TypeError):                      # the options are keyword-only
        train.rollout_train_step(None, None, _cpu_batch(1), None, None, None, STATS, [1.0])
