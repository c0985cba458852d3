"""Ensemble kernels and EnsembleRollout on the GPU: the perturbation against the float64 numpy restatement of its definition
(test_ensemble_cpu.noise_ref), the ensemble scores against a float64 torch restatement, and the rollout against the
single-trajectory rollout."""
import numpy as np
import pytest
import torch

import cases
import synth
from test_ensemble_cpu import perturb_ref

pytestmark = pytest.mark.gpu


def _stats_last(stats):
    s_mean, s_std, u_mean, u_std = stats
    return (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1),
            u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
            u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())


def _small_stats(gen):
    u = lambda shape, lo, hi: torch.rand(shape, generator=gen, device="cuda") * (hi - lo) + lo
    return (u((1, 4, 1, 1), -0.5, 0.5), u((1, 4, 1, 1), 0.5, 2.0), u((1, 5, 13, 1, 1), -0.5, 0.5), u((1, 5, 13, 1, 1), 0.5, 2.0))


# ---- perturbation --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,octaves,period,first", [(37, 96, 3, 12, 0), (37, 96, 2, 6, 5), (181, 360, 3, 5, 0),
                                                      (181, 360, 2, 12, 9)])
def test_perturb_matches_numpy_restatement(H, W, octaves, period, first):
    import pangu_pytorch_amd as P
    g = torch.Generator(device="cuda").manual_seed(H + first)
    sl = _small_stats(g)
    up = torch.randn((3, 5, 13, H, W), generator=g, device="cuda")
    sf = torch.randn((3, 4, H, W), generator=g, device="cuda")
    amp = [0.5, 0.3, 0.7, 0.2, 0.4, 0.6, 0.1, 0.8, 0.9]
    up0, sf0 = up.clone(), sf.clone()
    P.ensemble.perturb_(up, sf, sl, amp, 1234, octaves=octaves, period=period, first_member=first)
    ref_u, ref_s = perturb_ref(up0.cpu().numpy(), sf0.cpu().numpy(), sl[3].cpu().numpy(), sl[1].cpu().numpy(), amp, 1234,
                               octaves=octaves, period=period, first_member=first)
    scale = np.array([amp[p // 13] for p in range(65)] + amp[5:]) * np.concatenate(
        [sl[3].cpu().numpy().reshape(-1), sl[1].cpu().numpy().reshape(-1)])
    got_u = up.double().cpu().numpy().reshape(3, 65, H, W)
    got_s = sf.double().cpu().numpy()
    err_u = np.abs(got_u - ref_u.reshape(3, 65, H, W)).max(axis=(0, 2, 3)) / scale[:65]
    err_s = np.abs(got_s - ref_s).max(axis=(0, 2, 3)) / scale[65:]
    assert max(err_u.max(), err_s.max()) <= 1e-5, (err_u.max(), err_s.max())
    if first == 0:                                            # control member untouched, the others perturbed
        assert torch.equal(up[0], up0[0]) and torch.equal(sf[0], sf0[0])
    assert not torch.equal(up[1], up0[1])


def test_perturb_full_grid_planes_and_chunk_independence():
    import pangu_pytorch_amd as P
    H, W = 721, 1440
    g = torch.Generator(device="cuda").manual_seed(7)
    sl = _small_stats(g)
    up = torch.randn((3, 5, 13, H, W), generator=g, device="cuda")
    sf = torch.randn((3, 4, H, W), generator=g, device="cuda")
    up0, sf0 = up.clone(), sf.clone()
    P.ensemble.perturb_(up, sf, sl, 0.25, 99, first_member=0)
    planes = (0, 27, 64, 65, 68)
    ref_u, ref_s = perturb_ref(up0[1:].cpu().numpy(), sf0[1:].cpu().numpy(), sl[3].cpu().numpy(), sl[1].cpu().numpy(), 0.25, 99,
                               first_member=1, planes=planes)
    std = np.concatenate([sl[3].cpu().numpy().reshape(-1), sl[1].cpu().numpy().reshape(-1)])
    for p in planes:
        if p < 65:
            got, ref = up[1:, p // 13, p % 13].double().cpu().numpy(), ref_u[:, p // 13, p % 13]
        else:
            got, ref = sf[1:, p - 65].double().cpu().numpy(), ref_s[:, p - 65]
        assert np.abs(got - ref).max() <= 1e-5 * 0.25 * std[p], p
    assert torch.equal(up[0], up0[0]) and torch.equal(sf[0], sf0[0])
    # member 2 made alone (E = 1, first_member = 2) == member 2 of the batch, bit for bit
    u2, s2 = up0[2:3].clone(), sf0[2:3].clone()
    P.ensemble.perturb_(u2, s2, sl, 0.25, 99, first_member=2)
    assert torch.equal(u2[0], up[2]) and torch.equal(s2[0], sf[2])


# ---- scores --------------------------------------------------------------------------------------------------------

def _scores_ref(x, y, c, w):
    """float64 restatement: x (E, planes, H, W), y (planes, H, W), c (planes,), w (H,)."""
    E, N = x.shape[0], x.shape[-2] * x.shape[-1]
    wv = w.view(-1, 1)
    ws = lambda t: (wv * t).sum((-2, -1))
    m, var = x.mean(0), x.var(0, unbiased=True)
    mc, yc = m - c.view(-1, 1, 1), y - c.view(-1, 1, 1)
    pair = torch.zeros_like(m)
    for i in range(E):
        pair += (x[i] - x).abs().sum(0)
    crps = (x - y).abs().mean(0) - pair / (2 * E * (E - 1))
    return {"rmse_mean": torch.sqrt(ws((m - y) ** 2) / N), "acc_mean": ws(mc * yc) / torch.sqrt(ws(mc ** 2) * ws(yc ** 2)),
            "spread": torch.sqrt(ws(var) / N), "crps": ws(crps) / N, "mean": m, "std": var.sqrt()}


def _ensemble_data(E, H, W, seed, ties=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    base_u = torch.randn((5, 13, H, W), generator=g, device="cuda") * 3
    base_s = torch.randn((4, H, W), generator=g, device="cuda") * 3
    up = base_u + 0.5 * torch.randn((E, 5, 13, H, W), generator=g, device="cuda")
    sf = base_s + 0.5 * torch.randn((E, 4, H, W), generator=g, device="cuda")
    if ties:                                                  # a few members equal to others (not all of them)
        for a, b in ((1, 0),) + (((E - 1, 0), (E // 2, 1)) if E >= 5 else ()):
            up[a], sf[a] = up[b], sf[b]
    tu = base_u + 0.5 * torch.randn((5, 13, H, W), generator=g, device="cuda")
    ts = base_s + 0.5 * torch.randn((4, H, W), generator=g, device="cuda")
    return up.contiguous(), sf.contiguous(), tu, ts, _small_stats(g)


def _check_scores(P, up, sf, tu, ts, sl, tol=1e-5):
    su, ss = P.score.ensemble_scores(up, sf, tu, ts, sl, want_fields=True)
    H = up.shape[-2]
    w = P.score.latitude_weights(H, "cuda").double()
    for got, x, y, c in ((su, up.flatten(1, 2), tu.flatten(0, 1), sl[2]), (ss, sf, ts, sl[0])):
        ref = _scores_ref(x.double(), y.double(), c.double().reshape(-1), w)
        for k in ("rmse_mean", "acc_mean", "spread", "crps"):
            r, q = ref[k], got[k].reshape(-1).double()
            assert ((q - r).abs().max() / r.abs().max()).item() <= tol, (k, x.shape[0])
        for k in ("mean", "std"):
            r, q = ref[k], got[k].reshape(ref[k].shape).double()
            assert ((q - r).abs().max() / r.abs().max()).item() <= tol, k
    return su, ss


@pytest.mark.parametrize("E", [2, 3, 17, 50, 100, 128])
def test_scores_small_grid_vs_float64(E):
    import pangu_pytorch_amd as P
    up, sf, tu, ts, sl = _ensemble_data(E, 19, 32, E, ties=E >= 3)
    su, ss = _check_scores(P, up, sf, tu, ts, sl)
    su2, ss2 = P.score.ensemble_scores(up, sf, tu, ts, sl, want_fields=True)
    for a, b in ((su, su2), (ss, ss2)):                       # deterministic: bit-identical from call to call
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_scores_full_grid_and_score_module_agreement():
    import pangu_pytorch_amd as P
    up, sf, tu, ts, sl = _ensemble_data(4, 721, 1440, 3)
    su, ss = _check_scores(P, up, sf, tu, ts, sl)
    su2, _ = P.score.ensemble_scores(up, sf, tu, ts, sl)
    assert all(torch.equal(su[k], su2[k]) for k in su2)
    # the mean-field scores equal score.weighted_*_channels of the written mean field (different summation order)
    for got, y, c in ((su, tu, sl[2].reshape(5, 13, 1, 1)), (ss, ts, sl[0].reshape(4, 1, 1))):
        rmse = P.score.weighted_rmse_channels(got["mean"], y)
        acc = P.score.weighted_acc_channels((got["mean"] - c).contiguous(), (y - c).contiguous())
        assert ((rmse - got["rmse_mean"]).abs().max() / rmse.abs().max()).item() <= 1e-5
        assert ((acc - got["acc_mean"]).abs().max() / acc.abs().max()).item() <= 1e-5


# ---- rollout -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def setup():
    import pangu_pytorch_amd as P
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return P, m, cases.model_inputs("cuda")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rollout_zero_amplitude_equals_single_rollout(setup, dtype):
    P, m, (inp, inp_s, stats, maps, const_h) = setup
    sl = _stats_last(stats)
    m.set_compute_dtype(dtype)
    try:
        up_r, sf_r = P.rollout.rollout(m, inp, inp_s, stats, maps, const_h, sl, steps=2, graph=True)
        ens = P.ensemble.EnsembleRollout(m, inp, inp_s, stats, maps, const_h, sl, members=3, amplitude=0.0, seed=5, chunk=2)
        ens.step()
        ens.step()
        up, sf = ens.state()
        for e in range(3):
            assert torch.equal(up[e], up_r[0]) and torch.equal(sf[e], sf_r[0]), e
        tu, ts = cases.model_targets("cuda")
        su, ss = ens.scores(tu, ts)
        w = P.score.latitude_weights(up.shape[-2], "cuda").double().view(-1, 1)
        for got, x, y in ((su, up_r[0], tu[0]), (ss, sf_r[0], ts[0])):
            spread_ok = got["spread"].double() <= 1e-6 * x.double().std(dim=(-2, -1))
            assert bool(spread_ok.all())
            mae = (w * (x.double() - y.double()).abs()).sum((-2, -1)) / (x.shape[-2] * x.shape[-1])
            assert ((got["crps"].double() - mae).abs().max() / mae.abs().max()).item() <= 1e-5
        (mu, ms), (du, ds) = ens.mean_std()
        assert (mu - up_r[0]).abs().max().item() <= 1e-5 * up_r[0].abs().max().item() and du.abs().max().item() <= 1e-5
    finally:
        m.set_compute_dtype(torch.float32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rollout_chunking_is_bit_identical(setup, dtype):
    P, m, (inp, inp_s, stats, maps, const_h) = setup
    sl = _stats_last(stats)
    m.set_compute_dtype(dtype)
    try:
        states = []
        for chunk in (1, 3):
            ens = P.ensemble.EnsembleRollout(m, inp, inp_s, stats, maps, const_h, sl, members=3, amplitude=0.05, seed=11,
                                             chunk=chunk)
            ens.step()
            ens.step()
            states.append(tuple(t.clone() for t in ens.state()))
            del ens
        assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])
        assert not torch.equal(states[0][0][1], states[0][0][2])        # the members differ
    finally:
        m.set_compute_dtype(torch.float32)


def test_rollout_members_equal_eager_rollout_fp32(setup):
    """Each member == the eager rollout (graph=False) from its own perturbed initial state; reset() re-perturbs without
    re-capturing."""
    P, m, (inp, inp_s, stats, maps, const_h) = setup
    sl = _stats_last(stats)
    ens = P.ensemble.EnsembleRollout(m, inp, inp_s, stats, maps, const_h, sl, members=3, amplitude=0.05, seed=3)
    init = tuple(t.clone() for t in ens.state())
    ens.step()
    ens.step()
    up, sf = ens.state()
    for e in range(3):
        ref_u, ref_s = P.rollout.rollout(m, init[0][e:e + 1], init[1][e:e + 1], stats, maps, const_h, sl, steps=2, graph=False)
        assert torch.equal(up[e], ref_u[0]) and torch.equal(sf[e], ref_s[0]), e
    ens.reset(inp, inp_s)
    assert torch.equal(ens.state()[0], init[0]) and torch.equal(ens.state()[1], init[1])
    ens.reset(inp, inp_s, seed=4)
    assert torch.equal(ens.state()[0][0], init[0][0]) and not torch.equal(ens.state()[0][1], init[0][1])
