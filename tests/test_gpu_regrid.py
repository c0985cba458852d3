"""Conservative regridding on the GPU: pangu_regrid_planes_f32 against the float64 restatement of tests/test_regrid_cpu.py, the
Python surface (score.regrid, score.regrid_fields), data.HostDrain(regrid=...) and EnsembleRollout.scores(regrid=...).

The bound is derived, not measured: |got - ref| <= (T_lat + T_lon + 4) * 2^-24 * (|R_lat| |v| |R_lon|^T), the forward error of the
two sequential fp32 fma chains with fp32-rounded weights (test_regrid_cpu.error_bound).  Worst |error| / bound seen on an MI355X,
per case of test_kernel_matches_reference (which prints them; tools/bench_regrid.py records its own fields' in
profiles/regrid.json):
    13x24->7x12 0.259, with affine and levels 0.246;  13x24->5x8 (affine) 0.268;  19x30->7x9 0.296, with affine and levels 0.305;
    11x10->4x3 0.152;  41x40->5x4 (11 taps per axis) 0.105;  37x1440->7x240 0.179;  721x16->121x4 0.156;  721x1440->121x240 0.214;  views one float in: 0.270 / 0.182 /
    0.213;  with a NaN and two infinities planted 0.298 / 0.251;  the identity plan: bit for bit."""
import numpy as np
import pytest
import torch

from test_regrid_cpu import error_bound, regrid_ref, stencil_nonfinite

pytestmark = pytest.mark.gpu

POISON = -7.25e33
SCORE_RTOL = 1e-5                                # tests/test_gpu_quantiles.py's tolerance for the per-plane ensemble scores


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    P._lib.load()
    return P


_PLANS = {}


def plan_of(P, grid):
    if grid not in _PLANS:
        _PLANS[grid] = P.score.regrid_plan(*grid)
    return _PLANS[grid]


def field(planes, H, W, seed):
    """Smooth waves plus N(0, 1) noise on an offset of about 280 (a temperature in kelvin), seeded; numpy float32."""
    r = np.random.default_rng(seed)
    lat = np.linspace(0.5 * np.pi, -0.5 * np.pi, H)[None, :, None]
    lon = (2.0 * np.pi * np.arange(W) / W)[None, None, :]
    k = (1 + np.arange(planes) % 5)[:, None, None]
    x = 280.0 + 0.1 * np.arange(planes)[:, None, None] + 20.0 * np.cos(lat) * np.sin(k * lon) + 8.0 * np.sin(3 * lat)
    return (x + r.standard_normal((planes, H, W))).astype(np.float32)


def affine(planes, seed):
    r = np.random.default_rng(seed)
    return r.uniform(0.5, 3.0, planes).astype(np.float32), r.uniform(-200.0, 900.0, planes).astype(np.float32)


def abi_regrid(P, x, plan, mul=None, add=None, levels=0, guard=64):
    """x: a (planes, H_in, W_in) fp32 CUDA tensor (any 4-B aligned view) -> (planes, H_out, W_out) numpy through the C ABI on the
    current stream.  dst is filled with a poison value first and is `guard` floats longer than the output: the guard must come
    back untouched and no poison may be left in the output."""
    planes = x.shape[0]
    assert tuple(x.shape[1:]) == plan.in_grid and x.is_contiguous()
    n = planes * plan.H_out * plan.W_out
    dst = torch.full((n + guard,), POISON, device="cuda")
    dev = lambda t: None if t is None else (t if torch.is_tensor(t) else torch.from_numpy(t).cuda())
    mul, add = dev(mul), dev(add)
    P.score._regrid_launch(torch.cuda.current_stream().cuda_stream, x.data_ptr(), mul, add, dst.data_ptr(), planes, plan, levels,
                           x.device)
    torch.cuda.synchronize()
    assert bool((dst[n:] == POISON).all()), "wrote behind the output"
    out = dst[:n].view(planes, plan.H_out, plan.W_out)
    assert not bool((out == POISON).any()), "left part of the output unwritten"
    return out.cpu().numpy()


def check(plan, got, x, mul=None, add=None, levels=0, what=""):
    """got against regrid_ref within the derived bound; non-finite inputs: non-finite outputs exactly where the stencil holds one,
    the bound everywhere else (the reference is taken of the field with those values replaced, which the other cells never read).
    Returns the worst |error| / bound."""
    bad = ~np.isfinite(x)
    ref, mag = regrid_ref(np.where(bad, np.float32(0), x), plan, mul, add, levels)
    hit = np.zeros(ref.shape, bool)
    if bad.any():
        order = np.arange(x.shape[0])
        if levels > 1:
            order = order.reshape(-1, levels)[:, ::-1].reshape(-1)
        hit = stencil_nonfinite(bad[order], plan)
        assert hit.any() and not hit.all()
        assert np.array_equal(~np.isfinite(got), hit), f"{what}: non-finite outputs are not exactly the cells that hold one"
    ok = ~hit
    ratio = np.abs(got.astype(np.float64) - ref)[ok] / error_bound(plan, mag)[ok]
    worst = float(ratio.max())
    print(f"regrid {what} {plan.in_grid}->{plan.out_grid}: worst |error| / bound = {worst:.3f}")
    assert worst <= 1.0, what
    return worst


# (id, grid, planes, affine, levels)
CASES = [
    ("ratio2", (13, 24, 7, 12), 69, False, 0),
    ("ratio2-affine-levels", (13, 24, 7, 12), 65, True, 13),
    ("odd-ratio", (13, 24, 5, 8), 69, True, 0),
    ("non-integer", (19, 30, 7, 9), 69, False, 0),
    ("non-integer-affine-levels", (19, 30, 7, 9), 65, True, 13),
    ("off-16B-planes", (11, 10, 4, 3), 3, True, 3),
    ("ratio10-two-pieces", (41, 40, 5, 4), 3, True, 0),          # 11 taps per axis: stage 1 in two pieces, stage 2 past its 8 weights
    ("real-longitude", (37, 1440, 7, 240), 3, False, 0),
    ("real-latitude", (721, 16, 121, 4), 2, True, 2),
    ("product", (721, 1440, 121, 240), 2, False, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_matches_reference(P, case):
    name, grid, planes, with_affine, levels = case
    plan = plan_of(P, grid)
    x = field(planes, grid[0], grid[1], seed=len(name) * 1000 + planes)
    mul, add = affine(planes, 7) if with_affine else (None, None)
    xd = torch.from_numpy(x).cuda()
    got = abi_regrid(P, xd, plan, mul, add, levels)
    check(plan, got, x, mul, add, levels, name)
    again = abi_regrid(P, xd, plan, mul, add, levels)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "not bit-identical from run to run"


@pytest.mark.parametrize("grid, planes", [((13, 24, 7, 12), 69), ((37, 1440, 7, 240), 3), ((721, 1440, 121, 240), 2)],
                         ids=["small", "full-row", "product"])
def test_misaligned_view_takes_the_scalar_path(P, grid, planes):
    """The same field as a view one float into its buffer: 4-B loads, the same arithmetic in the same order."""
    plan = plan_of(P, grid)
    x = field(planes, grid[0], grid[1], seed=5)
    xd = torch.from_numpy(x).cuda()
    buf = torch.empty(x.size + 1, device="cuda")
    view = buf[1:].view(x.shape)
    view.copy_(xd)
    assert view.data_ptr() % 16 == 4 and xd.data_ptr() % 16 == 0
    got = abi_regrid(P, view, plan)
    check(plan, got, x, what="view+1")
    assert np.array_equal(got.view(np.uint32), abi_regrid(P, xd, plan).view(np.uint32))


def test_nonfinite_values_propagate(P):
    grid = (13, 24, 5, 8)
    plan = plan_of(P, grid)
    x = field(69, 13, 24, seed=11)
    x[3, 6, 10] = np.nan                          # away from the edges
    x[40, 7, 13] = np.inf
    x[40, 4, 5] = -np.inf
    mul, add = affine(69, 8)
    for m, a in ((None, None), (mul, add)):
        got = abi_regrid(P, torch.from_numpy(x).cuda(), plan, m, a)
        check(plan, got, x, m, a, what="nan+inf")
    # with the level reversal the values land in the reversed plane
    got = abi_regrid(P, torch.from_numpy(x[:65]).cuda(), plan, mul[:65], add[:65], 13)
    check(plan, got, x[:65], mul[:65], add[:65], 13, what="nan+inf, levels")
    assert not np.isfinite(got[12 - 3]).all() and np.isfinite(got[3]).all()


def test_identity_plan_returns_the_input(P):
    plan = plan_of(P, (13, 24, 13, 24))
    x = field(69, 13, 24, seed=2)
    x[5, 3, 4] = -0.0
    x[6, 0, 0] = np.inf
    got = abi_regrid(P, torch.from_numpy(x).cuda(), plan)
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def _stats_last(seed):
    r = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).cuda()
    return (t(r.uniform(-200, 900, (1, 4, 1, 1))), t(r.uniform(0.5, 3, (1, 4, 1, 1))),
            t(r.uniform(-200, 900, (1, 5, 13, 1, 1))), t(r.uniform(0.5, 3, (1, 5, 13, 1, 1))))


def _state(B, H, W, seed):
    x = field(B * 69, H, W, seed).reshape(B, 69, H, W)
    up = torch.from_numpy(np.ascontiguousarray(x[:, :65])).cuda().view(B, 5, 13, H, W)
    sf = torch.from_numpy(np.ascontiguousarray(x[:, 65:])).cuda()
    return up, sf


def test_python_surface_equals_the_abi(P):
    grid = (13, 24, 7, 12)
    plan = plan_of(P, grid)
    up, sf = _state(2, 13, 24, seed=21)
    sl = _stats_last(4)
    flat = lambda t: t.reshape(-1, 13, 24)
    eq = lambda t, a: np.array_equal(t.cpu().numpy().reshape(a.shape).view(np.uint32), a.view(np.uint32))
    # regrid: plain, with an affine and the level reversal, into `out`
    assert eq(P.score.regrid(up, plan), abi_regrid(P, flat(up), plan))
    mul, add = P.score.plane_affine(up, sl, up.device)
    want = abi_regrid(P, flat(up), plan, mul, add, 13)
    got = P.score.regrid(up, plan, mul, add, flip_levels=True)
    assert got.shape == (2, 5, 13, 7, 12) and eq(got, want)
    out = torch.full((2, 5, 13, 7, 12), POISON, device="cuda")
    assert P.score.regrid(up, plan, mul, add, flip_levels=True, out=out) is out and eq(out, want)
    # regrid_fields: plain (a plan or a pair) and de-normalising
    for pl in (plan, (7, 12)):
        gu, gs = P.score.regrid_fields(up, sf, pl)
        assert gs.shape == (2, 4, 7, 12) and eq(gu, abi_regrid(P, flat(up), plan)) and eq(gs, abi_regrid(P, flat(sf), plan))
    gu, gs = P.score.regrid_fields(up, sf, plan, sl)
    smul, sadd = P.score.plane_affine(sf, sl, sf.device)
    assert eq(gu, abi_regrid(P, flat(up), plan, mul, add)) and eq(gs, abi_regrid(P, flat(sf), plan, smul, sadd))
    # ... and against the reference with the affine: mul = std, add = mean per (sample, variable, level) plane
    s_mean, s_std, u_mean, u_std = (t.cpu().numpy() for t in sl)
    rep = lambda a, t: np.broadcast_to(a, t.shape[:-2] + (1, 1)).reshape(-1)
    check(plan, gu.cpu().numpy().reshape(-1, 7, 12), flat(up).cpu().numpy(), rep(u_std, up), rep(u_mean, up), what="fields upper")
    check(plan, gs.cpu().numpy().reshape(-1, 7, 12), flat(sf).cpu().numpy(), rep(s_std, sf), rep(s_mean, sf), what="fields surface")
    # mismatches raise
    with pytest.raises(ValueError, match="plan regrids"):
        P.score.regrid(up[..., :12, :].contiguous(), plan)
    with pytest.raises(ValueError, match="float32"):
        P.score.regrid(up.double(), plan)
    with pytest.raises(ValueError, match="contiguous"):
        P.score.regrid(up.transpose(1, 2), plan)
    with pytest.raises(ValueError, match="mul"):
        P.score.regrid(up, plan, mul[:5], add[:5])
    with pytest.raises(ValueError, match="out must be"):
        P.score.regrid(up, plan, out=torch.empty((2, 5, 13, 7, 13), device="cuda"))
    with pytest.raises(ValueError, match="plan regrids"):
        P.score.regrid_fields(up, sf, plan_of(P, (19, 30, 7, 9)))


@pytest.mark.parametrize("mode", ["float32", "int16"])
def test_host_drain_regrids(P, mode):
    """One 5-D and one 4-D tensor, normalised, with stats_last and flip_levels: the float32 item is score.regrid of the same tensors
    bit for bit; the int16 item is, array for array, what a plain drain delivers when it is fed the regridded tensors."""
    plan = plan_of(P, (13, 24, 7, 12))
    up, sf = _state(1, 13, 24, seed=31)
    up, sf = (up - 280.0) / 20.0, (sf - 280.0) / 20.0                  # "normalised" model outputs
    sl = _stats_last(9)
    want = [P.score.regrid(up, plan, *P.score.plane_affine(up, sl, up.device), flip_levels=True),
            P.score.regrid(sf, plan, *P.score.plane_affine(sf, sl, sf.device))]
    for regrid in (plan, (7, 12)):
        drain = P.data.HostDrain("cuda", mode=mode, depth=1, stats_last=sl, flip_levels=True, regrid=regrid)
        drain.submit([up, sf], tag="a")
        drain.submit([up, sf], tag="b")
        plain = P.data.HostDrain("cuda", mode=mode, depth=1)
        plain.submit(want, tag="w")
        ref = plain.get()
        for tag in ("a", "b"):
            item = drain.get()
            assert item.tag == tag and len(item.fields) == 2
            for f, r, w in zip(item.fields, ref.fields, want):
                if mode == "float32":
                    assert f.packed is None and f.values.shape == tuple(w.shape)
                    assert np.array_equal(f.values.view(np.uint32), w.cpu().numpy().view(np.uint32))
                else:
                    assert f.values is None and f.packed.shape == tuple(w.shape) and f.packed.dtype == np.int16
                    assert np.array_equal(f.packed, r.packed) and np.array_equal(f.scale_offset, r.scale_offset)
                    assert np.array_equal(f.nonfinite, r.nonfinite)
                assert f.to_float32().shape == tuple(w.shape)
        assert drain.get() is None
        with pytest.raises(ValueError):                                # another grid than the first submit's
            drain.submit([up[..., :12, :].contiguous(), sf[..., :12, :].contiguous()])
        drain.close()
        plain.close()
    bad = P.data.HostDrain("cuda", mode=mode, depth=1, regrid=plan)
    with pytest.raises(ValueError, match="plan regrids"):              # the plan's input grid is not the tensors'
        bad.submit([up[..., :12, :].contiguous(), sf[..., :12, :].contiguous()])
    bad.close()


def test_ensemble_scores_on_the_coarse_grid(P):
    """EnsembleRollout.scores(regrid=) on a state set by hand (no model step) equals ensemble_scores of the separately regridded
    members and target."""
    E = 4
    plan = plan_of(P, (13, 24, 7, 12))
    up, sf = _state(E, 13, 24, seed=41)
    tu, ts = _state(1, 13, 24, seed=42)
    sl = _stats_last(10)
    ens = object.__new__(P.ensemble.EnsembleRollout)
    ens.upper, ens.surface, ens.stats_last = up, sf, sl
    want = P.score.ensemble_scores(*P.score.regrid_fields(up, sf, plan), *P.score.regrid_fields(tu, ts, plan), sl)
    fine = ens.scores(tu, ts)
    for regrid, target in ((plan, (tu, ts)), ((7, 12), (tu[0], ts[0]))):
        got = ens.scores(*target, regrid=regrid)
        for g, w, f in zip(got, want, fine):
            assert set(g) == set(P.score.ENSEMBLE_KEYS)
            for k in g:
                assert g[k].shape == w[k].shape
                assert bool(((g[k] - w[k]).abs() <= SCORE_RTOL * w[k].abs()).all()), k
            assert not torch.equal(g["crps"], f["crps"])               # (and it is not the fine-grid score)
