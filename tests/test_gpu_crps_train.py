"""Fair-CRPS ensemble fine-tuning on the GPU: the fused loss kernels (csrc/crps_loss.hip) against the fp64 torch form and against
the identities that tie them to the weighted L1 loss and to score.ensemble_scores; train.ensemble_train_step against the torch-op
composition, its checkpointed mode against the one-graph mode (DropPath active, memory), and against train_step at amplitude 0."""
import ctypes

import pytest
import torch

import cases
import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _u(name, shape, scale=1.0, shift=0.0):
    return synth.uniform(shape, synth.name_seed("crps_" + name), scale, shift, device=DEV)


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ---- 1. the kernels against fp64 ---------------------------------------------------------------------------------------------------

def _fields(E, L, H, W, tag=""):
    """Members x (E,1,5,L,H,W), x_s (E,1,4,H,W) and the NORMALISED target t (1,5,L,H,W), t_s (1,4,H,W), with planted ties:
    member 1 == member 0 on row 1, member 0 == target on row 2, every member == target at one point, and with E > 2 three members
    tied on row 4 (rows exist at every H used here)."""
    x, x_s = _u(f"x{tag}", (E, 1, 5, L, H, W)), _u(f"xs{tag}", (E, 1, 4, H, W))
    t, t_s = _u(f"t{tag}", (1, 5, L, H, W)), _u(f"ts{tag}", (1, 4, H, W))
    return x, x_s, t, t_s


def _plant_ties(x, x_s, t, t_s):
    E = x.shape[0]
    x[1, ..., 1, :] = x[0, ..., 1, :]
    x_s[1, ..., 1, :] = x_s[0, ..., 1, :]
    x[0, ..., 2, :] = t[..., 2, :]
    x_s[0, ..., 2, :] = t_s[..., 2, :]
    x[:, 0, 1, 0, 3, 4] = t[0, 1, 0, 3, 4]
    x_s[:, 0, 2, 3, 4] = t_s[0, 2, 3, 4]
    if E > 2:
        x[2, ..., 4, :] = x[1, ..., 4, :] = x[0, ..., 4, :]
        x_s[2, ..., 4, :] = x_s[1, ..., 4, :] = x_s[0, ..., 4, :]


class _Case:
    """One call set-up of the two entries: everything the C ABI takes, and the fp64 reference."""

    def __init__(self, E, L, H, W, lat_weighted, with_stats, rev, misalign=False):
        from pangu_pytorch_amd import _lib, train
        self.lib, self.E, self.geom = _lib.load(), E, (1, 5, L, 4, H, W)
        x, x_s, t, t_s = _fields(E, L, H, W)
        if with_stats:
            # the target arrives in physical units; its normalised value is formed here with the kernel's two fp32 operations (a
            # subtract, a true division; on the host: IEEE for certain), so that ties and signs are those the kernel sees
            sl = (_u("sm", (1, 4, 1, 1), 300.0, 1e5), _u("ss", (1, 4, 1, 1), 100.0, 700.0), _u("um", (1, 5, L, 1, 1), 20.0, 250.0),
                  _u("us", (1, 5, L, 1, 1), 5.0, 30.0))
            phys, phys_s = t * sl[3] + sl[2], t_s * sl[1] + sl[0]
            t = ((phys.cpu() - sl[2].cpu()) / sl[3].cpu()).to(DEV)
            t_s = ((phys_s.cpu() - sl[0].cpu()) / sl[1].cpu()).to(DEV)
            self.stats = [s.reshape(-1).contiguous() for s in (sl[2], sl[3], sl[0], sl[1])]
            sp = [s.data_ptr() for s in self.stats]
        else:
            phys, phys_s, sp = t, t_s, [None] * 4
        _plant_ties(x, x_s, t, t_s)
        self.tn, self.tn_s = t, t_s                       # normalised, logical level order: what the reference takes
        self.target = phys.flip(-3).contiguous() if rev else phys.contiguous()
        self.target_s = phys_s.contiguous()
        if misalign:                                      # every field 4 bytes off a 16-byte boundary: the scalar path at W % 4 == 0
            off = lambda v: torch.cat([v.new_zeros(1), v.reshape(-1)])[1:].view(v.shape)
            self.keep = [off(x[e]) for e in range(E)]
            self.xs, self.xs_s = self.keep, [x_s[e] for e in range(E)]
        else:
            self.xs, self.xs_s = [x[e] for e in range(E)], [x_s[e] for e in range(E)]
        self.lat = train._crps_lat_weights(H, x.device) if lat_weighted else None
        self.lat_weighted = lat_weighted
        wu, ws = train._weights_on(x.device, torch.float32)
        self.g = torch.tensor(0.37, device=DEV)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.head = (_ptrs(self.xs), _ptrs(self.xs_s), E, self.target.data_ptr(), self.target_s.data_ptr(), wu.data_ptr(), ws.data_ptr(),
                     None if self.lat is None else self.lat.data_ptr())
        self.tail = (*self.geom, int(rev), *sp)

    def forward(self):
        nblk = self.lib.pangu_fair_crps_loss_blocks(self.E, *self.geom)
        assert nblk > 0
        partial = torch.full((nblk,), NAN, device=DEV)
        loss = torch.full((3,), NAN, device=DEV)
        assert self.lib.pangu_fair_crps_loss_fwd(self.stream, *self.head, partial.data_ptr(), loss.data_ptr(), *self.tail) == 0
        return loss

    def backward(self, in_place=False):
        """(d_upper, d_surface) lists; in_place: written over COPIES of the members handed in as the members."""
        if in_place:
            d, d_s = [v.clone() for v in self.xs], [v.clone() for v in self.xs_s]
            if any(v.data_ptr() % 16 for v in self.xs):           # keep the copies as misaligned as the originals
                d = [torch.cat([v.new_zeros(1), v.reshape(-1)])[1:].view(v.shape) for v in self.xs]
            head = (_ptrs(d), _ptrs(d_s)) + self.head[2:]
        else:
            d, d_s = [torch.full_like(v, NAN) for v in self.xs], [torch.full_like(v, NAN) for v in self.xs_s]
            if any(v.data_ptr() % 16 for v in self.xs):
                d = [torch.full((v.numel() + 1,), NAN, device=DEV)[1:].view(v.shape) for v in self.xs]
            head = self.head
        assert self.lib.pangu_fair_crps_loss_bwd(self.stream, *head, self.g.data_ptr(), _ptrs(d), _ptrs(d_s), *self.tail) == 0
        return d, d_s

    def reference(self):
        """fp64: loss, [d_upper], [d_surface] of train._fair_crps_loss_torch on .double() copies, upstream gradient g."""
        from pangu_pytorch_amd import train
        xs = [v.double().requires_grad_(True) for v in self.xs]
        xs_s = [v.double().requires_grad_(True) for v in self.xs_s]
        loss = train._fair_crps_loss_torch(xs, xs_s, self.tn.double(), self.tn_s.double(), lat_weighted=self.lat_weighted)
        grads = torch.autograd.grad(loss * self.g.double(), xs + xs_s)
        return loss.detach(), list(grads[:self.E]), list(grads[self.E:])


def _check_against_fp64(c):
    loss = c.forward()
    d, d_s = c.backward()
    ref, r, r_s = c.reference()
    rel = abs(float(loss[0]) - float(ref)) / abs(float(ref))
    worst = []
    for got, want in ((d, r), (d_s, r_s)):
        got, want = torch.stack(got).double(), torch.stack(want)
        assert torch.isfinite(got).all()
        worst.append(float((got - want).abs().max() / want.abs().max()))
    print(f"E={c.E} geom={c.geom}: loss rel {rel:.2e}, gradient worst abs / max|ref| upper {worst[0]:.2e} surface {worst[1]:.2e}")
    assert torch.isfinite(loss).all() and rel <= 1e-5, rel
    assert float(loss[0]) == pytest.approx(float(loss[1]) + 0.25 * float(loss[2]), rel=1e-6)
    assert max(worst) <= 1e-6, worst
    if c.E == 2:                # member 0 tied with the target on row 2: member 1's two signs cancel there, an exact zero
        assert float(d[1][..., 2, :].abs().max()) == 0.0 and float(d_s[1][..., 2, :].abs().max()) == 0.0
        assert float(d[0][..., 2, :].abs().min()) > 0.0
    # the gradients written over the member fields themselves, and a second identical call: the same bits
    di, di_s = c.backward(in_place=True)
    assert all(torch.equal(a, b) for a, b in zip(di + di_s, d + d_s))
    assert torch.equal(c.forward(), loss)
    d2, d2_s = c.backward()
    assert all(torch.equal(a, b) for a, b in zip(d2 + d2_s, d + d_s))


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("lat_weighted", [True, False])
@pytest.mark.parametrize("E", [2, 3, 5, 8, 16])
@pytest.mark.parametrize("shape", [(2, 5, 8), (3, 37, 24), (2, 5, 7)])
def test_kernels_against_fp64(shape, E, lat_weighted, with_stats, rev):
    """A plane smaller than a block, rows crossing block boundaries (37 x 24 = 888 elements: not a multiple of a batch), an
    unaligned plane (W = 7: the scalar path)."""
    _check_against_fp64(_Case(E, *shape, lat_weighted, with_stats, rev))


@pytest.mark.parametrize("E", [2, 16])
def test_scalar_path_on_misaligned_fields(E):
    """W % 4 == 0 but the upper-air members (and their gradient fields) start 4 bytes off a 16-byte boundary."""
    c = _Case(E, 3, 37, 24, True, True, True, misalign=True)
    assert all(v.data_ptr() % 16 == 4 for v in c.xs)
    _check_against_fp64(c)


def test_more_than_one_chunk_per_plane():
    """E = 16 takes 1024-element chunks: a 37 x 96 plane is 3.5 of them (a ragged last chunk), E = 2 (8192) one."""
    for E in (16, 2):
        _check_against_fp64(_Case(E, 2, 37, 96, True, False, False))


# ---- 2. identities ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("E", [2, 5, 16])
def test_identical_members_are_the_weighted_l1_loss(E):
    from pangu_pytorch_amd import _lib, train
    lib = _lib.load()
    L, H, W = 3, 37, 24
    o, o_s, t, t_s = _u("io", (1, 5, L, H, W)), _u("ios", (1, 4, H, W)), _u("it", (1, 5, L, H, W)), _u("its", (1, 4, H, W))
    t[0, 1, 0, 0, :3] = o[0, 1, 0, 0, :3]
    wu, ws = train._weights_on(o.device, torch.float32)
    g = torch.tensor(0.37, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    l1_geom = (1, 5, L * H * W, 4, H * W, L, 0, None, None, None, None)
    part = torch.empty(lib.pangu_weighted_l1_loss_blocks(*l1_geom[:6]), device=DEV)
    l1 = torch.full((3,), NAN, device=DEV)
    d1, d1_s = torch.full_like(o, NAN), torch.full_like(o_s, NAN)
    head = (stream, o.data_ptr(), t.data_ptr(), o_s.data_ptr(), t_s.data_ptr(), wu.data_ptr(), ws.data_ptr())
    assert lib.pangu_weighted_l1_loss_fwd(*head, part.data_ptr(), l1.data_ptr(), *l1_geom) == 0
    assert lib.pangu_weighted_l1_loss_bwd(*head, g.data_ptr(), d1.data_ptr(), d1_s.data_ptr(), *l1_geom) == 0
    xs, xs_s = [o.clone() for _ in range(E)], [o_s.clone() for _ in range(E)]
    geom = (1, 5, L, 4, H, W)
    part = torch.full((lib.pangu_fair_crps_loss_blocks(E, *geom),), NAN, device=DEV)
    loss = torch.full((3,), NAN, device=DEV)
    d, d_s = [torch.full_like(o, NAN) for _ in range(E)], [torch.full_like(o_s, NAN) for _ in range(E)]
    chead = (stream, _ptrs(xs), _ptrs(xs_s), E, t.data_ptr(), t_s.data_ptr(), wu.data_ptr(), ws.data_ptr(), None)
    tail = (*geom, 0, None, None, None, None)
    assert lib.pangu_fair_crps_loss_fwd(*chead, part.data_ptr(), loss.data_ptr(), *tail) == 0
    assert lib.pangu_fair_crps_loss_bwd(*chead, g.data_ptr(), _ptrs(d), _ptrs(d_s), *tail) == 0
    rel = (loss - l1).abs() / l1.abs()
    worst = max(float((torch.stack(a).sum(0) - b).abs().max() / b.abs().max()) for a, b in ((d, d1), (d_s, d1_s)))
    print(f"E={E}: identical members vs weighted L1: loss rel {rel.tolist()}, summed gradient worst abs / max {worst:.2e}")
    assert float(rel.max()) <= 1e-6
    assert worst <= 1e-6
    assert all(torch.equal(a, d[0]) for a in d)


def _scores_identity(E, H, W):
    from pangu_pytorch_amd import score, train
    x, x_s = _u(f"sx{H}", (E, 5, 13, H, W)), _u(f"sxs{H}", (E, 4, H, W))
    t, t_s = _u(f"st{H}", (1, 5, 13, H, W)), _u(f"sts{H}", (1, 4, H, W))
    sl = (torch.zeros(1, 4, 1, 1, device=DEV), torch.ones(1, 4, 1, 1, device=DEV), torch.zeros(1, 5, 13, 1, 1, device=DEV),
          torch.ones(1, 5, 13, 1, 1, device=DEV))
    su, ss = score.ensemble_scores(x, x_s, t, t_s, sl)
    wu, ws = train._weights_on(x.device, torch.float32)
    want_u = (wu.view(5, 1).double() * su["crps"].double()).mean()
    want_s = (ws.view(4).double() * ss["crps"].double()).mean()
    lat = train._crps_lat_weights(H, x.device)
    loss = train._fair_crps_launch_fwd([x[e:e + 1] for e in range(E)], [x_s[e:e + 1] for e in range(E)], t, t_s, False, (), lat)
    rel_u, rel_s = abs(float(loss[1]) - float(want_u)) / float(want_u), abs(float(loss[2]) - float(want_s)) / float(want_s)
    print(f"E={E} {H}x{W}: loss_upper vs mean(w * crps) rel {rel_u:.2e}, loss_surface rel {rel_s:.2e}")
    assert rel_u <= 1e-5 and rel_s <= 1e-5
    assert float(loss[0]) == pytest.approx(float(loss[1]) + 0.25 * float(loss[2]), rel=1e-6)


def test_loss_is_the_weighted_mean_of_ensemble_scores_crps():
    _scores_identity(3, 9, 8)


def test_loss_is_the_weighted_mean_of_ensemble_scores_crps_full_grid():
    _scores_identity(2, 721, 1440)
    torch.cuda.empty_cache()


def test_autograd_function_on_the_device():
    """train.fair_crps_loss on device tensors goes through FairCrpsLossFn: the loss and gradients of the fp64 torch form, with the
    statistics and the level reversal folded in."""
    from pangu_pytorch_amd import train
    E, L, H, W = 3, 2, 5, 8
    c = _Case(E, L, H, W, True, False, False)
    xs, xs_s = [v.clone().requires_grad_(True) for v in c.xs], [v.clone().requires_grad_(True) for v in c.xs_s]
    loss = train.fair_crps_loss(xs, xs_s, c.tn, c.tn_s)
    assert type(loss.grad_fn).__name__.startswith("FairCrpsLossFn")
    (loss * c.g).backward()
    ref, r, r_s = c.reference()
    assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
    for got, want in ((xs, r), (xs_s, r_s)):
        got, want = torch.stack([v.grad for v in got]).double(), torch.stack(want)
        assert float((got - want).abs().max() / want.abs().max()) <= 1e-6
    with pytest.raises(ValueError, match="members"):
        train.fair_crps_loss(xs[:1], xs_s[:1], c.tn, c.tn_s)


# ---- 3. the training step: one reference-initialised model at the full grid ----------------------------------------------------------

def _stats_last(stats):
    """The model's normalisation statistics ((13,1,1,5) level-major) as the (1,5,13,1,1) / (1,4,1,1) tensors of normData (the
    mapping tests/test_gpu_rollout_train.py uses)."""
    s_mean, s_std, u_mean, u_std = stats
    return (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1),
            u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
            u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())


class _Setup:
    pass


PERTURB = dict(amplitude=0.2, seed=11, octaves=3, period=12, persistence=0.5, control=True)


@pytest.fixture(scope="module")
def S():
    import pangu_pytorch_amd as P
    from pangu_pytorch_amd import rollout
    P._lib.load()
    s = _Setup()
    torch.manual_seed(0)
    s.m = P.PanguModel(device=DEV).to(DEV)                      # the reference's initialisation
    s.state0 = {k: v.clone() for k, v in s.m.state_dict().items()}
    s.inp, s.inp_s, s.stats, s.maps, s.const_h = cases.model_inputs(DEV)
    s.sl = _stats_last(s.stats)
    # a target in physical units whose normalised values are O(1): normBackData of uniform(-1, 1) fields
    s.tgt, s.tgt_s = rollout.norm_back(_u("mt", s.inp.shape), _u("mts", s.inp_s.shape), s.sl)
    s.batch = (s.inp, s.inp_s, s.tgt, s.tgt_s)
    yield s
    del s.m
    torch.cuda.empty_cache()


def _reset(S, dtype, train_mode=True):
    m = S.m
    m.load_state_dict(S.state0)
    m.set_compute_dtype(dtype)
    m.train(train_mode)
    for p in m.parameters():
        p.grad = None
    return m


def _snapshot(m):
    return ([p.detach().clone() for p in m.parameters()],
            [None if p.grad is None else p.grad.detach().clone() for p in m.parameters()])


def _worst_grad(got, ref):
    assert [a is None for a in got] == [b is None for b in ref]                  # the same parameters are without a gradient
    return max(((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item() for a, b in zip(got, ref) if b is not None)


def _worst_param(got, ref):
    return max(float((a - b).abs().max()) for a, b in zip(got, ref))


def _fused(S, m, E, seed, **kw):
    from pangu_pytorch_amd import train
    opt = train.make_optimizer(m)
    torch.manual_seed(seed)
    args = dict(PERTURB, **kw)
    loss = train.ensemble_train_step(m, opt, S.batch, S.stats, S.maps, S.const_h, S.sl, members=E, **args)
    return loss, _snapshot(m)


def _composition(S, m, E, seed):
    """The same step out of torch ops around the model: perturb_, E forwards with gradients, the torch form of the loss, one
    backward, train_step's optimizer tail."""
    from pangu_pytorch_amd import ensemble, ops, train
    opt = train.make_optimizer(m)
    torch.manual_seed(seed)
    opt.zero_grad(set_to_none=True)
    up, sf = S.inp.repeat(E, 1, 1, 1, 1), S.inp_s.repeat(E, 1, 1, 1)
    kw = dict(PERTURB)
    ensemble.perturb_(up, sf, S.sl, kw.pop("amplitude"), kw.pop("seed"), **kw)
    outs = [m(up[e:e + 1], sf[e:e + 1], S.stats, S.maps, S.const_h) for e in range(E)]
    loss = train._fair_crps_loss_torch([o for o, _ in outs], [o_s for _, o_s in outs], S.tgt, S.tgt_s, False, S.sl, True)
    del outs
    with ops.dropped_branch_grads("none"):
        loss.backward()
    if isinstance(opt, train.HipAdam):
        opt.step(missing_as_zero=True)
    else:
        opt.step()
    return loss.detach(), _snapshot(m)


def test_one_graph_step_vs_torch_composition_bf16(S):
    from pangu_pytorch_amd.layers import DropPath
    m = _reset(S, torch.bfloat16)
    dropped = lambda: sum(d.n_dropped for d in m.modules() if isinstance(d, DropPath))
    n0 = dropped()
    l_c, (p_c, g_c) = _composition(S, m, 2, 5)
    assert dropped() > n0                                  # stochastic depth is active
    m = _reset(S, torch.bfloat16)
    l_f, (p_f, g_f) = _fused(S, m, 2, 5, checkpoint=False)
    worst, rel = _worst_grad(g_f, g_c), abs(float(l_f) - float(l_c)) / abs(float(l_c))
    print(f"E=2 bf16 one graph vs torch composition: loss {float(l_f):.6f} rel {rel:.2e}, worst gradient rel-L2 {worst:.3e}, "
          f"worst parameter abs {_worst_param(p_f, p_c):.3e}")
    assert rel <= 1e-5                                     # (the fp32 torch mean is itself good to about 1e-6)
    assert worst < 1e-4, worst
    assert _worst_param(p_f, p_c) <= 2.5e-5


def test_checkpointed_equals_one_graph_and_saves_memory(S):
    from pangu_pytorch_amd import train
    torch.cuda.empty_cache()
    m = _reset(S, torch.bfloat16)
    opt = train.make_optimizer(m)
    torch.manual_seed(5)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    train.train_step(m, opt, S.batch, S.stats, S.maps, S.const_h, stats_last=S.sl)
    torch.cuda.synchronize()
    peak_one = torch.cuda.max_memory_allocated()
    del opt

    def run(checkpoint):
        m = _reset(S, torch.bfloat16)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        loss, (p, g) = _fused(S, m, 3, 5, checkpoint=checkpoint)
        torch.cuda.synchronize()
        return loss, p, g, torch.get_rng_state(), torch.cuda.max_memory_allocated()

    l_c, p_c, g_c, rng_c, peak_c = run(True)
    l_f, p_f, g_f, rng_f, peak_f = run(False)
    worst = _worst_grad(g_c, g_f)                          # (asserts that the same parameters are without a gradient)
    print(f"E=3 bf16: checkpointed vs one graph worst gradient rel-L2 {worst:.3e}, worst parameter abs {_worst_param(p_c, p_f):.3e}, "
          f"losses {float(l_c):.6f} / {float(l_f):.6f}; peak memory train_step {peak_one / 1e9:.1f} GB, checkpointed "
          f"{peak_c / 1e9:.1f} GB ({peak_c / peak_one:.2f}x), one graph {peak_f / 1e9:.1f} GB ({peak_f / peak_one:.2f}x)")
    assert torch.equal(l_c, l_f)                           # the same forward kernels on the same inputs, the same loss launches
    assert worst < 1e-4, worst
    assert _worst_param(p_c, p_f) <= 2.5e-5
    assert torch.equal(rng_c, rng_f)
    assert peak_c <= 1.5 * peak_one, (peak_c, peak_one)


def test_amplitude_zero_is_train_step_fp32(S):
    from pangu_pytorch_amd import train
    from pangu_pytorch_amd.layers import DropPath
    torch.cuda.empty_cache()
    drops = [(d, d.drop_prob) for d in S.m.modules() if isinstance(d, DropPath)]
    try:
        for d, _ in drops:
            d.drop_prob = 0.0                              # stochastic depth off
        m = _reset(S, torch.float32)
        opt = train.make_optimizer(m)
        l_ref = train.train_step(m, opt, S.batch, S.stats, S.maps, S.const_h, stats_last=S.sl)
        p_ref, _ = _snapshot(m)
        del opt
        m = _reset(S, torch.float32)
        l_new, (p_new, _) = _fused(S, m, 2, 5, amplitude=0.0, lat_weighted=False)
        rel = abs(float(l_new) - float(l_ref)) / abs(float(l_ref))
        print(f"E=2 fp32 amplitude 0: loss {float(l_new):.7f} vs train_step {float(l_ref):.7f} (rel {rel:.2e}), worst parameter abs "
              f"{_worst_param(p_new, p_ref):.3e}")
        assert rel <= 1e-6
        assert _worst_param(p_new, p_ref) <= 2.5e-5
    finally:
        for d, p in drops:
            d.drop_prob = p
        torch.cuda.empty_cache()
