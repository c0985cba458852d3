"""HipAdam's fused global-norm clipping, accumulation scale and non-finite-step guard on the GPU (csrc/adam.hip: grad_sumsq_kernel,
clip_state_kernel, adam_multi_kernel<true>) against float64 torch, torch's own fp32 clip arithmetic and torch.optim.Adam(fused=True),
and train.accumulated_train_step / a clipped rollout_train_step on a small model."""
import pytest
import torch

import cases
import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
# free-standing fp32 tensors: below / at / above one 4096-element block, n % 4 != 0 (scalar path), a 2-D tensor, many blocks with a
# ragged tail; the LAST one is left without a gradient and stepped under missing_as_zero=True
SHAPES = [(1,), (3,), (4095,), (4096,), (4097,), (8196,), (37, 129), (1000005,), (777,)]
NO_GRAD = len(SHAPES) - 1
SPLIT = 4                                  # two parameter groups: tensors [0, 4) and [4, 9) with their own lr / weight_decay
KW = dict(lr=3e-3, weight_decay=3e-2, betas=(0.9, 0.98), eps=1e-8)
GROUP2 = dict(lr=1e-2, weight_decay=1e-3)


def _params(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pa = [torch.nn.Parameter(torch.randn(s, generator=g, device=DEV)) for s in SHAPES]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    return pa, pb


def _groups(ps):
    return [{"params": ps[:SPLIT]}, {"params": ps[SPLIT:], **GROUP2}]


def _grads(seed, step):
    """One gradient per tensor (None for the tensor that goes without), of magnitudes that differ from tensor to tensor."""
    g = torch.Generator(device=DEV).manual_seed(1000 * seed + step)
    return [None if i == NO_GRAD else torch.randn(s, generator=g, device=DEV) * (10.0 ** (i % 3 - 1)) for i, s in enumerate(SHAPES)]


def _norm64(grads, grad_scale=1.0):
    return grad_scale * torch.sqrt(sum((g.double() ** 2).sum() for g in grads if g is not None))


def _pair_step(oa, ob, pa, pb, grads, missing_as_zero=True, grad_scale=1.0):
    """HipAdam steps on `grads` (left as they are); the twin's fused Adam steps on copies multiplied in place by the multiplier
    HipAdam reports (a zero gradient for a tensor without one, under missing_as_zero)."""
    for a, b, g in zip(pa, pb, grads):
        a.grad = None if g is None else g.clone()
        b.grad = (torch.zeros_like(b) if missing_as_zero else None) if g is None else g.clone()
    oa.step(missing_as_zero=missing_as_zero, grad_scale=grad_scale)
    for a, g in zip(pa, grads):
        assert (a.grad is None) if g is None else torch.equal(a.grad, g)        # step() does not write the gradients
    mult = oa.last_grad_multiplier
    for b in pb:
        if b.grad is not None:
            b.grad.mul_(mult)
    ob.step()


def _assert_same(oa, ob, pa, pb, what):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a.detach(), b.detach()), (what, i, float((a - b).abs().max()))
        if oa.state.get(a) and ob.state.get(b):
            assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]), (what, i)
            assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]), (what, i)


def _train():
    import pangu_pytorch_amd as P
    from pangu_pytorch_amd import train
    P._lib.load()
    return train


# ---- 1. the norm ------------------------------------------------------------------------------------------------------------------

def test_norm_against_float64_and_run_to_run():
    """last_grad_norm = fl32(sqrt(sum of squares)) with the sum accumulated in double: one rounding to fp32 away from the float64
    result, i.e. relative error <= 2^-24 < 2^-23; a second step over the same (untouched) gradients gives the same bits, partial by
    partial."""
    train = _train()
    pa, _ = _params(1)
    grads = _grads(1, 0)
    for a, g in zip(pa, grads):
        a.grad = g
    opt = train.HipAdam(_groups(pa), max_grad_norm=1.0, **KW)
    opt.step(missing_as_zero=True)
    n1, part1 = opt.last_grad_norm.clone(), opt._partials[1].clone()
    want = _norm64(grads)
    rel = abs(n1.double() - want) / want
    print(f"norm {float(n1):.9g} against float64 {float(want):.17g}: relative error {float(rel):.3e}")
    assert n1.dtype == torch.float32 and rel <= 2.0 ** -23
    assert part1.numel() == sum((p.numel() + 4095) // 4096 for p in pa)          # one partial per table block, both groups
    opt.step(missing_as_zero=True)
    assert torch.equal(opt.last_grad_norm, n1) and torch.equal(opt._partials[1], part1)
    for a, g, g0 in zip(pa, grads, _grads(1, 0)):                                # the gradients were only read
        assert a.grad is g and (g is None or torch.equal(g, g0))


# ---- 2. the multiplier ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm,grad_scale", [(1.0, 1.0), (1e30, 1.0), (1.0, 0.25), (None, 0.25), (1e30, 0.25)])
def test_multiplier_is_torchs_fp32_arithmetic(max_norm, grad_scale):
    """clip_grad_norm_'s arithmetic in fp32 on the reported fp32 norm -- min(1, max_norm / (norm + 1e-6)) -- times grad_scale,
    with IEEE fp32 ops (torch on the host), reproduces last_grad_multiplier bit for bit: clipping active (the norm is ~ 1e3),
    inactive (huge max_norm), and with an accumulation scale."""
    train = _train()
    pa, _ = _params(2)
    grads = _grads(2, 0)
    for a, g in zip(pa, grads):
        a.grad = g
    opt = train.HipAdam(_groups(pa), max_grad_norm=max_norm, **KW)
    opt.step(missing_as_zero=True, grad_scale=grad_scale)
    norm, mult = opt.last_grad_norm.cpu(), opt.last_grad_multiplier.cpu()
    want64 = _norm64(grads, grad_scale)
    assert abs(norm.double() - want64.cpu()) / want64.cpu() <= 2.0 ** -23          # the norm of the SCALED gradient
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    want = f32(grad_scale)
    if max_norm is not None:
        coef = torch.clamp(f32(max_norm) / (norm + f32(1e-6)), max=1.0)
        assert (float(coef) < 1.0) == (max_norm == 1.0)
        want = want * coef
    print(f"max_norm {max_norm} grad_scale {grad_scale}: norm {float(norm):.9g} multiplier {float(mult):.9g} want {float(want):.9g}")
    assert mult.dtype == torch.float32 and torch.equal(mult, want)
    assert int(opt.skipped_steps) == 0


# ---- 3. the update ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("uneven", [False, True])
@pytest.mark.parametrize("max_norm,grad_scale", [(1.0, 1.0), (50.0, 0.25)])
def test_update_is_fused_adam_on_scaled_gradients(max_norm, grad_scale, uneven):
    """Five steps against torch.optim.Adam(fused=True) on twins whose gradients were multiplied in place by the reported multiplier:
    parameters and both moments bit for bit, two groups, a tensor without a gradient stepped as zeros; `uneven`: two tensors join
    two steps late, so the step counts differ and the bias corrections are per table row."""
    train = _train()
    pa, pb = _params(3)
    oa = train.HipAdam(_groups(pa), max_grad_norm=max_norm, **KW)
    ob = torch.optim.Adam(_groups(pb), fused=True, **KW)
    if uneven:
        for step in range(2):
            grads = _grads(3, 100 + step)
            grads[2] = grads[6] = None
            _pair_step(oa, ob, pa, pb, grads, missing_as_zero=False, grad_scale=grad_scale)
            _assert_same(oa, ob, pa, pb, ("early", step))
    for step in range(5):
        _pair_step(oa, ob, pa, pb, _grads(3, step), grad_scale=grad_scale)
        _assert_same(oa, ob, pa, pb, step)
        assert float(oa.last_grad_multiplier) < grad_scale                       # clipping was active
    assert oa.state[pa[0]]["step"] == (7 if uneven else 5) and oa.state[pa[2]]["step"] == 5
    assert oa.state[pa[NO_GRAD]]["step"] == 5 and not torch.equal(pa[NO_GRAD].detach(), _params(3)[0][NO_GRAD].detach())


# ---- 4. the torch idiom -----------------------------------------------------------------------------------------------------------

def test_matches_clip_grad_norm_then_fused_adam():
    """What a user writes today -- clip_grad_norm_ (which rewrites the gradients) + fused Adam -- lands on the same parameters to
    rel-L2 1e-6 after five steps (torch's own fp32 norm differs from ours in its last bits, hence not to the bit)."""
    train = _train()
    pa, pb = _params(4)
    oa = train.HipAdam(_groups(pa), max_grad_norm=1.0, **KW)
    ob = torch.optim.Adam(_groups(pb), fused=True, **KW)
    for step in range(5):
        grads = _grads(4, step)
        for a, b, g in zip(pa, pb, grads):
            a.grad = None if g is None else g.clone()
            b.grad = torch.zeros_like(b) if g is None else g.clone()
        oa.step(missing_as_zero=True)
        total = torch.nn.utils.clip_grad_norm_(pb, 1.0)
        ob.step()
        assert abs(float(total) - float(oa.last_grad_norm)) <= 1e-5 * float(total)
    for i, (a, b) in enumerate(zip(pa, pb)):
        rel = float((a.detach().double() - b.detach().double()).norm() / b.detach().double().norm())
        print(f"tensor {i} {tuple(a.shape)}: rel-L2 against clip_grad_norm_ + fused Adam {rel:.3e}")
        assert rel <= 1e-6, (i, rel)


# ---- 5. the non-finite guard ------------------------------------------------------------------------------------------------------

def test_nonfinite_step_is_skipped_and_reconciled():
    train = _train()
    pa, pb = _params(5)
    oa = train.HipAdam(_groups(pa), skip_nonfinite=True, **KW)
    ob = torch.optim.Adam(_groups(pb), fused=True, **KW)
    _pair_step(oa, ob, pa, pb, _grads(5, 0))
    _assert_same(oa, ob, pa, pb, "before")
    assert float(oa.last_grad_multiplier) == 1.0 and int(oa.skipped_steps) == 0
    before = [(a.detach().clone(), oa.state[a]["exp_avg"].clone(), oa.state[a]["exp_avg_sq"].clone()) for a in pa]
    bad = _grads(5, 1)
    bad[7][123457] = float("inf")                                                # one Inf, deep inside the many-block tensor
    for a, g in zip(pa, bad):
        a.grad = g
    oa.step(missing_as_zero=True)
    assert int(oa.skipped_steps) == 1 and not bool(torch.isfinite(oa.last_grad_norm))
    for a, (p0, m0, v0) in zip(pa, before):
        assert torch.equal(a.detach(), p0) and torch.equal(oa.state[a]["exp_avg"], m0) and torch.equal(oa.state[a]["exp_avg_sq"], v0)
    assert oa.state[pa[0]]["step"] == 2                                          # the host counter ran ahead ...
    assert oa.reconcile_skips() == 1 and oa.state[pa[0]]["step"] == 1            # ... and is taken back
    assert oa.reconcile_skips() == 0 and oa.state[pa[0]]["step"] == 1
    for step in range(2, 5):                                                     # the twin never saw the bad step
        _pair_step(oa, ob, pa, pb, _grads(5, step))
        _assert_same(oa, ob, pa, pb, step)
    assert int(oa.skipped_steps) == 1 and oa.state[pa[0]]["step"] == 4
    # a NaN is caught as well
    bad = _grads(5, 9)
    bad[0][0] = float("nan")
    for a, g in zip(pa, bad):
        a.grad = g
    oa.step(missing_as_zero=True)
    assert int(oa.skipped_steps) == 2 and oa.reconcile_skips() == 1
    _assert_same(oa, ob, pa, pb, "after the NaN step")


def test_nonfinite_step_without_the_guard_propagates_as_in_torch():
    """skip_nonfinite=False, clipping on, one Inf: the norm is Inf, the coefficient 0, Inf * 0 = NaN reaches that parameter, exactly
    where clip_grad_norm_ + fused Adam puts it."""
    train = _train()
    pa, pb = _params(6)
    oa = train.HipAdam(_groups(pa), max_grad_norm=1.0, **KW)
    ob = torch.optim.Adam(_groups(pb), fused=True, **KW)
    grads = _grads(6, 0)
    grads[7][123457] = float("inf")
    for a, b, g in zip(pa, pb, grads):
        a.grad = None if g is None else g.clone()
        b.grad = torch.zeros_like(b) if g is None else g.clone()
    oa.step(missing_as_zero=True)
    torch.nn.utils.clip_grad_norm_(pb, 1.0)
    ob.step()
    assert int(oa.skipped_steps) == 0 and float(oa.last_grad_multiplier) == 0.0
    assert not bool(torch.isfinite(pa[7]).all())
    for a, b in zip(pa, pb):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b))


# ---- 6. a skipped step and the bf16 image -------------------------------------------------------------------------------------------

class _Images:
    """Stands for a model's fused_bf16.WeightShadow: the plain bf16 image of each parameter that has one."""

    def __init__(self, params):
        self.img = {id(p): torch.full(p.shape, 7.0, dtype=torch.bfloat16, device=DEV) for p in params}       # stale
        self.fresh = []

    def plain_image(self, p):
        return self.img.get(id(p))

    def mark_fresh(self, p):
        self.fresh.append(id(p))


class _Model:
    pass


def test_skipped_step_still_writes_the_bf16_image():
    """HipAdam marks imaged parameters fresh on the host without knowing whether the kernel skipped: after a skipped step the image
    is the bf16 cast of the UNCHANGED parameter even though it was stale before (vector path, scalar path n % 4 != 0, many blocks)."""
    train = _train()
    g = torch.Generator(device=DEV).manual_seed(6)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g, device=DEV)) for n in (8200, 4097, 5, 20000)]
    model = _Model()
    model._shadow = _Images(ps[:3])                                              # the last tensor has no image
    opt = train.HipAdam(ps, lr=1e-2, skip_nonfinite=True, shadow_of=model)
    p0 = [p.detach().clone() for p in ps]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g, device=DEV)
    ps[3].grad[777] = float("inf")
    opt.step()
    assert int(opt.skipped_steps) == 1
    assert sorted(model._shadow.fresh) == sorted(id(p) for p in ps[:3])
    for p, q in zip(ps, p0):
        assert torch.equal(p.detach(), q)
    for p in ps[:3]:
        assert torch.equal(model._shadow.img[id(p)], p.detach().to(torch.bfloat16))
    # and a step that is taken writes the image of the UPDATED parameter, as the unscaled kernel does
    ps[3].grad[777] = 0.5
    opt.reconcile_skips()
    opt.step()
    assert int(opt.skipped_steps) == 1
    for p, q in zip(ps, p0):
        assert not torch.equal(p.detach(), q)
    for p in ps[:3]:
        assert torch.equal(model._shadow.img[id(p)], p.detach().to(torch.bfloat16))


# ---- 7. defaults: today's launches ---------------------------------------------------------------------------------------------------

ENTRIES = ("pangu_adam_step_multi", "pangu_adam_step_multi_scaled", "pangu_grad_sumsq_multi", "pangu_grad_clip_state")


@pytest.fixture
def calls(monkeypatch):
    from pangu_pytorch_amd import _lib
    lib, n = _lib.load(), {k: 0 for k in ENTRIES}

    def counted(name, fn):
        def call(*a):
            n[name] += 1
            return fn(*a)
        return call
    for name in ENTRIES:
        monkeypatch.setattr(lib, name, counted(name, getattr(lib, name)))
    return n


def test_defaults_issue_only_the_one_launch_per_group(calls):
    train = _train()
    pa, pb = _params(7)
    oa, ob = train.HipAdam(_groups(pa), **KW), train.HipAdam(_groups(pb), **KW)
    for step in range(3):
        for a, b, g in zip(pa, pb, _grads(7, step)):
            a.grad, b.grad = g, (None if g is None else g.clone())
        oa.step(missing_as_zero=True)
        ob.step(missing_as_zero=True, grad_scale=1.0)
    _assert_same(oa, ob, pa, pb, "defaults")
    assert calls == {"pangu_adam_step_multi": 2 * 2 * 3, "pangu_adam_step_multi_scaled": 0, "pangu_grad_sumsq_multi": 0,
                     "pangu_grad_clip_state": 0}
    assert oa.last_grad_norm is None and oa.skipped_steps is None
    # any of the three options takes the other path: one sum per group, one record, one scaled step per group
    oc = train.HipAdam(_groups(pa), **KW)
    oc.step(missing_as_zero=True, grad_scale=0.5)
    assert calls == {"pangu_adam_step_multi": 12, "pangu_adam_step_multi_scaled": 2, "pangu_grad_sumsq_multi": 2,
                     "pangu_grad_clip_state": 1}
    assert float(oc.last_grad_multiplier) == 0.5


# ---- 8. in the training steps ------------------------------------------------------------------------------------------------------

class _Setup:
    pass


@pytest.fixture(scope="module")
def S():
    """A reference-initialised model of one block per layer (falling back to the full model should the GPU path refuse it), bf16,
    training mode with DropPath off; full-resolution synthetic fields."""
    import pangu_pytorch_amd as P
    from pangu_pytorch_amd import rollout
    P._lib.load()
    s = _Setup()
    s.inp, s.inp_s, s.stats, s.maps, s.const_h = cases.model_inputs(DEV)
    s_mean, s_std, u_mean, u_std = s.stats
    s.sl = (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1),
            u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
            u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())
    u = lambda name, shape: synth.uniform(shape, synth.name_seed("oc_" + name), device=DEV)
    s.targets = []
    for k in range(2):                     # physical-unit targets whose normalised values are O(1)
        s.targets += list(rollout.norm_back(u(f"t{k}", s.inp.shape), u(f"ts{k}", s.inp_s.shape), s.sl))
    torch.manual_seed(0)

    def build(depths):
        m = P.PanguModel(depths=depths, device=DEV).to(DEV)
        m.set_compute_dtype(torch.bfloat16)
        m.train()
        for mod in m.modules():
            if isinstance(mod, P.layers.DropPath):
                mod.drop_prob = 0.0
        with torch.no_grad():
            m(s.inp, s.inp_s, s.stats, s.maps, s.const_h)
        return m
    depths = [1, 1, 1, 1]
    try:
        m = build(depths)
    except RuntimeError as e:
        print(f"depths {depths} refused by the GPU path ({e}): the full model instead")
        depths = [2, 6, 6, 2]
        m = build(depths)
    print(f"integration model: depths {depths}, {sum(p.numel() for p in m.parameters()) / 1e6:.1f} M parameters")
    s.m = m
    s.state0 = {k: v.clone() for k, v in m.state_dict().items()}
    s.batch = (s.inp, s.inp_s, s.targets[0], s.targets[1])
    yield s
    del s.m


def _reset(S):
    S.m.load_state_dict(S.state0)
    for p in S.m.parameters():
        p.grad = None
    return S.m


def _snapshot(m):
    assert all(p.grad is not None for p in m.parameters())                       # DropPath is off: every branch ran
    return [p.detach().clone() for p in m.parameters()], [p.grad.detach().clone() for p in m.parameters()]


def _worst(got, ref, scale=1.0):
    return max(float(((a.double() * scale - b.double()).norm() / b.double().norm().clamp_min(1e-30))) for a, b in zip(got, ref))


@pytest.fixture(scope="module")
def one_step(S):
    """train.train_step on the batch from the initial state: (loss, parameters, gradients) -- computed once, shared."""
    train = _train()
    m = _reset(S)
    loss = train.train_step(m, train.make_optimizer(m), S.batch, S.stats, S.maps, S.const_h, stats_last=S.sl)
    return (loss.clone(),) + _snapshot(m)


LR = 5e-6                                  # make_optimizer's default


def _worst_abs(got, ref):
    return max(float((a - b).abs().max()) for a, b in zip(got, ref))


def test_accumulating_the_same_batch_twice_is_train_step(S, one_step):
    """(g + g) / 2 = g: the mean gradient of the same batch twice is that batch's gradient, up to the run-to-run spread of the
    backward's fp32 atomics (1e-6 rel-L2 per tensor, the bound tests/test_gpu_lora.py uses for re-run gradients); the loss is the
    same number.  The parameters after the step: on Adam's FIRST step every element moves by lr * g / (|g| + eps) < lr whatever
    the size of g, so two runs whose gradients differ in their last bits end within 2 lr of each other element by element (and a
    step taken with the SUM instead of the mean would show in neither bound but in the multiplier, which must be 1/2).
    Measured: gradients 6.5e-7 rel-L2 (two runs of train_step itself: 5.7e-7)."""
    train = _train()
    l_ref, p_ref, g_ref = one_step
    m = _reset(S)
    opt = train.make_optimizer(m)
    loss = train.accumulated_train_step(m, opt, [S.batch, S.batch], S.stats, S.maps, S.const_h, stats_last=S.sl)
    p_new, g_new = _snapshot(m)
    wg, wp = _worst(g_new, g_ref, 0.5), _worst_abs(p_new, p_ref)
    print(f"accumulated x2 against train_step: loss {float(loss):.9g} / {float(l_ref):.9g}, worst gradient rel-L2 {wg:.3e}, "
          f"worst parameter abs {wp:.3e}, multiplier {float(opt.last_grad_multiplier)}")
    assert float(opt.last_grad_multiplier) == 0.5
    assert abs(float(loss) - float(l_ref)) <= 1e-6 * abs(float(l_ref))
    assert wg <= 1e-6
    assert wp <= 2.01 * LR
    assert _worst_abs(p_new, [S.state0[k] for k, _ in m.named_parameters()]) > 0.5 * LR          # the step was taken


def test_accumulating_one_batch_is_train_step_bit_for_bit(S, one_step, calls):
    """n = 1 IS train_step: the same launches (the unscaled Adam entry, once; none of the clipping entries), the same loss to the bit,
    and -- from the same gradients -- the same parameters to the bit as train_step's own optimizer tail.  The gradients of two
    runs of the backward are NOT bit-identical in either function (fp32 atomics in the weight-gradient kernels: two runs of
    train_step itself differ by 5.7e-7 rel-L2), so they are compared at the 1e-6 the re-run gradients of tests/test_gpu_lora.py get,
    and the bit-for-bit comparison of the update starts from one set of gradients."""
    train = _train()
    l_ref, p_ref, g_ref = one_step
    m = _reset(S)
    opt = train.make_optimizer(m)
    loss = train.accumulated_train_step(m, opt, [S.batch], S.stats, S.maps, S.const_h, stats_last=S.sl)
    p_new, g_new = _snapshot(m)
    print(f"accumulated x1 against train_step: worst gradient rel-L2 {_worst(g_new, g_ref):.3e}, worst parameter abs "
          f"{_worst_abs(p_new, p_ref):.3e}")
    assert calls == {"pangu_adam_step_multi": 1, "pangu_adam_step_multi_scaled": 0, "pangu_grad_sumsq_multi": 0,
                     "pangu_grad_clip_state": 0}
    assert opt.last_grad_norm is None
    assert torch.equal(loss, l_ref)
    assert _worst(g_new, g_ref) <= 1e-6 and _worst_abs(p_new, p_ref) <= 2.01 * LR
    # train_step's tail on the very same gradients
    m = _reset(S)
    for p, g in zip(m.parameters(), g_new):
        p.grad = g
    train._optimizer_tail(train.make_optimizer(m), None)
    for i, (p, q) in enumerate(zip(m.parameters(), p_new)):
        assert torch.equal(p.detach(), q), ("parameter", i)


def test_clipped_rollout_train_step(S):
    train = _train()
    batch = (S.inp, S.inp_s) + tuple(S.targets)
    m = _reset(S)
    probe = train.make_optimizer(m, max_grad_norm=1e30)                          # reports the norm, clips nothing
    train.rollout_train_step(m, probe, batch, S.stats, S.maps, S.const_h, S.sl)
    norm = float(probe.last_grad_norm)
    assert norm > 0 and float(probe.last_grad_multiplier) == 1.0
    m = _reset(S)
    opt = train.make_optimizer(m, max_grad_norm=0.5 * norm, skip_nonfinite=True)
    total, per = train.rollout_train_step(m, opt, batch, S.stats, S.maps, S.const_h, S.sl)
    mult = float(opt.last_grad_multiplier)
    print(f"K = 2 rollout step: norm {norm:.6g}, clipped at half of it: multiplier {mult:.6g}, losses {per.tolist()}")
    assert per.shape == (2,) and bool(torch.isfinite(per).all()) and bool(torch.isfinite(total))
    assert 0.0 < mult < 1.0 and int(opt.skipped_steps) == 0
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
