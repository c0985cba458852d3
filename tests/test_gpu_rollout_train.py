"""Multi-step (rollout) fine-tuning on the GPU: the fused feed-back seed kernel bit for bit, train.rollout_train_step against
train_step (K = 1), against the torch-op composition model + rollout.norm_back + train.weighted_l1_loss (K = 2, bf16 / fp32 / LoRA),
its checkpointed mode against the one-graph mode (K = 3, DropPath active, memory), and under dist.FlatGradSync."""
import pytest
import torch

import cases
import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _u(name, shape, scale=1.0, shift=0.0):
    return synth.uniform(shape, synth.name_seed("rt_" + name), scale, shift, device=DEV)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("shape", [(1, 13, 721, 1440), (2, 3, 37, 24), (1, 2, 5, 7)])
def test_seed_kernel_bit_for_bit(shape, rev, with_stats):
    """pangu_rollout_l1_seed_bwd: without d_next == pangu_weighted_l1_loss_bwd; with d_next == that + d_next * std formed by two
    torch ops (the product rounded before the add), out of place and over the d_next buffers themselves.  A multi-chunk plane with a
    tail, a sub-chunk plane with B = 2, an unaligned plane (scalar path)."""
    from pangu_pytorch_amd import _lib, train
    lib = _lib.load()
    B, L, H, W = shape
    o, os_ = _u("o", (B, 5, L, H, W)), _u("os", (B, 4, H, W))
    sl = (_u("sm", (1, 4, 1, 1), 300.0, 1e5), _u("ss", (1, 4, 1, 1), 100.0, 700.0), _u("um", (1, 5, L, 1, 1), 20.0, 250.0),
          _u("us", (1, 5, L, 1, 1), 5.0, 30.0))
    if with_stats:
        t, ts = _u("tp", (B, 5, L, H, W), 40.0, 250.0), _u("tsp", (B, 4, H, W), 500.0, 1e5)
        st = [x.reshape(-1).contiguous() for x in (sl[2], sl[3], sl[0], sl[1])]
        sp = [x.data_ptr() for x in st]
    else:
        t, ts = _u("tn", (B, 5, L, H, W)), _u("tsn", (B, 4, H, W))
        sp = [None] * 4
        t[0, 1, 0, 0, :3] = o[0, 1, 0, 0, :3]               # exact zeros of out - target: sign(0) = 0
    if rev:
        t = t.flip(-3).contiguous()
    f_std_u, f_std_s = sl[3].reshape(-1).contiguous(), sl[1].reshape(-1).contiguous()
    wu, ws = train._weights_on(o.device, torch.float32)
    g = torch.tensor(0.37, device=DEV)
    geom = (B, 5, L * H * W, 4, H * W, L, int(rev))
    stream = torch.cuda.current_stream().cuda_stream
    head = (stream, o.data_ptr(), t.data_ptr(), os_.data_ptr(), ts.data_ptr(), wu.data_ptr(), ws.data_ptr(), g.data_ptr())

    d0, d0s = torch.full_like(o, float("nan")), torch.full_like(os_, float("nan"))
    assert lib.pangu_weighted_l1_loss_bwd(*head, d0.data_ptr(), d0s.data_ptr(), *geom, *sp) == 0
    # the last step of a chain: no d_next
    d1, d1s = torch.full_like(o, float("nan")), torch.full_like(os_, float("nan"))
    assert lib.pangu_rollout_l1_seed_bwd(*head, None, None, None, None, d1.data_ptr(), d1s.data_ptr(), *geom, *sp) == 0
    assert torch.equal(d1, d0) and torch.equal(d1s, d0s)
    assert torch.isfinite(d0).all() and d0.abs().max() > 0
    # a middle step: d_next of the loss gradient's own magnitude, so neither term swamps the other
    scale = float(d0.abs().max()) / 30.0
    dn, dns = _u("dn", o.shape, scale), _u("dns", os_.shape, scale)
    want, want_s = d0 + dn * sl[3], d0s + dns * sl[1]
    assert not torch.equal(want, d0)
    d2, d2s = torch.full_like(o, float("nan")), torch.full_like(os_, float("nan"))
    tail = (f_std_u.data_ptr(), f_std_s.data_ptr())
    assert lib.pangu_rollout_l1_seed_bwd(*head, dn.data_ptr(), dns.data_ptr(), *tail, d2.data_ptr(), d2s.data_ptr(), *geom, *sp) == 0
    assert torch.equal(d2, want) and torch.equal(d2s, want_s)
    # in place
    assert lib.pangu_rollout_l1_seed_bwd(*head, dn.data_ptr(), dns.data_ptr(), *tail, dn.data_ptr(), dns.data_ptr(), *geom, *sp) == 0
    assert torch.equal(dn, want) and torch.equal(dns, want_s)


# ---- the model-level tests share one reference-initialised model ------------------------------------------------------------------

def _stats_last(stats):
    """The model's normalisation statistics ((13,1,1,5) level-major, levels as the embedding reads them) as the (1,5,13,1,1) /
    (1,4,1,1) tensors of normData / normBackData (the mapping tests/test_gpu_rollout.py uses)."""
    s_mean, s_std, u_mean, u_std = stats
    return (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1),
            u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
            u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())


class _Setup:
    pass


@pytest.fixture(scope="module")
def S():
    import pangu_pytorch_amd as P
    from pangu_pytorch_amd import rollout
    P._lib.load()
    s = _Setup()
    s.P = P
    torch.manual_seed(0)
    s.m = P.PanguModel(device=DEV).to(DEV)                      # the reference's initialisation
    s.state0 = {k: v.clone() for k, v in s.m.state_dict().items()}
    s.inp, s.inp_s, s.stats, s.maps, s.const_h = cases.model_inputs(DEV)
    s.sl = _stats_last(s.stats)
    # targets in physical units whose normalised values are O(1): normBackData of uniform(-1, 1) fields
    s.targets = []
    for k in range(3):
        s.targets += list(rollout.norm_back(_u(f"t{k}", s.inp.shape), _u(f"ts{k}", s.inp_s.shape), s.sl))
    yield s
    del s.m


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


def _fused(S, m, K, seed, **kw):
    from pangu_pytorch_amd import train
    opt = train.make_optimizer(m)
    torch.manual_seed(seed)
    batch = (S.inp, S.inp_s) + tuple(S.targets[:2 * K])
    total, per = train.rollout_train_step(m, opt, batch, S.stats, S.maps, S.const_h, S.sl, **kw)
    return total, per, _snapshot(m)


def _composition(S, m, K, seed, lam):
    """The same K-step step out of what the parent commit has: model, rollout.norm_back, train.weighted_l1_loss, one backward,
    train_step's optimizer tail."""
    from pangu_pytorch_amd import ops, rollout, train
    opt = train.make_optimizer(m)
    torch.manual_seed(seed)
    opt.zero_grad(set_to_none=True)
    cur, cur_s, losses = S.inp, S.inp_s, []
    for k in range(K):
        out, out_s = m(cur, cur_s, S.stats, S.maps, S.const_h)
        losses.append(train.weighted_l1_loss(out, out_s, S.targets[2 * k], S.targets[2 * k + 1], stats_last=S.sl))
        if k + 1 < K:
            cur, cur_s = rollout.norm_back(out, out_s, S.sl)
    total = losses[0] * lam[0]
    for l, w in zip(losses[1:], lam[1:]):
        total = total + l * w
    with ops.dropped_branch_grads("none"):
        total.backward()
    if isinstance(opt, train.HipAdam):
        opt.step(missing_as_zero=True)
    else:
        opt.step()
    return total.detach(), torch.stack([l.detach() for l in losses]), _snapshot(m)


# ---- 2. K = 1 is train_step -------------------------------------------------------------------------------------------------------

def test_k1_is_train_step(S):
    from pangu_pytorch_amd import train
    m = _reset(S, torch.bfloat16)
    opt = train.make_optimizer(m)
    torch.manual_seed(5)
    l_ref = train.train_step(m, opt, (S.inp, S.inp_s, S.targets[0], S.targets[1]), S.stats, S.maps, S.const_h, stats_last=S.sl)
    p_ref, g_ref = _snapshot(m)
    m = _reset(S, torch.bfloat16)
    total, per, (p_new, g_new) = _fused(S, m, 1, 5)
    assert per.shape == (1,) and total.shape == ()
    assert torch.equal(total, l_ref) and torch.equal(per[0], l_ref)
    worst = _worst_grad(g_new, g_ref)
    print(f"K=1 vs train_step: worst gradient rel-L2 {worst:.3e}, worst parameter abs {_worst_param(p_new, p_ref):.3e}")
    assert worst < 1e-4, worst
    assert _worst_param(p_new, p_ref) <= 2.5e-5


# ---- 3. K = 2 against the torch-op composition ----------------------------------------------------------------------------------

def _k2_vs_composition(S, dtype, lora=False):
    lam = (0.4, 0.6)
    m = _reset(S, dtype)
    if lora:
        m.enable_lora()
        g = torch.Generator(device=DEV).manual_seed(3)
        with torch.no_grad():
            for mod in m.modules():
                if type(mod).__name__ == "LoraLinear":         # fresh adapters have B = 0, which zeroes d lora_A: give B values
                    mod.lora_B.copy_((torch.rand(mod.lora_B.shape, generator=g, device=DEV) * 2 - 1) * 0.02)
        m.invalidate_shadows()
        lora_state = {k: v.clone() for k, v in m.state_dict().items()}
        reset = lambda: (m.load_state_dict(lora_state), [setattr(p, "grad", None) for p in m.parameters()])
    else:
        reset = lambda: _reset(S, dtype)
    t_c, per_c, (p_c, g_c) = _composition(S, m, 2, 5, lam)
    reset()
    t_c2, per_c2, (_, g_c2) = _composition(S, m, 2, 5, lam)
    spread = _worst_grad(g_c2, g_c)
    del g_c2
    reset()
    t_f, per_f, (p_f, g_f) = _fused(S, m, 2, 5, lead_weights=lam)
    worst = _worst_grad(g_f, g_c)
    print(f"K=2 {dtype} lora={lora}: fused vs composition worst gradient rel-L2 {worst:.3e}; composition run twice {spread:.3e}; "
          f"worst parameter abs {_worst_param(p_f, p_c):.3e}; losses {per_f.tolist()}")
    assert torch.equal(per_f, per_c) and torch.equal(per_c2, per_c)
    assert torch.equal(t_f, t_c)
    if lora:
        names = [n for n, _ in m.named_parameters()]
        with_grad = {n for n, g in zip(names, g_f) if g is not None}
        assert with_grad and all("lora_" in n or n.startswith(("_output_layer.conv.", "_output_layer.conv_surface.")) for n in with_grad)
        assert any("lora_A" in n for n in with_grad) and any(n.startswith("_output_layer.conv.") for n in with_grad)
    assert worst < 1e-4, (worst, spread)


def test_k2_vs_composition_bf16(S):
    _k2_vs_composition(S, torch.bfloat16)


def _enough_memory_for_fp32():
    free, _ = torch.cuda.mem_get_info()
    if free < 160e9:
        print(f"fp32 K=2 needs about 135 GB; {free / 1e9:.0f} GB free")
        return False
    return True


def test_k2_vs_composition_fp32(S):
    torch.cuda.empty_cache()
    if not _enough_memory_for_fp32():
        pytest.skip("less than 160 GB of device memory free")
    try:
        _k2_vs_composition(S, torch.float32)
    finally:
        torch.cuda.empty_cache()


# ---- 4. checkpoint=True against checkpoint=False --------------------------------------------------------------------------------

def test_checkpointed_equals_one_graph_and_saves_memory(S):
    from pangu_pytorch_amd import train
    from pangu_pytorch_amd.layers import DropPath
    lam = (0.2, 0.3, 0.5)
    torch.cuda.empty_cache()
    m = _reset(S, torch.bfloat16)
    opt = train.make_optimizer(m)
    torch.manual_seed(5)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    train.train_step(m, opt, (S.inp, S.inp_s, S.targets[0], S.targets[1]), S.stats, S.maps, S.const_h, stats_last=S.sl)
    torch.cuda.synchronize()
    peak_one = torch.cuda.max_memory_allocated()
    del opt

    def run(checkpoint):
        m = _reset(S, torch.bfloat16)
        count = lambda: sum(d.n_dropped for d in m.modules() if isinstance(d, DropPath))
        at_call = []                                   # the counters in front of every forward of the model
        hook = m.register_forward_pre_hook(lambda mod, args: at_call.append(count()))
        try:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            total, per, (p, g) = _fused(S, m, 3, 5, lead_weights=lam, checkpoint=checkpoint)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
        finally:
            hook.remove()
        at_call.append(count())
        dropped = [b - a for a, b in zip(at_call, at_call[1:])]          # branches dropped per forward, in call order
        return total, per, p, g, torch.get_rng_state(), peak, dropped

    t_c, per_c, p_c, g_c, rng_c, peak_c, dropped_c = run(True)
    t_f, per_f, p_f, g_f, rng_f, peak_f, dropped_f = run(False)
    worst = _worst_grad(g_c, g_f)
    print(f"K=3 bf16: checkpointed vs one graph worst gradient rel-L2 {worst:.3e}; peak memory train_step {peak_one / 1e9:.1f} GB, "
          f"checkpointed {peak_c / 1e9:.1f} GB ({peak_c / peak_one:.2f}x), one graph {peak_f / 1e9:.1f} GB ({peak_f / peak_one:.2f}x); "
          f"branches dropped per forward {dropped_f} / by the checkpointed call's forwards {dropped_c}")
    # DropPath is active, and the checkpointed call's forwards are steps 0, 1 (pass 1), then 2, 1, 0 with gradients, each under the
    # draws of the one-graph call: its counters count every step but the last twice
    assert len(dropped_f) == 3 and sum(dropped_f) > 0
    assert dropped_c == [dropped_f[0], dropped_f[1], dropped_f[2], dropped_f[1], dropped_f[0]]
    assert torch.equal(per_c, per_f) and torch.equal(t_c, t_f)
    assert worst < 1e-4, worst
    assert torch.equal(rng_c, rng_f)
    assert peak_c <= 1.5 * peak_one, (peak_c, peak_one)


# ---- 5. dist.FlatGradSync --------------------------------------------------------------------------------------------------------

def test_flat_grad_sync(S):
    from pangu_pytorch_amd import dist
    lam = (0.4, 0.6)
    m = _reset(S, torch.bfloat16)
    _, per_ref, (p_ref, _) = _fused(S, m, 2, 5, lead_weights=lam)
    m = _reset(S, torch.bfloat16)
    sync = dist.FlatGradSync(m)
    try:
        _, per, (p_new, _) = _fused(S, m, 2, 5, lead_weights=lam, grad_sync=sync.finish)
        assert torch.equal(per, per_ref)
        worst = _worst_param(p_new, p_ref)
        print(f"K=2 bf16 under FlatGradSync: worst parameter abs difference {worst:.3e}")
        assert worst <= 2.5e-5
        m = _reset(S, torch.bfloat16)
        with pytest.raises(RuntimeError, match="FlatGradSync"):
            _fused(S, m, 2, 5, lead_weights=lam, grad_sync=sync.finish, checkpoint=True)
    finally:
        sync.remove()
        for p in m.parameters():
            p.grad = None


# ---- 3b. K = 2 with LoRA adapters (fp32; last: it rebuilds the module tree) -----------------------------------------------------

def test_k2_vs_composition_fp32_lora(S):
    torch.cuda.empty_cache()
    if not _enough_memory_for_fp32():
        pytest.skip("less than 160 GB of device memory free")
    try:
        _k2_vs_composition(S, torch.float32, lora=True)
    finally:
        S.m.merge_lora()
        for p in S.m.parameters():
            p.requires_grad_(True)
            p.grad = None
        S.m.load_state_dict(S.state0)
        torch.cuda.empty_cache()
