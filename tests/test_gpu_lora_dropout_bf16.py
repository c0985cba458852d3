"""LoRA adapter dropout on the bf16 training path of the MI355X: the keep mask of the bf16 kernels against its host restatement
(exactly), the three kernels against float64 torch on the numbers they multiply (the bf16 values of x, y, dy with bf16(A), bf16(B)),
the bf16 layer Functions against the fp32 Functions under the same torch.manual_seed (tests/test_gpu_lora_dropout.py pins those to
the oracle), and the whole model in bf16 (seeded steps, eval() unchanged, checkpointed rollout, the launch log, peak memory).

The bounds count bf16 roundings (unit roundoff U = 2^-8); they are not measurements."""
import copy

import pytest
import torch
import torch.nn.functional as F

import cases
import synth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U = 2.0 ** -8
KERNEL_TOL = U                     # tests/test_gpu_lora_bf16.py
BLOCK_TOL = 2e-2                   # the project's bf16-vs-fp32 block bound (tests/test_gpu_bf16.py)
P_DROP = 0.1

KN = [(192, 576), (192, 192), (192, 768), (768, 192), (384, 1152), (384, 384), (384, 1536), (1536, 384), (768, 384), (384, 768)]
RAGGED_KN = [(192, 576), (1536, 384), (768, 192)]
NEW_KERNELS = ("lora_dropout_fwd", "lora_wgrad_dropout", "lora_dropout_dx")
LIN_NAMES = ["linear.linear1", "linear.linear2", "attention.linear1", "attention.linear2"]


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available()
    P._lib.load()
    return P


def relnorm(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _keep(P, seed, M, K, p):
    return P.layers.lora_dropout_keep(seed, M, K, p, device="cuda")


def _operands(M, K, N, r, seed, strided):
    """bf16 x (M, K), y / dy (M, N) as tests/test_gpu_lora_bf16.py::_operands makes them; fp32 A, B at 0.1 randn."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if strided:            # row-strided views, as the block hands over halves of wider buffers
        x = torch.randn(M, K + 64, device="cuda", generator=g).to(BF)[:, 32:32 + K]
        y = torch.randn(M, N + 32, device="cuda", generator=g).to(BF)[:, :N]
    else:
        x = torch.randn(M, K, device="cuda", generator=g).to(BF)
        y = torch.randn(M, N, device="cuda", generator=g).to(BF)
    A = torch.randn(r, K, device="cuda", generator=g) * 0.1
    B = torch.randn(N, r, device="cuda", generator=g) * 0.1
    return x, y, A, B


def _like(t, fill=None, value=0.0):
    """A bf16 tensor of t's shape AND strides (row-strided operands stay row-strided): `value` everywhere, or a copy of `fill`."""
    base = torch.full((t.shape[0], t.stride(0)), value, dtype=BF, device=t.device)
    v = base[:, :t.shape[1]]
    if fill is not None:
        v.copy_(fill)
    return v


# ---- the mask, exactly

@pytest.mark.parametrize("K,groups", [(192, range(12)), (1536, (0, 47, 95))])
def test_kernel_mask_equals_the_restatement(P, K, groups):
    """x = 1, y = 0, s = 1, A = unit vectors onto 16 columns at a time, B = the first 16 columns of the identity: y[:, :16] IS c."""
    ob = P.ops_bf16
    M, N, r = 37, 64, 16
    B = torch.zeros(N, r, device="cuda")
    B[:r] = torch.eye(r, device="cuda")
    x = torch.ones(M, K + 64, dtype=BF, device="cuda")[:, 32:32 + K]
    masks = {}
    for p, seed in ((0.1, 7), (0.1, 8), (0.5, 7)):
        got = torch.zeros(M, K, dtype=torch.bool, device="cuda")
        seen = torch.zeros(K, dtype=torch.bool)
        c_keep = float(torch.tensor(p / (1 - p)).to(BF))
        for g in groups:
            A = torch.zeros(r, K, device="cuda")
            A[torch.arange(r), 16 * g + torch.arange(r)] = 1.0
            y = torch.zeros(M, N + 32, dtype=BF, device="cuda")[:, :N]
            ob.lora_dropout_fwd(x, y, A, B, 1.0, p, seed)
            c = y[:, :16].float()
            assert torch.equal(y[:, 16:], torch.zeros_like(y[:, 16:]))
            kept = c > 0
            assert torch.allclose(c[kept], torch.full_like(c[kept], c_keep), rtol=2.0 ** -7, atol=0)
            assert torch.equal(c[~kept], torch.full_like(c[~kept], -1.0))
            got[:, 16 * g:16 * g + 16] = kept
            seen[16 * g:16 * g + 16] = True
        want = _keep(P, seed, M, K, p)
        assert torch.equal(got[:, seen.cuda()], want[:, seen.cuda()]), (K, p, seed)
        masks[(p, seed)] = got[:, seen.cuda()]
    assert not torch.equal(masks[(0.1, 7)], masks[(0.1, 8)])          # two seeds, two masks


# ---- the forward kernel

def _check_fwd(P, M, K, N, r, p, seed, strided, worst):
    ob = P.ops_bf16
    s = 16.0 / r
    x, y0, A, B = _operands(M, K, N, r, seed=K * 7 + N + r + M, strided=strided)
    x_in = x.clone()
    c = torch.where(_keep(P, seed, M, K, p), p / (1 - p), -1.0).double()
    delta = s * ((c * x.double()) @ A.to(BF).double().t()) @ B.to(BF).double().t()
    del c
    tag = (M, K, N, r, strided)
    # from y = 0: the correction itself -- three roundings (the masked operand, u, the output)
    y = _like(y0)
    ob.lora_dropout_fwd(x, y, A, B, s, p, seed)
    e = relnorm(y, delta)
    worst["delta"] = max(worst.get("delta", (0, None)), (e, tag))
    assert e <= 3 * U, ("delta", tag, e)
    # on a random y: the sum, with h = gelu(y_out) into a NaN-filled buffer
    y = _like(y0, y0)
    h = _like(y0, value=float("nan"))
    ob.lora_dropout_fwd(x, y, A, B, s, p, seed, act=ob.ACT_GELU, h=h)
    ref = y0.double() + delta
    err, bound = (y.double() - ref).norm().item(), U * ref.norm().item() + 2 * U * delta.norm().item()
    worst["sum"] = max(worst.get("sum", (0, None)), (err / bound, tag))
    assert err <= bound, ("sum", tag, err, bound)
    assert bool(torch.isfinite(h.float()).all()), ("h fully written", tag)
    e = relnorm(h, F.gelu(y.double()))
    worst["gelu"] = max(worst.get("gelu", (0, None)), (e, tag))
    assert e <= U, ("gelu", tag, e)
    for _ in range(2):          # without the GELU output, and once more: the same bits
        y2 = _like(y0, y0)
        ob.lora_dropout_fwd(x, y2, A, B, s, p, seed)
        assert torch.equal(y2, y), ("bit-identical, and the same y with and without the GELU output", tag)
    assert torch.equal(x, x_in)
    if strided:
        assert x.stride(0) != K and y.stride(0) != N and h.stride(0) != N


def _report(what, worst):
    print(what + ": " + "; ".join(f"{k} {v[0]:.3e} at {v[1]}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("K,N", KN)
def test_fwd_all_projection_shapes(P, K, N):
    worst = {}
    for r in (4, 8, 16, 32):
        _check_fwd(P, 4099, K, N, r, P_DROP, seed=1000 + r, strided=False, worst=worst)
    _report(f"lora_dropout_fwd_bf16 ({K} -> {N}) worst relnorm (delta <= {3 * U:.3e}, gelu <= {U:.3e}; sum as a fraction of its bound)", worst)


@pytest.mark.parametrize("K,N", RAGGED_KN)
def test_fwd_ragged_and_strided(P, K, N):
    worst = {}
    for r in (4, 8, 16, 32):
        for M in (1, 37, 100003):
            _check_fwd(P, M, K, N, r, P_DROP, seed=M + r, strided=True, worst=worst)
    _report(f"lora_dropout_fwd_bf16 ragged ({K} -> {N})", worst)


# ---- the backward kernels

def _check_bwd(P, M, K, N, r, p, seed, strided, worst):
    ob = P.ops_bf16
    s = 16.0 / r
    x, dy, A, B = _operands(M, K, N, r, seed=K * 5 + N + r + M, strided=strided)
    x_in, dy_in = x.clone(), dy.clone()
    Ab, Bb = A.to(BF).double(), B.to(BF).double()
    keep = _keep(P, seed, M, K, p)
    xd = torch.where(keep, x.double() / (1 - p), 0.0)
    c = torch.where(keep, p / (1 - p), -1.0).double()
    del keep
    Vr = s * dy.double() @ Bb
    tag = (M, K, N, r, strided)

    def note(name, e):
        worst[name] = max(worst.get(name, (0, None)), (e, tag))

    dA, dB, V = ob.lora_wgrad_dropout(dy, x, A, B, s, p, seed)
    for name, got, ref, tol in (("dA", dA, Vr.t() @ xd, KERNEL_TOL), ("dB", dB, s * dy.double().t() @ (xd @ Ab.t()), KERNEL_TOL),
                                ("V", V, Vr, 1e-5)):
        e = relnorm(got, ref)
        note(name, e)
        assert e <= tol, (name, tag, e)
    del xd
    # a second call through the C entry into sentinel-filled outputs: bit-identical, nothing left unwritten
    dA2, dB2, V2 = (torch.full_like(t, float("nan")) for t in (dA, dB, V))
    ws = P.ops.wgrad_workspace(dy.device)
    rc = P._lib.load().pangu_lora_wgrad_dropout_bf16(torch.cuda.current_stream().cuda_stream, dy.data_ptr(), dy.stride(0), x.data_ptr(),
                                                     x.stride(0), A.data_ptr(), B.data_ptr(), dA2.data_ptr(), dB2.data_ptr(),
                                                     V2.data_ptr(), M, N, K, r, s, p, seed, ws.data_ptr(), ws.numel() * 4)
    assert rc == 0
    assert torch.equal(dA, dA2) and torch.equal(dB, dB2) and torch.equal(V, V2), tag
    assert torch.equal(x, x_in) and torch.equal(dy, dy_in), tag
    V_in = V.clone()
    # the input-gradient correction, from the kernel's own V: two roundings (V, the output)
    corr = c * (V.double() @ Ab)
    dx = _like(x, value=float("nan"))
    dx.zero_()
    ob.lora_dropout_dx(dx, V, A, p, seed)
    e = relnorm(dx, corr)
    note("dx from 0", e)
    assert e <= 2 * U, ("dx from 0", tag, e)
    g = torch.Generator(device="cuda").manual_seed(M + K)
    dx0 = torch.randn(M, K, device="cuda", generator=g).to(BF)
    dx = _like(x, dx0)
    ob.lora_dropout_dx(dx, V, A, p, seed)
    ref = dx0.double() + corr
    err, bound = (dx.double() - ref).norm().item(), U * ref.norm().item() + U * corr.norm().item()
    note("dx on random / bound", err / bound)
    assert err <= bound, ("dx on random", tag, err, bound)
    dx2 = _like(x, dx0)
    ob.lora_dropout_dx(dx2, V, A, p, seed)
    assert torch.equal(dx, dx2), tag
    # behind a GELU (the MLP's second projection): the correction carries gelu'(pre)
    pre = torch.randn(M, K, device="cuda", generator=g).to(BF)
    pre_in = pre.clone()
    pd = pre.double().requires_grad_(True)
    F.gelu(pd).sum().backward()
    dx = _like(x)
    ob.lora_dropout_dx(dx, V, A, p, seed, pre=pre)
    e = relnorm(dx, corr * pd.grad)
    note("dx behind the GELU", e)
    assert e <= 2 * U + 1e-5, ("dx behind the GELU", tag, e)
    assert torch.equal(V, V_in) and torch.equal(pre, pre_in), tag


@pytest.mark.parametrize("K,N", KN)
def test_bwd_all_projection_shapes(P, K, N):
    worst = {}
    for r in (4, 8, 16, 32):
        _check_bwd(P, 4099, K, N, r, P_DROP, seed=2000 + r, strided=False, worst=worst)
    _report(f"bf16 dropout backward ({K} -> {N}) worst relnorm (dA, dB <= {KERNEL_TOL:.3e}, V <= 1e-5, dx <= {2 * U:.3e})", worst)


@pytest.mark.parametrize("K,N", RAGGED_KN)
def test_bwd_ragged_and_strided(P, K, N):
    worst = {}
    for r in (4, 8, 16, 32):
        for M in (1, 37, 100003):
            _check_bwd(P, M, K, N, r, P_DROP, seed=M + r, strided=True, worst=worst)
    _report(f"bf16 dropout backward ragged ({K} -> {N})", worst)


# ---- the bf16 layer Functions against the fp32 Functions, same module, same torch.manual_seed

def _adapt(P, root, names, seed, p=P_DROP):
    """Replace the named nn.Linear children by LoraLinear(r=16, alpha=32, lora_dropout=p) with random adapters; freeze the rest."""
    mods = dict(root.named_modules())
    for n in names:
        parent, _, leaf = n.rpartition(".")
        setattr(mods[parent], leaf, P.layers.LoraLinear.from_linear(mods[n], 16, 32, p))
    for q in root.parameters():
        q.requires_grad_(False)
    g = torch.Generator(device="cpu").manual_seed(seed)
    mods = dict(root.named_modules())
    with torch.no_grad():
        for n in names:
            mods[n].lora_A.copy_(torch.randn(mods[n].lora_A.shape, generator=g).cuda() * 0.05)
            mods[n].lora_B.copy_(torch.randn(mods[n].lora_B.shape, generator=g).cuda() * 0.05)
            mods[n].lora_A.requires_grad_(True)
            mods[n].lora_B.requires_grad_(True)
    return mods


def _grads(root):
    return {k: (None if q.grad is None else q.grad.clone()) for k, q in root.named_parameters()}


def _seeds(mods, names):
    return [mods[n].last_dropout_seed for n in names]


def _compare(f32, bf, names, what):
    """(y, dx, parameter gradients, seeds) of the two runs: the same seeds, every tensor within the block bound, frozen tensors None."""
    assert f32[3] == bf[3] and all(s is not None for s in bf[3]), (what, "the same masks")
    worst = max((relnorm(bf[0].float(), f32[0]), "y"), (relnorm(bf[1].float(), f32[1]), "dx"))
    for k, g in f32[2].items():
        if k.endswith("lora_A") or k.endswith("lora_B"):
            worst = max(worst, (relnorm(bf[2][k], g), k))
        else:
            assert g is None and bf[2][k] is None, (what, k)
    assert worst[0] < BLOCK_TOL, (what, worst)
    return worst


def _dropout_block(P, C, roll):
    st = cases.STAGES[C]
    pre = cases.block_prefix(C, roll)
    blk = P.layers.EarthSpecificBlock(C, 0.0, st["heads"], device="cuda").cuda()
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    mods = _adapt(P, blk, LIN_NAMES, C + int(roll))
    blk.train()
    return blk, mods


@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("roll", [False, True])
def test_block_bf16_vs_fp32_same_masks(P, C, roll):
    from pangu_pytorch_amd import fused, fused_bf16
    st = cases.STAGES[C]
    W = 24
    blk, mods = _dropout_block(P, C, roll)
    x32 = cases.block_input(C, W, "cuda")
    cot = cases.cotangent(f"lora_block_{C}_{int(roll)}", x32.shape, "cuda")
    torch.manual_seed(21)
    xf = x32[0].clone().requires_grad_(True)
    y = fused.sample_block(blk, xf, st["Z"], st["H"], W, roll)
    (y * cot[0]).sum().backward()
    f32 = (y.detach(), xf.grad, _grads(blk), _seeds(mods, LIN_NAMES))
    blk.zero_grad(set_to_none=True)
    torch.manual_seed(21)
    xb = x32[0].to(BF).requires_grad_(True)
    P.ops.timing_start()
    y = fused.sample_block(blk, xb, st["Z"], st["H"], W, roll, sh=fused_bf16.WeightShadow())
    (y.float() * cot[0]).sum().backward()
    log = P.ops.timing_stop("mlp_fused_bf16", also=NEW_KERNELS)
    assert y.dtype == BF and log[2] == 0 and all(log[3][k][2] == 4 for k in NEW_KERNELS), log
    worst = _compare(f32, (y.detach(), xb.grad, _grads(blk), _seeds(mods, LIN_NAMES)), LIN_NAMES, (C, roll))
    print(f"bf16 dropout block C={C} roll={roll}: worst rel-L2 to the fp32 Function {worst[0]:.3e} ({worst[1]}, bound {BLOCK_TOL})")


def _block_fn_apply(P, blk, x, geom, s1, s2, sh):
    from pangu_pytorch_amd import autograd as AB
    L = P.layers
    att = blk.attention
    return AB.EarthBlockFn.apply(x, blk.norm1.weight, blk.norm1.bias, blk.norm2.weight, blk.norm2.bias,
                                 L.eff_weight(blk.linear.linear1), blk.linear.linear1.bias, L.eff_weight(blk.linear.linear2),
                                 blk.linear.linear2.bias, att.earth_specific_bias, L.eff_weight(att.linear1), att.linear1.bias,
                                 L.eff_weight(att.linear2), att.linear2.bias, geom, s1, s2, None, sh,
                                 *L.lora_args(blk.linear.linear1, blk.linear.linear2, att.linear1, att.linear2))


@pytest.mark.parametrize("s1,s2", [(0.0, 1.0), (1.0, 0.0)])
def test_block_bf16_dropped_branch(P, s1, s2):
    """A DropPath-dropped branch: the live branch's adapters are within the block bound of the fp32 Function's under the same
    masks; the dropped branch's adapters get what the fp32 Function hands them under the policy in force (zeros or None)."""
    from pangu_pytorch_amd import fused_bf16
    C, roll, W = 192, True, 24
    st = cases.STAGES[C]
    geom = (st["Z"], st["H"], W, st["heads"], roll)
    blk, mods = _dropout_block(P, C, roll)
    x32 = cases.block_input(C, W, "cuda")[0]
    cot = cases.cotangent(f"lora_block_{C}_{int(roll)}", x32.shape, "cuda")
    dropped, live = (LIN_NAMES[2:], LIN_NAMES[:2]) if s1 == 0.0 else (LIN_NAMES[:2], LIN_NAMES[2:])
    runs = {}
    for name, x, sh in (("f32", x32.clone(), None), ("bf16", x32.to(BF), fused_bf16.WeightShadow())):
        blk.zero_grad(set_to_none=True)
        x.requires_grad_(True)
        torch.manual_seed(22)
        y = _block_fn_apply(P, blk, x, geom, s1, s2, sh)
        (y.float() * cot).sum().backward()
        runs[name] = (y.detach().float(), x.grad.float(), _grads(blk), _seeds(mods, LIN_NAMES))
    f32, bf = runs["f32"], runs["bf16"]
    assert f32[3] == bf[3]
    worst = max((relnorm(bf[0], f32[0]), "y"), (relnorm(bf[1], f32[1]), "dx"))
    for n in live:
        for s in (".lora_A", ".lora_B"):
            worst = max(worst, (relnorm(bf[2][n + s], f32[2][n + s]), n + s))
    assert worst[0] < BLOCK_TOL, worst
    for n in dropped:
        for s in (".lora_A", ".lora_B"):
            want, got = f32[2][n + s], bf[2][n + s]
            if want is None:
                assert got is None, n + s
            else:
                assert float(want.abs().max()) == 0.0 and got is not None and torch.equal(got, want), n + s
    print(f"bf16 dropout block s1={s1} s2={s2}: worst rel-L2 of the live branch to the fp32 Function {worst[0]:.3e} ({worst[1]})")


def test_resample_bf16_vs_fp32_same_masks(P):
    """DownSampleFn / UpSampleFn at the geometry of tests/test_gpu_lora_bf16.py::test_resample_bf16_adapter_gradients_vs_merged_layers."""
    from pangu_pytorch_amd import fused, fused_bf16
    Z, H, W, C = 8, 181, 24, 192
    H2, W2 = 91, 12
    for kind in ("down", "up"):
        torch.manual_seed(3)
        layer = (P.layers.DownSample(C) if kind == "down" else P.layers.UpSample(2 * C, C)).cuda()
        names = ["linear"] if kind == "down" else ["linear1", "linear2"]
        with torch.no_grad():
            layer.norm.weight.uniform_(0.9, 1.1)
            layer.norm.bias.uniform_(-0.1, 0.1)
        mods = _adapt(P, layer, names, 4)
        layer.train()
        x0 = synth.uniform((Z * H * W, C) if kind == "down" else (Z * H2 * W2, 2 * C), 71 if kind == "down" else 72).cuda()
        n_out = (Z * H2 * W2, 2 * C) if kind == "down" else (Z * H * 2 * W2, C)
        cot = synth.uniform(n_out, 73).cuda()
        runs = []
        for x, sh in ((x0.clone(), None), (x0.to(BF), fused_bf16.WeightShadow())):
            layer.zero_grad(set_to_none=True)
            x.requires_grad_(True)
            torch.manual_seed(23)
            y = fused.sample_down(layer, x, Z, H, W, sh=sh) if kind == "down" else fused.sample_up(layer, x, Z, H2, W2, H, sh=sh)
            assert tuple(y.shape) == n_out and y.dtype == x.dtype
            (y.float() * cot).sum().backward()
            runs.append((y.detach().float(), x.grad.float(), _grads(layer), _seeds(mods, names)))
        worst = _compare(runs[0], runs[1], names, kind)
        print(f"bf16 dropout {kind}-sampling: worst rel-L2 to the fp32 Function {worst[0]:.3e} ({worst[1]}, bound {BLOCK_TOL})")


# ---- the whole model, bf16

def _randomise_adapters(model, seed, std=0.02):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(".lora_B") or n.endswith(".lora_A"):
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device))


def _stats_last(stats):
    s_mean, s_std, u_mean, u_std = stats
    return (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1),
            u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
            u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())


class _Setup:
    pass


@pytest.fixture(scope="module")
def S(P):
    s = _Setup()
    base = P.PanguModel(device="cuda").cuda().eval()
    base.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    s.plain = copy.deepcopy(base)
    s.plain.enable_lora(r=16, alpha=16, bf16_training=True)
    s.attn = copy.deepcopy(base)
    s.attn.enable_lora(r=16, alpha=16, lora_dropout=P_DROP, bf16_training=True, bf16_dropout=True,
                       target_modules=("attention.linear1", "attention.linear2"))
    s.m = base
    s.m.enable_lora(r=16, alpha=16, lora_dropout=P_DROP, bf16_training=True, bf16_dropout=True)
    for model in (s.m, s.plain, s.attn):
        _randomise_adapters(model, 5)
        model.set_compute_dtype(BF)
        for mod in model.modules():                                  # DropPath off
            if isinstance(mod, P.layers.DropPath):
                mod.drop_prob = 0.0
    s.state0 = {k: v.clone() for k, v in s.m.state_dict().items()}
    s.inp, s.inp_s, s.stats, s.maps, s.const_h = cases.model_inputs("cuda")
    s.tgt, s.tgt_s = cases.model_targets("cuda")
    yield s
    del s.m, s.plain, s.attn


def _adapter_grads(P, m):
    return {n + s: getattr(mod, s[1:]).grad.clone() for n, mod in m.named_modules() if type(mod) is P.layers.LoraLinear
            for s in (".lora_A", ".lora_B")}


def test_model_eval_is_the_model_without_dropout(P, S):
    S.m.load_state_dict(S.state0)
    S.m.eval()
    S.plain.eval()
    with torch.no_grad():
        o1, s1 = S.m(S.inp, S.inp_s, S.stats, S.maps, S.const_h)
        o0, s0 = S.plain(S.inp, S.inp_s, S.stats, S.maps, S.const_h)
    assert torch.equal(o1, o0) and torch.equal(s1, s0)
    # a train()-mode bf16 forward outside the gradient path stays refused, and so does one without the opt-in
    S.m.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match="bf16_dropout"):
        S.m(S.inp, S.inp_s, S.stats, S.maps, S.const_h)
    S.m._lora_bf16_dropout = False
    try:
        with pytest.raises(RuntimeError, match="bf16_dropout"):
            S.m(S.inp, S.inp_s, S.stats, S.maps, S.const_h)
    finally:
        S.m._lora_bf16_dropout = True
        S.m.eval()


def test_model_train_step_follows_manual_seed(P, S):
    from pangu_pytorch_amd import train

    def step(seed):
        S.m.load_state_dict(S.state0)
        S.m.train()
        opt = train.make_optimizer(S.m, lr=1e-3)
        torch.manual_seed(seed)
        loss = train.train_step(S.m, opt, (S.inp, S.inp_s, S.tgt, S.tgt_s), S.stats, S.maps, S.const_h)
        return loss, _adapter_grads(P, S.m)

    l7, g7 = step(7)
    l7b, g7b = step(7)
    l8, g8 = step(8)
    assert len(g7) == 2 * 67
    assert torch.equal(l7, l7b) and all(torch.equal(g7[k], g7b[k]) for k in g7)
    assert not torch.equal(l7, l8) and any(not torch.equal(g7[k], g8[k]) for k in g7)
    for k, g in g7.items():
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0.0, k


def test_model_checkpointed_rollout_equals_one_graph(P, S):
    from pangu_pytorch_amd import rollout, train
    sl = _stats_last(S.stats)
    targets = []
    for k in range(2):
        targets += list(rollout.norm_back(synth.uniform(S.inp.shape, synth.name_seed(f"ld_t{k}"), device="cuda"),
                                          synth.uniform(S.inp_s.shape, synth.name_seed(f"ld_ts{k}"), device="cuda"), sl))
    batch = (S.inp, S.inp_s) + tuple(targets)

    def run(checkpoint):
        S.m.load_state_dict(S.state0)
        S.m.train()
        for q in S.m.parameters():
            q.grad = None
        opt = train.make_optimizer(S.m)
        torch.manual_seed(5)
        total, per = train.rollout_train_step(S.m, opt, batch, S.stats, S.maps, S.const_h, sl, checkpoint=checkpoint)
        return total, per, _adapter_grads(P, S.m)

    t_c, per_c, g_c = run(True)
    t_f, per_f, g_f = run(False)
    assert torch.equal(per_c, per_f) and torch.equal(t_c, t_f)
    worst = max(relnorm(g_c[k], g_f[k]) for k in g_f)
    print(f"bf16 dropout rollout (K = 2): worst relnorm of an adapter gradient, checkpointed vs one graph {worst:.3e}")
    assert worst < 1e-4, worst


def test_launch_log_and_peak_memory(P, S):
    """p = 0: none of the three tags, 16 fused-MLP training launches.  p = 0.1 everywhere: each tag 67 times, no plain lora_wgrad, no
    fused-MLP launch.  Attention projections only: the fused-MLP launch stays (16).  Peak memory of the dropout step within 1 GB of
    the no-dropout step (V is transient, h is not saved)."""
    from pangu_pytorch_amd import train
    log, peak = {}, {}
    for tag, m in (("p0", S.plain), ("p", S.m), ("attn", S.attn)):
        if m is S.m:
            m.load_state_dict(S.state0)
        m.train()
        opt = train.make_optimizer(m, lr=0.0)
        train.train_step(m, opt, (S.inp, S.inp_s, S.tgt, S.tgt_s), S.stats, S.maps, S.const_h)      # warm-up: shadows, workspaces
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        P.ops.timing_start()
        train.train_step(m, opt, (S.inp, S.inp_s, S.tgt, S.tgt_s), S.stats, S.maps, S.const_h)
        log[tag] = P.ops.timing_stop("lora_wgrad", also=NEW_KERNELS + ("mlp_fused_bf16",))
        peak[tag] = torch.cuda.max_memory_allocated()
        m.eval()
        del opt
    fused_mlp = {t: log[t][3]["mlp_fused_bf16"][2] for t in log}
    assert log["p0"][2] == 67 and all(log["p0"][3][k][2] == 0 for k in NEW_KERNELS) and fused_mlp["p0"] == 16, log["p0"]
    assert log["p"][2] == 0 and all(log["p"][3][k][2] == 67 for k in NEW_KERNELS) and fused_mlp["p"] == 0, log["p"]
    assert all(log["attn"][3][k][2] == 32 for k in NEW_KERNELS) and fused_mlp["attn"] == 16, log["attn"]
    print(f"bf16 LoRA train_step peak memory: no dropout {peak['p0'] / 2 ** 30:.2f} GiB, dropout on all 67 {peak['p'] / 2 ** 30:.2f} GiB, "
          f"attention only {peak['attn'] / 2 ** 30:.2f} GiB")
    assert peak["p"] - peak["p0"] <= 1e9, peak
