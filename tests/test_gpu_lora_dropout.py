"""LoRA adapter dropout on the MI355X: the keep mask of the kernels against its host restatement (exactly), the forward and
backward correction kernels against float64 torch on their own operands, one block / DownSample / UpSample / Mlp /
EarthAttention3D against CPU autograd over the oracle's pieces with peft's formula and the restated masks, and the whole model
(eval() unchanged, seeded steps reproducible, checkpointed rollout).  References are float64; the masks come from
layers.lora_dropout_keep."""
import copy

import pytest
import torch
import torch.nn.functional as F

import cases
import pangu_oracle as O
import synth

pytestmark = pytest.mark.gpu
TIGHT = 3e-4                       # test_gpu_lora.py::test_block_adapter_gradients_vs_oracle
P_DROP = 0.1

# the 10 distinct (K -> N) projections of the model (test_gpu_lora.py)
KN = [(192, 576), (192, 192), (192, 768), (768, 192), (384, 1152), (384, 384), (384, 1536), (1536, 384), (768, 384), (384, 768)]
RAGGED_KN = [(192, 576), (1536, 384), (768, 192)]
NEW_KERNELS = ("lora_dropout_fwd", "lora_wgrad_dropout", "lora_dropout_dx")


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available()
    P._lib.load()
    return P


def relnorm(a, b):
    a, b = a.detach().double(), b.detach().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _keep(P, seed, M, K, p, device="cuda"):
    return P.layers.lora_dropout_keep(seed, M, K, p, device=device)


def _operands(M, K, N, r, seed, strided=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if strided:            # row-strided views, as the block hands over halves of wider buffers
        x = torch.randn(M, K + 64, device="cuda", generator=g)[:, 32:32 + K]
        y = torch.randn(M, N + 32, device="cuda", generator=g)[:, :N]
    else:
        x = torch.randn(M, K, device="cuda", generator=g)
        y = torch.randn(M, N, device="cuda", generator=g)
    A = torch.randn(r, K, device="cuda", generator=g) * 0.1
    B = torch.randn(N, r, device="cuda", generator=g) * 0.1
    return x, y, A, B


def _like(t, fill=None):
    """A tensor of t's shape AND strides (the row-strided operands stay row-strided), zero or a copy of t."""
    base = torch.zeros(t.shape[0], t.stride(0), device=t.device)
    v = base[:, :t.shape[1]]
    if fill is not None:
        v.copy_(fill)
    return v


# ---- the mask, exactly

@pytest.mark.parametrize("K,groups", [(192, range(12)), (1536, (0, 47, 95))])
def test_kernel_mask_equals_the_restatement(P, K, groups):
    """x = 1, y = 0, s = 1, A = unit vectors onto 16 columns at a time, B = the first 16 columns of the identity: y[:, :16] IS c."""
    M, N, r = 37, 64, 16
    B = torch.zeros(N, r, device="cuda")
    B[:r] = torch.eye(r, device="cuda")
    x = torch.ones(M, K + 64, device="cuda")[:, 32:32 + K]
    masks = {}
    for p, seed in ((0.1, 7), (0.1, 8), (0.5, 7)):
        got = torch.zeros(M, K, dtype=torch.bool, device="cuda")
        seen = torch.zeros(K, dtype=torch.bool)
        for g in groups:
            A = torch.zeros(r, K, device="cuda")
            A[torch.arange(r), 16 * g + torch.arange(r)] = 1.0
            y = torch.zeros(M, N + 32, device="cuda")[:, :N]
            P.ops.lora_dropout_fwd(x, y, A, B, 1.0, p, seed)
            c = y[:, :16]
            assert torch.equal(y[:, 16:], torch.zeros_like(y[:, 16:]))
            kept = c > 0
            assert torch.allclose(c[kept], torch.full_like(c[kept], p / (1 - p)), rtol=1e-6, atol=0)
            assert torch.equal(c[~kept], torch.full_like(c[~kept], -1.0))
            got[:, 16 * g:16 * g + 16] = kept
            seen[16 * g:16 * g + 16] = True
        want = _keep(P, seed, M, K, p)
        assert torch.equal(got[:, seen.cuda()], want[:, seen.cuda()]), (K, p, seed)
        masks[(p, seed)] = got[:, seen.cuda()]
    assert not torch.equal(masks[(0.1, 7)], masks[(0.1, 8)])          # two seeds, two masks


# ---- the forward kernel

def _check_fwd(P, M, K, N, r, p, seed, strided):
    s = 16.0 / r
    x, y0, A, B = _operands(M, K, N, r, seed=K * 7 + N + r + M, strided=strided)
    x_in = x.clone()
    c = torch.where(_keep(P, seed, M, K, p), p / (1 - p), -1.0).double()
    delta = s * ((c * x.double()) @ A.double().t()) @ B.double().t()
    tag = (M, K, N, r)
    # from y = 0: the correction itself
    y = _like(y0)
    P.ops.lora_dropout_fwd(x, y, A, B, s, p, seed)
    e = relnorm(y, delta)
    assert e <= 1e-5, ("delta", tag, e)
    # on a random y: the sum, with h = gelu(y_out)
    y = _like(y0, y0)
    h = _like(y0)
    P.ops.lora_dropout_fwd(x, y, A, B, s, p, seed, act=P.ops.ACT_GELU, h=h)
    e = relnorm(y, y0.double() + delta)
    assert e <= 1e-6, ("sum", tag, e)
    e = relnorm(h, F.gelu(y.double()))
    assert e <= 1e-6, ("gelu", tag, e)
    y2 = _like(y0, y0)
    P.ops.lora_dropout_fwd(x, y2, A, B, s, p, seed)
    assert torch.equal(y2, y), ("bit-identical, and the same y with and without the GELU output", tag)
    assert torch.equal(x, x_in)
    if strided:
        assert x.stride(0) != K and y.stride(0) != N and h.stride(0) != N


@pytest.mark.parametrize("K,N", KN)
def test_fwd_all_projection_shapes(P, K, N):
    for r in (4, 8, 16, 32):
        _check_fwd(P, 4099, K, N, r, P_DROP, seed=1000 + r, strided=False)


@pytest.mark.parametrize("K,N", RAGGED_KN)
def test_fwd_ragged_and_strided(P, K, N):
    for r in (4, 8, 16, 32):
        for M in (1, 37, 100003):
            _check_fwd(P, M, K, N, r, P_DROP, seed=M + r, strided=True)


# ---- the backward kernels

def _check_bwd(P, M, K, N, r, p, seed, strided):
    s = 16.0 / r
    x, dy, A, B = _operands(M, K, N, r, seed=K * 5 + N + r + M, strided=strided)
    x_in, dy_in = x.clone(), dy.clone()
    keep = _keep(P, seed, M, K, p)
    xd = torch.where(keep, x.double() / (1 - p), 0.0)
    c = torch.where(keep, p / (1 - p), -1.0).double()
    del keep
    Vr = s * dy.double() @ B.double()
    tag = (M, K, N, r)
    dA, dB, V = P.ops.lora_wgrad_dropout(dy, x, A, B, s, p, seed)
    for name, got, ref in (("dA", dA, Vr.t() @ xd), ("dB", dB, s * dy.double().t() @ (xd @ A.double().t())), ("V", V, Vr)):
        e = relnorm(got, ref)
        assert e <= 1e-5, (name, tag, e)
    dA2, dB2, V2 = P.ops.lora_wgrad_dropout(dy, x, A, B, s, p, seed)
    assert torch.equal(dA, dA2) and torch.equal(dB, dB2) and torch.equal(V, V2), tag
    assert torch.equal(x, x_in) and torch.equal(dy, dy_in), tag
    # the input-gradient correction, from the kernel's own V
    corr = c * (V.double() @ A.double())
    dx = _like(x)
    P.ops.lora_dropout_dx(dx, V, A, p, seed)
    e = relnorm(dx, corr)
    assert e <= 1e-5, ("dx from 0", tag, e)
    g = torch.Generator(device="cuda").manual_seed(M + K)
    dx0 = torch.randn(M, K, device="cuda", generator=g)
    dx = _like(x, dx0)
    P.ops.lora_dropout_dx(dx, V, A, p, seed)
    e = relnorm(dx, dx0.double() + corr)
    assert e <= 1e-6, ("dx on random", tag, e)
    dx2 = _like(x, dx0)
    P.ops.lora_dropout_dx(dx2, V, A, p, seed)
    assert torch.equal(dx, dx2), tag
    # behind a GELU (the MLP's second projection): the correction carries gelu'(pre)
    pre = torch.randn(M, K, device="cuda", generator=g)
    pd = pre.double().requires_grad_(True)
    F.gelu(pd).sum().backward()
    dx = _like(x)
    P.ops.lora_dropout_dx(dx, V, A, p, seed, pre=pre)
    e = relnorm(dx, corr * pd.grad)
    assert e <= 1e-5, ("dx behind the GELU", tag, e)


@pytest.mark.parametrize("K,N", KN)
def test_bwd_all_projection_shapes(P, K, N):
    for r in (4, 8, 16, 32):
        _check_bwd(P, 4099, K, N, r, P_DROP, seed=2000 + r, strided=False)


@pytest.mark.parametrize("K,N", RAGGED_KN)
def test_bwd_ragged_and_strided(P, K, N):
    for r in (4, 8, 16, 32):
        for M in (1, 37, 100003):
            _check_bwd(P, M, K, N, r, P_DROP, seed=M + r, strided=True)


# ---- layers against CPU autograd over the oracle's pieces, peft's formula, restated masks

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


class _Peft:
    """peft's lora.Linear forward on the CPU for the adapted modules of a layer: y = x W^T + b + s drop(x) A^T B^T with the mask
    restated from the seed the module drew; A and B are leaves."""

    def __init__(self, P, mods, names):
        self.P, self.mods = P, mods
        self.ab = {n: tuple(t.detach().cpu().requires_grad_(True) for t in (mods[n].lora_A, mods[n].lora_B)) for n in names}

    def __call__(self, n, x):
        mod = self.mods[n]
        A, B = self.ab[n]
        W = mod.weight.detach().cpu()
        b = None if mod.bias is None else mod.bias.detach().cpu()
        K = x.shape[-1]
        keep = self.P.layers.lora_dropout_keep(mod.last_dropout_seed, x.numel() // K, K, mod.lora_dropout).reshape(x.shape)
        xd = x * keep / (1.0 - mod.lora_dropout)
        y = x @ W.t() + mod.scaling * (xd @ A.t()) @ B.t()
        return y if b is None else y + b

    def check(self, names):
        for n in names:
            assert rel_err(self.mods[n].lora_A.grad, self.ab[n][0].grad) < TIGHT, (n, "A")
            assert rel_err(self.mods[n].lora_B.grad, self.ab[n][1].grad) < TIGHT, (n, "B")


def _same_without_grad(run, seed):
    """Train mode under no_grad equals train mode with grad for the same seed."""
    torch.manual_seed(seed)
    y1 = run()
    torch.manual_seed(seed)
    with torch.no_grad():
        y2 = run()
    assert not y2.requires_grad and torch.equal(y1.detach(), y2)
    return y1


@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("roll", [False, True])
def test_block_with_dropout_vs_oracle(P, C, roll):
    st = cases.STAGES[C]
    W = 24
    pre = cases.block_prefix(C, roll)
    blk = P.layers.EarthSpecificBlock(C, 0.0, st["heads"], device="cuda").cuda()
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    names = ["linear.linear1", "linear.linear2", "attention.linear1", "attention.linear2"]
    mods = _adapt(P, blk, names, C + int(roll))
    blk.train()
    x = cases.block_input(C, W, "cuda").requires_grad_(True)
    y = _same_without_grad(lambda: blk(x, st["Z"], st["H"], W, roll), 21)
    cot = cases.cotangent(f"lora_drop_block_{C}_{int(roll)}", y.shape, "cuda")
    (y * cot).sum().backward()
    # the reference
    p = {k: v.detach().cpu() for k, v in cases.block_params(C, roll).items()}
    g = lambda k: p[pre + k]
    peft = _Peft(P, mods, names)
    xr = x.detach().cpu().requires_grad_(True)
    qkv = peft("attention.linear1", xr)
    o, _ = O.window_attention_core(qkv, g("attention.linear1.bias"), g("attention.earth_specific_bias"), st["Z"], st["H"], W,
                                   st["heads"], roll)
    x1 = xr + F.layer_norm(peft("attention.linear2", o), (C,), g("norm1.weight"), g("norm1.bias"))
    m = peft("linear.linear2", F.gelu(peft("linear.linear1", x1)))
    ref = x1 + F.layer_norm(m, (C,), g("norm2.weight"), g("norm2.bias"))
    (ref * cot.cpu()).sum().backward()
    assert rel_err(y, ref) < TIGHT
    assert rel_err(x.grad, xr.grad) < TIGHT
    peft.check(names)
    # the dropout did something: the same block in eval() mode differs
    blk.eval()
    with torch.no_grad():
        assert rel_err(blk(x, st["Z"], st["H"], W, roll), ref) > 10 * TIGHT


def test_downsample_and_upsample_with_dropout_vs_oracle(P):
    Z, H, W, C = 8, 181, 24, 192
    sd = {k: synth.synth_param(k, s) for k, s in cases.model_param_shapes().items() if k.startswith(("downsample.", "upsample."))}
    # down
    m = P.layers.DownSample(C).cuda()
    m.load_state_dict({k[len("downsample."):]: v.cuda() for k, v in sd.items() if k.startswith("downsample.")})
    mods = _adapt(P, m, ["linear"], 3)
    m.train()
    x = synth.uniform((1, Z * H * W, C), 51).cuda().requires_grad_(True)
    y = _same_without_grad(lambda: m(x, Z, H, W), 22)
    cot = cases.cotangent("lora_drop_down", y.shape, "cuda")
    (y * cot).sum().backward()
    peft = _Peft(P, mods, ["linear"])
    xr = x.detach().cpu().requires_grad_(True)
    H2, W2 = (H + 1) // 2, W // 2
    t = F.pad(xr.view(1, Z, H, W, C), (0, 0, 0, 0, 0, 1))
    t = t.view(1, Z, H2, 2, W2, 2, C).permute(0, 1, 2, 4, 3, 5, 6).reshape(1, Z * H2 * W2, 4 * C)
    ref = peft("linear", F.layer_norm(t, (4 * C,), sd["downsample.norm.weight"], sd["downsample.norm.bias"]))
    (ref * cot.cpu()).sum().backward()
    assert rel_err(y, ref) < TIGHT and rel_err(x.grad, xr.grad) < TIGHT
    peft.check(["linear"])
    # up
    m = P.layers.UpSample(2 * C, C).cuda()
    m.load_state_dict({k[len("upsample."):]: v.cuda() for k, v in sd.items() if k.startswith("upsample.")})
    names = ["linear1", "linear2"]
    mods = _adapt(P, m, names, 4)
    m.train()
    x = synth.uniform((1, Z * H2 * W2, 2 * C), 52).cuda().requires_grad_(True)
    y = _same_without_grad(lambda: m(x, Z, H2, W2, H), 23)
    cot = cases.cotangent("lora_drop_up", y.shape, "cuda")
    (y * cot).sum().backward()
    peft = _Peft(P, mods, names)
    xr = x.detach().cpu().requires_grad_(True)
    t = peft("linear1", xr)
    t = t.view(1, Z, H2, W2, 2, 2, C).permute(0, 1, 2, 4, 3, 5, 6).reshape(1, Z, 2 * H2, 2 * W2, C)
    t = t[:, :, :H].reshape(1, Z * H * 2 * W2, C)
    ref = peft("linear2", F.layer_norm(t, (C,), sd["upsample.norm.weight"], sd["upsample.norm.bias"]))
    (ref * cot.cpu()).sum().backward()
    assert rel_err(y, ref) < TIGHT and rel_err(x.grad, xr.grad) < TIGHT
    peft.check(names)


def test_mlp_and_attention_modules_with_dropout_vs_oracle(P):
    C, roll = 192, True
    st = cases.STAGES[C]
    pre = cases.block_prefix(C, roll)
    blk = P.layers.EarthSpecificBlock(C, 0.0, st["heads"], device="cuda").cuda()
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    p = {k: v.detach().cpu() for k, v in cases.block_params(C, roll).items()}
    names = ["linear1", "linear2"]
    # Mlp on its own, an odd number of rows
    mlp = blk.linear
    mods = _adapt(P, mlp, names, 5)
    mlp.train()
    x = synth.uniform((3, 37, C), 61).cuda().requires_grad_(True)
    y = _same_without_grad(lambda: mlp(x), 24)
    cot = cases.cotangent("lora_drop_mlp", y.shape, "cuda")
    (y * cot).sum().backward()
    peft = _Peft(P, mods, names)
    xr = x.detach().cpu().requires_grad_(True)
    ref = peft("linear2", F.gelu(peft("linear1", xr.reshape(-1, C)))).reshape(x.shape)
    (ref * cot.cpu()).sum().backward()
    assert rel_err(y, ref) < TIGHT and rel_err(x.grad, xr.grad) < TIGHT
    peft.check(names)
    # EarthAttention3D on its own
    att = blk.attention
    mods = _adapt(P, att, names, 6)
    att.train()
    xw = cases.attention_window_input(C, 2, "cuda").requires_grad_(True)
    mask = blk.gen_mask(torch.zeros(1, st["Z"], st["H"] + 5, 24, C, device="cuda"))
    y = _same_without_grad(lambda: att(xw, mask), 25)
    cot = cases.cotangent("lora_drop_attn", y.shape, "cuda")
    (y * cot).sum().backward()
    peft = _Peft(P, mods, names)
    xr = xw.detach().cpu().requires_grad_(True)
    nLon, types, n, _ = xr.shape
    heads = st["heads"]
    qkv = peft("linear1", xr.reshape(-1, C)).view(nLon, types, n, 3, heads, 32).permute(3, 0, 1, 4, 2, 5)
    q, k, v = qkv[0] * 32 ** -0.5, qkv[1], qkv[2]
    s = q @ k.transpose(-2, -1) + p[pre + "attention.earth_specific_bias"][0].unsqueeze(0) + mask.cpu().view(nLon, types, 1, n, n)
    o = (torch.softmax(s, dim=-1) @ v).permute(0, 1, 3, 2, 4).reshape(-1, C)
    ref = peft("linear2", o).reshape(xr.shape)
    (ref * cot.cpu()).sum().backward()
    assert rel_err(y, ref) < TIGHT and rel_err(xw.grad, xr.grad) < TIGHT
    peft.check(names)


# ---- the whole model

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
    s.plain.enable_lora(r=16, alpha=16)
    _randomise_adapters(s.plain, 5)
    s.m = base
    s.m.enable_lora(r=16, alpha=16, lora_dropout=P_DROP)
    _randomise_adapters(s.m, 5)
    for model in (s.m, s.plain):
        for mod in model.modules():                                  # DropPath off
            if isinstance(mod, P.layers.DropPath):
                mod.drop_prob = 0.0
    s.state0 = {k: v.clone() for k, v in s.m.state_dict().items()}
    s.inp, s.inp_s, s.stats, s.maps, s.const_h = cases.model_inputs("cuda")
    s.tgt, s.tgt_s = cases.model_targets("cuda")
    yield s
    del s.m, s.plain


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
    assert worst < 1e-4, worst


def test_no_dropout_is_the_old_launch_sequence(P, S):
    """The launch log of a training step with lora_dropout = 0 names none of the new kernels; with 0.1 it names all three."""
    from pangu_pytorch_amd import train
    log = {}
    for tag, m in (("p0", S.plain), ("p", S.m)):
        if m is S.m:
            m.load_state_dict(S.state0)
        m.train()
        opt = train.make_optimizer(m, lr=0.0)
        P.ops.timing_start()
        train.train_step(m, opt, (S.inp, S.inp_s, S.tgt, S.tgt_s), S.stats, S.maps, S.const_h)
        log[tag] = P.ops.timing_stop("lora_wgrad", also=NEW_KERNELS)
        m.eval()
        del opt
    assert log["p0"][2] == 67 and all(log["p0"][3][k][2] == 0 for k in NEW_KERNELS)
    assert log["p"][2] == 0 and all(log["p"][3][k][2] == 67 for k in NEW_KERNELS)
