"""Native LoRA on the MI355X: the adapter-gradient and merge kernels against float64 torch, the adapted forward against the
base / merged model (bit for bit), the adapter gradients of one block against CPU autograd over the oracle with
W_eff = W + s B A built under autograd, the full-size adapter gradients against the full fine-tune path's dW_eff, and three
training steps.  Reads tests/golden only through the oracle's synthetic cases."""
import copy

import pytest
import torch

import cases
import pangu_oracle as O
import synth

pytestmark = pytest.mark.gpu
TIGHT = 3e-4                       # test_gpu_backward.py::test_block_backward_golden

# the 10 distinct (K -> N) projections of the model and their token counts
SHAPES = [(192, 576, 521280), (192, 192, 521280), (192, 768, 521280), (768, 192, 521280),
          (384, 1152, 131040), (384, 384, 131040), (384, 1536, 131040), (1536, 384, 131040),
          (768, 384, 131040), (384, 768, 131040)]


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available()
    P._lib.load()
    return P


def relnorm(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _ref_wgrad(dy, x, A, B, s):
    dy, x, A, B = (t.double() for t in (dy, x, A, B))
    return s * (dy @ B).t() @ x, s * dy.t() @ (x @ A.t())


def _operands(M, K, N, r, seed, strided=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if strided:            # row-strided views, as the block hands over halves of wider buffers
        x = torch.randn(M, K + 64, device="cuda", generator=g)[:, 32:32 + K]
        dy = torch.randn(M, N + 32, device="cuda", generator=g)[:, :N]
    else:
        x = torch.randn(M, K, device="cuda", generator=g)
        dy = torch.randn(M, N, device="cuda", generator=g)
    A = torch.randn(r, K, device="cuda", generator=g) * 0.1
    B = torch.randn(N, r, device="cuda", generator=g) * 0.1
    return dy, x, A, B


@pytest.mark.parametrize("K,N,M", SHAPES)
def test_lora_wgrad_all_projection_shapes(P, K, N, M):
    for r in (4, 8, 16, 32):
        dy, x, A, B = _operands(M, K, N, r, seed=K * 7 + N + r)
        dA, dB = P.ops.lora_wgrad(dy, x, A, B, 16.0 / r)
        rA, rB = _ref_wgrad(dy, x, A, B, 16.0 / r)
        assert relnorm(dA, rA) <= 1e-5, (K, N, r, relnorm(dA, rA))
        assert relnorm(dB, rB) <= 1e-5, (K, N, r, relnorm(dB, rB))
        del dy, x


@pytest.mark.parametrize("K,N", [(192, 576), (384, 1536), (1536, 384), (768, 192)])
def test_lora_wgrad_ragged_strided_and_deterministic(P, K, N):
    for r in (4, 8, 16, 32):
        for M in (1, 37, 4099, 100003):
            dy, x, A, B = _operands(M, K, N, r, seed=M + r, strided=True)
            assert x.stride(0) != K and dy.stride(0) != N
            dA, dB = P.ops.lora_wgrad(dy, x, A, B, 0.5)
            rA, rB = _ref_wgrad(dy, x, A, B, 0.5)
            assert relnorm(dA, rA) <= 1e-5 and relnorm(dB, rB) <= 1e-5, (K, N, r, M)
            dA2, dB2 = P.ops.lora_wgrad(dy, x, A, B, 0.5)
            assert torch.equal(dA, dA2) and torch.equal(dB, dB2)        # no atomics: bit-identical run to run


def test_lora_merge_kernel(P):
    for (K, N, _) in SHAPES:
        for r in (4, 16, 32):
            g = torch.Generator(device="cuda").manual_seed(K + N + r)
            W = torch.randn(N, K, device="cuda", generator=g) * 0.02
            A = torch.randn(r, K, device="cuda", generator=g) * 0.1
            B = torch.randn(N, r, device="cuda", generator=g) * 0.1
            We = P.ops.lora_merge(W, A, B, 2.0)
            ref = W.double() + 2.0 * B.double() @ A.double()
            assert relnorm(We, ref) <= 1e-6, (K, N, r)
            assert torch.equal(We, P.ops.lora_merge(W, A, B, 2.0))


def _randomise_adapters(model, seed, std=0.02):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(".lora_B") or n.endswith(".lora_A"):
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device))


@pytest.fixture(scope="module")
def full_models(P):
    base = P.PanguModel(device="cuda").cuda().eval()
    base.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    return base


def test_forward_fresh_adapter_and_merged_model_bit_identical(P, full_models):
    base = full_models
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    m = copy.deepcopy(base)
    m.enable_lora(r=16, alpha=16)
    with torch.no_grad():
        for dt in (torch.float32, torch.bfloat16):
            base.set_compute_dtype(dt)
            m.set_compute_dtype(dt)
            o0, s0 = base(inp, inp_s, stats, maps, const_h)
            o1, s1 = m(inp, inp_s, stats, maps, const_h)
            assert torch.equal(o0, o1) and torch.equal(s0, s1), dt            # B = 0: exactly the base model
            del o0, s0, o1, s1
        _randomise_adapters(m, 5)
        merged = copy.deepcopy(m)
        merged.merge_lora()
        for n, mod in m.named_modules():                                      # the merged weight IS the W_eff the forward used
            if type(mod) is P.layers.LoraLinear:
                assert torch.equal(dict(merged.named_modules())[n].weight, mod.effective_weight().view_as(mod.weight))
        for dt in (torch.float32, torch.bfloat16):
            m.set_compute_dtype(dt)
            merged.set_compute_dtype(dt)
            o1, s1 = m(inp, inp_s, stats, maps, const_h)
            o2, s2 = merged(inp, inp_s, stats, maps, const_h)
            assert torch.equal(o1, o2) and torch.equal(s1, s2), dt
            del o1, s1, o2, s2
        m.set_compute_dtype(torch.float32)
        merged.set_compute_dtype(torch.float32)
        base.set_compute_dtype(torch.float32)
        s_mean, s_std, u_mean, u_std = stats
        stats_last = (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1),
                      u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
                      u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())
        outs = []
        for model in (m, merged):
            gs = P.rollout.GraphedStep(model, inp, inp_s, stats, maps, const_h, stats_last, feed_back=True)
            for _ in range(2):
                o, os_ = gs.step()
            outs.append((o.clone(), os_.clone()))
            del gs
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("roll", [False, True])
def test_block_adapter_gradients_vs_oracle(P, C, roll):
    st = cases.STAGES[C]
    W = 24
    pre = cases.block_prefix(C, roll)
    blk = P.layers.EarthSpecificBlock(C, 0.1, st["heads"], device="cuda").cuda().eval()
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    lin_names = ["linear.linear1", "linear.linear2", "attention.linear1", "attention.linear2"]
    mods = dict(blk.named_modules())
    for n in lin_names:
        parent, _, leaf = n.rpartition(".")
        setattr(mods[parent], leaf, P.layers.LoraLinear.from_linear(mods[n], 16, 32))
    for p in blk.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device="cpu").manual_seed(C + int(roll))
    mods = dict(blk.named_modules())
    with torch.no_grad():
        for n in lin_names:
            mods[n].lora_A.copy_(torch.randn(mods[n].lora_A.shape, generator=g).cuda() * 0.05)
            mods[n].lora_B.copy_(torch.randn(mods[n].lora_B.shape, generator=g).cuda() * 0.05)
            mods[n].lora_A.requires_grad_(True)
            mods[n].lora_B.requires_grad_(True)
    x = cases.block_input(C, W, "cuda").requires_grad_(True)
    y = blk(x, st["Z"], st["H"], W, roll)
    cot = cases.cotangent(f"lora_block_{C}_{int(roll)}", y.shape, "cuda")
    (y * cot).sum().backward()
    # CPU autograd of the oracle with W_eff = W + s B A under autograd
    p = {k: v.detach().cpu() for k, v in cases.block_params(C, roll).items()}
    ab = {}
    for n in lin_names:
        A = mods[n].lora_A.detach().cpu().requires_grad_(True)
        B = mods[n].lora_B.detach().cpu().requires_grad_(True)
        ab[n] = (A, B)
        p[pre + n + ".weight"] = p[pre + n + ".weight"] + mods[n].scaling * (B @ A)
    xr = x.detach().cpu().requires_grad_(True)
    ref = O.earth_block(p, pre, xr, st["Z"], st["H"], W, st["heads"], roll)
    (ref * cot.cpu()).sum().backward()
    assert rel_err(y, ref) < TIGHT
    assert rel_err(x.grad, xr.grad) < TIGHT
    for n in lin_names:
        assert rel_err(mods[n].lora_A.grad, ab[n][0].grad) < TIGHT, (n, "A")
        assert rel_err(mods[n].lora_B.grad, ab[n][1].grad) < TIGHT, (n, "B")
    for k, q in blk.named_parameters():
        if not (k.endswith("lora_A") or k.endswith("lora_B")):
            assert q.grad is None, k                                         # frozen base tensors: nothing returned


def test_fullsize_adapter_gradients_vs_full_finetune(P, full_models):
    """dA == s B^T dW_eff and dB == s dW_eff A^T, with dW_eff the gradient of the existing full fine-tune path on the merged
    model; the output convolutions' gradients match that path."""
    from pangu_pytorch_amd import train
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    tgt, tgt_s = cases.model_targets("cuda")
    m = copy.deepcopy(full_models)
    m.enable_lora(r=16, alpha=16)
    _randomise_adapters(m, 11)
    merged = copy.deepcopy(m)
    merged.merge_lora()
    for q in merged.parameters():
        q.requires_grad_(True)
    out, out_s = merged(inp, inp_s, stats, maps, const_h)
    train.weighted_l1_loss(out, out_s, tgt, tgt_s).backward()
    del out, out_s
    ref = {n: q.grad for n, q in merged.named_parameters()}
    del merged
    out, out_s = m(inp, inp_s, stats, maps, const_h)
    train.weighted_l1_loss(out, out_s, tgt, tgt_s).backward()
    del out, out_s
    n_ad = 0
    for n, mod in m.named_modules():
        if type(mod) is P.layers.LoraLinear:
            dW = ref[n + ".weight"].double()
            s, A, B = mod.scaling, mod.lora_A.detach().double(), mod.lora_B.detach().double()
            assert relnorm(mod.lora_A.grad, s * B.t() @ dW) <= 1e-4, n
            assert relnorm(mod.lora_B.grad, s * dW @ A.t()) <= 1e-4, n
            assert mod.weight.grad is None
            n_ad += 1
    assert n_ad == 67
    # the output convolutions take the same kernels on bit-identical operands (the forwards agree bit for bit); their bias
    # column sums (and the weight tails of the largest slabs) are accumulated with fp32 atomics by linear_wgrad, so two runs of
    # that path agree to rounding, not to the bit
    for k in ("conv.weight", "conv.bias", "conv_surface.weight", "conv_surface.bias"):
        assert relnorm(dict(m.named_parameters())["_output_layer." + k].grad, ref["_output_layer." + k]) <= 1e-6, k


def test_lora_training_steps_and_grad_sync(P, full_models):
    from pangu_pytorch_amd import dist, train
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    tgt, tgt_s = cases.model_targets("cuda")
    m = copy.deepcopy(full_models)
    m.enable_lora(r=16, alpha=16)
    m.train()
    for mod in m.modules():                                  # DropPath off
        if isinstance(mod, P.layers.DropPath):
            mod.drop_prob = 0.0
    base = {n: q.detach().clone() for n, q in m.named_parameters() if not q.requires_grad}
    opt = train.make_optimizer(m, lr=1e-3)
    assert isinstance(opt, train.HipAdam)
    for _ in range(3):
        train.train_step(m, opt, (inp, inp_s, tgt, tgt_s), stats, maps, const_h)
    for n, q in m.named_parameters():
        if n in base:
            assert torch.equal(q, base[n]), n                 # frozen tensors bit-for-bit unchanged
    trainable = [q for q in m.parameters() if q.requires_grad]
    assert {id(q) for q, v in list(opt.state.items()) if v} == {id(q) for q in trainable}     # Adam state: trainable tensors only
    assert any(float(mod.lora_B.detach().abs().max()) > 0 for mod in m.modules() if type(mod) is P.layers.LoraLinear)
    m.eval()
    with torch.no_grad():
        o1, s1 = m(inp, inp_s, stats, maps, const_h)
        merged = copy.deepcopy(m)
        merged.merge_lora()
        o2, s2 = merged(inp, inp_s, stats, maps, const_h)
    assert torch.equal(o1, o2) and torch.equal(s1, s2)
    del o1, s1, o2, s2, merged
    # one-rank FlatGradSync: buckets cover exactly the trainable tensors; gradients equal those without the sync
    opt.zero_grad(set_to_none=True)
    out, out_s = m(inp, inp_s, stats, maps, const_h)
    train.weighted_l1_loss(out, out_s, tgt, tgt_s).backward()
    del out, out_s
    plain = {id(q): q.grad.clone() for q in trainable}
    opt.zero_grad(set_to_none=True)
    sync = dist.FlatGradSync(m)
    try:
        covered = [id(q) for _, _, views in sync.buckets for q, _ in views]
        assert sorted(covered) == sorted(id(q) for q in trainable)
        out, out_s = m(inp, inp_s, stats, maps, const_h)
        train.weighted_l1_loss(out, out_s, tgt, tgt_s).backward()
        del out, out_s
        sync.finish()
        adapters = {id(q) for mod in m.modules() if type(mod) is P.layers.LoraLinear for q in (mod.lora_A, mod.lora_B)}
        for q in trainable:
            if id(q) in adapters:
                assert torch.equal(q.grad, plain[id(q)])            # lora_wgrad: deterministic
            else:      # the output convolutions: linear_wgrad accumulates their bias sums / slab tails with fp32 atomics
                assert relnorm(q.grad, plain[id(q)]) <= 1e-6
    finally:
        sync.remove()
    # refusals
    m.set_compute_dtype(torch.bfloat16)
    with pytest.raises(RuntimeError, match="bf16 training with LoRA"):
        m(inp, inp_s, stats, maps, const_h)
    m.set_compute_dtype(torch.float32)
    with pytest.raises(RuntimeError, match="LoRA adapters"):
        train.GraphedTrainStep(m, opt, (inp, inp_s, tgt, tgt_s), stats, maps, const_h)
