"""bf16 LoRA training on the MI355X: the bf16 adapter-gradient kernel against float64 torch on the numbers it multiplies, the
adapted bf16 layer Functions against the same layers with the adapters merged (all parameters trainable, the existing bf16
path), and the whole adapted model through three bf16 training steps."""
import copy

import pytest
import torch

import cases
import synth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# the 10 distinct (K -> N) projections of the model (tests/test_gpu_lora.py::SHAPES, without their token counts)
SHAPES = [(192, 576), (192, 192), (192, 768), (768, 192), (384, 1152), (384, 384), (384, 1536), (1536, 384), (768, 384),
          (384, 768)]
# kernel vs float64 on the kernel's own operands: only the ONE bf16 rounding of U = x A^T / V = dy B (2^-9 per element) and fp32
# accumulation separate them
KERNEL_TOL = 2.0 ** -8
# adapter gradient vs s B^T dW_eff / s dW_eff A^T of the merged run: three independent 2^-9 roundings (the bf16 image of A / B,
# U / V, and the order difference to the bf16 weight-gradient kernel) sum to less than 2^-7
IDENTITY_TOL = 2.0 ** -7
DX_TOL = 2.0 ** -9
LIN_NAMES = ["linear.linear1", "linear.linear2", "attention.linear1", "attention.linear2"]


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available()
    P._lib.load()
    return P


def relnorm(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _ref_wgrad(dy, x, A, B, s):
    dy, x, A, B = (t.double() for t in (dy, x, A, B))
    return s * (dy @ B).t() @ x, s * dy.t() @ (x @ A.t())


def _operands(M, K, N, seed, strided):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if strided:            # row-strided views, as the block hands over halves of wider buffers
        x = torch.randn(M, K + 64, device="cuda", generator=g).to(BF)[:, 32:32 + K]
        dy = torch.randn(M, N + 32, device="cuda", generator=g).to(BF)[:, :N]
    else:
        x = torch.randn(M, K, device="cuda", generator=g).to(BF)
        dy = torch.randn(M, N, device="cuda", generator=g).to(BF)
    return dy, x


@pytest.mark.parametrize("K,N", SHAPES)
def test_lora_wgrad_bf16_vs_float64(P, K, N):
    """Every projection shape x every rank x M in {one row, less than one step, ragged, more than one workgroup slab} x
    {contiguous, row-strided}: relnorm <= 2^-8 against float64 on the bf16 values of x, dy, bf16(A), bf16(B); a second call is
    bit-identical; sentinel-filled outputs are fully overwritten."""
    ob, lib = P.ops_bf16, P._lib.load()
    worst = (-1.0, None)
    for M in (1, 37, 4099, 100003):
        for strided in (False, True):
            dy, x = _operands(M, K, N, seed=K * 7 + N + M, strided=strided)
            assert (x.stride(0) != K and dy.stride(0) != N) == strided
            for r in (4, 8, 16, 32):
                g = torch.Generator(device="cuda").manual_seed(r + M)
                A = torch.randn(r, K, device="cuda", generator=g) * 0.1
                B = torch.randn(N, r, device="cuda", generator=g) * 0.1
                s = 16.0 / r
                dA, dB = ob.lora_wgrad(dy, x, A, B, s)
                rA, rB = _ref_wgrad(dy, x, A.to(BF), B.to(BF), s)
                eA, eB = relnorm(dA, rA), relnorm(dB, rB)
                worst = max(worst, (eA, ("dA", M, strided, r)), (eB, ("dB", M, strided, r)))
                assert eA <= KERNEL_TOL and eB <= KERNEL_TOL, (K, N, M, strided, r, eA, eB)
                # a second call through the C entry into sentinel-filled outputs: bit-identical, nothing left unwritten
                dA2 = torch.full_like(dA, float("nan"))
                dB2 = torch.full_like(dB, float("nan"))
                ws = P.ops.wgrad_workspace(dy.device)
                rc = lib.pangu_lora_wgrad_bf16(torch.cuda.current_stream().cuda_stream, dy.data_ptr(), dy.stride(0), x.data_ptr(),
                                               x.stride(0), A.data_ptr(), B.data_ptr(), dA2.data_ptr(), dB2.data_ptr(), M, N, K, r,
                                               s, ws.data_ptr(), ws.numel() * 4)
                assert rc == 0
                assert torch.equal(dA, dA2) and torch.equal(dB, dB2), (K, N, M, strided, r)
    print(f"lora_wgrad_bf16 ({K} -> {N}): worst relnorm to float64 {worst[0]:.3e} at {worst[1]} (bound {KERNEL_TOL:.3e})")


# ---------------------------------------------------------------------------------------------------------------- one block
def _adapted_block(P, C, roll):
    """The block of tests/test_gpu_lora.py::test_block_adapter_gradients_vs_oracle: adapters (r = 16, alpha = 32) on all four
    projections, base tensors frozen."""
    st = cases.STAGES[C]
    pre = cases.block_prefix(C, roll)
    blk = P.layers.EarthSpecificBlock(C, 0.1, st["heads"], device="cuda").cuda().eval()
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    mods = dict(blk.named_modules())
    for n in LIN_NAMES:
        parent, _, leaf = n.rpartition(".")
        setattr(mods[parent], leaf, P.layers.LoraLinear.from_linear(mods[n], 16, 32))
    for p in blk.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device="cpu").manual_seed(C + int(roll))
    mods = dict(blk.named_modules())
    with torch.no_grad():
        for n in LIN_NAMES:
            mods[n].lora_A.copy_(torch.randn(mods[n].lora_A.shape, generator=g).cuda() * 0.05)
            mods[n].lora_B.copy_(torch.randn(mods[n].lora_B.shape, generator=g).cuda() * 0.05)
            mods[n].lora_A.requires_grad_(True)
            mods[n].lora_B.requires_grad_(True)
    return blk


def _merged(P, mod):
    """A deep copy of `mod` with every adapter folded into its base weight (PanguModel.merge_lora on a sub-module), all
    parameters trainable: the full fine-tune of the same function."""
    m = copy.deepcopy(mod)
    with torch.no_grad():
        for name, sub in list(m.named_modules()):
            for cname, child in list(sub.named_children()):
                if type(child) is P.layers.LoraLinear:
                    child.weight.copy_(child.effective_weight().view_as(child.weight))
                    setattr(sub, cname, child.to_linear())
    for q in m.parameters():
        q.requires_grad_(True)
        q.grad = None
    return m


def _check_identity(adapted, merged, names, what):
    """dA == s B^T dW_eff and dB == s dW_eff A^T (float64 products on the fp32 A, B), dW_eff from the merged run."""
    am, mm = dict(adapted.named_modules()), dict(merged.named_modules())
    worst = (-1.0, None)
    for n in names:
        lin = am[n]
        dW = mm[n].weight.grad.double()
        s, A, B = lin.scaling, lin.lora_A.detach().double(), lin.lora_B.detach().double()
        eA, eB = relnorm(lin.lora_A.grad, s * B.t() @ dW), relnorm(lin.lora_B.grad, s * dW @ A.t())
        worst = max(worst, (eA, n + ".lora_A"), (eB, n + ".lora_B"))
        assert eA <= IDENTITY_TOL and eB <= IDENTITY_TOL, (what, n, eA, eB)
        assert lin.weight.grad is None and (lin.bias is None or lin.bias.grad is None), (what, n)
    return worst


@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("roll", [False, True])
def test_block_bf16_adapter_gradients_vs_merged_block(P, C, roll):
    from pangu_pytorch_amd import fused, fused_bf16
    st = cases.STAGES[C]
    W = 24
    blk = _adapted_block(P, C, roll)
    merged = _merged(P, blk)
    x32 = cases.block_input(C, W, "cuda")
    cot = cases.cotangent(f"lora_block_{C}_{int(roll)}", x32.shape, "cuda")
    runs = {}
    for name, b in (("adapted", blk), ("merged", merged)):
        x = x32[0].to(BF).requires_grad_(True)
        y = fused.sample_block(b, x, st["Z"], st["H"], W, roll, sh=fused_bf16.WeightShadow())
        (y.float() * cot[0]).sum().backward()
        runs[name] = (y.detach(), x.grad)
    assert torch.equal(runs["adapted"][0], runs["merged"][0])                  # the same bf16 images of W_eff, the same kernels
    e_dx = relnorm(runs["adapted"][1], runs["merged"][1])
    assert e_dx <= DX_TOL, e_dx
    worst = _check_identity(blk, merged, LIN_NAMES, (C, roll))
    for k, q in blk.named_parameters():
        if not (k.endswith("lora_A") or k.endswith("lora_B")):
            assert q.grad is None, k                                         # frozen base tensors: nothing returned
    # against the fp32 LoRA block (tests/test_gpu_lora.py checks that one against the oracle): the project's bf16-vs-fp32 block
    # bound, rel-L2 < 2e-2 per tensor (tests/test_gpu_bf16.py::test_block_backward_bf16_vs_fp32)
    bf_grads = {k: q.grad.clone() for k, q in blk.named_parameters() if q.grad is not None}
    blk.zero_grad(set_to_none=True)
    xf = x32.clone().requires_grad_(True)
    (blk(xf, st["Z"], st["H"], W, roll) * cot).sum().backward()
    worst32 = max((relnorm(bf_grads[k], q.grad), k) for k, q in blk.named_parameters() if q.grad is not None)
    print(f"bf16 LoRA block C={C} roll={roll}: dx relnorm to the merged run {e_dx:.3e}; worst identity relnorm {worst[0]:.3e} "
          f"({worst[1]}, bound {IDENTITY_TOL:.3e}); worst rel-L2 to the fp32 LoRA block {worst32[0]:.3e} ({worst32[1]})")
    assert len(bf_grads) == 8 and worst32[0] < 2e-2, worst32


def _block_fn_apply(P, blk, x, geom, s1, s2, sh):
    from pangu_pytorch_amd import autograd as AB
    L = P.layers
    att = blk.attention
    return AB.EarthBlockFn.apply(x, blk.norm1.weight, blk.norm1.bias, blk.norm2.weight, blk.norm2.bias,
                                 L.eff_weight(blk.linear.linear1), blk.linear.linear1.bias, L.eff_weight(blk.linear.linear2),
                                 blk.linear.linear2.bias, att.earth_specific_bias, L.eff_weight(att.linear1), att.linear1.bias,
                                 L.eff_weight(att.linear2), att.linear2.bias, geom, s1, s2, None, sh,
                                 *L.lora_args(blk.linear.linear1, blk.linear.linear2, att.linear1, att.linear2))


@pytest.mark.parametrize("C,roll", [(192, True), (384, False)])
@pytest.mark.parametrize("s1,s2", [(0.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize("policy", ["zeros", "none"])
def test_block_bf16_dropped_branches(P, C, roll, s1, s2, policy):
    """A DropPath-dropped branch: its adapters get what the fp32 LoRA Function hands them under the same policy (zeros or None);
    the live branch's adapter gradients satisfy the identity against the merged block run with the same keep factors."""
    from pangu_pytorch_amd import fused_bf16
    st = cases.STAGES[C]
    W = 24
    geom = (st["Z"], st["H"], W, st["heads"], roll)
    blk = _adapted_block(P, C, roll)
    merged = _merged(P, blk)
    x32 = cases.block_input(C, W, "cuda")[0]
    cot = cases.cotangent(f"lora_block_{C}_{int(roll)}", x32.shape, "cuda")
    dropped, live = (LIN_NAMES[2:], LIN_NAMES[:2]) if s1 == 0.0 else (LIN_NAMES[:2], LIN_NAMES[2:])
    mods = dict(blk.named_modules())
    # the fp32 LoRA Function
    y = _block_fn_apply(P, blk, x32.clone().requires_grad_(True), geom, s1, s2, None)
    with P.ops.dropped_branch_grads(policy):
        (y * cot).sum().backward()
    f32 = {n: (mods[n].lora_A.grad, mods[n].lora_B.grad) for n in LIN_NAMES}
    blk.zero_grad(set_to_none=True)
    outs = {}
    for name, b in (("adapted", blk), ("merged", merged)):
        x = x32.to(BF).requires_grad_(True)
        y = _block_fn_apply(P, b, x, geom, s1, s2, fused_bf16.WeightShadow())
        with P.ops.dropped_branch_grads(policy):
            (y.float() * cot).sum().backward()
        outs[name] = (y.detach(), x.grad)
    assert torch.equal(outs["adapted"][0], outs["merged"][0])
    assert relnorm(outs["adapted"][1], outs["merged"][1]) <= DX_TOL
    for n in dropped:
        for got, want in zip((mods[n].lora_A.grad, mods[n].lora_B.grad), f32[n]):
            if want is None:
                assert got is None, (n, policy)
            else:
                assert float(want.abs().max()) == 0.0 and got is not None and torch.equal(got, want), (n, policy)
    assert all((f32[n][0] is None) == (policy == "none") for n in dropped)
    worst = _check_identity(blk, merged, live, (C, roll, s1, s2))
    print(f"bf16 LoRA block C={C} s1={s1} s2={s2} {policy}: worst identity relnorm of the live branch {worst[0]:.3e} ({worst[1]})")


# ---------------------------------------------------------------------------------------------- down- and up-sampling
def test_resample_bf16_adapter_gradients_vs_merged_layers(P):
    """DownSampleFn / UpSampleFn with adapters in bf16 at the geometry of tests/test_gpu_bf16.py::test_resample_ln_backward_bf16."""
    from pangu_pytorch_amd import fused, fused_bf16
    Z, H, W, C = 8, 181, 24, 192
    H2, W2 = 91, 12
    torch.manual_seed(3)
    for kind in ("down", "up"):
        layer = (P.layers.DownSample(C) if kind == "down" else P.layers.UpSample(2 * C, C)).cuda()
        names = ["linear"] if kind == "down" else ["linear1", "linear2"]
        with torch.no_grad():
            layer.norm.weight.uniform_(0.9, 1.1)
            layer.norm.bias.uniform_(-0.1, 0.1)
        for n in names:
            setattr(layer, n, P.layers.LoraLinear.from_linear(getattr(layer, n), 16, 32))
        for q in layer.parameters():
            q.requires_grad_(False)
        with torch.no_grad():
            for n in names:
                lin = getattr(layer, n)
                lin.lora_A.normal_(0.0, 0.05).requires_grad_(True)
                lin.lora_B.normal_(0.0, 0.05).requires_grad_(True)
        merged = _merged(P, layer)
        x0 = synth.uniform((Z * H * W, C) if kind == "down" else (Z * H2 * W2, 2 * C), 71 if kind == "down" else 72).to(BF).cuda()
        n_out = (Z * H2 * W2, 2 * C) if kind == "down" else (Z * H * 2 * W2, C)
        cot = synth.uniform(n_out, 73).cuda()
        outs = {}
        for name, m in (("adapted", layer), ("merged", merged)):
            x = x0.clone().requires_grad_(True)
            sh = fused_bf16.WeightShadow()
            y = fused.sample_down(m, x, Z, H, W, sh=sh) if kind == "down" else fused.sample_up(m, x, Z, H2, W2, H, sh=sh)
            assert tuple(y.shape) == n_out and y.dtype == BF
            (y.float() * cot).sum().backward()
            outs[name] = (y.detach(), x.grad)
        assert torch.equal(outs["adapted"][0], outs["merged"][0]), kind
        assert relnorm(outs["adapted"][1], outs["merged"][1]) <= DX_TOL, kind
        worst = _check_identity(layer, merged, names, kind)
        assert layer.norm.weight.grad is None and layer.norm.bias.grad is None
        print(f"bf16 LoRA {kind}-sampling: worst identity relnorm {worst[0]:.3e} ({worst[1]}, bound {IDENTITY_TOL:.3e})")


# ---------------------------------------------------------------------------------------------------------------- whole model
def _randomise_adapters(model, seed, std=0.02):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith(".lora_B") or n.endswith(".lora_A"):
                p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device))


def test_model_bf16_lora_training_steps_and_grad_sync(P):
    from pangu_pytorch_amd import dist, train
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    tgt, tgt_s = cases.model_targets("cuda")
    base = P.PanguModel(device="cuda").cuda().eval()
    base.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    m = copy.deepcopy(base)
    m.enable_lora(r=16, alpha=16, bf16_training=True)
    m.set_compute_dtype(BF)
    m.train()
    for mod in m.modules():                                  # DropPath off
        if isinstance(mod, P.layers.DropPath):
            mod.drop_prob = 0.0
    frozen = {n: q.detach().clone() for n, q in m.named_parameters() if not q.requires_grad}
    opt = train.make_optimizer(m, lr=1e-3)
    assert isinstance(opt, train.HipAdam)
    sizes = []
    for _ in range(3):
        loss = train.train_step(m, opt, (inp, inp_s, tgt, tgt_s), stats, maps, const_h)
        assert torch.isfinite(loss).item()
        sh = m._shadow
        sizes.append((len(sh.cache), len(sh.jobs), len(sh.makers)))
    assert sizes[2] == sizes[1], sizes                        # images of W_eff are keyed by their module: nothing accumulates
    # gradient accumulation: two backward passes on one set of W_eff images, one optimizer step
    loss = train.accumulated_train_step(m, opt, [(inp, inp_s, tgt, tgt_s)] * 2, stats, maps, const_h)
    assert torch.isfinite(loss).item()
    assert (len(m._shadow.cache), len(m._shadow.jobs), len(m._shadow.makers)) == sizes[2]
    assert all(isinstance(p, torch.nn.Parameter) for j in m._shadow.jobs.values() for p in j[1])
    for n, q in m.named_parameters():
        if n in frozen:
            assert torch.equal(q, frozen[n]), n                # frozen tensors bit-for-bit unchanged
    trainable = [q for q in m.parameters() if q.requires_grad]
    assert {id(q) for q, v in list(opt.state.items()) if v} == {id(q) for q in trainable}     # Adam state: trainable tensors only
    assert any(float(mod.lora_B.detach().abs().max()) > 0 for mod in m.modules() if type(mod) is P.layers.LoraLinear)
    # the adapted bf16 forward is the merged model's, bit for bit: inference ...
    m.eval()
    merged = copy.deepcopy(m)
    assert merged._lora_bf16_training is True
    merged.merge_lora()
    merged.set_compute_dtype(BF)
    with torch.no_grad():
        o1, s1 = m(inp, inp_s, stats, maps, const_h)
        o2, s2 = merged(inp, inp_s, stats, maps, const_h)
    assert torch.equal(o1, o2) and torch.equal(s1, s2)
    del o1, s1, o2, s2
    # ... and on the training path (the layer Functions, the module-keyed images of W_eff)
    opt.zero_grad(set_to_none=True)
    out, out_s = m(inp, inp_s, stats, maps, const_h)
    for q in merged.parameters():
        q.requires_grad_(True)
    o2, s2 = merged(inp, inp_s, stats, maps, const_h)
    assert out.requires_grad and o2.requires_grad
    assert torch.equal(out, o2) and torch.equal(out_s, s2)
    del o2, s2, merged
    # one-rank FlatGradSync: buckets cover exactly the trainable tensors; adapter gradients equal those without the sync
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
        assert len(adapters) == 2 * 67
        for q in trainable:
            if id(q) in adapters:
                assert torch.equal(q.grad, plain[id(q)])            # lora_wgrad: deterministic
    finally:
        sync.remove()
    # bf16 adapter training is opt-in: the default keeps refusing
    d = copy.deepcopy(base)
    d.enable_lora(r=16, alpha=16)
    d.set_compute_dtype(BF)
    with pytest.raises(RuntimeError, match="bf16 training with LoRA"):
        d(inp, inp_s, stats, maps, const_h)
    with pytest.raises(RuntimeError, match="LoRA adapters"):
        train.GraphedTrainStep(m, opt, (inp, inp_s, tgt, tgt_s), stats, maps, const_h)
