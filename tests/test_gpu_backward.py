"""Backward parity of the HIP path: kernels vs torch autograd over the CPU oracle, layers and the whole training
step vs golden gradients produced by the reference's own backward (oracle/gen_golden.py).  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch

import cases
import pangu_oracle as O
import synth

pytestmark = pytest.mark.gpu
REL = 1e-3
TIGHT = 3e-4


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available()
    P._lib.load()
    return P


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("M,N,K", [(4096, 192, 192), (5000, 576, 192), (3001, 768, 192), (2500, 192, 768),
                                   (4111, 1152, 384), (2222, 384, 1536), (3333, 160, 384), (1999, 64, 384),
                                   (2777, 192, 112), (100, 384, 768)])
def test_linear_wgrad(P, M, N, K):
    dc, a = synth.uniform((M, N), 61), synth.uniform((M, K), 62)
    dw, db = P.ops.linear_wgrad(dc.cuda(), a.cuda())
    assert rel_err(dw, dc.double().t() @ a.double()) < TIGHT
    assert rel_err(db, dc.double().sum(0)) < TIGHT


def test_linear_wgrad_random_shapes(P):
    """Ragged token counts and every tile family of the weight-gradient GEMMs (fp32 and bf16) against fp64 products."""
    import random
    from pangu_pytorch_amd import ops_bf16 as ob
    rnd = random.Random(5)
    torch.manual_seed(5)
    for _ in range(24):
        N = rnd.choice([160, 192, 384, 576, 768, 1152, 64, 136])
        K = rnd.choice([64, 112, 128, 192, 384, 768, 160])
        M = rnd.randint(1, 9000)
        dc = torch.randn(M, N, device="cuda")
        a = torch.randn(M, K, device="cuda")
        dw, db = P.ops.linear_wgrad(dc, a)
        ref_w, ref_b = dc.double().t() @ a.double(), dc.double().sum(0)
        assert ((dw.double() - ref_w).norm() / ref_w.norm()).item() < 3e-6, (M, N, K)
        assert ((db.double() - ref_b).norm() / ref_b.norm()).item() < 3e-6, (M, N, K)
        if K % 8 == 0:
            dcb, ab = dc.bfloat16(), a.bfloat16()
            dw, db = ob.linear_wgrad(dcb, ab)
            ref_w, ref_b = dcb.double().t() @ ab.double(), dcb.double().sum(0)
            assert ((dw.double() - ref_w).norm() / ref_w.norm()).item() < 1e-5, (M, N, K)
            assert ((db.double() - ref_b).norm() / ref_b.norm()).item() < 1e-5, (M, N, K)


def test_linear_wgrad_strided(P):
    full = synth.uniform((3000, 576), 63).cuda()
    a = synth.uniform((3000, 192), 64).cuda()
    dw, db = P.ops.linear_wgrad(full[:, 192:384], a)
    assert rel_err(dw, full[:, 192:384].cpu().double().t() @ a.cpu().double()) < TIGHT


def test_gelu_fwd_aux_and_bwd_epilogue(P):
    M, N, K = 1500, 768, 192
    a, w, b = synth.uniform((M, K), 65), synth.uniform((N, K), 66, 0.1), synth.uniform((N,), 67, 0.3)
    pre = torch.empty((M, N), device="cuda")
    h = P.ops.linear(a.cuda(), w.cuda(), b.cuda(), act=P.ops.ACT_GELU, aux=pre)
    ref_pre = a @ w.t() + b
    assert rel_err(pre, ref_pre) < TIGHT and rel_err(h, torch.nn.functional.gelu(ref_pre)) < TIGHT
    dm, w2 = synth.uniform((M, 192), 68), synth.uniform((192, N), 69, 0.05)
    got = P.ops.linear(dm.cuda(), w2.t().contiguous().cuda(), None, act=P.ops.ACT_GELU_BWD, aux=pre)
    x = ref_pre.clone().requires_grad_(True)
    (torch.nn.functional.gelu(x) * (dm @ w2)).sum().backward()
    assert rel_err(got, x.grad) < TIGHT


@pytest.mark.parametrize("C", [192, 384, 768])
def test_ln_residual_bwd(P, C):
    N = 2051
    y = synth.uniform((N, C), 71, 2.0, 0.3).requires_grad_(True)
    g = synth.uniform((C,), 72, 0.1, 1.0).requires_grad_(True)
    b = synth.uniform((C,), 73, 0.1).requires_grad_(True)
    dout = synth.uniform((N, C), 74)
    (1.25 * torch.nn.functional.layer_norm(y, (C,), g, b) * dout).sum().backward()
    dy, dg, db = P.ops.ln_residual_bwd(dout.cuda(), y.detach().cuda(), g.detach().cuda(), 1.25)
    assert rel_err(dy, y.grad) < TIGHT and rel_err(dg, g.grad) < TIGHT and rel_err(db, b.grad) < TIGHT


@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("shifted", [False, True])
def test_window_attention_bwd(P, C, shifted):
    st = cases.STAGES[C]
    Z, H, W, heads = st["Z"], st["H"], 24, st["heads"]
    N = Z * H * W
    qkv = synth.uniform((1, N, 3 * C), 81, 1.5).requires_grad_(True)
    b1 = synth.uniform((3 * C,), 82, 0.5).requires_grad_(True)
    esb = synth.uniform((1, st["types"], heads, 144, 144), 83, 0.5).requires_grad_(True)
    do = synth.uniform((1, N, C), 84)
    ref, ref_lse = O.window_attention_core(qkv, b1, esb, Z, H, W, heads, shifted)
    (ref * do).sum().backward()
    o, lse = P.ops.window_attention(qkv[0].detach().cuda(), b1.detach().cuda(), esb[0].detach().cuda(), Z, H, W, heads,
                                    shifted, want_lse=True)
    dqkv, dqb, desb = P.ops.window_attention_bwd(qkv[0].detach().cuda(), b1.detach().cuda(), esb[0].detach().cuda(), o,
                                                 lse, do[0].cuda(), Z, H, W, heads, shifted)
    assert rel_err(dqkv, qkv.grad[0]) < TIGHT
    assert rel_err(desb, esb.grad[0]) < TIGHT
    assert rel_err(dqb, b1.grad) < TIGHT

@pytest.mark.parametrize("Z,H,W,heads", [(4, 7, 24, 3), (2, 13, 12, 2)])
@pytest.mark.parametrize("shifted", [False, True])
def test_window_attention_bwd_other_geometries(P, Z, H, W, heads, shifted):
    """Backward on geometries other than the model's (odd head count = unpaired block order), fp32 and bf16 kernels."""
    from pangu_pytorch_amd import ops_bf16 as ob
    C = 32 * heads
    N = Z * H * W
    types = (Z // 2) * ((H + 5) // 6)
    for bf in (False, True):
        dt = torch.bfloat16 if bf else torch.float32
        qkv = synth.uniform((1, N, 3 * C), 81, 1.5).to(dt).float().requires_grad_(True)
        b1 = synth.uniform((3 * C,), 82, 0.5).to(dt).float().requires_grad_(True)
        esb = synth.uniform((1, types, heads, 144, 144), 83, 0.5).to(dt).float().requires_grad_(True)
        do = synth.uniform((1, N, C), 84).to(dt).float()
        ref, _ = O.window_attention_core(qkv, b1, esb, Z, H, W, heads, shifted)
        (ref * do).sum().backward()
        mod = ob if bf else P.ops
        q, bb, e, d = (t.detach().to(dt).cuda() for t in (qkv[0], b1, esb[0], do[0]))
        o, lse = mod.window_attention(q, bb, e, Z, H, W, heads, shifted, want_lse=True)
        dqkv, dqb, desb = mod.window_attention_bwd(q, bb, e, o, lse, d, Z, H, W, heads, shifted)
        tol = 3e-2 if bf else TIGHT
        assert rel_err(dqkv, qkv.grad[0]) < tol
        assert rel_err(desb, esb.grad[0]) < tol
        assert rel_err(dqb, b1.grad) < tol


@pytest.mark.parametrize("C", [192, 384])
@pytest.mark.parametrize("roll", [False, True])
def test_block_backward_golden(P, golden_dir, C, roll):
    """All 13 parameter gradients + dx of one EarthSpecificBlock vs the reference's autograd."""
    tag = f"block_{C}_{int(roll)}"
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    st = cases.STAGES[C]
    blk = P.layers.EarthSpecificBlock(C, 0.1, st["heads"], device="cuda").cuda().eval()
    pre = cases.block_prefix(C, roll)
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    x = cases.block_input(C, 24, "cuda").requires_grad_(True)
    y = blk(x, st["Z"], st["H"], 24, roll)
    assert cases.compare_summary(y, g, tag + ".out", REL) < TIGHT
    (y * cases.cotangent(tag, y.shape, "cuda")).sum().backward()
    assert cases.compare_summary(x.grad, g, tag + ".dx", REL) < TIGHT
    for k, p in blk.named_parameters():
        err = cases.compare_summary(p.grad, g, tag + ".d_" + k, REL)
        assert err < TIGHT, (k, err)


def test_fullres_layers_backward_golden(P, golden_dir):
    g = np.load(os.path.join(golden_dir, "layers_fullres.npz"))
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")

    def check(module, prefix, tagp):
        for k, p in module.named_parameters():
            err = cases.compare_summary(p.grad, g, f"{tagp}.d_{k}", REL)
            assert err < TIGHT, (tagp, k, err)

    x0 = m._input_layer(inp, inp_s, stats, maps, const_h)
    (x0 * cases.cotangent("embed", x0.shape, "cuda")).sum().backward()
    check(m._input_layer, "_input_layer.", "embed")
    del x0
    xin = synth.uniform((1, 8 * 181 * 360, 192), synth.name_seed("down_in"), device="cuda").requires_grad_(True)
    y = m.downsample(xin, 8, 181, 360)
    (y * cases.cotangent("down", y.shape, "cuda")).sum().backward()
    assert cases.compare_summary(xin.grad, g, "down.dx", REL) < TIGHT
    check(m.downsample, "downsample.", "down")
    xin = synth.uniform((1, 8 * 91 * 180, 384), synth.name_seed("up_in"), device="cuda").requires_grad_(True)
    y = m.upsample(xin)
    (y * cases.cotangent("up", y.shape, "cuda")).sum().backward()
    assert cases.compare_summary(xin.grad, g, "up.dx", REL) < TIGHT
    check(m.upsample, "upsample.", "up")
    xin = synth.uniform((1, 8 * 181 * 360, 384), synth.name_seed("recover_in"), device="cuda").requires_grad_(True)
    o, os_ = m._output_layer(xin, 8, 181, 360)
    ((o * cases.cotangent("recover", o.shape, "cuda")).sum() + (os_ * cases.cotangent("recover_s", os_.shape, "cuda")).sum()).backward()
    assert cases.compare_summary(xin.grad, g, "recover.dx", REL) < TIGHT
    check(m._output_layer, "_output_layer.", "recover")


def test_full_training_step_golden(P, golden_dir):
    """Training-step body of reference models/pangu_sample.py:52-71 (eval mode => DropPath off): loss and every one
    of the 223 parameter gradients vs the reference's backward (which re-computes each block; we do not)."""
    path = os.path.join(golden_dir, "model_bwd.npz")
    if not os.path.exists(path):
        pytest.skip("model_bwd.npz not generated")
    g = np.load(path)
    from pangu_pytorch_amd import train
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    tgt, tgt_s = cases.model_targets("cuda")
    out, out_s = m(inp, inp_s, stats, maps, const_h)
    loss = train.weighted_l1_loss(out, out_s, tgt, tgt_s)
    loss.backward()
    assert abs(loss.item() - float(g["model.loss"][0])) / float(g["model.loss"][0]) < 1e-5
    # Tolerances.  The L1 loss' gradient is sign(o - t): an output within rounding distance of its target flips a
    # +-w/N term between two correct fp32 implementations, so element-wise gradient samples carry O(1e-3..1e-2)
    # noise where sums cancel (measured: 2.2e-3 on _output_layer.conv.bias, up to 8.4e-3 on single bias-table
    # samples, changing with any last-bit change of the forward).  The sign-free check of the same backward is
    # test_full_backward_smooth_golden below; here the gradient MASS per tensor (sum |g|, no cancellation) must
    # agree to 1e-3 (measured <= 2.1e-4) and samples to 2e-2.
    SAMPLE_TOL, MASS_TOL = 2e-2, 1e-3
    worst, worst_mass = ("", 0.0), ("", 0.0)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        flat = p.grad.detach().float().flatten()
        pos = synth.sample_positions(flat.numel(), cases.NSAMP, synth.name_seed("pos_model.d_" + k), device=flat.device)[:256]
        gs = torch.as_tensor(g[f"model.d_{k}.samples"])
        gabs = float(g[f"model.d_{k}.abs_sum"][0])
        scale = max(gs.abs().max().item(), gabs / flat.numel())
        err = ((flat[pos].cpu() - gs).abs().max().item()) / scale
        mass = abs(flat.double().abs().sum().item() - gabs) / gabs
        if err > worst[1]:
            worst = (k, err)
        if mass > worst_mass[1]:
            worst_mass = (k, mass)
    assert worst[1] < SAMPLE_TOL, worst
    assert worst_mass[1] < MASS_TOL, worst_mass


def test_full_backward_smooth_golden(P, golden_dir):
    """Whole-model backward under a smooth loss (sum(out * cotangent) / numel): all 223 gradients vs the reference's
    autograd, without the L1 sign discontinuity -> tight tolerance."""
    path = os.path.join(golden_dir, "model_bwd_smooth.npz")
    if not os.path.exists(path):
        pytest.skip("model_bwd_smooth.npz not generated")
    g = np.load(path)
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    out, out_s = m(inp, inp_s, stats, maps, const_h)
    loss = ((out * cases.cotangent("model_out", out.shape, "cuda")).sum() +
            (out_s * cases.cotangent("model_out_s", out_s.shape, "cuda")).sum()) / out.numel()
    loss.backward()
    ref_loss = float(g["model.loss"][0])
    assert abs(loss.item() - ref_loss) < 1e-3 * max(abs(ref_loss), 1e-3)
    worst, worst_mass = ("", 0.0), ("", 0.0)
    for k, p in m.named_parameters():
        flat = p.grad.detach().float().flatten()
        pos = synth.sample_positions(flat.numel(), cases.NSAMP, synth.name_seed("pos_model.d_" + k), device=flat.device)[:256]
        gs = torch.as_tensor(g[f"model.d_{k}.samples"])
        gabs = float(g[f"model.d_{k}.abs_sum"][0])
        scale = max(gs.abs().max().item(), gabs / flat.numel())
        err = ((flat[pos].cpu() - gs).abs().max().item()) / scale
        mass = abs(flat.double().abs().sum().item() - gabs) / gabs
        worst = max(worst, (k, err), key=lambda t: t[1])
        worst_mass = max(worst_mass, (k, mass), key=lambda t: t[1])
    assert worst[1] < REL, worst
    assert worst_mass[1] < REL, worst_mass


@pytest.mark.parametrize("s1,s2", [(0.0, 1.25), (1.25, 0.0), (1.25, 1.25)])
def test_block_droppath_branches(P, s1, s2):
    """Training-mode stochastic depth (timm DropPath, reference layers.py:140,250-251): a kept branch is scaled by
    1/(1-p), a dropped branch contributes nothing (and is not computed); forward and every gradient vs torch autograd
    over the oracle with the same per-branch factors."""
    C, roll, W = 192, True, 12
    st = cases.STAGES[C]
    blk = P.layers.EarthSpecificBlock(C, 0.2, st["heads"], device="cuda").cuda().train()
    pre = cases.block_prefix(C, roll)
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    seq = iter([s1, s2])
    blk.drop_path.sample_scale = lambda training: next(seq)
    x = cases.block_input(C, W, "cuda").requires_grad_(True)
    y = blk(x, st["Z"], st["H"], W, roll)
    cot = cases.cotangent("dp", y.shape, "cuda")
    (y * cot).sum().backward()
    # oracle with explicit branch factors
    p = {k: v.requires_grad_(True) for k, v in cases.block_params(C, roll).items()}
    g = lambda k: p[pre + k]
    xr = x.detach().cpu().requires_grad_(True)
    a = O.window_attention(xr, g("attention.linear1.weight"), g("attention.linear1.bias"), g("attention.linear2.weight"),
                           g("attention.linear2.bias"), g("attention.earth_specific_bias"), st["Z"], st["H"], W,
                           st["heads"], roll)
    x1 = xr + s1 * torch.nn.functional.layer_norm(a, (C,), g("norm1.weight"), g("norm1.bias"))
    m = O.mlp(x1, g("linear.linear1.weight"), g("linear.linear1.bias"), g("linear.linear2.weight"), g("linear.linear2.bias"))
    ref = x1 + s2 * torch.nn.functional.layer_norm(m, (C,), g("norm2.weight"), g("norm2.bias"))
    (ref * cot.cpu()).sum().backward()
    assert rel_err(y, ref) < TIGHT and rel_err(x.grad, xr.grad) < TIGHT
    for k, q in blk.named_parameters():
        want = p[pre + k].grad
        if want is None or float(want.abs().max()) == 0.0:
            assert q.grad is None or float(q.grad.abs().max()) == 0.0, k
        else:
            assert rel_err(q.grad, want) < TIGHT, k


def test_reference_loop_body_three_steps_with_dropped_branches(P):
    """the reference's loop body UNCHANGED (models/pangu_sample.py:45-77: `optimizer.zero_grad()`,
    `model.train()`, forward, torch-op L1, `loss.backward()`, `optimizer.step()` with `torch.optim.Adam(lr=5e-6,
    weight_decay=3e-6)`, finetune_fully.py:121) around the HIP block, three steps with fixed DropPath draws (all kept / MLP
    branch dropped / attention branch dropped), against the same loop over the oracle where a dropped branch is COMPUTED and
    multiplied by zero (timm DropPath, layers.py:250-251).  The parameters of a dropped branch must take Adam's zero-gradient
    step (weight decay moves them by ~lr, the moments decay, `step` advances): under the old default (gradient None) Adam
    skipped them, a 5e-6 deviation per step."""
    C, roll, W = 192, True, 12
    st = cases.STAGES[C]
    blk = P.layers.EarthSpecificBlock(C, 0.2, st["heads"], device="cuda").cuda()
    pre = cases.block_prefix(C, roll)
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    p0 = {k: q.detach().clone().cpu() for k, q in blk.named_parameters()}
    ref = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    x = cases.block_input(C, W, "cuda")
    tgt = cases.cotangent("ref_loop_target", x.shape, "cuda")
    draws = [(1.25, 1.25), (1.25, 0.0), (0.0, 1.25)]
    seq = iter([s for d in draws for s in d])
    blk.drop_path.sample_scale = lambda training: next(seq)
    opt = torch.optim.Adam(blk.parameters(), lr=5e-6, weight_decay=3e-6)
    opt_ref = torch.optim.Adam(list(ref.values()), lr=5e-6, weight_decay=3e-6)
    g = lambda k: ref[k]
    mlp_names = ("linear.linear1.weight", "linear.linear1.bias", "linear.linear2.weight", "linear.linear2.bias", "norm2.weight", "norm2.bias")
    for step, (s1, s2) in enumerate(draws):
        # ---- the reference's loop body, HIP model
        opt.zero_grad()
        blk.train()
        y = blk(x, st["Z"], st["H"], W, roll)
        loss = torch.mean(torch.abs(y - tgt) * 1.5)
        loss.backward()
        assert all(q.grad is not None for q in blk.parameters()), [k for k, q in blk.named_parameters() if q.grad is None]
        before = {k: q.detach().clone() for k, q in blk.named_parameters()} if s2 == 0.0 else None
        opt.step()
        if before is not None:      # the dropped MLP branch's parameters moved (Adam's weight-decay step on a zero gradient)
            for k in mlp_names[:4]:
                assert float((dict(blk.named_parameters())[k].detach() - before[k]).abs().max()) > 1e-6, k
        # ---- the same loop over the oracle, branches computed and scaled (x 0 when dropped)
        opt_ref.zero_grad()
        xr = x.detach().cpu()
        a = O.window_attention(xr, g("attention.linear1.weight"), g("attention.linear1.bias"), g("attention.linear2.weight"),
                               g("attention.linear2.bias"), g("attention.earth_specific_bias"), st["Z"], st["H"], W, st["heads"], roll)
        x1 = xr + s1 * torch.nn.functional.layer_norm(a, (C,), g("norm1.weight"), g("norm1.bias"))
        m = O.mlp(x1, g("linear.linear1.weight"), g("linear.linear1.bias"), g("linear.linear2.weight"), g("linear.linear2.bias"))
        yr = x1 + s2 * torch.nn.functional.layer_norm(m, (C,), g("norm2.weight"), g("norm2.bias"))
        lr_ = torch.mean(torch.abs(yr - tgt.cpu()) * 1.5)
        lr_.backward()
        opt_ref.step()
        assert abs(float(loss.detach()) - float(lr_.detach())) < 1e-5 * abs(float(lr_.detach())), (step, float(loss.detach()), float(lr_.detach()))
    # Adam's first steps are lr * sign-like (g / (|g| + eps)): an element whose gradient is at the rounding level of the fp32
    # kernels can take a step of the other sign (2 * lr = 1e-5 apart); everything else agrees to ~1e-8.  Bound the bulk tightly
    # and the share of such elements.
    worst = []
    n_out = n_all = 0
    for k, q in blk.named_parameters():
        d = (q.detach().cpu() - ref[k].detach()).abs()
        n_out += int((d > 1e-6).sum())
        n_all += d.numel()
        worst.append((float(d.max()), float(torch.quantile(d.flatten()[:1 << 22].float(), 0.999)), k))
        moved = (ref[k].detach() - p0[k]).abs().max()
        assert float(moved) > 1e-6, k            # every parameter was stepped in the reference run (also the dropped branches')
    worst.sort(reverse=True)
    print("reference loop, 3 steps: worst |p_hip - p_ref| (max, p99.9, name):", worst[:4], "elements > 1e-6:", n_out, "of", n_all)
    assert max(w[1] for w in worst) <= 1e-6, worst[:4]
    assert n_out <= 2e-4 * n_all, (n_out, n_all)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_dropped_branch_gradient_policy(P, dt):
    """What a block returns for the parameters of a DropPath-dropped branch: explicit zero tensors by DEFAULT ("zeros": the
    reference's autograd result, layers.py:250-251 -- branch computed, multiplied by zero -- so any optimizer of any foreign loop
    steps them as the reference does) and None under ops.dropped_branch_grads("none"), which train.train_step selects around its
    own backward (it gives those parameters the zero-gradient step without materialising zeros)."""
    assert P.ops.dropped_branch_policy() == "zeros"                  # the drop-in default
    C, roll, W = 192, False, 12
    st = cases.STAGES[C]
    blk = P.layers.EarthSpecificBlock(C, 0.2, st["heads"], device="cuda").cuda().train()
    pre = cases.block_prefix(C, roll)
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    mlp_names = ("linear.linear1.weight", "linear.linear1.bias", "linear.linear2.weight", "linear.linear2.bias", "norm2.weight", "norm2.bias")
    try:
        for policy in ("none", "zeros"):
            P.ops.set_dropped_branch_grads(policy)
            blk.zero_grad(set_to_none=True)
            seq = iter([1.25, 0.0])                       # attention branch kept, MLP branch dropped
            blk.drop_path.sample_scale = lambda training: next(seq)
            x = cases.block_input(C, W, "cuda")
            if dt == "bf16":
                from pangu_pytorch_amd import autograd, fused_bf16
                att = blk.attention
                s1, s2 = blk.drop_path.sample_scale(True), blk.drop_path.sample_scale(True)
                y = autograd.EarthBlockFn.apply(
                    x[0].to(torch.bfloat16).requires_grad_(True), blk.norm1.weight, blk.norm1.bias, blk.norm2.weight, blk.norm2.bias,
                    blk.linear.linear1.weight, blk.linear.linear1.bias, blk.linear.linear2.weight, blk.linear.linear2.bias,
                    att.earth_specific_bias, att.linear1.weight, att.linear1.bias, att.linear2.weight, att.linear2.bias,
                    (st["Z"], st["H"], W, att.head_number, roll), s1, s2, None, fused_bf16.WeightShadow())
            else:
                y = blk(x.requires_grad_(True), st["Z"], st["H"], W, roll)
            (y.float() * cases.cotangent("dp", y.shape, "cuda")).sum().backward()
            named = dict(blk.named_parameters())
            for k in mlp_names:
                if policy == "none":
                    assert named[k].grad is None, k
                else:
                    assert named[k].grad is not None and named[k].grad.shape == named[k].shape and float(named[k].grad.abs().max()) == 0.0, k
            assert named["attention.linear1.weight"].grad is not None and float(named["attention.linear1.weight"].grad.abs().max()) > 0
    finally:
        P.ops.set_dropped_branch_grads("zeros")


def test_block_backward_batch_of_two(P):
    """A batch of two through the autograd path == the two samples run one by one: outputs per sample, input gradients
    per sample, parameter gradients summed (the per-sample slicing is a view / one unbind, never a SelectBackward)."""
    C, roll, W = 384, True, 12
    st = cases.STAGES[C]
    blk = P.layers.EarthSpecificBlock(C, 0.0, st["heads"], device="cuda").cuda().eval()
    pre = cases.block_prefix(C, roll)
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    x0 = cases.block_input(C, W, "cuda")
    x1 = synth.uniform(x0.shape, 4242, device="cuda")
    cot = cases.cotangent("b2", (2,) + tuple(x0.shape[1:]), "cuda")
    xb = torch.cat([x0, x1], 0).requires_grad_(True)
    yb = blk(xb, st["Z"], st["H"], W, roll)
    (yb * cot).sum().backward()
    gb = {k: q.grad.clone() for k, q in blk.named_parameters()}
    blk.zero_grad(set_to_none=True)
    singles = []
    for i, xi in enumerate((x0, x1)):
        xi = xi.clone().requires_grad_(True)
        yi = blk(xi, st["Z"], st["H"], W, roll)
        (yi * cot[i:i + 1]).sum().backward()
        singles.append((yi.detach(), xi.grad))
    for i, (yi, gi) in enumerate(singles):
        assert torch.equal(yb[i:i + 1].detach(), yi)
        assert torch.equal(xb.grad[i:i + 1], gi)
    for k, q in blk.named_parameters():
        assert rel_err(gb[k], q.grad) < 1e-5, k         # sums of two atomically accumulated gradients: order may differ
