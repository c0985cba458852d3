"""The exact-split fp32 projection (csrc/gemm_f32_split.hip): fp32 operands as exact sums of three bf16 values, six partial
products on the bf16 matrix pipe.  Needs an MI355X: run with `-m gpu`.

The error rule everywhere (the acceptance rule of the kernel): against an fp64 product of the same fp32 inputs, the rel-L2 error of
the split kernel is at most 1.5 x the error of the fp32-MFMA kernel (ops.linear) on the same inputs -- the margin is for a different
summation order -- and never above 2e-6, the bound tests/test_gpu_parity.py::test_linear_random_shapes sets for ops.linear."""
import os
import types

import numpy as np
import pytest
import torch

import cases
import synth

pytestmark = pytest.mark.gpu
ABS_BOUND = 2e-6


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    P._lib.load()
    return P


def _ref64(a, w, b, act):
    ref = a.double() @ w.double().t()
    if b is not None:
        ref = ref + b.double()
    return torch.nn.functional.gelu(ref) if act else ref


def _l2(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


def _check(P, a, w, b, act, tag):
    """The error rule on one problem; -> the split result."""
    image = P.ops.split_weight_image(w)
    got = P.ops.linear_split(a, image, w.shape[0], b, act=act)
    base = P.ops.linear(a, w, b, act=act)
    ref = _ref64(a, w, b, act)
    e_split, e_f32 = _l2(got, ref), _l2(base, ref)
    print(f"{tag}: split {e_split:.3e} fp32 {e_f32:.3e} ratio {e_split / max(e_f32, 1e-30):.3f}")
    assert e_split <= min(1.5 * e_f32, ABS_BOUND), (tag, e_split, e_f32)
    return got


def _bf16_bits_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


@pytest.mark.parametrize("N,K", [(192, 16), (576, 192), (384, 400)])
def test_split_image_is_exact(P, N, K):
    """hi + mid + lo == W exactly (fp64 sum of the three bf16 planes, un-permuted by the pure-Python layout statement), over
    magnitudes 2^-40 .. 2^40, both signs, +-0, and values whose mid or lo part is zero."""
    L = P.split_layout
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn((N, K), generator=g) * torch.exp2(torch.randint(-40, 41, (N, K), generator=g).float())
    flat = w.view(-1)
    flat[0], flat[1] = 0.0, -0.0
    flat[2], flat[3] = 1.0, -3.0                                   # bf16 numbers: mid = lo = 0
    flat[4] = 1.0 + 2.0 ** -9                                      # hi + mid, lo = 0
    flat[5] = 1.0 + 2.0 ** -20                                     # mid takes any residual a bf16 can hold (2^-20): lo = 0
    flat[6] = -(1.0 + 2.0 ** -7 + 2.0 ** -15 + 2.0 ** -23)         # all 24 bits over the three parts
    flat[7], flat[8] = 2.0 ** -40, -(2.0 ** 40)
    image = P.ops.split_weight_image(w.cuda())
    assert image.dtype == torch.uint8 and image.numel() == 6 * N * K
    u16 = image.cpu().numpy().view(np.uint16)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    planes = [_bf16_bits_to_f64(u16[L.image_index(N, K, p, n, k)]) for p in range(3)]      # (the statement is plain integer arithmetic)
    w64 = w.numpy().astype(np.float64)
    assert np.array_equal(planes[0] + planes[1] + planes[2], w64)
    assert np.array_equal(np.signbit(planes[0]), np.signbit(w64))                            # -0 keeps its sign in hi
    for i in (2, 3):
        assert planes[1].flat[i] == 0.0 and planes[2].flat[i] == 0.0
    assert planes[1].flat[4] != 0.0 and planes[2].flat[4] == 0.0
    assert planes[1].flat[5] == 2.0 ** -20 and planes[2].flat[5] == 0.0
    assert planes[0].flat[6] == -(1.0 + 2.0 ** -7) and planes[1].flat[6] == -(2.0 ** -15) and planes[2].flat[6] == -(2.0 ** -23)
    # the layout statement itself, element by element, on a sample
    for (p, nn_, kk) in [(0, 0, 0), (1, N - 1, K - 1), (2, N // 2, 9 % K), (0, 191, 8 % K)]:
        assert L.image_index(N, K, p, nn_, kk) == L.image_index(N, K, p, n, k)[nn_, kk]


@pytest.mark.parametrize("M", [1, 127, 129, 1000])
def test_parity_against_fp64(P, M):
    """Every N x K of the served family at this M, act none / GELU, with and without bias."""
    torch.manual_seed(M)
    for N in (192, 384, 576):
        for K in (16, 32, 48, 192, 400):      # 1, 2, 3 k-steps: up to the ring depth
            a = torch.randn(M, K, device="cuda")
            w = torch.randn(N, K, device="cuda") / K ** 0.5
            b = torch.randn(N, device="cuda")
            for act in (0, 1):
                for bias in (None, b):
                    _check(P, a, w, bias, act, f"M{M} N{N} K{K} act{act} bias{int(bias is not None)}")


def test_strided_rows(P):
    """Row-strided `a` and `out`; the columns beside the strided `out` stay zero."""
    a_full = synth.uniform((700, 384), 21).cuda()
    w = synth.uniform((192, 192), 22, 0.07).cuda()
    b = synth.uniform((192,), 23, 0.5).cuda()
    image = P.ops.split_weight_image(w)
    out_full = torch.zeros((700, 384), device="cuda")
    P.ops.linear_split(a_full[:, 192:], image, 192, b, out=out_full[:, :192])
    dense = _check(P, a_full[:, 192:].contiguous(), w, b, 0, "strided")
    assert torch.equal(out_full[:, :192], dense)
    assert float(out_full[:, 192:].abs().max()) == 0.0
    out_full.zero_()
    P.ops.linear_split(a_full[:, :192], image, 192, None, act=P.ops.ACT_GELU, out=out_full[:, 192:])
    assert torch.equal(out_full[:, 192:], P.ops.linear_split(a_full[:, :192].contiguous(), image, 192, None, act=P.ops.ACT_GELU))
    assert float(out_full[:, :192].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K", [(129, 192, 192), (1000, 576, 400)])
def test_wide_dynamic_range(P, M, N, K):
    """Operands mixing magnitudes 2^-20 .. 2^20 within a row."""
    g = torch.Generator(device="cuda").manual_seed(5)
    mag = lambda shape: torch.exp2(torch.randint(-20, 21, shape, generator=g, device="cuda").float())
    a = torch.randn((M, K), generator=g, device="cuda") * mag((M, K))
    w = torch.randn((N, K), generator=g, device="cuda") * mag((N, K))
    _check(P, a, w, None, 0, f"wide M{M} N{N} K{K}")


def test_non_finite_rows(P):
    """A row of `a` holding an Inf or a NaN gives a non-finite output row; every other row is untouched."""
    torch.manual_seed(3)
    M, N, K = 200, 384, 192
    a = torch.randn(M, K, device="cuda")
    w = torch.randn(N, K, device="cuda") / K ** 0.5
    b = torch.randn(N, device="cuda")
    image = P.ops.split_weight_image(w)
    clean = P.ops.linear_split(a, image, N, b)
    bad = a.clone()
    bad[7, 5], bad[130, 191], bad[199, 0] = float("inf"), float("nan"), float("-inf")
    got = P.ops.linear_split(bad, image, N, b)
    rows = torch.tensor([7, 130, 199], device="cuda")
    assert not torch.isfinite(got[rows]).any()
    keep = torch.ones(M, dtype=torch.bool, device="cuda")
    keep[rows] = False
    assert torch.equal(got[keep], clean[keep]) and torch.isfinite(clean).all()


def test_fallback_and_image_cache(P):
    """What a block's plain projection does (fused._plain_proj): an unserved shape (N % 4, K % 16: no image) goes to ops.linear,
    a switched-off block gives ops.linear's result bit for bit; a served weight takes the split kernel, a LoRA layer on the image of its merged weight; a
    weight edited in place (`copy_` under no_grad) gets a new image, observed through param_stamp.  K = 112 (a K padded to 16s)
    is served."""
    torch.manual_seed(4)
    on, off = types.SimpleNamespace(split_projections=True), types.SimpleNamespace(split_projections=False)
    x = torch.randn(300, 384, device="cuda")
    with torch.no_grad():
        for unserved, xu in ((torch.nn.Linear(384, 162, device="cuda"), x),                     # N % 4 != 0
                             (torch.nn.Linear(24, 192, device="cuda"), x[:, :24])):             # K % 16 != 0
            assert P.ops.split_image(unserved, unserved.weight) is None
            # the split kernels serve every shape the fp32-MFMA kernel serves, so what _plain_proj falls back to is ops.linear's
            # own refusal of the shape: the same error, nothing else tried
            with pytest.raises(RuntimeError, match="linear_fwd failed") as want:
                P.ops.linear(xu, unserved.weight, unserved.bias)
            with pytest.raises(RuntimeError) as got:
                P.fused._plain_proj(on, unserved, xu)
            assert str(got.value) == str(want.value)
        lin = torch.nn.Linear(384, 192, device="cuda")
        assert torch.equal(P.fused._plain_proj(off, lin, x), P.ops.linear(x, lin.weight, lin.bias))
        # a LoRA layer computes on the image of its merged weight W_eff: with B = 0 the base layer's bits, and after an adapter
        # update a new image, the one a merged model's plain layer gets
        lora = P.layers.LoraLinear.from_linear(lin, 4, 4)
        assert torch.equal(P.fused._plain_proj(on, lora, x), P.fused._plain_proj(on, lin, x))
        for _ in range(2):
            lora.lora_B.normal_()
            w_eff = P.layers.eff_weight(lora)
            assert w_eff is not lora.weight
            assert torch.equal(P.fused._plain_proj(on, lora, x),
                               P.ops.linear_split(x, P.ops.split_weight_image(w_eff), 192, lora.bias))
            assert torch.equal(P.fused._plain_proj(off, lora, x), P.ops.linear(x, w_eff, lora.bias))
        # served: the split kernel from the cached image
        image = P.ops.split_image(lin, lin.weight)
        assert image is not None and P.ops.split_image(lin, lin.weight) is image
        y = P.fused._plain_proj(on, lin, x, act=P.ops.ACT_GELU)
        assert torch.equal(y, P.ops.linear_split(x, image, 192, lin.bias, act=P.ops.ACT_GELU))
        stamp = P.ops.param_stamp(lin.weight)
        lin.weight.copy_(torch.randn_like(lin.weight))
        assert P.ops.param_stamp(lin.weight) != stamp
        image2 = P.ops.split_image(lin, lin.weight)
        assert image2 is not image and torch.equal(image2, P.ops.split_weight_image(lin.weight))
        assert not torch.equal(image2, image)
        lin112 = torch.nn.Linear(112, 192, device="cuda")
        assert P.ops.split_image(lin112, lin112.weight) is not None
        _check(P, torch.randn(650, 112, device="cuda"), lin112.weight.detach(), lin112.bias.detach(), 0, "K112")


@pytest.mark.parametrize("N", [192, 384])
def test_whole_tiles_keep_their_image_and_bits(P, N):
    """N % 192 == 0 has no rows behind N (6 N K bytes) and the bits recorded for tests/test_gpu_split_fingerprint.py, on that
    list's inputs: the one entry serves these shapes with the kernel that has no column guard."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import gemm_f32_fingerprint as F
    with open(os.path.join(root, "profiles", "gemm_f32_shared_loops_fingerprint_new.json")) as f:
        want = json.load(f)
    M, K = 129, 48
    a, w, b = F.t("a", M, K), F.t("w", N, K, scale=K ** -0.5), F.t("b", N)
    image = P.ops.split_weight_image(w)
    assert image.dtype == torch.uint8 and image.numel() == 6 * N * K == 6 * P.ops.split_image_rows(N) * K
    for act in (P.ops.ACT_NONE, P.ops.ACT_GELU):
        for bias in (b, None):
            key = f"linear_split M={M} N={N} K={K} {F.ACT_NAMES[act]} bias={int(bias is not None)}"
            assert F.digest(P.ops.linear_split(a, image, N, bias, act=act)) == want[key], key


def test_one_block_split_against_fp32_kernels(P, golden_dir):
    """A C = 384 block in eval mode on (Z, H, W) = (8, 91, 24): the split projections against the same block with the switch off
    (relative difference <= 1e-5), both within the existing bound against the reference's golden output."""
    C, roll = 384, True
    st = cases.STAGES[C]
    blk = P.layers.EarthSpecificBlock(C, 0.1, st["heads"], device="cuda").cuda().eval()
    pre = cases.block_prefix(C, roll)
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    x = cases.block_input(C, 24, "cuda")
    g = np.load(os.path.join(golden_dir, f"block_{C}_{int(roll)}.npz"))
    with torch.no_grad():
        assert blk.split_projections
        y_split = blk(x, st["Z"], st["H"], 24, roll)
        blk.split_projections = False
        y_f32 = blk(x, st["Z"], st["H"], 24, roll)
    diff = ((y_split - y_f32).abs().max() / y_f32.abs().max()).item()
    print(f"block split vs fp32 kernels: {diff:.3e}")
    assert diff <= 1e-5
    assert not torch.equal(y_split, y_f32)                        # (the two arms really are different kernels)
    for y in (y_split, y_f32):
        assert cases.compare_summary(y, g, f"block_{C}_{int(roll)}.out", 1e-3) < 2e-4
