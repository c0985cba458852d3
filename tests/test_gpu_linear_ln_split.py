"""The exact-split fused projection + LayerNorm + residual (csrc/gemm_ln_f32_split.hip): the main loop gemm_f32_split.hip runs
(csrc/split_f32.h) under the epilogue gemm_ln_f32_dma.hip runs (csrc/ln_epilogue_f32.h).  Needs an MI355X: run with `-m gpu`.

The error rule (the rule of tests/test_gpu_linear_split.py applied to the fused op): against the fp64 value of
shortcut + s * LN(a @ W^T + b) on the same fp32 inputs, the rel-L2 error of the split op is at most 1.5 x the error of
ops.linear_ln_residual (the fp32-MFMA kernel) -- the margin is for the different summation order -- and its max-abs / max error is
below TIGHT = 2e-4, the bound tests/test_gpu_parity.py::test_linear_ln_residual sets for the fp32 kernel."""
import os
import types

import numpy as np
import pytest
import torch

import cases
import synth

pytestmark = pytest.mark.gpu
TIGHT = 2e-4


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    P._lib.load()
    return P


def _ref64(a, w, b, sc, g, be, s):
    y = a.double() @ w.double().t()
    if b is not None:
        y = y + b.double()
    return sc.double() + s * torch.nn.functional.layer_norm(y, (w.shape[0],), g.double(), be.double(), 1e-5)


def _errs(got, ref):
    d = got.double() - ref
    return (d.norm() / ref.norm()).item(), (d.abs().max() / ref.abs().max()).item()


def _problem(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=g, device="cuda")
    return dict(a=r(M, K), w=r(N, K) / K ** 0.5, b=r(N), sc=1.5 * r(M, N), g=1.0 + 0.5 * r(N), be=0.3 * r(N))


def _both(P, p, bias=True, s=1.0):
    """-> (split result, fp32-MFMA result) on one problem."""
    b = p["b"] if bias else None
    image = P.ops.split_weight_image(p["w"])
    got = P.ops.linear_ln_residual_split(p["a"], image, p["w"].shape[0], b, p["sc"], p["g"], p["be"], branch_scale=s)
    base = P.ops.linear_ln_residual(p["a"], p["w"], b, p["sc"], p["g"], p["be"], branch_scale=s)
    return got, base


def _check(P, p, bias, s, tag, rows=None, tight=True):
    """The error rule on one problem (on `rows` of it); -> the split result."""
    got, base = _both(P, p, bias, s)
    ref = _ref64(p["a"], p["w"], p["b"] if bias else None, p["sc"], p["g"], p["be"], s)
    sel = slice(None) if rows is None else rows
    (e_split, m_split), (e_f32, m_f32) = _errs(got[sel], ref[sel]), _errs(base[sel], ref[sel])
    print(f"{tag}: split {e_split:.3e} (max {m_split:.3e}) fp32 {e_f32:.3e} (max {m_f32:.3e}) ratio {e_split / max(e_f32, 1e-30):.3f}")
    assert e_split <= 1.5 * e_f32, (tag, e_split, e_f32)
    if tight:
        assert m_split < TIGHT, (tag, m_split)
    return got


@pytest.mark.parametrize("M", [1, 127, 129, 1000])
def test_parity_against_fp64(P, M):
    """Every N x K x bias x branch_scale at this M: K = 16 .. 64 are 1, 2, 3 (the ring depth) and 4 k-steps, K = 400 wraps the
    ring eight times."""
    for N in (192, 384):
        for K in (16, 32, 48, 64, 400):
            p = _problem(M, N, K, 1000 * M + N + K)
            for bias in (True, False):
                for s in (1.0, 0.5):
                    _check(P, p, bias, s, f"M{M} N{N} K{K} bias{int(bias)} s{s}")


@pytest.mark.parametrize("N", [192, 384])
def test_strided_rows(P, N):
    """Row-strided `a`, `shortcut` and `out` (column halves of wider buffers): the dense call's bits, untouched columns stay zero."""
    M, K = 700, N
    p = _problem(M, N, K, 21 + N)
    image = P.ops.split_weight_image(p["w"])
    dense = _check(P, p, True, 0.5, f"strided N{N}")
    a_full = torch.zeros((M, 2 * K), device="cuda")
    a_full[:, K:] = p["a"]
    sc_full = torch.zeros((M, 2 * N), device="cuda")
    sc_full[:, :N] = p["sc"]
    out_full = torch.zeros((M, 2 * N), device="cuda")
    P.ops.linear_ln_residual_split(a_full[:, K:], image, N, p["b"], sc_full[:, :N], p["g"], p["be"], out=out_full[:, N:],
                                   branch_scale=0.5)
    assert torch.equal(out_full[:, N:], dense)
    assert float(out_full[:, :N].abs().max()) == 0.0


@pytest.mark.parametrize("N", [192, 384])
def test_tile_position_independence(P, N):
    """A row's result does not depend on where in a tile (or in which tile) it is computed."""
    p = _problem(1000, N, 400, 31 + N)
    image = P.ops.split_weight_image(p["w"])
    run = lambda sl: P.ops.linear_ln_residual_split(p["a"][sl], image, N, p["b"], p["sc"][sl], p["g"], p["be"], branch_scale=0.5)
    full = run(slice(0, 1000))
    assert torch.equal(full[:129], run(slice(0, 129)))
    assert torch.equal(full[999:], run(slice(999, 1000)))


@pytest.mark.parametrize("N", [192, 384])
def test_layernorm_edges(P, N):
    """Rows at the edges of the one-pass variance, the fp32-MFMA kernel's behaviour on the same inputs as the yardstick.
    Column 0 of W is 1, so a row c * e_0 of `a` has the product c in every column, exactly, in both kernels: the two results are
    then the same bits.  Rows with |mean| ~ 1e3 std lose about (1e3)^2 * 2^-24 of the variance to cancellation in either kernel:
    on 256 such rows the 1.5 x rule holds, the 2e-4 bound is not asked of them (the fp32 kernel misses it as well)."""
    M, K = 300, 64
    p = _problem(M, N, K, 41 + N)
    p["w"][:, 0] = 1.0
    a = p["a"]
    a[3] = 0.0
    a[3, 0] = 3.7                                             # constant product, not a power of two: E[y^2] - mean^2 rounds about 0
    a[40] = 0.0
    a[40, 0] = 0.5                                            # constant product with exact sums: variance exactly 0
    a[200] = 0.0                                              # all-zero row
    spread = (a[44:300] @ p["w"].t()).std(1)
    a[44:300, 0] = 1e3 * spread                               # |mean| ~ 1e3 std on rows 44 .. 299 (row 200 stays zero: spread 0)
    got, base = _both(P, p, bias=False, s=1.0)
    assert torch.isfinite(got).all()
    for r in (3, 40, 200):
        assert torch.equal(got[r], base[r]), r
    for r in (40, 200):                                       # variance 0, rstd = 1/sqrt(eps), y - mean = 0: out = shortcut + beta
        assert torch.equal(got[r], p["sc"][r] + p["be"]), r
    dev = ((got[3] - p["sc"][3] - p["be"]).abs().max()).item()
    print(f"N{N} constant row 3.7: |out - (shortcut + beta)| max {dev:.3e}")
    rows = torch.tensor([r for r in range(44, 300) if r != 200], device="cuda")
    _check(P, p, False, 1.0, f"N{N} mean >> spread", rows=rows, tight=False)
    rest = torch.tensor([r for r in range(0, 44) if r not in (3, 40)], device="cuda")
    _check(P, p, False, 1.0, f"N{N} ordinary rows beside them", rows=rest)


@pytest.mark.parametrize("N", [192, 384])
def test_non_finite_rows(P, N):
    """Inf / NaN / -Inf in three rows of `a` (different 32-row groups, different tiles): those output rows are non-finite, every
    other row keeps the bits of the clean run."""
    M, K = 400, 192
    p = _problem(M, N, K, 51 + N)
    clean, _ = _both(P, p)
    bad = dict(p, a=p["a"].clone())
    bad["a"][7, 5], bad["a"][170, 191], bad["a"][326, 0] = float("inf"), float("nan"), float("-inf")
    got, _ = _both(P, bad)
    rows = torch.tensor([7, 170, 326], device="cuda")
    assert not torch.isfinite(got[rows]).any()
    keep = torch.ones(M, dtype=torch.bool, device="cuda")
    keep[rows] = False
    assert torch.equal(got[keep], clean[keep]) and torch.isfinite(clean).all()


@pytest.mark.parametrize("M,N,K", [(129, 192, 192), (1000, 384, 400)])
def test_wide_dynamic_range(P, M, N, K):
    """Operands mixing magnitudes 2^-20 .. 2^20 within a row."""
    g = torch.Generator(device="cuda").manual_seed(5)
    mag = lambda shape: torch.exp2(torch.randint(-20, 21, shape, generator=g, device="cuda").float())
    p = _problem(M, N, K, 61 + N)
    p["a"] = torch.randn((M, K), generator=g, device="cuda") * mag((M, K))
    p["w"] = torch.randn((N, K), generator=g, device="cuda") * mag((N, K))
    _check(P, p, True, 1.0, f"wide M{M} N{N} K{K}")


def test_dispatch(P, monkeypatch):
    """What a block's fused projection does (fused._ln_proj): the switch off gives ops.linear_ln_residual's bits; a served layer
    takes the split op from the cached image; a weight edited in place gets a new image; a LoRA layer computes on the image of its
    merged weight; use_split_projections(False) on a model drops the images and selects the fp32 kernels."""
    torch.manual_seed(6)
    on, off = types.SimpleNamespace(split_projections=True), types.SimpleNamespace(split_projections=False)
    x, sc = torch.randn(300, 768, device="cuda"), torch.randn(300, 192, device="cuda")
    norm = torch.nn.LayerNorm(192, device="cuda")
    with torch.no_grad():
        norm.weight.normal_(1.0, 0.3)
        norm.bias.normal_(0.0, 0.3)
        lin = torch.nn.Linear(768, 192, device="cuda")
        f32 = lambda w, b, **kw: P.ops.linear_ln_residual(x, w, b, sc, norm.weight, norm.bias, **kw)
        split = lambda im, b, **kw: P.ops.linear_ln_residual_split(x, im, 192, b, sc, norm.weight, norm.bias, **kw)
        assert torch.equal(P.fused._ln_proj(off, lin, x, sc, norm, branch_scale=0.5), f32(lin.weight, lin.bias, branch_scale=0.5))
        image = P.ops.split_image(lin, lin.weight)
        assert image is not None and P.ops.split_image(lin, lin.weight) is image
        y = P.fused._ln_proj(on, lin, x, sc, norm, branch_scale=0.5)
        assert torch.equal(y, split(image, lin.bias, branch_scale=0.5)) and P.ops.split_image(lin, lin.weight) is image
        assert not torch.equal(y, f32(lin.weight, lin.bias, branch_scale=0.5))
        out = torch.zeros_like(sc)
        assert P.fused._ln_proj(on, lin, x, sc, norm, out=out, branch_scale=0.5) is out and torch.equal(out, y)
        # a shape fused.py keeps on the fp32-MFMA kernel gets no image; taken off the list it takes the split op
        lin_nd, x_nd, sc_nd = torch.nn.Linear(192, 192, device="cuda"), torch.randn(130, 192, device="cuda"), torch.randn(130, 192, device="cuda")
        with monkeypatch.context() as mp:
            mp.setattr(P.fused, "_SPLIT_NOT_DISPATCHED", {(192, 192)})
            assert torch.equal(P.fused._ln_proj(on, lin_nd, x_nd, sc_nd, norm),
                               P.ops.linear_ln_residual(x_nd, lin_nd.weight, lin_nd.bias, sc_nd, norm.weight, norm.bias))
            assert lin_nd not in P.ops._split_images
        assert (192, 192) not in P.fused._SPLIT_NOT_DISPATCHED
        assert torch.equal(P.fused._ln_proj(on, lin_nd, x_nd, sc_nd, norm),
                           P.ops.linear_ln_residual_split(x_nd, P.ops.split_weight_image(lin_nd.weight), 192, lin_nd.bias, sc_nd,
                                                          norm.weight, norm.bias))
        assert lin_nd in P.ops._split_images
        # LoRA: B = 0 gives the base layer's bits; after an adapter update the bits of the image of W_eff
        lora = P.layers.LoraLinear.from_linear(lin, 4, 4)
        assert torch.equal(P.fused._ln_proj(on, lora, x, sc, norm), P.fused._ln_proj(on, lin, x, sc, norm))
        for _ in range(2):
            lora.lora_B.normal_()
            w_eff = P.layers.eff_weight(lora)
            assert w_eff is not lora.weight
            assert torch.equal(P.fused._ln_proj(on, lora, x, sc, norm), split(P.ops.split_weight_image(w_eff), lora.bias))
            assert torch.equal(P.fused._ln_proj(off, lora, x, sc, norm), f32(w_eff, lora.bias))
        # a weight edited in place
        stamp = P.ops.param_stamp(lin.weight)
        lin.weight.copy_(torch.randn_like(lin.weight) / 768 ** 0.5)
        assert P.ops.param_stamp(lin.weight) != stamp
        image2 = P.ops.split_image(lin, lin.weight)
        assert image2 is not image and torch.equal(image2, P.ops.split_weight_image(lin.weight))
        assert torch.equal(P.fused._ln_proj(on, lin, x, sc, norm), split(image2, lin.bias))
        # a model
        m = P.PanguModel(depths=[1, 1, 1, 1], device="cuda").cuda().eval()
        blk = next(b for b in m.modules() if isinstance(b, P.layers.EarthSpecificBlock))
        C = blk.norm1.weight.shape[0]
        lin2 = blk.linear.linear2
        h, s2 = torch.randn(200, 4 * C, device="cuda"), torch.randn(200, C, device="cuda")
        assert blk.split_projections
        y_on = P.fused._ln_proj(blk, lin2, h, s2, blk.norm2)
        assert lin2 in P.ops._split_images
        assert torch.equal(y_on, P.ops.linear_ln_residual_split(h, P.ops.split_weight_image(lin2.weight), C, lin2.bias, s2,
                                                                 blk.norm2.weight, blk.norm2.bias))
        m.use_split_projections(False)
        assert not blk.split_projections and lin2 not in P.ops._split_images
        y_off = P.fused._ln_proj(blk, lin2, h, s2, blk.norm2)
        assert lin2 not in P.ops._split_images
        assert torch.equal(y_off, P.ops.linear_ln_residual(h, lin2.weight, lin2.bias, s2, blk.norm2.weight, blk.norm2.bias))


@pytest.mark.parametrize("C", [384, 192])
def test_one_block_on_vs_off(P, golden_dir, C):
    """One block in eval mode at (Z, H, W) = (8, 91, 24) / (8, 181, 24), every dispatched projection split against the switch off:
    both arms within the existing bound against the reference's golden output, and not the same bits."""
    roll = True
    st = cases.STAGES[C]
    blk = P.layers.EarthSpecificBlock(C, 0.1, st["heads"], device="cuda").cuda().eval()
    pre = cases.block_prefix(C, roll)
    blk.load_state_dict({k: synth.synth_param(pre + k, s, "cuda") for k, s in cases.block_param_shapes(C).items()})
    x = cases.block_input(C, 24, "cuda")
    g = np.load(os.path.join(golden_dir, f"block_{C}_{int(roll)}.npz"))
    with torch.no_grad():
        assert blk.split_projections
        y_split = blk(x, st["Z"], st["H"], 24, roll)
        assert blk.linear.linear2 in P.ops._split_images
        assert (blk.attention.linear2 in P.ops._split_images) == ((C, C) not in P.fused._SPLIT_NOT_DISPATCHED)
        blk.split_projections = False
        y_f32 = blk(x, st["Z"], st["H"], 24, roll)
    diff = ((y_split - y_f32).abs().max() / y_f32.abs().max()).item()
    print(f"block C{C} split vs fp32 kernels: {diff:.3e}")
    assert not torch.equal(y_split, y_f32)
    for y in (y_split, y_f32):
        assert cases.compare_summary(y, g, f"block_{C}_{int(roll)}.out", 1e-3) < 2e-4
