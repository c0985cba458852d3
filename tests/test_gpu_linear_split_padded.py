"""The exact-split fp32 projection (csrc/gemm_f32_split.hip) at N % 192 != 0: any N % 4 == 0 on the 192-column tile, by an image
extended with zero rows and an epilogue that neither reads bias nor writes C at a column >= N.  Needs an MI355X: run with `-m gpu`.

The acceptance rule of the column guard is that it changes no product: the launch gives the bits of `linear_split` on the
zero-extended weight and bias (N % 192 == 0: the kernel without the guard).  The error rule is the one of tests/test_gpu_linear_split.py: against an fp64 product of the same
fp32 inputs, rel-L2 error <= min(1.5 x the error of ops.linear on the same inputs, 2e-6).  It is asserted at M = 300 (1200 outputs
at N = 4: the ratio of two rel-L2 errors needs a sample, and the bits at the other M are pinned to the unpadded kernel anyway)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
ABS_BOUND = 2e-6
E_SHAPE = -1
SHAPES = [(160, 384), (64, 384), (4, 16), (196, 48)]        # (N, K): recovery upper air / surface, one segment, two n-tiles
NAN_BITS = 0x7FC00123


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    P._lib.load()
    return P


def _problem(N, K, M, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn((M, K), generator=g, device="cuda")
    w = torch.randn((N, K), generator=g, device="cuda") / K ** 0.5
    b = torch.randn((N,), generator=g, device="cuda")
    return a, w, b


def _extended(P, w, b):
    """W and bias extended with zeros to the padded row count."""
    N, K = w.shape
    Np = P.ops.split_image_rows(N)
    w_ext = torch.zeros((Np, K), device="cuda")
    w_ext[:N] = w
    b_ext = torch.zeros((Np,), device="cuda")
    b_ext[:N] = b
    return Np, w_ext, b_ext


def _l2(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("N,K", SHAPES)
def test_padded_image_is_image_of_zero_extended_weight(P, N, K):
    """Byte for byte; in particular a zero row is +0 in all three planes."""
    _, w, b = _problem(N, K, 1, N + K)
    Np, w_ext, _ = _extended(P, w, b)
    assert Np == 192 * ((N + 191) // 192) == P.split_layout.image_rows(N)
    image = P.ops.split_weight_image(w)
    assert image is not None and image.dtype == torch.uint8 and image.numel() == 6 * Np * K
    assert torch.equal(image, P.ops.split_weight_image(w_ext))


@pytest.mark.parametrize("M", [1, 127, 129, 300])
def test_padded_launch_bits(P, M):
    """Every (N, K), act none / GELU, with and without bias: the first N columns of the unpadded kernel on the zero-extended
    operands, bit for bit."""
    for N, K in SHAPES:
        a, w, b = _problem(N, K, M, 7 * M + N)
        Np, w_ext, b_ext = _extended(P, w, b)
        image, image_ext = P.ops.split_weight_image(w), P.ops.split_weight_image(w_ext)
        for act in (P.ops.ACT_NONE, P.ops.ACT_GELU):
            for bias, bias_ext in ((None, None), (b, b_ext)):
                got = P.ops.linear_split(a, image, N, bias, act=act)
                want = P.ops.linear_split(a, image_ext, Np, bias_ext, act=act)
                assert got.shape == (M, N) and torch.equal(got, want[:, :N]), (M, N, K, act, bias is not None)


def test_padded_launch_matches_the_recorded_digests(P):
    """The bits of the commit before the image got one form, recorded through its column-padded entry
    (tools/gemm_f32_fingerprint.py guarded_cases, profiles/split_one_form_guarded_parent.json)."""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import gemm_f32_fingerprint as F
    with open(os.path.join(root, "profiles", "split_one_form_guarded_parent.json")) as f:
        want = json.load(f)
    assert tuple(F.GUARDED_SHAPES) == tuple(SHAPES) and len(want) == 3 * len(SHAPES) * 4
    got = F.guarded_cases({})
    assert set(got) == set(want) and [k for k in sorted(want) if got[k] != want[k]] == []


@pytest.mark.parametrize("N,K", SHAPES)
def test_padded_launch_stays_in_bounds(P, N, K):
    """`out` is a column slice of a wider buffer that also has rows behind M, `a` a row-strided view: every byte outside the
    M x N block keeps its NaN bit pattern, and the block is the dense call's."""
    M, rows, c0, ld = 129, 140, 8, N + 24
    a_full, w_full, b = _problem(N, 2 * K, M, 3 * N + K)
    a, w = a_full[:, K:], w_full[:, K:].contiguous()
    image = P.ops.split_weight_image(w)
    buf = torch.full((rows, ld), NAN_BITS, dtype=torch.int32, device="cuda")
    out = buf.view(torch.float32)[:M, c0:c0 + N]
    assert a.stride(0) == 2 * K and out.stride(0) == ld
    P.ops.linear_split(a, image, N, b, act=P.ops.ACT_GELU, out=out)
    dense = P.ops.linear_split(a.contiguous(), image, N, b, act=P.ops.ACT_GELU)
    assert torch.isfinite(dense).all() and torch.equal(out, dense)
    outside = torch.ones((rows, ld), dtype=torch.bool, device="cuda")
    outside[:M, c0:c0 + N] = False
    assert bool((buf[outside] == NAN_BITS).all())
    assert int(outside.sum()) == rows * ld - M * N


@pytest.mark.parametrize("N,K", SHAPES)
def test_padded_error_rule(P, N, K):
    a, w, b = _problem(N, K, 300, 11 * N + K)
    image = P.ops.split_weight_image(w)
    for act in (P.ops.ACT_NONE, P.ops.ACT_GELU):
        ref = a.double() @ w.double().t() + b.double()
        if act:
            ref = torch.nn.functional.gelu(ref)
        e_split = _l2(P.ops.linear_split(a, image, N, b, act=act), ref)
        e_f32 = _l2(P.ops.linear(a, w, b, act=act), ref)
        print(f"N{N} K{K} act{act}: split {e_split:.3e} fp32 {e_f32:.3e} ratio {e_split / max(e_f32, 1e-30):.3f}")
        assert e_split <= min(1.5 * e_f32, ABS_BOUND), (N, K, act, e_split, e_f32)


def test_padded_refusals(P):
    """N % 4 != 0 or K % 16 != 0: no image, PANGU_E_SHAPE from both C entries (nothing launched).  A 160-row layer is served from
    the module cache; its image handed over as that of a weight of another shape is refused."""
    lib = P._lib.load()
    s = torch.cuda.current_stream().cuda_stream
    scratch = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for N, K in ((6, 16), (161, 384), (160, 24), (4, 8)):
        w = torch.randn((N, K), device="cuda")
        assert P.ops.split_weight_image(w) is None
        a, out = torch.randn((8, K), device="cuda"), torch.zeros((8, N), device="cuda")
        assert lib.pangu_split_weight_bf16x3(s, w.data_ptr(), N, K, scratch.data_ptr()) == E_SHAPE
        assert lib.pangu_linear_fwd_split(s, a.data_ptr(), K, scratch.data_ptr(), None, out.data_ptr(), N, 8, N, K, 0) == E_SHAPE
        torch.cuda.synchronize()
        assert float(out.abs().max()) == 0.0 and int(scratch.max()) == 0
    lin160 = torch.nn.Linear(384, 160, device="cuda")
    image = P.ops.split_image(lin160, lin160.weight)
    assert image is not None and P.ops.split_image(lin160, lin160.weight) is image
    assert torch.equal(image, P.ops.split_weight_image(lin160.weight))
    with pytest.raises(RuntimeError):
        P.ops.linear_split(torch.randn(8, 384, device="cuda"), image, 196, None)      # the image of another (N, K)
