#!/usr/bin/env python3
"""Error (and, with --time, kernel time) of the exact-split fp32 projection against the fp32-MFMA kernel on one MI355X:
rel-L2 and max-abs / max error of both against an fp64 product of the same fp32 inputs, as a markdown table.

  python tools/split_error.py [--time] > profiles/f32_split_error.md
  python tools/split_error.py --ln [--time] > profiles/f32_split_ln_error.md      (the fused projection + LayerNorm + residual)

Shapes: the cases of tests/test_gpu_parity.py::test_linear, the generator of ::test_linear_random_shapes, and the four plain
projections of the model at M = 4096.  A shape the split kernel does not serve is listed as such.  --ln: the cases of
tests/test_gpu_linear_ln_split.py::test_parity_against_fp64 and ::test_wide_dynamic_range, and the four fused projections of the
model at M = 4096, against the fp64 value of shortcut + s * LN(a W^T + b).

  python tools/split_error.py --attn > profiles/attn_f32_split_error.md       (the window-attention core)
--attn: the cases of tests/test_gpu_attn_split.py (six geometries, unshifted / shifted, and the peaked shifted inputs) at five seeds
each, fp32-MFMA kernel and exact-split kernel against the oracle evaluated in fp64.

  python tools/split_error.py --resample                                      (the projections outside the blocks)
--resample: down-sampling, the two of up-sampling, patch embedding and patch recovery (upper air and surface) at M = 4096, five
seeds each."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch  # noqa: E402
import synth  # noqa: E402
from pangu_pytorch_amd import ops  # noqa: E402

TEST_LINEAR = [
    (1000, 192, 192, 0, True), (4099, 576, 192, 0, True), (2048, 768, 192, 1, True), (777, 192, 768, 0, True),
    (1531, 1152, 384, 0, True), (513, 1536, 384, 1, True), (300, 384, 1536, 0, True), (999, 384, 768, 0, False),
    (1234, 160, 384, 0, True), (321, 64, 384, 0, True), (650, 192, 112, 0, True), (128, 128, 16, 0, False),
]
MODEL = [(4096, 576, 192, 0, "s0 qkv"), (4096, 768, 192, 1, "s0 mlp1+gelu"), (4096, 1152, 384, 0, "s1 qkv"),
         (4096, 1536, 384, 1, "s1 mlp1+gelu")]
FULL = [(521280, 576, 192, 0, "s0 qkv"), (521280, 768, 192, 1, "s0 mlp1+gelu"), (131040, 1152, 384, 0, "s1 qkv"),
        (131040, 1536, 384, 1, "s1 mlp1+gelu")]


def errors(got, ref):
    d = got.double() - ref
    return (d.norm() / ref.norm()).item(), (d.abs().max() / ref.abs().max()).item()


def measure(a, w, b, act):
    N, K = w.shape
    ref = a.double() @ w.double().t()
    if b is not None:
        ref = ref + b.double()
    if act:
        ref = torch.nn.functional.gelu(ref)
    f32 = errors(ops.linear(a, w, b, act=act), ref)      # (the split kernel serves every shape this one serves)
    return f32, errors(ops.linear_split(a, ops.split_weight_image(w), N, b, act=act), ref)


def row(tag, M, N, K, act, bias, f32, split):
    head = f"| {tag} | {M}x{N}x{K} | {'gelu' if act else 'none'} | {'yes' if bias else 'no'} | {f32[0]:.3e} / {f32[1]:.3e} |"
    return head + f" {split[0]:.3e} / {split[1]:.3e} | {split[0] / f32[0]:.3f} |"


def timeit(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


LN_MODEL = [(4096, 192, 192, "s0 proj"), (4096, 192, 768, "s0 mlp2"), (4096, 384, 384, "s1 proj"), (4096, 384, 1536, "s1 mlp2")]
LN_FULL = [(521280, 192, 192, "s0 proj"), (521280, 192, 768, "s0 mlp2"), (131040, 384, 384, "s1 proj"), (131040, 384, 1536, "s1 mlp2")]


def ln_problem(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=g, device="cuda")
    return r(M, K), r(N, K) / K ** 0.5, r(N), 1.5 * r(M, N), 1.0 + 0.5 * r(N), 0.3 * r(N)


def ln_measure(a, w, b, sc, g, be, s):
    N = w.shape[0]
    y = a.double() @ w.double().t()
    if b is not None:
        y = y + b.double()
    ref = sc.double() + s * torch.nn.functional.layer_norm(y, (N,), g.double(), be.double(), 1e-5)
    f32 = errors(ops.linear_ln_residual(a, w, b, sc, g, be, branch_scale=s), ref)
    return f32, errors(ops.linear_ln_residual_split(a, ops.split_weight_image(w), N, b, sc, g, be, branch_scale=s), ref)


def main_ln():
    print("# Exact-split fused projection + LayerNorm + residual: error against fp64\n")
    print("rel-L2 / (max-abs / max) of `pangu_linear_ln_residual_fwd` (fp32 MFMA) and `pangu_linear_ln_residual_fwd_split` (six bf16 "
          "MFMA terms, one accumulator, the same epilogue) against the fp64 value of shortcut + s * LN(a W^T + b) on the same fp32 "
          "inputs; ratio = split rel-L2 / fp32 rel-L2.  Made by `tools/split_error.py --ln`.\n")
    print("| set | MxNxK | s | bias | fp32 MFMA | split | ratio |")
    print("|---|---|---|---|---|---|---|")
    worst, worst_l2, worst_max = 0.0, 0.0, 0.0

    def one(tag, M, N, K, bias, s, prob):
        nonlocal worst, worst_l2, worst_max
        a, w, b, sc, g, be = prob
        f32, split = ln_measure(a, w, b if bias else None, sc, g, be, s)
        print(f"| {tag} | {M}x{N}x{K} | {s} | {'yes' if bias else 'no'} | {f32[0]:.3e} / {f32[1]:.3e} | {split[0]:.3e} / {split[1]:.3e} "
              f"| {split[0] / f32[0]:.3f} |")
        worst, worst_l2, worst_max = max(worst, split[0] / f32[0]), max(worst_l2, split[0]), max(worst_max, split[1])

    for M in (1, 127, 129, 1000):
        for N in (192, 384):
            for K in (16, 32, 48, 64, 400):
                prob = ln_problem(M, N, K, 1000 * M + N + K)
                for bias in (True, False):
                    for s in (1.0, 0.5):
                        one("parity", M, N, K, bias, s, prob)
    for M, N, K in [(129, 192, 192), (1000, 384, 400)]:
        gen = torch.Generator(device="cuda").manual_seed(5)
        mag = lambda shape: torch.exp2(torch.randint(-20, 21, shape, generator=gen, device="cuda").float())
        prob = list(ln_problem(M, N, K, 61 + N))
        prob[0] = torch.randn((M, K), generator=gen, device="cuda") * mag((M, K))
        prob[1] = torch.randn((N, K), generator=gen, device="cuda") * mag((N, K))
        one("wide range", M, N, K, True, 1.0, prob)
    for M, N, K, name in LN_MODEL:
        one(name, M, N, K, True, 1.0, ln_problem(M, N, K, 11 + K))
    print(f"\nWorst ratio {worst:.3f} (required <= 1.5); worst split rel-L2 {worst_l2:.3e}; worst split max-abs / max "
          f"{worst_max:.3e} (required < 2e-4).")
    if "--time" in sys.argv:
        print("\n## Kernel time at the model's shapes (HIP events, 10 launches)\n")
        print("| projection | MxNxK | fp32 MFMA ms | split ms | speed-up | split TFLOP/s |")
        print("|---|---|---|---|---|---|")
        for M, N, K, name in LN_FULL:
            a, w, b, sc, g, be = ln_problem(M, N, K, 3)
            out = torch.empty(M, N, device="cuda")
            image = ops.split_weight_image(w)
            t0 = timeit(lambda: ops.linear_ln_residual(a, w, b, sc, g, be, out=out))
            t1 = timeit(lambda: ops.linear_ln_residual_split(a, image, N, b, sc, g, be, out=out))
            print(f"| {name} | {M}x{N}x{K} | {t0:.3f} | {t1:.3f} | {t0 / t1:.2f}x | {2.0 * M * N * K / t1 / 1e9:.0f} |")


ATTN_GEOMS = [(2, 1, 12, 1), (4, 7, 24, 2), (2, 13, 36, 5), (6, 19, 12, 3), (8, 181, 24, 6), (8, 91, 24, 12)]


def main_attn():
    import pangu_oracle as O
    print("# Exact-split window attention: error against the oracle in fp64\n")
    print("rel-L2 / max-abs of `pangu_window_attn_fwd` (fp32 MFMA) and `pangu_window_attn_fwd_split` (six bf16 MFMA terms per "
          "product, one accumulator) against `oracle/pangu_oracle.py::window_attention_core` in fp64 on the same fp32 inputs: the "
          "cases of tests/test_gpu_attn_split.py (amp 1.5: test_error_no_worse_than_fp32_mfma_kernel; amp 9.0, shifted: "
          "test_peaked_and_masked_rows) at five seeds.  Ratios = split / fp32 MFMA.  Made by `tools/split_error.py --attn`.\n")
    print("| (Z, H, W, heads) | shifted | amp | seed | fp32 MFMA | split | rel-L2 ratio | max-abs ratio |")
    print("|---|---|---|---|---|---|---|---|")
    r_l2, r_max = [], []
    for Z, H, W, heads in ATTN_GEOMS:
        C, N, types = 32 * heads, Z * H * W, (Z // 2) * ((H + 5) // 6)
        for shifted, amp in ((False, 1.5), (True, 1.5), (True, 9.0)):
            for seed in (91, 191, 291, 391, 491):
                qkv, b1 = synth.uniform((1, N, 3 * C), seed, amp), synth.uniform((3 * C,), seed + 1, amp / 3.0)
                esb = synth.uniform((1, types, heads, 144, 144), seed + 2, 0.5)
                ref = O.window_attention_core(qkv.double(), b1.double(), esb.double(), Z, H, W, heads, shifted)[0][0]
                dev = (qkv[0].cuda(), b1.cuda(), esb[0].cuda())
                e = []
                for split in (False, True):
                    d = ops.window_attention(*dev, Z, H, W, heads, shifted, split=split).double().cpu() - ref
                    e.append(((d.norm() / ref.norm()).item(), d.abs().max().item()))
                r_l2.append(e[1][0] / e[0][0])
                r_max.append(e[1][1] / e[0][1])
                print(f"| {(Z, H, W, heads)} | {int(shifted)} | {amp} | {seed} | {e[0][0]:.3e} / {e[0][1]:.3e} | {e[1][0]:.3e} / "
                      f"{e[1][1]:.3e} | {r_l2[-1]:.3f} | {r_max[-1]:.3f} |")
    print(f"\nrel-L2 ratio: min {min(r_l2):.3f}, median {sorted(r_l2)[len(r_l2) // 2]:.3f}, max {max(r_l2):.3f}; "
          f"max-abs ratio: min {min(r_max):.3f}, median {sorted(r_max)[len(r_max) // 2]:.3f}, max {max(r_max):.3f} "
          f"({len(r_l2)} cases).")


RESAMPLE = [(4096, 384, 768, False, "down"), (4096, 768, 384, False, "up1"), (4096, 160, 384, True, "recover"),
            (4096, 192, 192, False, "up2"), (4096, 192, 192, True, "embed"), (4096, 192, 112, True, "embed surf"),
            (4096, 64, 384, True, "recover surf")]


def main_resample():
    print("# Exact-split projection at the shapes outside the blocks: error against an fp64 product\n")
    print("rel-L2 / (max-abs / max) of `pangu_linear_fwd` (fp32 MFMA) and `pangu_linear_fwd_split` on the same fp32 inputs, "
          "five seeds per shape; ratio = split rel-L2 / fp32 rel-L2.  Made by `tools/split_error.py --resample`.\n")
    print("| projection | MxNxK | bias | seed | fp32 MFMA | split | ratio |")
    print("|---|---|---|---|---|---|---|")
    worst, worst_abs = 0.0, 0.0
    for M, N, K, bias, name in RESAMPLE:
        for seed in range(5):
            g = torch.Generator(device="cuda").manual_seed(100 * seed + N + K)
            a = torch.randn((M, K), generator=g, device="cuda")
            w = torch.randn((N, K), generator=g, device="cuda") / K ** 0.5
            b = torch.randn((N,), generator=g, device="cuda") if bias else None
            ref = a.double() @ w.double().t()
            if bias:
                ref = ref + b.double()
            f32 = errors(ops.linear(a, w, b), ref)
            split = errors(ops.linear_split(a, ops.split_weight_image(w), N, b), ref)
            print(f"| {name} | {M}x{N}x{K} | {'yes' if bias else 'no'} | {seed} | {f32[0]:.3e} / {f32[1]:.3e} | {split[0]:.3e} / "
                  f"{split[1]:.3e} | {split[0] / f32[0]:.3f} |")
            worst, worst_abs = max(worst, split[0] / f32[0]), max(worst_abs, split[0])
    print(f"\nWorst ratio {worst:.3f} (required <= 1.5); worst split rel-L2 {worst_abs:.3e} (required < 2e-6).")


def main():
    if "--resample" in sys.argv:
        return main_resample()
    if "--ln" in sys.argv:
        return main_ln()
    if "--attn" in sys.argv:
        return main_attn()
    print("# Exact-split fp32 projection: error against an fp64 product\n")
    print("rel-L2 / (max-abs / max) of `pangu_linear_fwd` (fp32 MFMA) and `pangu_linear_fwd_split` (six bf16 MFMA terms, one "
          "accumulator) on the same fp32 inputs; ratio = split rel-L2 / fp32 rel-L2.  Made by `tools/split_error.py`.\n")
    print("| set | MxNxK | act | bias | fp32 MFMA | split | ratio |")
    print("|---|---|---|---|---|---|---|")
    worst = 0.0
    worst_abs = 0.0
    for M, N, K, act, bias in TEST_LINEAR:
        a = synth.uniform((M, K), 11).cuda()
        w = synth.uniform((N, K), 12, 1.0 / K ** 0.5).cuda()
        b = synth.uniform((N,), 13, 0.5).cuda() if bias else None
        f32, split = measure(a, w, b, act)
        print(row("test_linear", M, N, K, act, bias, f32, split))
        if split:
            worst, worst_abs = max(worst, split[0] / f32[0]), max(worst_abs, split[0])
    rnd = random.Random(7)
    torch.manual_seed(7)
    for _ in range(40):
        N = rnd.choice([160, 192, 384, 576, 768, 1152, 1536, 132, 176, 64])
        K = 16 * rnd.randint(1, 100)
        M = rnd.randint(1, 3000)
        act = rnd.choice([0, 0, 1, 3])
        a = torch.randn(M, K, device="cuda")
        w = torch.randn(N, K, device="cuda") / K ** 0.5
        b = torch.randn(N, device="cuda") if rnd.random() < 0.7 else None
        if act == 3:
            torch.randn(M, N, device="cuda")          # (keeps the generator's random stream; the split kernel has no ADD epilogue)
            act = 0
        f32, split = measure(a, w, b, act)
        print(row("random_shapes", M, N, K, act, b is not None, f32, split))
        if split:
            worst, worst_abs = max(worst, split[0] / f32[0]), max(worst_abs, split[0])
    torch.manual_seed(11)
    for M, N, K, act, name in MODEL:
        a = torch.randn(M, K, device="cuda")
        w = torch.randn(N, K, device="cuda") / K ** 0.5
        b = torch.randn(N, device="cuda")
        f32, split = measure(a, w, b, act)
        print(row(name, M, N, K, act, True, f32, split))
        worst, worst_abs = max(worst, split[0] / f32[0]), max(worst_abs, split[0])
    print(f"\nWorst ratio {worst:.3f} (required <= 1.5); worst split rel-L2 {worst_abs:.3e} (required < 2e-6).")
    if "--time" in sys.argv:
        print("\n## Kernel time at the model's shapes (HIP events, 10 launches)\n")
        print("| projection | MxNxK | fp32 MFMA ms | split ms | speed-up | split TFLOP/s |")
        print("|---|---|---|---|---|---|")
        for M, N, K, act, name in FULL:
            a = torch.randn(M, K, device="cuda")
            w = torch.randn(N, K, device="cuda") / K ** 0.5
            b = torch.randn(N, device="cuda")
            out = torch.empty(M, N, device="cuda")
            image = ops.split_weight_image(w)
            t0 = timeit(lambda: ops.linear(a, w, b, act=act, out=out))
            t1 = timeit(lambda: ops.linear_split(a, image, N, b, act=act, out=out))
            print(f"| {name} | {M}x{N}x{K} | {t0:.3f} | {t1:.3f} | {t0 / t1:.2f}x | {2.0 * M * N * K / t1 / 1e9:.0f} |")


if __name__ == "__main__":
    main()
