#!/usr/bin/env python3
"""SHA-256 of the outputs of the fp32 GEMM entry points (ops.linear, linear_split, linear_ln_residual, linear_ln_residual_split)
over a fixed list of small cases, as JSON: two builds of the library compute the same bits iff the two outputs are equal.

  PANGU_HIP_LIB=<other build>/libpangu_hip.so python tools/gemm_f32_fingerprint.py > a.json
  python tools/gemm_f32_fingerprint.py > b.json && cmp a.json b.json

`--edges` prints instead the digests of the exact-split entry points over `edge_cases()`: the shapes at the edges of the wave
tiling (row cuts inside a wave, between waves, in the second tile; one to four k-steps), row-strided operands, every epilogue
switch.  tests/test_gpu_split_fingerprint.py holds both lists against the digests recorded from the parent of the row-owning tiling.

Inputs are closed-form (oracle/synth.py seeds); needs an MI355X."""
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import synth  # noqa: E402
from pangu_pytorch_amd import ops  # noqa: E402

MS = (1, 129, 1000)
ACT_NAMES = {ops.ACT_NONE: "none", ops.ACT_GELU: "gelu", ops.ACT_GELU_BWD: "gelu_bwd", ops.ACT_ADD: "add"}


def t(name, *shape, scale=1.0):
    return synth.uniform(shape, synth.name_seed("fingerprint." + name), scale=scale, device="cuda")


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for x in tensors:
        h.update(x.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


EDGE_MS = (1, 31, 32, 33, 96, 127, 128, 129, 200)      # cuts inside wave 0, between waves, inside the last wave, second tile
EDGE_KS = (16, 32, 48, 64)                              # one .. four k-steps: ring prologue only, ring exactly full, first wrap
EDGE_LONG_K = 1536                                      # the K from which the N = 384 LayerNorm entry takes row-owning waves
EDGE_PAD_ROWS = 3                                       # rows behind M of the output buffer: never written
EDGE_POISON = -1.2345e30


def edge_cases():
    """(entry point, M, N, K, strided, bias, act | branch_scale): strided = row-strided A (lda = K + 8) and output (ldc = 2 N,
    the left half of a concat buffer)."""
    cases = []
    for M, N, K, strided, bias in itertools.product(EDGE_MS, (192, 384, 576), EDGE_KS, (0, 1), (1, 0)):
        cases += [("linear_split", M, N, K, strided, bias, act) for act in (ops.ACT_NONE, ops.ACT_GELU)]
    for M, N, K, strided, bias in itertools.product(EDGE_MS, (192, 384), EDGE_KS + (EDGE_LONG_K,), (0, 1), (1, 0)):
        cases += [("linear_ln_residual_split", M, N, K, strided, bias, scale) for scale in (1.0, 0.5)]
    return cases


def edge_key(case):
    fn, M, N, K, strided, bias, last = case
    tail = ACT_NAMES[last] if fn == "linear_split" else f"branch_scale={last}"
    return f"{fn} M={M} N={N} K={K} strided={strided} bias={bias} {tail}"


def edge_run(case, cache=None):
    """Run one edge case into a poisoned buffer of M + EDGE_PAD_ROWS rows; returns (buffer, view that was written)."""
    fn, M, N, K, strided, bias, last = case
    cache = {} if cache is None else cache

    def cached(name, *shape, scale=1.0):
        k = (name, shape, scale)
        if k not in cache:
            cache[k] = t(name, *shape, scale=scale)
        return cache[k]
    a = cached("a", M, K + 8 * strided)[:, :K]
    if ("img", N, K) not in cache:
        cache["img", N, K] = ops.split_weight_image(cached("w", N, K, scale=K ** -0.5))
    img, b = cache["img", N, K], cached("b", N) if bias else None
    buf = torch.full((M + EDGE_PAD_ROWS, N * (1 + strided)), EDGE_POISON, device="cuda")
    view = buf[:M, :N]
    if fn == "linear_split":
        ops.linear_split(a, img, N, b, act=last, out=view)
    else:
        g, be = cached("gamma", N, scale=0.5) + 1.0, cached("beta", N, scale=0.1)
        ops.linear_ln_residual_split(a, img, N, b, cached("sc", M, N), g, be, out=view, branch_scale=last)
    return buf, view


def edges():
    cache = {}
    return {edge_key(c): digest(edge_run(c, cache)[0]) for c in edge_cases()}


def split_cases(out, fp32_mfma_too=False):
    """The exact-split entries of the main list (and, beside them, the fp32-MFMA LayerNorm entries on the same inputs)."""
    for M, N, K in itertools.product(MS, (192, 384, 576), (16, 32, 48, 400)):
        a, w, b = t("a", M, K), t("w", N, K, scale=K ** -0.5), t("b", N)
        img = ops.split_weight_image(w)
        for act, bias in itertools.product((ops.ACT_NONE, ops.ACT_GELU), (b, None)):
            y = ops.linear_split(a, img, N, bias, act=act)
            out[f"linear_split M={M} N={N} K={K} {ACT_NAMES[act]} bias={int(bias is not None)}"] = digest(y)
    for M, N, K in itertools.product(MS, (192, 384), (16, 32, 48, 400)):
        a, w, b, sc = t("a", M, K), t("w", N, K, scale=K ** -0.5), t("b", N), t("sc", M, N)
        g, be = t("gamma", N, scale=0.5) + 1.0, t("beta", N, scale=0.1)
        img = ops.split_weight_image(w)
        for bias, scale in itertools.product((b, None), (1.0, 0.5)):
            tag = f"M={M} N={N} K={K} bias={int(bias is not None)} branch_scale={scale}"
            if fp32_mfma_too:
                out["linear_ln_residual " + tag] = digest(ops.linear_ln_residual(a, w, bias, sc, g, be, branch_scale=scale))
            out["linear_ln_residual_split " + tag] = digest(ops.linear_ln_residual_split(a, img, N, bias, sc, g, be, branch_scale=scale))
    return out


GUARDED_SHAPES = ((160, 384), (64, 384), (4, 16), (196, 48))      # (N, K), N % 192 != 0: the instantiation with the column guard


def guarded_cases(out):
    """linear_split where the last 192-column tile is cut (profiles/split_one_form_guarded_parent.json: the digests of the
    commit before the image got one form, taken through its column-padded entry)."""
    for M, (N, K) in itertools.product(MS, GUARDED_SHAPES):
        a, w, b = t("a", M, K), t("w", N, K, scale=K ** -0.5), t("b", N)
        img = ops.split_weight_image(w)
        for act, bias in itertools.product((ops.ACT_NONE, ops.ACT_GELU), (b, None)):
            y = ops.linear_split(a, img, N, bias, act=act)
            out[f"linear_split M={M} N={N} K={K} {ACT_NAMES[act]} bias={int(bias is not None)}"] = digest(y)
    return out


def main():
    if "--edges" in sys.argv:
        json.dump(edges(), sys.stdout, indent=0, sort_keys=True)
        print()
        return
    out = {}
    for M, N, K in itertools.product(MS, (160, 192, 384, 576), (16, 48, 400)):
        a, w, b, aux = t("a", M, K), t("w", N, K, scale=K ** -0.5), t("b", N), t("aux", M, N)
        for act, bias in itertools.product(ACT_NAMES, (b, None)):
            x = aux.clone() if act != ops.ACT_NONE else None      # GELU writes the pre-activation there: hashed too
            y = ops.linear(a, w, bias, act=act, aux=x)
            out[f"linear M={M} N={N} K={K} {ACT_NAMES[act]} bias={int(bias is not None)}"] = digest(y, *([x] if x is not None else []))
    split_cases(out, fp32_mfma_too=True)
    guarded_cases(out)
    json.dump(out, sys.stdout, indent=0, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
