#!/usr/bin/env python3
"""SHA-256 of the outputs of the fp32 GEMM entry points (ops.linear, linear_split, linear_ln_residual, linear_ln_residual_split)
over a fixed list of small cases, as JSON: two builds of the library compute the same bits iff the two outputs are equal.

  PANGU_HIP_LIB=<other build>/libpangu_hip.so python tools/gemm_f32_fingerprint.py > a.json
  python tools/gemm_f32_fingerprint.py > b.json && cmp a.json b.json

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


def main():
    out = {}
    for M, N, K in itertools.product(MS, (160, 192, 384, 576), (16, 48, 400)):
        a, w, b, aux = t("a", M, K), t("w", N, K, scale=K ** -0.5), t("b", N), t("aux", M, N)
        for act, bias in itertools.product(ACT_NAMES, (b, None)):
            x = aux.clone() if act != ops.ACT_NONE else None      # GELU writes the pre-activation there: hashed too
            y = ops.linear(a, w, bias, act=act, aux=x)
            out[f"linear M={M} N={N} K={K} {ACT_NAMES[act]} bias={int(bias is not None)}"] = digest(y, *([x] if x is not None else []))
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
            out["linear_ln_residual " + tag] = digest(ops.linear_ln_residual(a, w, bias, sc, g, be, branch_scale=scale))
            out["linear_ln_residual_split " + tag] = digest(ops.linear_ln_residual_split(a, img, N, bias, sc, g, be, branch_scale=scale))
    json.dump(out, sys.stdout, indent=0, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
