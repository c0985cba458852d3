#!/usr/bin/env python3
"""SHA-256 of everything the bf16 GEMM entry points write (ops_bf16.linear, linear_gelu_bwd, linear_ln_residual) over a fixed
list of small cases, as JSON: two builds of the library compute the same bits iff the two outputs are equal.

  PANGU_HIP_LIB=<other build>/libpangu_hip.so python tools/gemm_bf16_fingerprint.py > a.json
  python tools/gemm_bf16_fingerprint.py > b.json && cmp a.json b.json
(per case the first 64 bits of its digest, and one SHA-256 over all the full digests)

The list walks every dispatch arm of csrc/gemm_bf16.hip, gemm_ws_bf16.hip and gemm_ln_bf16.hip and the edges of each tiling (row
cuts inside a wave, between waves, in the second tile; ragged last column tile; one to three K-steps; a part-empty K-step).  The
main output goes into a poisoned buffer with PAD_ROWS rows behind M and, where it is strided, a right half; so does the GELU
pre-activation `aux`.  tests/test_gpu_bf16_fingerprint.py holds the list against the digests recorded from the parent of the
shared-header layout (profiles/gemm_bf16_shared_fingerprint_parent.json).

Inputs are closed-form (oracle/synth.py seeds); needs an MI355X."""
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_f32_fingerprint as F32  # noqa: E402  (puts the repository and oracle/ on sys.path)
import torch  # noqa: E402
from pangu_pytorch_amd import ops, ops_bf16  # noqa: E402

PAD_ROWS = 3                    # rows behind M of an output buffer: never written
POISON = -1.2345e30
ACT_NAMES = {ops.ACT_NONE: "none", ops.ACT_GELU: "gelu+aux", ops.ACT_GELU_BWD: "gelu_bwd", ops.ACT_ADD: "add"}

MS = (1, 63, 64, 65, 127, 128, 129, 200)            # cuts inside wave row 0, between the wave rows, in the second tile
NS = (64, 128, 136, 160, 192, 576)                  # TN = 1, 2, 1, 3, 3, 3; 136 and 160 end in a ragged column tile
RING_KS = (32, 64, 96)                              # the LDS-DMA ring kernel (K % 32 == 0, K < 1024): one, two, three steps
STAGED_KS = (8, 40, 72)                             # the register-staged kernel: a part-empty K-step of 64
STAGED_FROM = 1024                                  # K from which the register-staged kernel takes the multiples of 32 too
WS_MS, WS_NS, WS_KS = (4096, 4099, 4353), (160, 192, 576), (32, 96, 192)      # weights-stationary arm: M >= 4096, K <= 192
LN_MS = (1, 63, 65, 128, 129, 257, 300)
LN_KS = {192: (40, 64, 192, 416, 384, 448),         # register-staged x3 | ring of three | 256-row tiles, K-steps of 64, x2
         384: (40, 64, 96, 160, 192, 256)}          # register-staged x2 | ring of three x2 | K-steps of 64 x2
LN_PERSISTENT = ((192, 416), (192, 384), (384, 96), (384, 192))      # one (N, K) per persistent launch arm
LN_LONG_M = 65793                                   # 515 tiles of 128 rows / 257 of 256: more tiles than workgroups on all four arms


t = F32.t


def digest(*tensors):
    """F32.digest of the raw bits (numpy has no bfloat16)."""
    return F32.digest(*[x.view(torch.int16) if x.dtype == torch.bfloat16 else x for x in tensors])


def _options():
    """(act, bias, fp32 output, strided) the plain entry allows: GELU_BWD has no bias; GELU_BWD and ADD are bf16 only."""
    out = []
    for act, bias, f32, strided in itertools.product(ACT_NAMES, (1, 0), (0, 1), (0, 1)):
        if act in (ops.ACT_GELU_BWD, ops.ACT_ADD) and f32:
            continue
        if act == ops.ACT_GELU_BWD and bias:
            continue
        out.append((act, bias, f32, strided))
    return out


def cases():
    """(entry, M, N, K, strided, bias, act, fp32 output | with h): strided = row-strided A (lda = K + 8) and, where the entry takes
    an output, a strided output (the left half of a 2N buffer)."""
    out = []
    # every row / column / K edge of both plain kernels, plain epilogue
    for M, N, K in itertools.product(MS, NS, RING_KS + STAGED_KS):
        out.append(("linear", M, N, K, 0, 1, ops.ACT_NONE, 0))
    # every epilogue switch on both kernels at every TN, with a full first and a cut second row tile
    for N, K in itertools.product(NS, (32, 40)):
        out += [("linear", 129, N, K, s, b, act, f32) for act, b, f32, s in _options() if (s, b, act, f32) != (0, 1, ops.ACT_NONE, 0)]
    for N in (64, 128, 576):                                # TN = 1, 2, 3 of the register-staged kernel at its threshold
        out.append(("linear", 1, N, STAGED_FROM, 0, 1, ops.ACT_NONE, 0))
        out += [("linear", 129, N, STAGED_FROM, s, b, act, f32) for act, b, f32, s in _options()]
    for M, N, K in itertools.product(WS_MS, WS_NS, WS_KS):
        for act, bias in itertools.product((ops.ACT_NONE, ops.ACT_GELU), (1, 0)):
            out += [("linear", M, N, K, s, bias, act, 0) for s in ((0, 1) if (M, K) == (4099, 192) else (0,))]
    for C, M, strided, h in itertools.product((192, 384), (1, 129, 200), (0, 1), (1, 0)):
        out.append(("linear_gelu_bwd", M, 4 * C, C, strided, 0, ops.ACT_GELU_BWD, h))
    for N in (192, 384):
        for K, M, (bias, strided) in itertools.product(LN_KS[N], LN_MS, ((1, 0), (0, 1))):      # bias on / off, contiguous / strided
            out.append(("linear_ln_residual", M, N, K, strided, bias, ops.ACT_NONE, 0))
    out += [("linear_ln_residual", LN_LONG_M, N, K, 0, 1, ops.ACT_NONE, 0) for N, K in LN_PERSISTENT]
    return out


def key(case):
    fn, M, N, K, strided, bias, act, last = case
    tail = {"linear": f" {ACT_NAMES[act]} out={'f32' if last else 'bf16'}", "linear_gelu_bwd": f" h={last}", "linear_ln_residual": ""}[fn]
    return f"{fn} M={M} N={N} K={K} strided={strided} bias={bias}{tail}".replace("linear_ln_residual", "linear_ln")


def _poisoned(rows, cols, dtype):
    return torch.full((rows, cols), POISON, dtype=dtype, device="cuda")


def run(case, cache=None):
    """Run one case; returns [(buffer, view that the entry point wrote)] for every tensor it writes."""
    fn, M, N, K, strided, bias, act, last = case
    cache = {} if cache is None else cache

    def bf(name, *shape, scale=1.0, shift=0.0):
        k = (name, shape, scale, shift)
        if k not in cache:
            cache[k] = (t(name, *shape, scale=scale) + shift).to(torch.bfloat16 if name not in ("b", "gamma", "beta") else torch.float32)
        return cache[k]
    a = bf("a", M, K + 8 * strided)[:, :K]
    w = bf("w", N, K, scale=K ** -0.5)
    b = bf("b", N) if bias else None
    if fn == "linear_gelu_bwd":
        dpre, h = ops_bf16.linear_gelu_bwd(a, w, bf("aux", M, N), want_h=bool(last))
        return [(x, x) for x in (dpre, h) if x is not None]
    buf = _poisoned(M + PAD_ROWS, N * (1 + strided), torch.float32 if (fn == "linear" and last) else torch.bfloat16)
    view = buf[:M, :N]
    if fn == "linear_ln_residual":
        ops_bf16.linear_ln_residual(a, w, b, bf("sc", M, N), bf("gamma", N, scale=0.5, shift=1.0), bf("beta", N, scale=0.1), out=view)
        return [(buf, view)]
    if act == ops.ACT_GELU:                              # the pre-activation is written there
        xbuf = _poisoned(M + PAD_ROWS, N, torch.bfloat16)
        ops_bf16.linear(a, w, b, act=act, out=view, aux=xbuf[:M])
        return [(buf, view), (xbuf, xbuf[:M])]
    ops_bf16.linear(a, w, b, act=act, out=view, aux=bf("aux", M, N) if act != ops.ACT_NONE else None)
    return [(buf, view)]


def untouched(buf, view):
    """Every row and column of `buf` outside the written `view` still holds the poison."""
    M, N = view.shape
    p = torch.full((), POISON, dtype=buf.dtype, device=buf.device)
    return bool((buf[M:] == p).all()) and bool((buf[:M, N:] == p).all())


def record(digests):
    """What is kept of {key: SHA-256}: the first 64 bits per case (they name the case that moved) and the SHA-256 of all the
    full digests in key order (it moves with any of their bits)."""
    return {"all": hashlib.sha256("".join(digests[k] for k in sorted(digests)).encode()).hexdigest(),
            "cases": {k: digests[k][:16] for k in sorted(digests)}}


def main():
    cache = {}
    json.dump(record({key(c): digest(*[buf for buf, _ in run(c, cache)]) for c in cases()}), sys.stdout, indent=0)
    print()


if __name__ == "__main__":
    main()
