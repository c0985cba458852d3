#!/usr/bin/env python3
"""LoRA measurements (LoRA section):

  python tools/bench_lora.py [--steps 5] [--warmup 2] [--rank 16] [--skip-train]

1. `ops.lora_wgrad` per (K -> N) projection of the model at its real token count, against its roof
   max(bytes / 6.29 TB/s, FLOPs / 157.3 TF/s), bytes = 4 M (K + N), FLOPs = 4 M r (K + N).
2. In one process, same seeded batch, DropPath off, alternating: the fp32 `train.train_step` of the full fine-tune against the
   LoRA fine-tune (enable_lora(r)), ms/step for both, their ratio, and the peak memory of each.
Prints one JSON line per section."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM, MFMA = 6.29e12, 157.3e12
SHAPES = [(192, 576, 521280), (192, 192, 521280), (192, 768, 521280), (768, 192, 521280),
          (384, 1152, 131040), (384, 384, 131040), (384, 1536, 131040), (1536, 384, 131040),
          (768, 384, 131040), (384, 768, 131040)]


def kernels(P, r, reps=20):
    rows = []
    for K, N, M in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(K + N)
        x = torch.randn(M, K, device="cuda", generator=g)
        dy = torch.randn(M, N, device="cuda", generator=g)
        A = torch.randn(r, K, device="cuda", generator=g) * 0.1
        B = torch.randn(N, r, device="cuda", generator=g) * 0.1
        for _ in range(3):
            P.ops.lora_wgrad(dy, x, A, B, 1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            P.ops.lora_wgrad(dy, x, A, B, 1.0)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / reps
        byt, flop = 4.0 * M * (K + N), 4.0 * M * r * (K + N)
        roof_ms = max(byt / HBM, flop / MFMA) * 1e3
        rows.append({"K": K, "N": N, "M": M, "r": r, "ms": round(ms, 4), "roof_ms": round(roof_ms, 4),
                     "frac_of_roof": round(roof_ms / ms, 3), "TBps": round(byt / ms / 1e9, 3)})
        del x, dy
    return rows


def train_compare(P, r, steps, warmup):
    import cases
    import synth
    from pangu_pytorch_amd import train
    base = P.PanguModel(device="cuda").cuda()
    base.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    for m in base.modules():
        if isinstance(m, P.layers.DropPath):
            m.drop_prob = 0.0
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    tgt, tgt_s = cases.model_targets("cuda")
    batch = (inp, inp_s, tgt, tgt_s)
    full = copy.deepcopy(base).train()
    lora = copy.deepcopy(base).train()
    del base
    lora.enable_lora(r=r, alpha=r)
    runs = {"full": (full, train.make_optimizer(full)), "lora": (lora, train.make_optimizer(lora))}
    times = {k: [] for k in runs}
    peak = {}
    for i in range(warmup + steps):
        for k, (m, opt) in runs.items():            # alternating: both see the same clocks and thermal state
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            train.train_step(m, opt, batch, stats, maps, const_h)
            b.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append(a.elapsed_time(b))
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated())
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return {"rank": r, "steps": steps, "full_ms": round(med["full"], 2), "lora_ms": round(med["lora"], 2),
            "ratio": round(med["lora"] / med["full"], 3), "full_peak_GB": round(peak["full"] / 1e9, 2),
            "lora_peak_GB": round(peak["lora"] / 1e9, 2),
            "trainable_params": {"full": sum(p.numel() for p in full.parameters() if p.requires_grad),
                                 "lora": sum(p.numel() for p in lora.parameters() if p.requires_grad)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rank", type=int, default=16)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    import pangu_pytorch_amd as P
    P._lib.load()
    print(json.dumps({"lora_wgrad": kernels(P, a.rank)}), flush=True)
    if not a.skip_train:
        print(json.dumps({"train_step": train_compare(P, a.rank, a.steps, a.warmup)}), flush=True)


if __name__ == "__main__":
    main()
