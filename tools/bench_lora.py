#!/usr/bin/env python3
"""LoRA measurements (LoRA section):

  python tools/bench_lora.py [--dtype fp32|bf16] [--steps 5] [--warmup 2] [--rank 16] [--skip-train]

1. `ops.lora_wgrad` per (K -> N) projection of the model at its real token count, against its roof
   max(bytes / 6.29 TB/s, FLOPs / 157.3 TF/s), bytes = 4 M (K + N), FLOPs = 4 M r (K + N).
2. In one process, same seeded batch, DropPath off, alternating: the fp32 `train.train_step` of the full fine-tune against the
   LoRA fine-tune (enable_lora(r)), ms/step for both, their ratio, and the peak memory of each.
Prints one JSON line per section.

--dtype bf16: `ops_bf16.lora_wgrad` per shape against its roof 2 M (K + N) / 6.29 TB/s and against `ops_bf16.linear_wgrad` of the
same shape (the launch a LoRA step skips); then, alternating in one process, the bf16 full fine-tune step, the bf16 LoRA step
(enable_lora(r, bf16_training=True)) and the fp32 LoRA step: ms/step, ratios, peak memory, and the host + GPU time of re-making
the 67 W_eff images after an optimizer step.  One JSON line, also written to profiles/lora_bf16.json.

--lora-dropout P (fp32): the adapter-dropout kernels per shape at r = --rank -- `ops.lora_dropout_fwd` (with and without the GELU
output) and `ops.lora_dropout_dx` against their HBM floors 4 M (K + 2N) (+ 4 M N) and 4 M (2K + r) bytes at 6.29 TB/s, and
`ops.lora_wgrad_dropout` against `ops.lora_wgrad` on the same operands; then, alternating in one process, DropPath off, the fp32
LoRA step with lora_dropout = P against the same model with 0: ms/step, ratio, peak memory.  One JSON line, also written to
profiles/lora_dropout.json.

--dtype bf16 --lora-dropout P: the same for the bf16 kernels (`ops_bf16.lora_dropout_fwd` / `lora_dropout_dx` / `lora_wgrad_dropout`,
floors 2 M (K + 2N) (+ 2 M N) and 2 M 2K + 4 M r (+ 2 M K with pre) bytes; `lora_wgrad_dropout` against the plain bf16 `lora_wgrad`),
then the bf16 LoRA step (enable_lora(r, bf16_training=True, bf16_dropout=True)) with lora_dropout = P against the same model with 0,
with the per-family device-event totals of both.  One JSON line, also written to profiles/lora_dropout_bf16.json."""
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


def _time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernels_bf16(P, r, reps=20):
    ob = P.ops_bf16
    rows = []
    for K, N, M in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(K + N)
        x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
        dy = torch.randn(M, N, device="cuda", generator=g).to(torch.bfloat16)
        A = torch.randn(r, K, device="cuda", generator=g) * 0.1
        B = torch.randn(N, r, device="cuda", generator=g) * 0.1
        # alternately, twice each: both kernels see the same clocks
        ms, wg = [], []
        for _ in range(2):
            ms.append(_time(lambda: ob.lora_wgrad(dy, x, A, B, 1.0), reps))
            wg.append(_time(lambda: ob.linear_wgrad(dy, x, want_bias=False), reps))
        ms, wg = min(ms), min(wg)
        byt = 2.0 * M * (K + N)
        roof_ms = byt / HBM * 1e3
        rows.append({"K": K, "N": N, "M": M, "r": r, "ms": round(ms, 4), "roof_ms": round(roof_ms, 4),
                     "frac_of_roof": round(roof_ms / ms, 3), "TBps": round(byt / ms / 1e9, 3),
                     "linear_wgrad_ms": round(wg, 4), "vs_linear_wgrad": round(ms / wg, 3)})
        del x, dy
    return rows


def kernels_dropout(P, r, p, reps=20, bf16=False):
    ops = P.ops_bf16 if bf16 else P.ops
    dt, esz = (torch.bfloat16, 2.0) if bf16 else (torch.float32, 4.0)
    rows = []
    for K, N, M in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(K + N)
        x = torch.randn(M, K, device="cuda", generator=g).to(dt)
        dy = torch.randn(M, N, device="cuda", generator=g).to(dt)
        y, h, dx = torch.zeros(M, N, device="cuda", dtype=dt), torch.empty(M, N, device="cuda", dtype=dt), torch.zeros(M, K, device="cuda", dtype=dt)
        pre = torch.randn(M, K, device="cuda", generator=g).to(dt) if bf16 else None
        A = torch.randn(r, K, device="cuda", generator=g) * 0.1
        B = torch.randn(N, r, device="cuda", generator=g) * 0.1
        V = ops.lora_wgrad_dropout(dy, x, A, B, 1.0, p, 1)[2]
        ms = {k: [] for k in ("fwd", "fwd_gelu", "dx", "wgrad_dropout", "wgrad") + (("dx_pre",) if bf16 else ())}
        for _ in range(2):                       # alternately, twice each: all see the same clocks
            ms["fwd"].append(_time(lambda: ops.lora_dropout_fwd(x, y, A, B, 1e-3, p, 1), reps))
            ms["fwd_gelu"].append(_time(lambda: ops.lora_dropout_fwd(x, y, A, B, 1e-3, p, 1, act=ops.ACT_GELU, h=h), reps))
            ms["dx"].append(_time(lambda: ops.lora_dropout_dx(dx, V, A, p, 1), reps))
            if bf16:
                ms["dx_pre"].append(_time(lambda: ops.lora_dropout_dx(dx, V, A, p, 1, pre=pre), reps))
            ms["wgrad_dropout"].append(_time(lambda: ops.lora_wgrad_dropout(dy, x, A, B, 1.0, p, 1), reps))
            ms["wgrad"].append(_time(lambda: ops.lora_wgrad(dy, x, A, B, 1.0), reps))
        ms = {k: min(v) for k, v in ms.items()}
        floor = {"fwd": esz * M * (K + 2 * N), "fwd_gelu": esz * M * (K + 3 * N), "dx": esz * M * 2 * K + 4.0 * M * r}
        if bf16:
            floor["dx_pre"] = esz * M * 3 * K + 4.0 * M * r
        row = {"K": K, "N": N, "M": M, "r": r, "p": p}
        for k, byt in floor.items():
            fl = byt / HBM * 1e3
            row.update({k + "_ms": round(ms[k], 4), k + "_floor_ms": round(fl, 4), k + "_x_floor": round(ms[k] / fl, 3)})
        row.update({"wgrad_dropout_ms": round(ms["wgrad_dropout"], 4), "wgrad_ms": round(ms["wgrad"], 4),
                    "wgrad_dropout_vs_wgrad": round(ms["wgrad_dropout"] / ms["wgrad"], 3)})
        rows.append(row)
        del x, dy, y, h, dx, V, pre
    return rows


FAMILIES = ("linear_bf16", "wgrad_bf16", "attn_bf16", "attn_bwd_bf16", "mlp_fused_bf16", "lora_wgrad", "lora_dropout_fwd",
            "lora_dropout_dx", "lora_wgrad_dropout")


def train_compare_dropout(P, r, p, steps, warmup, bf16=False):
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
    plain = copy.deepcopy(base).train()
    plain.enable_lora(r=r, alpha=r, bf16_training=bf16)
    drop = base.train()
    drop.enable_lora(r=r, alpha=r, lora_dropout=p, bf16_training=bf16, bf16_dropout=bf16)
    if bf16:
        plain.set_compute_dtype(torch.bfloat16)
        drop.set_compute_dtype(torch.bfloat16)
    runs = {"lora": (plain, train.make_optimizer(plain)), "lora_dropout": (drop, train.make_optimizer(drop))}
    times = {k: [] for k in runs}
    peak = {}
    torch.manual_seed(0)
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
    # the new launches' own share of the last kind of step (device events around each launch)
    P.ops.timing_start()
    train.train_step(drop, runs["lora_dropout"][1], batch, stats, maps, const_h)
    tags = ("lora_dropout_fwd", "lora_dropout_dx", "lora_wgrad_dropout")
    tot = P.ops.timing_stop(tags[0], also=tags)[3]
    families = {}
    if bf16:                # device-event totals per launch family, of both kinds of step
        for k, (m, opt) in runs.items():
            P.ops.timing_start()
            train.train_step(m, opt, batch, stats, maps, const_h)
            fam = P.ops.timing_stop(FAMILIES[0], also=FAMILIES)[3]
            families[k] = {t: {"ms": round(v[0], 2), "launches": v[2]} for t, v in fam.items() if v[2]}
    return {"rank": r, "p": p, "steps": steps, **{k + "_ms": round(v, 2) for k, v in med.items()},
            "ratio": round(med["lora_dropout"] / med["lora"], 3), "added_ms": round(med["lora_dropout"] - med["lora"], 2),
            **{k + "_peak_GB": round(v / 1e9, 2) for k, v in peak.items()},
            "launches_in_step": {k: {"ms": round(v[0], 2), "GB": round(v[1] / 1e9, 1), "launches": v[2]} for k, v in tot.items()},
            **({"families_ms": families} if bf16 else {})}


def train_compare_bf16(P, r, steps, warmup):
    import time

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
    full.set_compute_dtype(torch.bfloat16)
    lora = copy.deepcopy(base).train()
    lora.enable_lora(r=r, alpha=r, bf16_training=True)
    lora.set_compute_dtype(torch.bfloat16)
    lora32 = copy.deepcopy(base).train()
    lora32.enable_lora(r=r, alpha=r)
    del base
    runs = {k: (m, train.make_optimizer(m)) for k, m in (("full_bf16", full), ("lora_bf16", lora), ("lora_fp32", lora32))}
    times = {k: [] for k in runs}
    peak = {}
    for i in range(warmup + steps):
        for k, (m, opt) in runs.items():            # alternating: all see the same clocks and thermal state
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
    # the per-step remake of the W_eff images (merge kernel + plain / transposed / packed casts of 67 projections), on its own:
    # the state right after an optimizer step, then every image the training step asks for
    sh = lora._shadow
    lins = [m for m in lora.modules() if type(m) is P.layers.LoraLinear]
    blocks = [m for m in lora.modules() if type(m) is P.layers.EarthSpecificBlock]
    in_mlp = {id(l) for b in blocks for l in (b.linear.linear1, b.linear.linear2)}

    def remake():
        P.ops.bump_weights_epoch()
        for b in blocks:
            sh.get_mlp(P.layers.eff_weight(b.linear.linear1), P.layers.eff_weight(b.linear.linear2))
        for l in lins:
            w = l.effective_weight()
            if id(l) not in in_mlp:          # (the MLP projections' forward image is the packed one above)
                sh.get(w)
            sh.get_t(w)
    remake()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gpu_ms = _time(remake, 5, warm=1)
    host_ms = (time.perf_counter() - t0) * 1e3 / 6
    return {"rank": r, "steps": steps, **{k + "_ms": round(v, 2) for k, v in med.items()},
            "ratio_lora_bf16_to_full_bf16": round(med["lora_bf16"] / med["full_bf16"], 3),
            "ratio_lora_bf16_to_lora_fp32": round(med["lora_bf16"] / med["lora_fp32"], 3),
            **{k + "_peak_GB": round(v / 1e9, 2) for k, v in peak.items()},
            "w_eff_remake_gpu_ms": round(gpu_ms, 3), "w_eff_remake_wall_ms": round(host_ms, 3),
            "trainable_params": {k: sum(p.numel() for p in m.parameters() if p.requires_grad) for k, (m, _) in runs.items()}}


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
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--lora-dropout", type=float, default=0.0, metavar="P")
    a = ap.parse_args()
    import pangu_pytorch_amd as P
    P._lib.load()
    if a.lora_dropout > 0.0:
        bf16 = a.dtype == "bf16"
        res = {"box": torch.cuda.get_device_name(0), "dtype": a.dtype,
               "lora_dropout_kernels": kernels_dropout(P, a.rank, a.lora_dropout, bf16=bf16)}
        if not a.skip_train:
            res["train_step"] = train_compare_dropout(P, a.rank, a.lora_dropout, a.steps, a.warmup, bf16=bf16)
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(ROOT, "profiles", "lora_dropout_bf16.json" if bf16 else "lora_dropout.json"), "w") as f:
            f.write(line + "\n")
        return
    if a.dtype == "bf16":
        res = {"lora_wgrad_bf16": kernels_bf16(P, a.rank)}
        if not a.skip_train:
            res["train_step_bf16"] = train_compare_bf16(P, a.rank, a.steps, a.warmup)
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(ROOT, "profiles", "lora_bf16.json"), "w") as f:
            f.write(line + "\n")
        return
    print(json.dumps({"lora_wgrad": kernels(P, a.rank)}), flush=True)
    if not a.skip_train:
        print(json.dumps({"train_step": train_compare(P, a.rank, a.steps, a.warmup)}), flush=True)


if __name__ == "__main__":
    main()
