#!/usr/bin/env python3
"""Lead-window statistics measurements:

  python tools/bench_leadstats.py [--reps 100] [--rounds 7] [--steps 7] [--out profiles/leadstats.json]

1. kernel: pangu_lead_stats_update_f32 on the full field (69 planes of 721 x 1440), each configuration ALTERNATED in one process
   with a plain streaming copy (pangu_stage_planes_f32) that moves the same number of bytes -- the field read at 4 B per element
   plus every kept accumulator read and written, written only at a first lead -- `--reps` launches between two events per sample
   and `--rounds` samples per variant (median, min and max reported):
     (mean, min, max);  (mean) alone;  the full set with T = 1;  a first-lead launch of (mean, min, max).
   Aim: 1.25 x the copy of the same bytes for the fp32-only sets.
2. rollout: a `--steps`-step graphed bf16 rollout with (mean, min, max), and with the mean alone, over the windows (0,7), (0,3),
   (3,7) folded in after every step, alternated with the same rollout without it.  Aim: at most 1.05 x per step.
Prints one JSON line per section and writes all of it to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM = 6.29e12
H, W, PLANES = 721, 1440, 69
ELEMS = PLANES * H * W
WINDOWS = ((0, 7), (0, 3), (3, 7))
KERNEL_AIM, ROLLOUT_AIM = 1.25, 1.05

# name -> (kept fields, T, first lead)
CONFIGS = {
    "mean_min_max": (("sum", "min", "max"), 0, False),
    "mean": (("sum",), 0, False),
    "full_T1": (("sum", "min", "max", "when_min", "when_max", "count", "run", "longest"), 1, False),
    "mean_min_max_first_lead": (("sum", "min", "max"), 0, True),
}
FP32_ONLY = ("mean_min_max", "mean", "mean_min_max_first_lead")


def _sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def bytes_per_element(kept, first):
    acc = sum(4 if k in ("sum", "min", "max") else 1 for k in kept)
    return 4 + (acc if first else 2 * acc)


def kernel(P, reps, rounds):
    lib = P._lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((PLANES, H, W), generator=g, device="cuda")
    y = torch.randn((PLANES, H, W), generator=g, device="cuda")
    thr = torch.zeros((1, PLANES), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    copy_src = torch.randn(ELEMS * 5, generator=g, device="cuda")             # the largest copy: 19 B per element each way
    copy_dst = torch.empty_like(copy_src)
    variants = {}
    for name, (kept, T, first) in CONFIGS.items():
        fields = {k: torch.empty(((T,) if k in ("count", "run", "longest") else ()) + (PLANES, H, W),
                                 dtype=torch.float32 if k in ("sum", "min", "max") else torch.uint8, device="cuda") for k in kept}
        launch = lambda src, lead, first, fields=fields, T=T: P.score._lead_stats_launch(
            st, src.data_ptr(), None, None, fields, thr, T, PLANES, H * W, 0, lead, first)
        launch(x, 0, True)                           # the accumulators hold a first lead before the timed updates
        total = bytes_per_element(kept, first) * ELEMS
        variants[name] = ((lambda launch=launch, first=first: launch(y, 0 if first else 1, first)), total)
        # the copy of the same bytes: total / 2 read and total / 2 written, as 69 planes of a multiple of 4 floats
        n = int(total / 2 / 4 / PLANES) // 4 * 4
        variants[name + "_copy"] = ((lambda n=n: P._lib.check(lib.pangu_stage_planes_f32(
            st, copy_src.data_ptr(), None, None, copy_dst.data_ptr(), PLANES, n, 0), "stage")), 2.0 * 4 * PLANES * n)
    for fn, _ in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):                          # alternate
        for k, (fn, _) in variants.items():
            times[k].append(_sample(fn, reps))
    rows = []
    for name, (kept, T, first) in CONFIGS.items():
        t, c = times[name], times[name + "_copy"]
        med, cmed = statistics.median(t), statistics.median(c)
        total = variants[name][1]
        rows.append({"config": name, "kept": list(kept), "T": T, "first_lead": first, "bytes_per_element": bytes_per_element(kept, first),
                     "bytes": total, "ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                     "copy_bytes": variants[name + "_copy"][1], "copy_ms_median": round(cmed, 4), "copy_ms_min": round(min(c), 4),
                     "copy_ms_max": round(max(c), 4), "samples": rounds, "launches_per_sample": reps,
                     "x_copy": round(med / cmed, 3), "hbm_floor_ms": round(total / HBM * 1e3, 4),
                     "GBps": round(total / (med * 1e-3) / 1e9, 1), "copy_GBps": round(variants[name + "_copy"][1] / (cmed * 1e-3) / 1e9, 1)})
    accept = {"aim_x_copy": KERNEL_AIM, "fp32_only": {r["config"]: r["x_copy"] for r in rows if r["config"] in FP32_ONLY}}
    accept["met"] = all(v <= KERNEL_AIM for v in accept["fp32_only"].values())
    return rows, accept


def rollout(P, steps, rounds):
    import cases
    import synth
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    s_mean, s_std, u_mean, u_std = stats
    sl = (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1), u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
          u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())
    m.set_compute_dtype(torch.bfloat16)
    gs = P.rollout.GraphedStep(m, inp, inp_s, stats, maps, const_h, sl, feed_back=True)
    windows = tuple(w for w in WINDOWS if w[1] <= steps) or ((0, steps),)
    aggs = {"lead_stats": P.score.LeadWindowStats(windows, ("mean", "min", "max")),
            "lead_stats_mean_only": P.score.LeadWindowStats(windows, ("mean",))}

    def run(variant):
        agg = aggs.get(variant)
        gs.load(inp, inp_s)
        if agg is not None:
            agg.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            gs.step()
            if agg is not None:
                agg.update(k, gs.inp, gs.inp_surface)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    variants = ("resident",) + tuple(aggs)
    for v in variants:
        run(v)                                       # warm-up: the accumulators, the code object
    times = {v: [] for v in variants}
    for _ in range(rounds):                          # alternate
        for v in variants:
            times[v].append(run(v))
    launches = 2 * sum(b - a for a, b in windows)
    row = {"section": "rollout", "dtype": "bfloat16", "steps": steps, "rounds": rounds, "windows": [list(w) for w in windows],
           "update_launches": launches}
    for v in variants:
        row[v] = {"ms_per_step_min": round(min(times[v]) / steps, 3), "ms_per_step_median": round(statistics.median(times[v]) / steps, 3),
                  "ms_per_step_max": round(max(times[v]) / steps, 3)}
    for v, agg in aggs.items():
        # what the updates of one rollout move, at the kernel section's byte count: the floor of their cost
        per_update = bytes_per_element(agg._kept, False) * ELEMS
        first = bytes_per_element(agg._kept, True) * ELEMS
        moved = sum((b - a - 1) * per_update + first for a, b in windows)
        row[v].update({"stats": list(agg.stats), "accumulator_bytes": agg.bytes(), "bytes_moved_per_step": moved / steps,
                       "hbm_floor_ms_per_step": round(moved / steps / HBM * 1e3, 3),
                       "x_resident": round(row[v]["ms_per_step_median"] / row["resident"]["ms_per_step_median"], 3)})
        row[v]["met"] = row[v]["x_resident"] <= ROLLOUT_AIM
    row["aim_x_resident"] = ROLLOUT_AIM
    m.set_compute_dtype(torch.float32)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leadstats.json"))
    ap.add_argument("--skip-rollout", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_leadstats.py measures on an MI355X: no HIP device found")
    import pangu_pytorch_amd as P
    P._lib.load()
    result = {"hbm_Bps": HBM, "elements": ELEMS}
    with torch.no_grad():
        result["kernel"], result["kernel_acceptance"] = kernel(P, a.reps, a.rounds)
        print(json.dumps({"section": "kernel", "rows": result["kernel"], "acceptance": result["kernel_acceptance"]}), flush=True)
        if not a.skip_rollout:
            result["rollout"] = rollout(P, a.steps, max(3, a.rounds - 2))
            print(json.dumps(result["rollout"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
