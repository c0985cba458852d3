#!/usr/bin/env python3
"""Ensemble measurements (ensemble section):

  python tools/bench_ensemble.py [--reps 10] [--steps 3] [--members 10,50] [--skip-kernels] [--skip-reliability] [--skip-quantiles]
                                 [--skip-rollout]

1. stats: score.ensemble_scores on the full grid at E = 50 and 100, with and without the mean / std fields, against the HBM
   floor (E + 1) * 286.6 MB (+ 2 * 286.6 MB with fields) / 6.29 TB/s.
2. perturb: ensemble.perturb_ at E = 50 against the floor 2 * E * 286.6 MB / 6.29 TB/s.
3. reliability: score.ensemble_reliability at E = 50 and 100, T = 0 and 4, with and without the probability fields, against the
   floor (E + 1) * 286.6 MB (+ T * 286.6 MB of fields) / 6.29 TB/s.
4. quantiles: score.ensemble_quantiles at E = 50 and 100, Q = 3 (0.1, 0.5, 0.9): fields only, scores only and both, against the
   floor (E (+ 1 with a target) + Q with fields) * 286.6 MB / 6.29 TB/s, and against score.ensemble_scores with targets at the same
   E in the same process (the kernel that runs the same sorting network): fields only should be no slower than that.
5. rollout: EnsembleRollout (scores at every step) against rollout.GraphedStep B = 1, timed alternately in one process, per
   member-step, fp32 and bf16, with the peak memory of each.
Prints one JSON line per section."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM = 6.29e12
H, W = 721, 1440
MEMBER_BYTES = 4.0 * 69 * H * W          # 286.6 MB


def _time(fn, reps):
    for _ in range(2):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _stats_last(g):
    u = lambda shape, lo, hi: torch.rand(shape, generator=g, device="cuda") * (hi - lo) + lo
    return (u((1, 4, 1, 1), -0.5, 0.5), u((1, 4, 1, 1), 0.5, 2.0), u((1, 5, 13, 1, 1), -0.5, 0.5), u((1, 5, 13, 1, 1), 0.5, 2.0))


def kernels(P, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    sl = _stats_last(g)
    tu = torch.randn((5, 13, H, W), generator=g, device="cuda")
    ts = torch.randn((4, H, W), generator=g, device="cuda")
    rows = []
    for E in (50, 100):
        up = torch.randn((E, 5, 13, H, W), generator=g, device="cuda")
        sf = torch.randn((E, 4, H, W), generator=g, device="cuda")
        for fields in (False, True):
            ms = _time(lambda: P.score.ensemble_scores(up, sf, tu, ts, sl, want_fields=fields), reps)
            floor = (E + 1 + 2 * fields) * MEMBER_BYTES / HBM * 1e3
            rows.append({"kernel": "stats", "E": E, "fields": fields, "ms": round(ms, 3), "hbm_floor_ms": round(floor, 3),
                         "x_floor": round(ms / floor, 2), "target_x_floor": 2.0})
        if E == 50:
            ms = _time(lambda: P.ensemble.perturb_(up, sf, sl, 0.01, 1, control=False), reps)
            floor = 2 * E * MEMBER_BYTES / HBM * 1e3
            rows.append({"kernel": "perturb", "E": E, "octaves": 3, "period": 12, "ms": round(ms, 3), "hbm_floor_ms": round(floor, 3),
                         "x_floor": round(ms / floor, 2), "target_x_floor": 1.5})
        del up, sf
        torch.cuda.empty_cache()
    return rows


def reliability(P, reps):
    """score.ensemble_reliability (verification mode) on the full grid: T = 0 (rank histogram only) and T = 4, with and without
    the probability fields, against (E + 1) member reads (+ T field writes) at the HBM rate.  Target: the streaming bar, 1.5x."""
    g = torch.Generator(device="cuda").manual_seed(0)
    tu = torch.randn((5, 13, H, W), generator=g, device="cuda")
    ts = torch.randn((4, H, W), generator=g, device="cuda")
    # events of probability about 0.5, 0.16, 0.02 and 0.001 for standard normal members
    levels = torch.tensor([0.0, 1.0, 2.0, 3.0], device="cuda")
    thr = (levels.view(4, 1, 1).expand(4, 5, 13).contiguous(), levels.view(4, 1).expand(4, 4).contiguous())
    rows = []
    for E in (50, 100):
        up = torch.randn((E, 5, 13, H, W), generator=g, device="cuda")
        sf = torch.randn((E, 4, H, W), generator=g, device="cuda")
        for T, fields in ((0, False), (4, False), (4, True)):
            ms = _time(lambda: P.score.ensemble_reliability(up, sf, tu, ts, thr if T else None, seed=1, want_fields=fields), reps)
            floor = (E + 1 + T * fields) * MEMBER_BYTES / HBM * 1e3
            rows.append({"kernel": "reliability", "E": E, "T": T, "prob": fields, "ms": round(ms, 3), "hbm_floor_ms": round(floor, 3),
                         "x_floor": round(ms / floor, 2), "target_x_floor": 1.5})
        del up, sf
        torch.cuda.empty_cache()
    return rows


def quantiles(P, reps):
    """score.ensemble_quantiles on the full grid, Q = 3 levels (0.1, 0.5, 0.9: all interpolated at E = 50 and 100).  The aim is
    fields only no slower than score.ensemble_scores with targets on the same members, timed next to it."""
    g = torch.Generator(device="cuda").manual_seed(0)
    sl = _stats_last(g)
    tu = torch.randn((5, 13, H, W), generator=g, device="cuda")
    ts = torch.randn((4, H, W), generator=g, device="cuda")
    q = (0.1, 0.5, 0.9)
    rows = []
    for E in (50, 100):
        up = torch.randn((E, 5, 13, H, W), generator=g, device="cuda")
        sf = torch.randn((E, 4, H, W), generator=g, device="cuda")
        stats_ms = _time(lambda: P.score.ensemble_scores(up, sf, tu, ts, sl), reps)
        for mode, tgt, fields in (("fields", False, True), ("scores", True, False), ("both", True, True)):
            args = (tu, ts) if tgt else (None, None)
            ms = _time(lambda: P.score.ensemble_quantiles(up, sf, q, *args, want_fields=fields), reps)
            floor = (E + tgt + len(q) * fields) * MEMBER_BYTES / HBM * 1e3
            rows.append({"kernel": "quantiles", "E": E, "Q": len(q), "mode": mode, "ms": round(ms, 3), "hbm_floor_ms": round(floor, 3),
                         "x_floor": round(ms / floor, 2), "stats_with_targets_ms": round(stats_ms, 3),
                         "x_stats": round(ms / stats_ms, 3), "target_x_stats": 1.0 if mode == "fields" else None})
        del up, sf
        torch.cuda.empty_cache()
    return rows


def rollout(P, members, steps):
    import cases
    import synth
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    tu, ts = cases.model_targets("cuda")
    s_mean, s_std, u_mean, u_std = stats
    sl = (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1), u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
          u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        m.set_compute_dtype(dtype)
        for E in members:
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            gs = P.rollout.GraphedStep(m, inp, inp_s, stats, maps, const_h, sl, feed_back=True)
            torch.cuda.synchronize()
            peak_single = torch.cuda.max_memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            ens = P.ensemble.EnsembleRollout(m, inp, inp_s, stats, maps, const_h, sl, members=E, amplitude=0.05, seed=1)
            torch.cuda.synchronize()
            capture_s = time.perf_counter() - t0

            def ens_step():
                ens.step()
                ens.scores(tu, ts)

            single, multi = [], []
            ens_step()
            gs.step()
            for _ in range(steps):               # alternate: one single-trajectory step, one ensemble step
                single.append(_one(gs.step))
                multi.append(_one(ens_step))
            peak_ens = torch.cuda.max_memory_allocated()
            s_ms, e_ms = min(single), min(multi)
            rows.append({"section": "rollout", "dtype": str(dtype).replace("torch.", ""), "E": E, "graphed_step_b1_ms": round(s_ms, 2),
                         "ensemble_step_ms": round(e_ms, 2), "per_member_step_ms": round(e_ms / E, 2),
                         "ratio_per_member_step": round(e_ms / E / s_ms, 4), "target_ratio": 1.03,
                         "capture_s": round(capture_s, 1), "peak_gb_graphed_step": round(peak_single / 1e9, 2),
                         "peak_gb_ensemble": round(peak_ens / 1e9, 2)})
            del ens, gs
    m.set_compute_dtype(torch.float32)
    return rows


def _one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--members", default="10,50")
    ap.add_argument("--skip-rollout", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-reliability", action="store_true")
    ap.add_argument("--skip-quantiles", action="store_true")
    a = ap.parse_args()
    import pangu_pytorch_amd as P
    P._lib.load()
    with torch.no_grad():
        if not a.skip_kernels:
            print(json.dumps({"section": "kernels", "rows": kernels(P, a.reps)}), flush=True)
        if not a.skip_reliability:
            print(json.dumps({"section": "reliability", "rows": reliability(P, a.reps)}), flush=True)
        if not a.skip_quantiles:
            print(json.dumps({"section": "quantiles", "rows": quantiles(P, a.reps)}), flush=True)
        if not a.skip_rollout:
            for row in rollout(P, [int(x) for x in a.members.split(",")], a.steps):
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
