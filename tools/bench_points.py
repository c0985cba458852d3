#!/usr/bin/env python3
"""Point-observation measurements:

  python tools/bench_points.py [--reps 50] [--rounds 7] [--steps 7] [--out profiles/points.json]

1. kernel: pangu_sample_points_f32 and pangu_point_scores_f32 (one region without region bits, and four regions) on the full field
   (69 planes of 721 x 1440) at N = 10 000 and N = 1 000 000 uniformly random points, in random order and sorted row-major (the
   plan keeps the caller's order, and neighbouring lanes share cache lines only where neighbouring points do), each ALTERNATED in
   one process with the torch composition of the same arithmetic: advanced-indexing gathers of the four taps plus the lerp with
   its selects, and for the scores the terms, torch.where by validity and region and float64 reductions.  `--reps` launches between
   two events per sample, `--rounds` samples per variant (median, min and max reported).  The composition is the yardstick; the aim
   is to beat it.  Beside the times: the bytes a launch must touch -- the plan, the outputs and observations, and the distinct 128-B
   lines of the field under the taps -- and the time those bytes take at the HBM peak.
2. rollout: a `--steps`-step graphed bf16 rollout with a PointSeries of 10 000 sites recorded after every step, and with an
   ObservationAccumulator scoring 10 000 reports after every step, alternated with the same rollout without them.  Reported: the
   overhead per step in ms, and the spread of the hook-free runs.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 6.29e12
H, W, PLANES = 721, 1440, 69
SIZES = (10_000, 1_000_000)
SITES = 10_000
LINE = 128
REGIONS4 = {"global": "global", "tropics": "tropics", "nh": "nh_extratropics", "europe": "europe"}


def _sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def random_points(n, seed):
    r = np.random.default_rng(seed)
    return r.uniform(-90.0, 90.0, n), r.uniform(0.0, 360.0, n)


def field_bytes_under_taps(plan):
    """The distinct 128-B lines of ONE plane that the four taps of the plan's points fall in, in bytes."""
    row, col = plan.row.cpu().numpy().astype(np.int64), plan.col.cpu().numpy().astype(np.int64)
    r1, c1 = np.minimum(row + 1, H - 1), (col + 1) % W
    offs = np.concatenate([row * W + col, row * W + c1, r1 * W + col, r1 * W + c1])
    return int(np.unique(offs * 4 // LINE).size) * LINE


def torch_sample(x, t):
    """The torch composition of the pinned sampling: four gathers, the lerp, selects for zero weights."""
    row, col, r1, c1, wy, wx = t
    v00, v01, v10, v11 = x[:, row, col], x[:, row, c1], x[:, r1, col], x[:, r1, c1]
    ux, uy = 1.0 - wx, 1.0 - wy
    l0 = torch.where(wx == 0, v00, v00 * ux + v01 * wx)
    l1 = torch.where(wx == 0, v10, v10 * ux + v11 * wx)
    return torch.where(wy == 0, l0, l0 * uy + l1 * wy)


def torch_scores(x, t, obs, masks):
    """The torch composition of the scores: the sample, the terms, validity and region by torch.where, float64 reductions."""
    f = torch_sample(x, t)
    d = f - obs
    terms = (d, d.abs(), d * d, f, obs, f * obs, f * f, obs * obs)
    valid = ~torch.isnan(obs)
    out = torch.empty((x.shape[0], len(masks), 10), dtype=torch.float64, device=x.device)
    for r, m in enumerate(masks):
        inside = valid if m is None else valid & m
        n = inside.sum(-1).double()
        out[:, r, 0] = n
        out[:, r, 9] = n
        for k, term in enumerate(terms):
            out[:, r, 1 + k] = torch.where(inside, term, torch.zeros_like(term)).double().sum(-1)
    return d, out


def kernel(P, reps, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((PLANES, H, W), generator=g, device="cuda")
    rows = []
    for n, order in ((n, order) for n in SIZES for order in ("random", "sorted")):
        lat, lon = random_points(n, n)
        if order == "sorted":                            # row-major: what a caller with a dense set of points should hand over
            k = np.lexsort((lon, -lat))
            lat, lon = lat[k], lon[k]
        plans = {1: P.score.point_plan(H, W, lat, lon, device="cuda"), 4: P.score.point_plan(H, W, lat, lon, REGIONS4, device="cuda")}
        plan = plans[1]
        long = lambda v: v.to(torch.int64)
        t = (long(plan.row), long(plan.col), torch.clamp(long(plan.row) + 1, max=H - 1), (long(plan.col) + 1) % W, plan.wy, plan.wx)
        obs = torch.randn((PLANES, n), generator=g, device="cuda")
        obs[torch.rand((PLANES, n), generator=g, device="cuda") < 1.0 / 3.0] = float("nan")
        out = torch.empty((PLANES, n), device="cuda")
        masks = {1: [None], 4: [((plans[4].bits >> r) & 1).bool() for r in range(4)]}
        up, sf = x[:65].view(5, 13, H, W), x[65:].view(4, H, W)          # the public entry wants the two tensors; one launch each
        ou, os_ = obs[:65].view(5, 13, n).contiguous(), obs[65:].contiguous()
        outs = (out[:65].view(5, 13, n), out[65:])
        variants = {
            "sample": lambda: P.score.sample_points(up, sf, plan, out=outs),
            "sample_torch": lambda: torch_sample(x, t),
        }
        for R in (1, 4):
            variants[f"scores_R{R}"] = lambda R=R: P.score.observation_scores(up, sf, ou, os_, plans[R], want_departures=True)
            variants[f"scores_R{R}_torch"] = lambda R=R: torch_scores(x, t, obs, masks[R])
        # the two sides agree before they are timed
        variants["sample"]()
        assert torch.equal(out, torch_sample(x, t)), "the torch composition restates other arithmetic"
        su, ss, du, ds = variants["scores_R4"]()
        _, ref = torch_scores(x, t, obs, masks[4])
        mine = torch.cat((su.sums.reshape(65, 4, 10), ss.sums))
        same_sign = [2, 3, 7, 8]                         # sums of terms of one sign: fp32 partial sums agree to a few 1e-7
        assert torch.equal(mine[..., 0], ref[..., 0]) and torch.allclose(mine[..., same_sign], ref[..., same_sign], rtol=1e-5, atol=0)
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        nreps = max(3, reps // 10) if n >= 100_000 else reps
        times = {k: [] for k in variants}
        for _ in range(rounds):                          # alternate
            for k, fn in variants.items():
                times[k].append(_sample(fn, nreps))
        field = field_bytes_under_taps(plan) * PLANES
        touched = {"sample": field + PLANES * n * 4 + n * 16 * PLANES,                    # the taps' lines, out, the plan per plane
                   "scores_R1": field + PLANES * n * (4 + 4) + n * 16 * PLANES,           # + obs read, departures written
                   "scores_R4": field + PLANES * n * (4 + 4) + n * 17 * PLANES}
        for name in ("sample", "scores_R1", "scores_R4"):
            tk, tt = times[name], times[name + "_torch"]
            med, tmed = statistics.median(tk), statistics.median(tt)
            rows.append({"what": name, "N": n, "order": order, "planes": PLANES, "ms_median": round(med, 4), "ms_min": round(min(tk), 4),
                         "ms_max": round(max(tk), 4), "torch_ms_median": round(tmed, 4), "torch_ms_min": round(min(tt), 4),
                         "torch_ms_max": round(max(tt), 4), "x_torch": round(med / tmed, 4), "beats_torch": med < tmed,
                         "samples": rounds, "launches_per_sample": nreps, "field_bytes_under_taps": field,
                         "field_share_touched": round(field / (PLANES * H * W * 4), 4), "bytes_touched": touched[name],
                         "hbm_floor_ms": round(touched[name] / HBM * 1e3, 4), "x_hbm_floor": round(med / (touched[name] / HBM * 1e3), 2),
                         "GBps": round(touched[name] / (med * 1e-3) / 1e9, 1), "points_per_us": round(PLANES * n / (med * 1e3), 1)})
        del plans, obs, out, t, masks
        torch.cuda.empty_cache()
    return rows


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
    plan = P.score.point_plan(H, W, *random_points(SITES, 1), device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = []
    for _ in range(steps):
        ou, os_ = torch.randn((1, 5, 13, SITES), generator=g, device="cuda"), torch.randn((1, 4, SITES), generator=g, device="cuda")
        ou[torch.rand(ou.shape, generator=g, device="cuda") < 1.0 / 3.0] = float("nan")
        obs.append((ou, os_))
    series = P.score.PointSeries(plan, steps)

    def run(variant):
        acc = P.score.ObservationAccumulator(steps, plan, clim=sl) if variant == "observations" else None
        gs.load(inp, inp_s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):                           # what rollout(sites=) / rollout(observations=, obs=) issue per step
            gs.step()
            if variant == "sites":
                series.record(k, gs.inp, gs.inp_surface)
            if acc is not None:
                acc.score(k, gs.inp, gs.inp_surface, *obs[k])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    variants = ("resident", "sites", "observations")
    for v in variants:
        run(v)                                           # warm-up: the series' table, the code object
    times = {v: [] for v in variants}
    for _ in range(rounds):                              # alternate
        for v in variants:
            times[v].append(run(v))
    row = {"section": "rollout", "dtype": "bfloat16", "steps": steps, "rounds": rounds, "N": SITES}
    for v in variants:
        row[v] = {"ms_per_step_min": round(min(times[v]) / steps, 3), "ms_per_step_median": round(statistics.median(times[v]) / steps, 3),
                  "ms_per_step_max": round(max(times[v]) / steps, 3)}
    res = row["resident"]
    row["resident_spread_ms_per_step"] = round(res["ms_per_step_max"] - res["ms_per_step_min"], 3)
    for v in ("sites", "observations"):
        row[v]["overhead_ms_per_step"] = round(row[v]["ms_per_step_median"] - res["ms_per_step_median"], 3)
        row[v]["x_resident"] = round(row[v]["ms_per_step_median"] / res["ms_per_step_median"], 4)
    m.set_compute_dtype(torch.float32)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "points.json"))
    ap.add_argument("--skip-rollout", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_points.py measures on an MI355X: no HIP device found")
    import pangu_pytorch_amd as P
    P._lib.load()
    result = {"hbm_Bps": HBM, "grid": [H, W], "planes": PLANES, "line_bytes": LINE}
    with torch.no_grad():
        result["kernel"] = kernel(P, a.reps, a.rounds)
        print(json.dumps({"section": "kernel", "rows": result["kernel"]}), flush=True)
        if not a.skip_rollout:
            result["rollout"] = rollout(P, a.steps, a.rounds)
            print(json.dumps(result["rollout"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
