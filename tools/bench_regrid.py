#!/usr/bin/env python3
"""Conservative-regridding measurements:

  python tools/bench_regrid.py [--reps 200] [--rounds 7] [--steps 7] [--out profiles/regrid.json]

1. kernels, the full field (69 planes of 721 x 1440), ALTERNATED in one process, `--reps` launches between two events per sample
   and `--rounds` samples per variant (median, min and max reported):
     pangu_regrid_planes_f32 to 121 x 240, 181 x 360 and 73 x 144, with and without the de-normalising affine,
     pangu_stage_planes_f32 of the same field (the streaming copy: 286.6 MB read + 286.6 MB written),
   against the floor of one 286.6 MB read plus the output written at 6.29 TB/s.  Acceptance: the regrid to 121 x 240 is not slower
   than the copy of the same run.
2. error: worst |error| / bound of the kernel against the float64 remap with the plan's dense matrices, per test shape (the bound
   of tests/test_gpu_regrid.py: (T_lat + T_lon + 4) 2^-24 |R_lat| |v| |R_lon|^T).
3. rollout: a `--steps`-step graphed bf16 rollout, alternated: resident, drained at full resolution and drained with
   regrid=(121, 240), int16 and float32, wall clock until everything is on the host and copied out of the page-locked slot.
   Acceptance: the regridded drain is not slower per step than the full-resolution drain of the same run.
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
FIELD_BYTES = 4.0 * PLANES * H * W          # 286.6 MB
TARGETS = ((121, 240), (181, 360), (73, 144))


def _sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernels(P, reps, rounds):
    lib = P._lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((PLANES, H, W), generator=g, device="cuda")
    mul = torch.rand(PLANES, generator=g, device="cuda") + 0.5
    add = torch.randn(PLANES, generator=g, device="cuda")
    copy = torch.empty((PLANES, H, W), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    variants = {}
    for grid in TARGETS:
        plan = P.score.regrid_plan(H, W, *grid)
        out = torch.empty((PLANES,) + grid, device="cuda")
        for aff in (False, True):
            m, a = (mul, add) if aff else (None, None)
            variants[(f"regrid_{grid[0]}x{grid[1]}", aff)] = (
                lambda plan=plan, out=out, m=m, a=a: P.score._regrid_launch(st, x.data_ptr(), m, a, out.data_ptr(), PLANES, plan, 0,
                                                                            x.device),
                FIELD_BYTES + 4.0 * PLANES * grid[0] * grid[1], (plan.lat_taps, plan.lon_taps))
    for aff in (False, True):
        pm, pa = (mul.data_ptr(), add.data_ptr()) if aff else (None, None)
        variants[("stage_f32", aff)] = (
            lambda pm=pm, pa=pa: P._lib.check(lib.pangu_stage_planes_f32(st, x.data_ptr(), pm, pa, copy.data_ptr(), PLANES, H * W, 0),
                                              "stage"), 2.0 * FIELD_BYTES, None)
    for fn, _, _ in variants.values():          # warm-up: code objects, the plans' device tables
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):                     # alternate
        for k, (fn, _, _) in variants.items():
            times[k].append(_sample(fn, reps))
    rows = []
    for (name, aff), (_, floor_bytes, taps) in variants.items():
        t = times[(name, aff)]
        med = statistics.median(t)
        floor = floor_bytes / HBM * 1e3
        rows.append({"kernel": name, "affine": aff, "planes": PLANES, "taps": taps, "ms_median": round(med, 4), "ms_min": round(min(t), 4),
                     "ms_max": round(max(t), 4), "samples": rounds, "launches_per_sample": reps, "floor_bytes": floor_bytes,
                     "hbm_floor_ms": round(floor, 4), "x_floor": round(med / floor, 3),
                     "GBps_of_floor_bytes": round(floor_bytes / (med * 1e-3) / 1e9, 1)})
    by = {(r["kernel"], r["affine"]): r for r in rows}
    accept = {"regrid_121x240_ms": by[("regrid_121x240", True)]["ms_median"], "stage_f32_ms": by[("stage_f32", True)]["ms_median"]}
    accept["regrid_not_slower_than_copy"] = all(by[("regrid_121x240", a)]["ms_median"] <= by[("stage_f32", a)]["ms_median"]
                                                for a in (False, True))
    return rows, accept


ERROR_SHAPES = (((13, 24, 7, 12), 69), ((13, 24, 5, 8), 69), ((19, 30, 7, 9), 69), ((11, 10, 4, 3), 3), ((37, 1440, 7, 240), 3),
                ((721, 16, 121, 4), 2), ((721, 1440, 121, 240), 2), ((721, 1440, 181, 360), 2), ((721, 1440, 73, 144), 2))


def errors(P):
    rows = []
    for grid, planes in ERROR_SHAPES:
        plan = P.score.regrid_plan(*grid)
        r = np.random.default_rng(planes * 1000 + grid[0])
        lat = np.linspace(0.5 * np.pi, -0.5 * np.pi, grid[0])[None, :, None]
        lon = (2.0 * np.pi * np.arange(grid[1]) / grid[1])[None, None, :]
        x = (280.0 + 20.0 * np.cos(lat) * np.sin(3 * lon) + r.standard_normal((planes, grid[0], grid[1]))).astype(np.float32)
        mul = r.uniform(0.5, 3.0, planes).astype(np.float32)
        add = r.uniform(-200.0, 900.0, planes).astype(np.float32)
        r_lat, r_lon = plan.dense()
        row = {"grid": list(grid), "planes": planes, "taps": [plan.lat_taps, plan.lon_taps]}
        for aff in (False, True):
            v = ((x * mul[:, None, None]).astype(np.float32) + add[:, None, None]).astype(np.float32) if aff else x
            ref = np.einsum("Jj,pji,Ii->pJI", r_lat, v.astype(np.float64), r_lon, optimize=True)
            mag = np.einsum("Jj,pji,Ii->pJI", r_lat, np.abs(v).astype(np.float64), r_lon, optimize=True)
            t = lambda a: torch.from_numpy(a).cuda()
            got = P.score.regrid(t(x), plan, t(mul) if aff else None, t(add) if aff else None).cpu().numpy().astype(np.float64)
            bound = (plan.lat_taps + plan.lon_taps + 4) * 2.0 ** -24 * mag
            row["worst_error_over_bound_affine" if aff else "worst_error_over_bound"] = round(float((np.abs(got - ref) / bound).max()), 3)
        rows.append(row)
    return rows


def rollout(P, steps, rounds):
    import cases
    import synth
    from bench_drain import Writer
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    s_mean, s_std, u_mean, u_std = stats
    sl = (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1), u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
          u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())
    threads = P.data.default_copy_threads()
    m.set_compute_dtype(torch.bfloat16)
    gs = P.rollout.GraphedStep(m, inp, inp_s, stats, maps, const_h, sl, feed_back=True)
    drained = {"full_int16": ("int16", None), "regrid_int16": ("int16", (121, 240)), "full_float32": ("float32", None),
               "regrid_float32": ("float32", (121, 240))}
    writers = {v: Writer(P, threads) for v in drained}
    drains = {v: P.data.HostDrain("cuda", mode=mode, depth=2, sink=writers[v], regrid=regrid) for v, (mode, regrid) in drained.items()}
    # One copy stream for all four, as in a forecast run, which holds one drain.  With a high-priority stream per drain, one of
    # several drains in a process saw its graph replays slowed (measured: 14.2 instead of 11.3 ms per step for the second of two
    # drains, 11.3 when it is the only one; supposedly its stream shares a hardware queue with the compute stream).
    for d in drains.values():
        d.stream = drains["full_int16"].stream

    def run(variant):
        gs.load(inp, inp_s)
        if variant in drains:
            writers[variant].expect(steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            gs.step()
            if variant in drains:
                drains[variant].submit([gs.inp, gs.inp_surface], tag=k)
        torch.cuda.synchronize()
        t_gpu = time.perf_counter() - t0
        if variant in drains:
            assert writers[variant].done.wait(60.0), "the sink did not finish"
        return t_gpu * 1e3, (time.perf_counter() - t0) * 1e3

    variants = ("resident",) + tuple(drained)
    for v in variants:
        run(v)                                   # warm-up: ring allocation, page-locking, the writer's buffers
    for d in drains.values():
        d.stats["producer_wait_s"] = 0.0
    times = {v: [] for v in variants}
    for _ in range(rounds):                      # alternate
        for v in variants:
            times[v].append(run(v))
    for d in drains.values():
        d.close()
    row = {"section": "rollout", "dtype": "bfloat16", "steps": steps, "rounds": rounds, "sink_copy_threads": threads}
    base = min(t[1] for t in times["resident"]) / steps
    for v in variants:
        done = [t[1] for t in times[v]]
        row[v] = {"ms_per_step_min": round(min(done) / steps, 3), "ms_per_step_median": round(statistics.median(done) / steps, 3),
                  "ms_per_step_max": round(max(done) / steps, 3),
                  "gpu_done_ms_per_step_min": round(min(t[0] for t in times[v]) / steps, 3), "x_resident": round(min(done) / steps / base, 3)}
    for v, d in drains.items():
        s = d.summary()
        row[v].update({"bytes_per_item": s["bytes_per_item"], "d2h_ms_per_item": round(s["d2h_ms_per_item"], 3),
                       "producer_wait_ms_per_item": round(d.stats["producer_wait_s"] / (rounds * steps) * 1e3, 3)})
    row["regrid_not_slower_than_full"] = {mode: row[f"regrid_{mode}"]["ms_per_step_median"] <= row[f"full_{mode}"]["ms_per_step_median"]
                                          for mode in ("int16", "float32")}
    try:                                         # the committed full-resolution figures of profiles/drain.json, for comparison
        with open(os.path.join(ROOT, "profiles", "drain.json")) as f:
            old = [r for r in json.load(f)["rollout"] if r["dtype"] == "bfloat16"][0]
        row["profiles_drain_json"] = {k: old[k]["ms_per_step_min"] for k in ("resident", "int16", "float32")}
    except (OSError, KeyError, IndexError, ValueError):
        row["profiles_drain_json"] = None
    m.set_compute_dtype(torch.float32)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid.json"))
    ap.add_argument("--skip-rollout", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regrid.py measures on an MI355X: no HIP device found")
    import pangu_pytorch_amd as P
    P._lib.load()
    result = {"hbm_Bps": HBM, "field_bytes": FIELD_BYTES}
    with torch.no_grad():
        result["kernels"], result["kernel_acceptance"] = kernels(P, a.reps, a.rounds)
        print(json.dumps({"section": "kernels", "rows": result["kernels"], "acceptance": result["kernel_acceptance"]}), flush=True)
        result["error"] = errors(P)
        print(json.dumps({"section": "error", "rows": result["error"]}), flush=True)
        if not a.skip_rollout:
            result["rollout"] = rollout(P, a.steps, max(3, a.rounds - 2))
            print(json.dumps(result["rollout"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
