#!/usr/bin/env python3
"""Regional-scorecard measurements:

  python tools/bench_scorecard.py [--reps 50] [--rounds 9] [--out profiles/scorecard.json]

Everything on the full field (65 upper-air and 4 surface planes of 721 x 1440, two entry calls per sample, as
score.deterministic_scores makes them), ALTERNATED in one process, `--reps` samples between two events and `--rounds` timings per
variant (median, min and max reported):
  pangu_scorecard_sums_f32 at R = 1 (no mask), R = 4 (global and the three latitude bands) and R = 8 (those, Europe, North America,
    the North Pacific and a synthetic land mask), each with clim_kind 0 (none), 1 (a scalar per plane) and 2 (a field: a third read);
  pangu_lat_weighted_sums on the same tensors (the existing four-sum kernel with fp32 atomics: the same two reads);
  pangu_stage_planes_f32 of the field (the streaming copy tools/bench_regrid.py measures: 286.6 MB read + 286.6 MB written), scaled
    to the bytes the scorecard reads.
Aims (not asserted anywhere): R = 1 not slower than pangu_lat_weighted_sums, R = 8 at most 1.25 x it.
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 6.29e12
H, W, PLANES, UPPER = 721, 1440, 69, 65
FIELD_BYTES = 4.0 * PLANES * H * W          # 286.6 MB
BANDS = {"global": "global", "nh_extratropics": "nh_extratropics", "tropics": "tropics", "sh_extratropics": "sh_extratropics"}


def synthetic_land(h, w):
    """A smooth land-sea pattern with a few continents per latitude circle (about 40 % land), as a bool (h, w) tensor."""
    lat = np.linspace(0.5 * np.pi, -0.5 * np.pi, h)[:, None]
    lon = (2.0 * np.pi * np.arange(w) / w)[None, :]
    return torch.from_numpy(np.sin(3 * lon + 2 * np.sin(2 * lat)) * np.cos(2 * lat) + 0.3 * np.sin(7 * lon + 5 * lat) > 0.15)


def _sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(P, reps, rounds):
    lib = P._lib.load()
    S = P.score
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = 280.0 + 10.0 * torch.randn((PLANES, H, W), generator=g, device="cuda")
    target = pred + torch.randn((PLANES, H, W), generator=g, device="cuda")
    clim_field = 279.0 + torch.randn((PLANES, H, W), generator=g, device="cuda")
    clim_scalar = 279.0 + torch.randn(PLANES, generator=g, device="cuda")
    copy = torch.empty((PLANES, H, W), device="cuda")
    w = S.latitude_weights(H, "cuda")
    st = torch.cuda.current_stream().cuda_stream
    land = synthetic_land(H, W)
    plans = {1: None, 4: S.region_bits(H, W, BANDS, "cuda"),
             8: S.region_bits(H, W, dict(BANDS, europe="europe", north_america="north_america", north_pacific="north_pacific",
                                         land=dict(mask=land)), "cuda")}
    mixed = {}
    for R, plan in plans.items():                # share of mask words whose four bytes differ: these go point by point
        if plan is not None:
            b = plan.bits.cpu().numpy().reshape(H, W // 4, 4)
            mixed[R] = float((b != b[..., :1]).any(axis=-1).mean())
    tensors = ((0, UPPER), (UPPER, PLANES - UPPER))      # (first plane, planes) of the upper-air and the surface call

    def scorecard(R, kind):
        plan = plans[R]
        sums = torch.empty((PLANES, R, 10), dtype=torch.float64, device="cuda")
        ws = torch.empty(S.scorecard_workspace_bytes(PLANES, H, R), dtype=torch.uint8, device="cuda")
        bits = None if plan is None else plan.bits.data_ptr()

        def clim_ptr(first):
            if kind == 0:
                return None
            return (clim_scalar.data_ptr() + 4 * first) if kind == 1 else (clim_field.data_ptr() + 4 * first * H * W)

        def fn():
            for first, n in tensors:
                P._lib.check(lib.pangu_scorecard_sums_f32(
                    st, pred.data_ptr() + 4 * first * H * W, target.data_ptr() + 4 * first * H * W, 0, clim_ptr(first), kind,
                    w.data_ptr(), bits, R, sums.data_ptr() + 80 * first * R, ws.data_ptr(), ws.numel(), n, H, W), "scorecard")
        return fn

    old_out = torch.zeros((PLANES, 4), device="cuda")

    def lat_weighted_sums():
        for first, n in tensors:
            P._lib.check(lib.pangu_lat_weighted_sums(st, pred.data_ptr() + 4 * first * H * W, target.data_ptr() + 4 * first * H * W,
                                                     w.data_ptr(), old_out.data_ptr() + 16 * first, n, H, W), "lat_weighted_sums")

    def stage_copy():
        P._lib.check(lib.pangu_stage_planes_f32(st, pred.data_ptr(), None, None, copy.data_ptr(), PLANES, H * W, 0), "stage")

    variants = {("scorecard", R, kind): scorecard(R, kind) for R in (1, 4, 8) for kind in (0, 1, 2)}
    variants[("lat_weighted_sums", 1, 0)] = lat_weighted_sums
    variants[("stage_f32", 0, 0)] = stage_copy
    for fn in variants.values():                 # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):                      # alternate
        for k, fn in variants.items():
            times[k].append(_sample(fn, reps))
    med = {k: statistics.median(t) for k, t in times.items()}
    copy_ms, old_ms = med[("stage_f32", 0, 0)], med[("lat_weighted_sums", 1, 0)]
    rows = []
    for (name, R, kind), t in times.items():
        read = FIELD_BYTES * (3 if kind == 2 else 2) if name != "stage_f32" else 2 * FIELD_BYTES
        row = {"kernel": name, "R": R, "clim_kind": kind, "ms_median": round(med[(name, R, kind)], 4), "ms_min": round(min(t), 4),
               "ms_max": round(max(t), 4), "samples": rounds, "calls_per_sample": reps, "bytes": read,
               "hbm_floor_ms": round(read / HBM * 1e3, 4), "GBps": round(read / (med[(name, R, kind)] * 1e-3) / 1e9, 1)}
        if name != "stage_f32":
            row["copy_floor_ms"] = round(copy_ms * read / (2 * FIELD_BYTES), 4)      # the measured copy, scaled to these bytes
            row["x_copy_floor"] = round(med[(name, R, kind)] / row["copy_floor_ms"], 3)
            row["x_lat_weighted_sums"] = round(med[(name, R, kind)] / old_ms, 3)
        if name == "scorecard" and R in mixed:
            row["mixed_mask_words"] = round(mixed[R], 5)
        rows.append(row)
    aims = {"R1_not_slower_than_lat_weighted_sums": med[("scorecard", 1, 0)] <= old_ms,
            "R1_x_lat_weighted_sums": round(med[("scorecard", 1, 0)] / old_ms, 3),
            "R8_at_most_1.25x_lat_weighted_sums": med[("scorecard", 8, 0)] <= 1.25 * old_ms,
            "R8_x_lat_weighted_sums": round(med[("scorecard", 8, 0)] / old_ms, 3)}
    return rows, aims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scorecard.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scorecard.py measures on an MI355X: no HIP device found")
    import pangu_pytorch_amd as P
    P._lib.load()
    with torch.no_grad():
        rows, aims = measure(P, a.reps, a.rounds)
    result = {"hbm_Bps": HBM, "field_bytes": FIELD_BYTES, "grid": [H, W], "planes": [UPPER, PLANES - UPPER], "kernels": rows, "aims": aims}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
