#!/usr/bin/env python3
"""Event-verification measurements:

  python tools/bench_events.py [--reps 20] [--rounds 9] [--out profiles/events.json]

Everything on the full field (65 upper-air and 4 surface planes of 721 x 1440, two entry calls per sample, as score.event_scores
makes them), ALTERNATED in one process, `--reps` samples between two events and `--rounds` timings per variant (median, min and
max reported):
  (a) pangu_event_scores_f32, T = 1, radii (0,)              the contingency table alone: no stencil, no halo
  (b) T = 1, radii (0, 2, 8, 16)
  (c) T = 4, radii (0, 2, 8, 16)
  (d) case (c) with a domain mask (the northern extratropics of a RegionPlan)
  pangu_scorecard_sums_f32 at one region, no climatology     the same two reads, ten moment sums
  pangu_traffic_copy of the field                            286.6 MB read + 286.6 MB written: the streaming floor for the 573 MB
                                                             that every case above reads
Aim (not asserted anywhere): (a) not slower than the scorecard pass beyond the spread of the alternated samples.
Prints one JSON line and writes it to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM = 6.29e12
H, W, PLANES, UPPER = 721, 1440, 69, 65
FIELD_BYTES = 4.0 * PLANES * H * W          # 286.6 MB
CASES = {"a": (1, (0,), False), "b": (1, (0, 2, 8, 16), False), "c": (4, (0, 2, 8, 16), False), "d": (4, (0, 2, 8, 16), True)}
COPY_WORKGROUPS = 2048


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
    target = pred + 3.0 * torch.randn((PLANES, H, W), generator=g, device="cuda")
    copy = torch.empty((PLANES, H, W), device="cuda")
    w = S.latitude_weights(H, "cuda")
    st = torch.cuda.current_stream().cuda_stream
    plan = S.region_bits(H, W, {"tropics": "tropics", "nh": "nh_extratropics"}, "cuda")
    # events at the 50, 75, 90 and 97.5 % quantiles of the field: 280 + 10 z
    thr_all = torch.tensor([280.0, 286.74, 292.82, 299.6], device="cuda")[:, None].expand(4, PLANES).contiguous()
    tensors = ((0, UPPER), (UPPER, PLANES - UPPER))      # (first plane, planes) of the upper-air and the surface call

    def events(T, radii, masked):
        N = len(radii)
        host_radii = (ctypes.c_int * N)(*radii)
        counts = torch.empty((2, T, PLANES, 4), dtype=torch.int64, device="cuda")
        wsums = torch.empty((2, T, PLANES, 4), dtype=torch.float64, device="cuda")
        fss = torch.empty((2, T, PLANES, N, 2), dtype=torch.float64, device="cuda")
        ws = torch.empty(S.event_scores_workspace_bytes(PLANES, H, T, N), dtype=torch.uint8, device="cuda")
        thr = [thr_all[:T, first:first + n].contiguous() for first, n in tensors]
        bits = plan.bits.data_ptr() if masked else None

        def fn():
            for i, (first, n) in enumerate(tensors):
                P._lib.check(lib.pangu_event_scores_f32(
                    st, pred.data_ptr() + 4 * first * H * W, target.data_ptr() + 4 * first * H * W, 0, thr[i].data_ptr(), T, host_radii,
                    N, w.data_ptr(), bits, 1, counts[i].data_ptr(), wsums[i].data_ptr(), fss[i].data_ptr(), ws.data_ptr(), ws.numel(),
                    n, H, W), "event_scores")
        return fn

    sums = torch.empty((PLANES, 1, 10), dtype=torch.float64, device="cuda")
    sc_ws = torch.empty(S.scorecard_workspace_bytes(PLANES, H, 1), dtype=torch.uint8, device="cuda")

    def scorecard():
        for first, n in tensors:
            P._lib.check(lib.pangu_scorecard_sums_f32(
                st, pred.data_ptr() + 4 * first * H * W, target.data_ptr() + 4 * first * H * W, 0, None, 0, w.data_ptr(), None, 1,
                sums.data_ptr() + 80 * first, sc_ws.data_ptr(), sc_ws.numel(), n, H, W), "scorecard")

    def traffic_copy():
        P._lib.check(lib.pangu_traffic_copy(st, pred.data_ptr(), copy.data_ptr(), int(FIELD_BYTES), COPY_WORKGROUPS), "traffic_copy")

    variants = {"events_" + k: events(*v) for k, v in CASES.items()}
    variants["scorecard_R1"] = scorecard
    variants["traffic_copy"] = traffic_copy
    for fn in variants.values():                 # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):                      # alternate
        for k, fn in variants.items():
            times[k].append(_sample(fn, reps))
    med = {k: statistics.median(t) for k, t in times.items()}
    copy_ms, card_ms = med["traffic_copy"], med["scorecard_R1"]
    rows = []
    for name, t in times.items():
        row = {"kernel": name, "ms_median": round(med[name], 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
               "samples": rounds, "calls_per_sample": reps, "bytes": 2 * FIELD_BYTES, "hbm_floor_ms": round(2 * FIELD_BYTES / HBM * 1e3, 4),
               "GBps": round(2 * FIELD_BYTES / (med[name] * 1e-3) / 1e9, 1)}
        if name.startswith("events_"):
            T, radii, masked = CASES[name[-1]]
            row.update({"T": T, "radii": list(radii), "masked": masked, "x_copy_floor": round(med[name] / copy_ms, 3),
                        "x_scorecard": round(med[name] / card_ms, 3)})
        elif name == "scorecard_R1":
            row["x_copy_floor"] = round(med[name] / copy_ms, 3)
        rows.append(row)
    spread = max(times["scorecard_R1"]) - min(times["scorecard_R1"])
    aims = {"a_x_scorecard": round(med["events_a"] / card_ms, 3), "scorecard_spread_ms": round(spread, 4),
            "a_not_slower_than_scorecard_beyond_spread": med["events_a"] <= card_ms + spread,
            "c_over_T_times_b": round(med["events_c"] / (4 * med["events_b"]), 3)}
    return rows, aims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_events.py measures on an MI355X: no HIP device found")
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
