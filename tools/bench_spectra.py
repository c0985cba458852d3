#!/usr/bin/env python3
"""Zonal-spectrum measurements:

  python tools/bench_spectra.py [--items 1,50] [--window 0.3] [--out profiles/spectra.json]

score.zonal_spectrum on the full grid (69 planes of 721 x 1440) for N = 1 and N = 50 states, K = 720 and K = 180 wavenumbers,
B = 1 and B = 4 bands, with and without `minus`.  One call is the upper and the surface tensor: two transform launches and two
reduce launches.  Timed with device events over at least `window` seconds of calls after a warm-up of the same shape.  Per row:
  ms             per call,
  tflops         executed: 4 * N * 49 749 rows * 721 folded samples * (K + 1) wavenumbers (two f32 MFMA products, Re and Im)
                 over ms -- the algorithm's count, not the padded tiles',
  share_of_peak  tflops over the 157.3 TF/s f32-MFMA peak,
  x_hbm_floor    ms over one read of the fields (and one of minus) at 6.29 TB/s,
  bound          which of the two floors is the larger one (the kernel is MFMA-bound by design).
Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM = 6.29e12
PEAK_F32_MFMA = 157.3e12
H, W = 721, 1440
PLANES = 69
ITEM_BYTES = 4.0 * PLANES * H * W          # 286.6 MB


def _time(fn, window):
    for _ in range(2):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(3, int(window * 1e3 / max(a.elapsed_time(b), 1e-3)) + 1)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def rows(P, items, window):
    g = torch.Generator(device="cuda").manual_seed(0)
    mu = torch.randn((5, 13, H, W), generator=g, device="cuda")
    ms_ = torch.randn((4, H, W), generator=g, device="cuda")
    named = [(-90, 90), (-90, -20), (-20, 20), (20, 90)]
    out = []
    for N in items:
        up = torch.randn((N, 5, 13, H, W), generator=g, device="cuda") + 300.0
        sf = torch.randn((N, 4, H, W), generator=g, device="cuda") + 300.0
        for K in (720, 180):
            for B in (1, 4):
                for minus in (False, True):
                    args = (mu, ms_) if minus else (None, None)
                    ms, reps = _time(lambda: P.score.zonal_spectrum(up, sf, *args, bands=named[:B], kmax=K), window)
                    flop = 4.0 * N * PLANES * H * (W // 2 + 1) * (K + 1)
                    mfma_floor = flop / PEAK_F32_MFMA * 1e3
                    hbm_floor = (N + minus) * ITEM_BYTES / HBM * 1e3
                    tf = flop / (ms * 1e-3) / 1e12
                    out.append({"N": N, "K": K, "B": B, "minus": minus, "ms": round(ms, 4), "reps": reps, "tflops": round(tf, 1),
                                "share_of_peak": round(tf * 1e12 / PEAK_F32_MFMA, 3), "mfma_floor_ms": round(mfma_floor, 4),
                                "hbm_floor_ms": round(hbm_floor, 4), "x_hbm_floor": round(ms / hbm_floor, 1),
                                "bound": "f32 MFMA" if mfma_floor >= hbm_floor else "HBM"})
        del up, sf
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", default="1,50")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of calls per timed row")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectra.json"))
    a = ap.parse_args()
    import pangu_pytorch_amd as P
    P._lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectra needs an MI355X: there is nothing to time without one")
    with torch.no_grad():
        res = {"section": "zonal_spectrum", "grid": [PLANES, H, W], "peak_f32_mfma_tflops": PEAK_F32_MFMA / 1e12,
               "hbm_tb_s": HBM / 1e12, "aim_share_of_peak": [0.83, 0.86],
               "rows": rows(P, [int(x) for x in a.items.split(",")], a.window)}
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
