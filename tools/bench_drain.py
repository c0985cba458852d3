#!/usr/bin/env python3
"""Output-pipeline measurements:

  python tools/bench_drain.py [--reps 20] [--rounds 5] [--steps 7] [--out profiles/drain.json]

1. kernels: pangu_pack_planes_i16 (both launches) and pangu_stage_planes_f32 alone at 69 planes of 721 x 1440, with de-normalisation
   and level reversal on, against their HBM floors: pack = two reads of 286.6 MB (the field exceeds the 256 MB Infinity Cache, so the
   quantise launch reads it again) + one 143.3 MB write; stage = one read + one write of 286.6 MB; at 6.29 TB/s.
2. rollout: a `--steps`-step graphed rollout (one GraphedStep with feed-back, re-loaded for every run), bf16 and fp32, four ways timed
   ALTERNATELY in one process, wall clock from the first replay until everything asked for is on the host:
     (a) resident     nothing leaves the device (what bench.py's rollout number is)
     (b) drain int16  data.HostDrain after every step, sink = a writer that copies every byte out of the page-locked slot
     (c) drain fp32   the same, unpacked
     (d) .cpu()       both physical fields pulled with Tensor.cpu() after every step -- the reference's way
   The yardstick of (b) is (a) of the same process: aim (b) <= (a) + pack + 3 % per step.
Prints one JSON line per section and writes all of it to --out."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 6.29e12
H, W = 721, 1440
FIELD_BYTES = 4.0 * 69 * H * W          # 286.6 MB


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


def kernels(P, reps):
    lib = P._lib.load()
    g = torch.Generator(device="cuda").manual_seed(0)
    elems = H * W
    x = torch.randn((69, H, W), generator=g, device="cuda")
    mul = torch.rand(69, generator=g, device="cuda") + 0.5
    add = torch.randn(69, generator=g, device="cuda")
    q = torch.empty((69, H, W), dtype=torch.int16, device="cuda")
    f = torch.empty((69, H, W), dtype=torch.float32, device="cuda")
    so = torch.empty((69, 2), device="cuda")
    nf = torch.empty((69,), dtype=torch.int32, device="cuda")
    ws_bytes = lib.pangu_pack_i16_ws_bytes(69, elems)
    ws = torch.empty((ws_bytes // 4,), device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def pack(levels):
        P._lib.check(lib.pangu_pack_planes_i16(st, x.data_ptr(), mul.data_ptr(), add.data_ptr(), q.data_ptr(), so.data_ptr(),
                                               nf.data_ptr(), ws.data_ptr(), ws_bytes, 69, elems, levels), "pack")

    def stage(levels):
        P._lib.check(lib.pangu_stage_planes_f32(st, x.data_ptr(), mul.data_ptr(), add.data_ptr(), f.data_ptr(), 69, elems, levels),
                     "stage")

    rows = []
    for name, fn, floor_bytes, target in (("pack_i16", pack, 2.5 * FIELD_BYTES, 1.5), ("stage_f32", stage, 2.0 * FIELD_BYTES, 1.5)):
        for levels in (0, 23):           # 69 = 3 x 23: every plane reads another one
            ms = _time(lambda: fn(levels), reps)
            floor = floor_bytes / HBM * 1e3
            rows.append({"kernel": name, "planes": 69, "levels": levels, "ms": round(ms, 4), "hbm_floor_ms": round(floor, 4),
                         "x_floor": round(ms / floor, 2), "target_x_floor": target,
                         "GBps": round(floor_bytes / (ms * 1e-3) / 1e9, 1)})
    return rows


class Writer:
    """The sink of (b) / (c): copies every byte of an item out of its page-locked slot into its own buffers (what a file writer's
    first step is), with the host threads of the input side's staging copy."""

    def __init__(self, P, threads):
        self.P, self.threads, self.bufs, self.count, self.done = P, threads, None, 0, threading.Event()
        self.want = 0

    def expect(self, n):
        self.count, self.want = 0, n
        self.done.clear()

    def __call__(self, item):
        arrays = [f.packed if f.packed is not None else f.values for f in item.fields]
        if self.bufs is None or any(b.nbytes != a.nbytes for a, b in zip(arrays, self.bufs)):
            self.bufs = [np.empty(a.shape, a.dtype) for a in arrays]
        lib = self.P._lib.load()
        for a, b in zip(arrays, self.bufs):
            self.P._lib.check(lib.pangu_host_copy(b.ctypes.data, a.ctypes.data, a.nbytes, self.threads), "host_copy")
        self.count += 1
        if self.count == self.want:
            self.done.set()


def rollout(P, steps, rounds, pack_ms):
    import cases
    import synth
    m = P.PanguModel(device="cuda").cuda().eval()
    m.load_state_dict(synth.fill_state_dict(cases.model_param_shapes(), "cuda"))
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    s_mean, s_std, u_mean, u_std = stats
    sl = (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1), u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
          u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())
    threads = P.data.default_copy_threads()
    rows = []
    for dtype in (torch.bfloat16, torch.float32):
        m.set_compute_dtype(dtype)
        gs = P.rollout.GraphedStep(m, inp, inp_s, stats, maps, const_h, sl, feed_back=True)
        writers = {mode: Writer(P, threads) for mode in ("int16", "float32")}
        drains = {mode: P.data.HostDrain("cuda", mode=mode, depth=2, sink=writers[mode]) for mode in writers}

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
                elif variant == "cpu":
                    gs.inp.cpu(), gs.inp_surface.cpu()
            torch.cuda.synchronize()
            t_gpu = time.perf_counter() - t0
            if variant in drains:
                assert writers[variant].done.wait(60.0), "the sink did not finish"
            return t_gpu * 1e3, (time.perf_counter() - t0) * 1e3

        variants = ("resident", "int16", "float32", "cpu")
        for v in variants:
            run(v)                                   # warm-up: ring allocation, page-locking, the writer's buffers
        for d in drains.values():
            d.stats["producer_wait_s"] = 0.0
        times = {v: [] for v in variants}
        for _ in range(rounds):                      # alternate the four ways
            for v in variants:
                times[v].append(run(v))
        for d in drains.values():
            d.close()
        row = {"section": "rollout", "dtype": str(dtype).replace("torch.", ""), "steps": steps, "rounds": rounds,
               "sink_copy_threads": threads, "pack_ms": pack_ms}
        base = min(t[1] for t in times["resident"]) / steps
        for v in variants:
            done = [t[1] for t in times[v]]
            row[v] = {"ms_per_step_min": round(min(done) / steps, 3), "ms_per_step_median": round(statistics.median(done) / steps, 3),
                      "gpu_done_ms_per_step_min": round(min(t[0] for t in times[v]) / steps, 3),
                      "x_resident": round(min(done) / steps / base, 3)}
        for mode, d in drains.items():
            s = d.summary()
            row[mode].update({"d2h_GBps": s["d2h_GBps"] and round(s["d2h_GBps"], 1), "d2h_ms_per_item": round(s["d2h_ms_per_item"], 3),
                              "producer_wait_ms_per_item": round(d.stats["producer_wait_s"] / (rounds * steps) * 1e3, 3),
                              "bytes_per_item": s["bytes_per_item"]})
        row["aim_int16_ms_per_step"] = round((base + pack_ms) * 1.03, 3)
        row["aim_met"] = row["int16"]["ms_per_step_min"] <= row["aim_int16_ms_per_step"]
        rows.append(row)
        del gs, drains, writers
        torch.cuda.empty_cache()
    m.set_compute_dtype(torch.float32)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drain.json"))
    ap.add_argument("--skip-rollout", action="store_true")
    a = ap.parse_args()
    import pangu_pytorch_amd as P
    P._lib.load()
    result = {"hbm_Bps": HBM, "field_bytes": FIELD_BYTES}
    with torch.no_grad():
        result["kernels"] = kernels(P, a.reps)
        print(json.dumps({"section": "kernels", "rows": result["kernels"]}), flush=True)
        if not a.skip_rollout:
            pack_ms = min(r["ms"] for r in result["kernels"] if r["kernel"] == "pack_i16")
            result["rollout"] = rollout(P, a.steps, a.rounds, pack_ms)
            for row in result["rollout"]:
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
