#!/usr/bin/env python3
"""Fair-CRPS ensemble fine-tuning measurements:

  python tools/bench_ensemble_train.py [--steps 4] [--warmup 2] [--rounds 3] [--out profiles/ensemble_train.json]

One process, one seeded batch, DropPath off, reference-initialised weights; the arms alternate inside every round, so they see
the same clocks and thermal state.
1. The loss kernels alone (`pangu_fair_crps_loss_fwd` / `_bwd`, csrc/crps_loss.hip) at the model's shape with E = 2, 4, 8 members
   against their HBM floors at 6.29 TB/s, one read per input field and one write per output field of 286 MB: forward E + 1 fields
   read, backward E + 1 read and E written (out of place and over the member fields themselves).
2. ms per call (device events) and `max_memory_allocated` of `train.ensemble_train_step` in bf16 at E = 2, 4, checkpoint on and
   off, next to `train.train_step` (unchanged by the ensemble work) and one forward of the training path in the same process:
   the step's target is E x (train_step + one forward).  Per arm: the median over rounds of the round's median, and every value.
Writes ONE JSON line to --out (and prints it)."""
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
FIELD_BYTES = 4 * (5 * 13 + 4) * 721 * 1440


def _median(v):
    return sorted(v)[len(v) // 2]


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stats_last_of(stats):
    s_mean, s_std, u_mean, u_std = stats
    return (s_mean.view(1, 4, 1, 1), s_std.view(1, 4, 1, 1),
            u_mean.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous(),
            u_std.reshape(13, 5).flip(0).t().reshape(1, 5, 13, 1, 1).contiguous())


def loss_kernels(Es=(2, 4, 8), reps=20, rounds=3):
    """The production call of the step: latitude weights on, the target in physical units (statistics folded in)."""
    from pangu_pytorch_amd import train
    g = torch.Generator(device="cuda").manual_seed(1)
    u = lambda shape, scale=1.0, shift=0.0: (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * scale + shift
    t, ts = u((1, 5, 13, 721, 1440), 40.0, 250.0), u((1, 4, 721, 1440), 500.0, 1e5)
    sl = (u((1, 4, 1, 1), 300.0, 1e5), u((1, 4, 1, 1), 100.0, 700.0), u((1, 5, 13, 1, 1), 20.0, 250.0), u((1, 5, 13, 1, 1), 5.0, 30.0))
    st = train._flat_stats(sl, t.device, 5, 13, 4)
    lat = train._crps_lat_weights(721, t.device)
    one = torch.ones((), device="cuda")
    out = {}
    for E in Es:
        xs, xs_s = [u(t.shape) for _ in range(E)], [u(ts.shape) for _ in range(E)]
        d, d_s = [torch.empty_like(v) for v in xs], [torch.empty_like(v) for v in xs_s]
        fwd = lambda: train._fair_crps_launch_fwd(xs, xs_s, t, ts, False, st, lat)
        bwd = lambda: train._fair_crps_launch_bwd(xs, xs_s, t, ts, False, st, lat, one, d, d_s)
        for f in (fwd, bwd):
            for _ in range(3):
                f()
        t_f, t_b = [], []
        for _ in range(rounds):                       # the two alternate
            t_f.append(_time(fwd, reps))
            t_b.append(_time(bwd, reps))
        # (last: it overwrites the members; the arithmetic does not depend on the values)
        t_i = [_time(lambda: train._fair_crps_launch_bwd(xs, xs_s, t, ts, False, st, lat, one, xs, xs_s), reps) for _ in range(rounds)]
        floor_f, floor_b = (E + 1) * FIELD_BYTES / HBM * 1e3, (2 * E + 1) * FIELD_BYTES / HBM * 1e3
        out[f"E{E}"] = {"fwd_ms": round(_median(t_f), 4), "fwd_floor_ms": round(floor_f, 4), "fwd_x_floor": round(_median(t_f) / floor_f, 3),
                        "bwd_ms": round(_median(t_b), 4), "bwd_floor_ms": round(floor_b, 4), "bwd_x_floor": round(_median(t_b) / floor_b, 3),
                        "bwd_in_place_ms": round(_median(t_i), 4), "all_fwd_ms": [round(v, 4) for v in t_f],
                        "all_bwd_ms": [round(v, 4) for v in t_b]}
        del xs, xs_s, d, d_s
        torch.cuda.empty_cache()
    return out


def train_arms(P, Es, steps, warmup, rounds):
    import cases
    from pangu_pytorch_amd import rollout, train
    torch.manual_seed(0)
    m = P.PanguModel(device="cuda").cuda().train()
    m.set_compute_dtype(torch.bfloat16)
    for mod in m.modules():
        if isinstance(mod, P.layers.DropPath):
            mod.drop_prob = 0.0
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    sl = stats_last_of(stats)
    g = torch.Generator(device="cuda").manual_seed(2)
    tgt, tgt_s = rollout.norm_back(torch.rand(inp.shape, generator=g, device="cuda") * 2 - 1,
                                   torch.rand(inp_s.shape, generator=g, device="cuda") * 2 - 1, sl)
    batch = (inp, inp_s, tgt, tgt_s)
    opt = train.make_optimizer(m)
    consts = (stats, maps, const_h)

    def forward_only():                               # the forward of the training path, its graph dropped
        out, out_s = m(inp, inp_s, *consts)
        del out, out_s

    arms = {"train_step": lambda: train.train_step(m, opt, batch, *consts, stats_last=sl), "train_forward": forward_only}
    for E in Es:
        kw = dict(members=E, amplitude=0.2, seed=3)
        arms[f"ensemble_E{E}_checkpoint"] = lambda kw=kw: train.ensemble_train_step(m, opt, batch, *consts, sl, checkpoint=True, **kw)
        arms[f"ensemble_E{E}_one_graph"] = lambda kw=kw: train.ensemble_train_step(m, opt, batch, *consts, sl, checkpoint=False, **kw)
    times = {k: [[] for _ in range(rounds)] for k in arms}
    peak = {k: 0 for k in arms}
    for r in range(-1, rounds):                       # round -1: the warm-up calls of every arm
        for k, fn in arms.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(warmup if r < 0 else steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if r >= 0:
                    times[k][r].append(round(a.elapsed_time(b), 2))
            peak[k] = max(peak[k], torch.cuda.max_memory_allocated())
    out = {"dtype": "bfloat16", "steps": steps, "warmup": warmup, "rounds": rounds}
    for k in arms:
        out[k] = {"ms": _median([_median(v) for v in times[k]]), "peak_GB": round(peak[k] / 1e9, 2), "all_ms": times[k]}
    step, fwd = out["train_step"]["ms"], out["train_forward"]["ms"]
    for E in Es:
        out[f"E{E}_x_train_step_ms"] = round(E * step, 2)                       # E plain steps: the one-graph mode's yardstick
        out[f"E{E}_x_train_step_plus_forward_ms"] = round(E * (step + fwd), 2)   # the checkpointed mode's target
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_train.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ensemble_train.py needs a HIP device: nothing is measured without one")
    import pangu_pytorch_amd as P
    P._lib.load()
    res = {"hbm_TBps": HBM / 1e12, "field_MB": round(FIELD_BYTES / 1e6, 1), "fair_crps_loss_kernels": loss_kernels(),
           "ensemble_train": train_arms(P, (2, 4), a.steps, a.warmup, a.rounds)}
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
