#!/usr/bin/env python3
"""Multi-step (rollout) fine-tuning measurements:

  python tools/bench_rollout_train.py [--steps 5] [--warmup 2] [--rounds 3] [--skip-fp32]

One process, one seeded batch, DropPath off, reference-initialised weights; the arms of one compute dtype alternate inside every
round, so they see the same clocks and thermal state.
1. The seed kernel alone (`pangu_rollout_l1_seed_bwd`) at the model's shape against its HBM floor (read out, target, d_next, write
   d_out: 4 x 286 MB at 6.29 TB/s), next to the three torch-side passes it replaces (loss backward, multiply, add).
2. ms per call (device events) and `max_memory_allocated` of: `train.train_step`; `train.rollout_train_step` at K = 1, 2, 3 (bf16)
   and K = 1, 2 (fp32), checkpoint off and on; the torch-op composition (model + rollout.norm_back + train.weighted_l1_loss, one plain
   backward) at the same K.  Per arm: the median over rounds of the round's median, and every value.
Prints one JSON line per section."""
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


def seed_kernel(P, reps=20):
    from pangu_pytorch_amd import _lib, train
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(1)
    u = lambda shape, scale=1.0, shift=0.0: (torch.rand(shape, generator=g, device="cuda") * 2 - 1) * scale + shift
    o, os_, t, ts = u((1, 5, 13, 721, 1440)), u((1, 4, 721, 1440)), u((1, 5, 13, 721, 1440), 40.0, 250.0), u((1, 4, 721, 1440), 500.0, 1e5)
    dn, dns = u(o.shape, 1e-9), u(os_.shape, 1e-9)
    sl = (u((1, 4, 1, 1), 300.0, 1e5), u((1, 4, 1, 1), 100.0, 700.0), u((1, 5, 13, 1, 1), 20.0, 250.0), u((1, 5, 13, 1, 1), 5.0, 30.0))
    st = [x.reshape(-1).contiguous() for x in (sl[2], sl[3], sl[0], sl[1])]
    wu, ws = train._weights_on(o.device, torch.float32)
    gr = torch.tensor(0.5, device="cuda")
    d, ds = torch.empty_like(o), torch.empty_like(os_)
    geom = (1, 5, 13 * 721 * 1440, 4, 721 * 1440, 13, 0)
    stream = torch.cuda.current_stream().cuda_stream
    head = (stream, o.data_ptr(), t.data_ptr(), os_.data_ptr(), ts.data_ptr(), wu.data_ptr(), ws.data_ptr(), gr.data_ptr())
    sp = [x.data_ptr() for x in st]

    def fused(dst, dst_s):
        _lib.check(lib.pangu_rollout_l1_seed_bwd(*head, dn.data_ptr(), dns.data_ptr(), st[1].data_ptr(), st[3].data_ptr(),
                                                 dst.data_ptr(), dst_s.data_ptr(), *geom, *sp), "rollout_l1_seed_bwd")

    def torch_ops():
        _lib.check(lib.pangu_weighted_l1_loss_bwd(*head, d.data_ptr(), ds.data_ptr(), *geom, *sp), "weighted_l1_loss_bwd")
        return d + dn * sl[3], ds + dns * sl[1]

    def loss_bwd():
        _lib.check(lib.pangu_weighted_l1_loss_bwd(*head, d.data_ptr(), ds.data_ptr(), *geom, *sp), "weighted_l1_loss_bwd")

    for f in (lambda: fused(d, ds), torch_ops, loss_bwd):
        for _ in range(3):
            f()
    floor = 4 * FIELD_BYTES / HBM * 1e3
    out = {"floor_ms": round(floor, 4), "out_of_place_ms": round(_time(lambda: fused(d, ds), reps), 4),
           "loss_bwd_alone_ms": round(_time(loss_bwd, reps), 4), "loss_bwd_mul_add_torch_ms": round(_time(torch_ops, reps), 4)}
    out["in_place_ms"] = round(_time(lambda: fused(dn, dns), reps), 4)      # (last: it overwrites d_next)
    out["x_floor"] = round(out["out_of_place_ms"] / floor, 3)
    return out


def composition_step(model, optimizer, batch, statistics, maps, const_h, stats_last, lam):
    """The K-step step out of torch ops around the model: what a user would write without train.rollout_train_step."""
    from pangu_pytorch_amd import ops, rollout, train
    K = len(batch) // 2 - 1
    optimizer.zero_grad(set_to_none=True)
    cur, cur_s, total = batch[0], batch[1], None
    for k in range(K):
        out, out_s = model(cur, cur_s, statistics, maps, const_h)
        loss = train.weighted_l1_loss(out, out_s, batch[2 + 2 * k], batch[3 + 2 * k], stats_last=stats_last) * lam[k]
        total = loss if total is None else total + loss
        if k + 1 < K:
            cur, cur_s = rollout.norm_back(out, out_s, stats_last)
    with ops.dropped_branch_grads("none"):
        total.backward()
    optimizer.step(missing_as_zero=True)
    return total.detach()


def train_arms(P, dtype, Ks, steps, warmup, rounds):
    import cases
    from pangu_pytorch_amd import rollout, train
    torch.manual_seed(0)
    m = P.PanguModel(device="cuda").cuda().train()
    m.set_compute_dtype(dtype)
    for mod in m.modules():
        if isinstance(mod, P.layers.DropPath):
            mod.drop_prob = 0.0
    inp, inp_s, stats, maps, const_h = cases.model_inputs("cuda")
    sl = stats_last_of(stats)
    g = torch.Generator(device="cuda").manual_seed(2)
    targets = []
    for _ in range(max(Ks)):
        targets += list(rollout.norm_back(torch.rand(inp.shape, generator=g, device="cuda") * 2 - 1,
                                          torch.rand(inp_s.shape, generator=g, device="cuda") * 2 - 1, sl))
    opt = train.make_optimizer(m)
    consts = (stats, maps, const_h)
    arms = {"train_step": lambda: train.train_step(m, opt, (inp, inp_s, targets[0], targets[1]), *consts, stats_last=sl)}
    for K in Ks:
        batch = (inp, inp_s) + tuple(targets[:2 * K])
        lam = [1.0 / K] * K
        arms[f"rollout_K{K}"] = lambda b=batch: train.rollout_train_step(m, opt, b, *consts, sl)
        arms[f"rollout_K{K}_checkpoint"] = lambda b=batch: train.rollout_train_step(m, opt, b, *consts, sl, checkpoint=True)
        if K > 1:
            arms[f"torch_composition_K{K}"] = lambda b=batch, l=lam: composition_step(m, opt, b, *consts, sl, l)
    times = {k: [[] for _ in range(rounds)] for k in arms}
    peak = {k: 0 for k in arms}
    for r in range(-1, rounds):                     # round -1: the warm-up calls of every arm
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
    out = {"dtype": str(dtype).replace("torch.", ""), "steps": steps, "warmup": warmup, "rounds": rounds}
    for k in arms:
        out[k] = {"ms": _median([_median(v) for v in times[k]]), "peak_GB": round(peak[k] / 1e9, 2), "all_ms": times[k]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-fp32", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rollout_train.py needs a HIP device: nothing is measured without one")
    import pangu_pytorch_amd as P
    P._lib.load()
    print(json.dumps({"rollout_seed_kernel": seed_kernel(P)}), flush=True)
    print(json.dumps({"rollout_train": train_arms(P, torch.bfloat16, (1, 2, 3), a.steps, a.warmup, a.rounds)}), flush=True)
    if not a.skip_fp32:
        torch.cuda.empty_cache()
        print(json.dumps({"rollout_train": train_arms(P, torch.float32, (1, 2), a.steps, a.warmup, a.rounds)}), flush=True)


if __name__ == "__main__":
    main()
