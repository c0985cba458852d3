#!/usr/bin/env python3
"""Gradient clipping in front of the optimizer step, measured:

  python tools/bench_optimizer.py [--pairs 7] [--reps 10] [--warmup 3] [--max-norm 1.0]

The full model's 223 parameter tensors (1.1 GB) with resident random gradients; no forward or backward runs.  One process, the two
arms alternate inside every pair, device events around `reps` calls:
  (a) torch.nn.utils.clip_grad_norm_(params, max_norm) + HipAdam.step()   -- what a user writes without the option
  (b) HipAdam(max_grad_norm=max_norm).step()                              -- sum of squares, device record, scaled Adam
Then the pieces of (b) on their own, launched through the optimizer's job table: the sum-of-squares pass against its HBM floor
(gradient bytes at 6.29 TB/s), the one-workgroup record kernel, the scaled Adam launch next to the plain one.
Prints one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-norm", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optimizer.py needs a HIP device: nothing is measured without one")
    import pangu_pytorch_amd as P
    from pangu_pytorch_amd import _lib, train
    lib = _lib.load()
    torch.manual_seed(0)
    model = P.PanguModel(device="cuda").cuda()
    params = [p for p in model.parameters()]
    g = torch.Generator(device="cuda").manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device="cuda") * 1e-3
    n = sum(p.numel() for p in params)
    kw = dict(lr=5e-6, weight_decay=3e-6)
    plain, fused = train.HipAdam(params, **kw), train.HipAdam(params, max_grad_norm=a.max_norm, **kw)

    def arm_a():
        torch.nn.utils.clip_grad_norm_(params, a.max_norm)
        plain.step()

    def arm_b():
        fused.step()

    for fn in (arm_a, arm_b):
        for _ in range(a.warmup):
            fn()
    pairs = []
    for _ in range(a.pairs):
        ta = _time(arm_a, a.reps)
        tb = _time(arm_b, a.reps)
        pairs.append((round(ta, 4), round(tb, 4)))

    # the pieces of (b), through the job table the optimizer built
    _, table, n_jobs, blocks = fused._tables[0]
    partials, state = fused._partials[1], fused._clip_state[1]
    stream = torch.cuda.current_stream().cuda_stream
    adam = (stream, table.data_ptr(), n_jobs, blocks, 5e-6, 0.9, 0.999, 3e-6, 1e-8, 0.1, 0.03)
    pieces = {
        "sumsq": lambda: _lib.check(lib.pangu_grad_sumsq_multi(stream, table.data_ptr(), n_jobs, blocks, partials.data_ptr()), "sumsq"),
        "record": lambda: _lib.check(lib.pangu_grad_clip_state(stream, partials.data_ptr(), blocks, state.data_ptr(), 1, a.max_norm, 1.0, 0),
                                     "record"),
        "adam_scaled": lambda: _lib.check(lib.pangu_adam_step_multi_scaled(*adam, state.data_ptr()), "adam_scaled"),
        "adam_plain": lambda: _lib.check(lib.pangu_adam_step_multi(*adam), "adam_plain"),
    }
    piece_ms = {}
    for k, fn in pieces.items():
        for _ in range(a.warmup):
            fn()
        piece_ms[k] = round(_median([_time(fn, a.reps) for _ in range(a.pairs)]), 4)
    floor = 4 * n / HBM * 1e3
    out = {"parameters": n, "tensors": len(params), "table_blocks": blocks, "max_norm": a.max_norm, "reps": a.reps,
           "clip_grad_norm_plus_step_ms": _median([p[0] for p in pairs]), "fused_step_ms": _median([p[1] for p in pairs]),
           "pairs_ms": pairs, "fused_not_slower_in_every_pair": all(b <= a_ for a_, b in pairs),
           "pieces_ms": piece_ms, "sumsq_floor_ms": round(floor, 4), "sumsq_x_floor": round(piece_ms["sumsq"] / floor, 3),
           "norm": float(fused.last_grad_norm), "multiplier": float(fused.last_grad_multiplier)}
    print(json.dumps({"optimizer_clip": out}), flush=True)


if __name__ == "__main__":
    main()
