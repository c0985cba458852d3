"""Training-step pieces around the model (counterpart of reference models/pangu_sample.py:45-77).

The loss is the caller's code in the reference (plain torch ops on the two output fields); it is restated here so
bench/tests/finetune loops need nothing from the reference's era5_data package.
"""
import torch

UPPER_WEIGHTS = (3.00, 0.60, 1.50, 0.77, 0.54)       # reference era5_data/config.py:45
SURFACE_WEIGHTS = (1.50, 0.77, 0.66, 3.00)           # reference era5_data/config.py:46


def norm_data(target, target_surface, stats_last):
    """reference era5_data/utils_data.py:315-321; stats_last = (s_mean(1,4,1,1), s_std, u_mean(1,5,13,1,1), u_std)."""
    s_mean, s_std, u_mean, u_std = stats_last
    return (target - u_mean) / u_std, (target_surface - s_mean) / s_std


_loss_weights = {}      # (device, dtype) -> (w_upper, w_surface) on the device


def _weights_on(device, dtype):
    """The two weight vectors, uploaded once per (device, dtype): torch.tensor(list, device=cuda) is a synchronous
    host-to-device copy, i.e. one that waits for the whole forward in front of it -- 14 ms of host stall per call in the
    bf16 training step, after which the backward launches start from an empty queue."""
    key = (device, dtype)
    w = _loss_weights.get(key)
    if w is None:
        w = (torch.tensor(UPPER_WEIGHTS, dtype=dtype).view(1, 5, 1, 1, 1).to(device),
             torch.tensor(SURFACE_WEIGHTS, dtype=dtype).view(1, 4, 1, 1).to(device))
        _loss_weights[key] = w
    return w


def _weighted_l1_loss_torch(output, output_surface, target, target_surface, target_levels_reversed=False, stats_last=None):
    if target_levels_reversed:
        target = target.flip(-3)                       # the reader's `[::-1]` (reference era5_data/utils_data.py:117)
    if stats_last is not None:
        target, target_surface = norm_data(target, target_surface, stats_last)
    wu, ws = _weights_on(output.device, output.dtype)
    loss_surface = torch.mean(torch.abs(output_surface - target_surface) * ws)
    loss_upper = torch.mean(torch.abs(output - target) * wu)
    return loss_upper + loss_surface * 0.25


_stats_flat = {}      # (ids of the four statistics tensors) -> (the tensors, their flat fp32 device copies)


def _flat_stats(stats_last, device, Vu, L, Vs):
    """stats_last = (s_mean (1,Vs,1,1), s_std, u_mean (1,Vu,L,1,1), u_std) -> four flat contiguous fp32 device tensors, converted
    once per set of statistics tensors (they are constants of a training run)."""
    key = tuple(id(t) for t in stats_last) + (str(device),)
    hit = _stats_flat.get(key)
    if hit is not None and all(a is b for a, b in zip(hit[0], stats_last)):
        return hit[1]
    s_mean, s_std, u_mean, u_std = stats_last
    if u_mean.numel() != Vu * L or u_std.numel() != Vu * L or s_mean.numel() != Vs or s_std.numel() != Vs:
        raise RuntimeError(f"weighted_l1_loss: stats_last shapes {[tuple(t.shape) for t in stats_last]} for {Vu} x {L} upper / {Vs} surface planes")
    flat = tuple(t.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous() for t in (u_mean, u_std, s_mean, s_std))
    if len(_stats_flat) > 8:
        _stats_flat.clear()
    _stats_flat[key] = (tuple(stats_last), flat)
    return flat


class WeightedL1LossFn(torch.autograd.Function):
    """The loss and its gradient as one HIP pass each (csrc/loss.hip): the torch expression reads / writes the 286 MB fields
    fourteen times per step (0.9 ms); the forward here reads them once, the backward once more and writes the two gradients.
    The target side of the reference's loop body is folded into the same two passes: `normData` of the targets
    (era5_data/utils_data.py:315-321, called at models/pangu_sample.py:57) when `stats_last` is given, and the reader's level
    reversal (utils_data.py:117) when the target arrives with ascending levels (`target_levels_reversed`)."""

    @staticmethod
    def forward(ctx, output, output_surface, target, target_surface, target_levels_reversed=False, stats_last=None):
        from . import _lib
        lib = _lib.load()
        wu, ws = _weights_on(output.device, torch.float32)
        with torch.cuda.device(output.device):
            return WeightedL1LossFn._forward(ctx, lib, wu, ws, output, output_surface, target, target_surface,
                                             bool(target_levels_reversed), stats_last)

    @staticmethod
    def _forward(ctx, lib, wu, ws, output, output_surface, target, target_surface, rev, stats_last):
        from . import _lib
        from .ops import _stream
        B, Vu, L = output.shape[0], output.shape[1], output.shape[2]
        Vs = output_surface.shape[1]
        geom = (B, Vu, output[0, 0].numel(), Vs, output_surface[0, 0].numel(), L)
        nblk = lib.pangu_weighted_l1_loss_blocks(*geom)
        if nblk <= 0:
            raise RuntimeError(f"weighted_l1_loss: unsupported shapes {tuple(output.shape)} {tuple(output_surface.shape)}")
        st = _flat_stats(stats_last, output.device, Vu, L, Vs) if stats_last is not None else ()
        sp = tuple(t.data_ptr() for t in st) if st else (None,) * 4
        partial = torch.empty((nblk,), dtype=torch.float32, device=output.device)
        loss = torch.empty((3,), dtype=torch.float32, device=output.device)
        _lib.check(lib.pangu_weighted_l1_loss_fwd(_stream(output), output.data_ptr(), target.data_ptr(), output_surface.data_ptr(),
                                                  target_surface.data_ptr(), wu.data_ptr(), ws.data_ptr(), partial.data_ptr(),
                                                  loss.data_ptr(), *geom, int(rev), *sp), "weighted_l1_loss_fwd")
        ctx.save_for_backward(output, output_surface, target, target_surface, *st)
        ctx.geom, ctx.rev = geom, rev
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        from .ops import _stream
        output, output_surface, target, target_surface, *st = ctx.saved_tensors
        wu, ws = _weights_on(output.device, torch.float32)
        d_o, d_os = torch.empty_like(output), torch.empty_like(output_surface)
        g = g.to(torch.float32).contiguous()
        sp = tuple(t.data_ptr() for t in st) if st else (None,) * 4
        with torch.cuda.device(output.device):
            _lib.check(_lib.load().pangu_weighted_l1_loss_bwd(
                _stream(output), output.data_ptr(), target.data_ptr(), output_surface.data_ptr(), target_surface.data_ptr(),
                wu.data_ptr(), ws.data_ptr(), g.data_ptr(), d_o.data_ptr(), d_os.data_ptr(), *ctx.geom, int(ctx.rev), *sp),
                "weighted_l1_loss_bwd")
        return d_o, d_os, None, None, None, None


def _hip_loss_ok(output, output_surface, target, target_surface):
    ts = (output, output_surface, target, target_surface)
    return (all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == output.device for t in ts)
            and output.dim() == 5 and output_surface.dim() == 4 and output.shape == target.shape
            and output_surface.shape == target_surface.shape and output.shape[0] == output_surface.shape[0]
            and output.shape[1] == len(UPPER_WEIGHTS) and output_surface.shape[1] == len(SURFACE_WEIGHTS)
            and not target.requires_grad and not target_surface.requires_grad)


def weighted_l1_loss(output, output_surface, target, target_surface, target_levels_reversed=False, stats_last=None):
    """reference models/pangu_sample.py:61-67: mean(|o-t| * w_upper) + 0.25 * mean(|o_s-t_s| * w_surface).  Contiguous fp32
    fields on a HIP device take the two-pass HIP form (WeightedL1LossFn); anything else (other dtypes, CPU tensors of the
    host-side tests, targets that need gradients) is the reference's own torch expression.
    stats_last: the targets are in physical units and are normalised first (`normData`, :57); target_levels_reversed: the upper-air
    target is stored with ascending levels (as on disk) -- both are folded into the HIP passes."""
    if _hip_loss_ok(output, output_surface, target, target_surface):
        return WeightedL1LossFn.apply(output, output_surface, target, target_surface, target_levels_reversed, stats_last)
    return _weighted_l1_loss_torch(output, output_surface, target, target_surface, target_levels_reversed, stats_last)


class HipAdam(torch.optim.Optimizer):
    """torch.optim.Adam's update (L2 weight decay, no amsgrad / maximize) for fp32 parameters on a HIP device, ONE launch per
    parameter group over a device-resident job table (csrc/adam.hip: the arithmetic of torch's fused Adam, bit-identical; 14
    launches of <= 320 workgroups there, 1.8 ms for the model's 7.7 GB).  State layout and hyper-parameter names are
    torch.optim.Adam's (`step`, `exp_avg`, `exp_avg_sq`; lr / betas / eps / weight_decay per group), so schedulers work unchanged.
    Optimizer steps advance ops' weights epoch through the global post-step hook like any torch optimizer."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, shadow_of=None, max_grad_norm=None,
                 skip_nonfinite=False):
        """max_grad_norm: clip the global gradient norm (over every group) to it, as torch.nn.utils.clip_grad_norm_ in front of
        the step would -- without writing the gradients.  skip_nonfinite: a step whose gradients hold a NaN or an Inf leaves
        parameters and moments alone (what torch's GradScaler does through fused Adam's `found_inf`).  Either, or
        `step(grad_scale=)`, turns the one launch per group into: one sum-of-squares pass per group (csrc/adam.hip, double partials
        in a fixed order), one launch that forms the device record (norm, multiplier, skip, skips so far), and one scaled Adam launch
        per group that reads the record.  Nothing waits for the device: see `last_grad_norm`, `last_grad_multiplier`,
        `skipped_steps`, `reconcile_skips`."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"HipAdam: max_grad_norm must be > 0 (got {max_grad_norm})")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = {}        # group index -> (signature, device table, n_jobs, total blocks)
        # shadow_of: a PanguModel whose bf16 weight shadows (fused_bf16.WeightShadow) this optimizer keeps current for the plain
        # casts -- the Earth-specific bias tables, 94 % of the bytes: the kernel writes the bf16 image next to the updated fp32
        # value instead of the refresh launch re-reading 1.04 GB
        self._shadow_of = shadow_of
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._init_clip()

    def _init_clip(self):
        self._clip_state = None      # (device, the 24-byte record as 6 int32) -- allocated by the first clipped / scaled / guarded step
        self._partials = None        # (total blocks of all groups, double tensor): one partial sum of squares per table block
        self._skips_seen = 0         # `skipped_steps` at the last reconcile_skips()
        self._guarded = {}           # parameter -> guarded steps it took part in since the last reconcile_skips()

    def _record(self, lo, hi, dtype):
        return None if self._clip_state is None else self._clip_state[1][lo:hi].view(dtype)[0]

    @property
    def last_grad_norm(self):
        """fp32 device scalar: the global norm of grad_scale * gradients in the last clipped / scaled / guarded step, before
        clipping (None before the first such step).  Reading it is the caller's synchronisation, not the optimizer's."""
        return self._record(0, 1, torch.float32)

    @property
    def last_grad_multiplier(self):
        """fp32 device scalar: what that step multiplied every gradient by, grad_scale * min(1, max_grad_norm / (norm + 1e-6))."""
        return self._record(1, 2, torch.float32)

    @property
    def skipped_steps(self):
        """int64 device scalar: steps skipped so far for non-finite gradients (skip_nonfinite=True)."""
        return self._record(4, 6, torch.int64)

    def reconcile_skips(self):
        """Take the skipped steps out of the host step counters: reads `skipped_steps` (ONE host synchronisation; call it every
        so often, not every step) and rewinds state[p]["step"] of every parameter stepped under skip_nonfinite since the last
        call by the number of steps skipped since then.  Returns that number.

        Why it exists: the bias corrections are host scalars computed from state[p]["step"], and `step()` cannot know whether the
        kernel skipped, so the counter advances through a skipped step.  Until this is called the following steps use the bias
        corrections of a step count that is too high by the number of skips (parameters and moments are untouched by the skip
        itself); once it has been called, the trajectory is that of torch's fused Adam with `found_inf`, which does not advance
        `step` on a skipped step.  Exact when every guarded step since the last call stepped the same parameters (what
        train_step / rollout_train_step / accumulated_train_step do); a parameter that took part in fewer guarded steps than
        were skipped is rewound by the steps it took part in."""
        if self._clip_state is None:
            return 0
        total = int(self.skipped_steps.item())
        new, self._skips_seen = total - self._skips_seen, total
        if new > 0:
            for p, k in self._guarded.items():
                st = self.state.get(p)
                if st:
                    st["step"] = max(0, int(st["step"]) - min(new, k))
            self._tables = {}        # per-row bias corrections (tensors at different step counts) are part of the tables
        self._guarded = {}
        return new

    # the device job tables hold raw pointers into the optimizer state: anything that can replace state tensors drops them
    def load_state_dict(self, state_dict):
        self._tables = {}
        return super().load_state_dict(state_dict)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("skip_nonfinite", False)
        if "_clip_state" not in self.__dict__:
            self._init_clip()

    def add_param_group(self, param_group):
        self._tables = {}
        return super().add_param_group(param_group)

    @torch.no_grad()
    def step(self, closure=None, missing_as_zero=False, grad_scale=1.0):
        """missing_as_zero: parameters without a gradient are stepped with a ZERO gradient (moments decay, weight decay applies)
        instead of being skipped -- what the reference's DropPath-dropped branches get (the branch is computed and multiplied by
        zero there) -- without materialising the zeros.
        grad_scale: the update uses grad_scale * gradient (1/n after n accumulated backward passes); the norm that is clipped
        and reported is that of the scaled gradient.  The gradients themselves are not written."""
        import math
        import struct

        from . import _lib
        from .ops import _stream
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        grad_scale = float(grad_scale)
        if not (math.isfinite(grad_scale) and grad_scale > 0):
            raise ValueError(f"HipAdam.step: grad_scale must be finite and > 0 (got {grad_scale})")
        fused = self.max_grad_norm is not None or self.skip_nonfinite or grad_scale != 1.0
        work = []                # per group with rows: (group, device table, n_jobs, blocks, bias corrections, imaged parameters, shadows)
        for gi, group in enumerate(self.param_groups):
            rows, first, dev = [], 0, None
            beta1, beta2 = group["betas"]
            ws = getattr(self._shadow_of, "_shadow", None) if self._shadow_of is not None else None
            imaged = []
            for p in group["params"]:
                if p.grad is None and not (missing_as_zero and p.requires_grad):
                    continue
                g = p.grad
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and
                        (g is None or (g.dtype == torch.float32 and g.device == p.device))):
                    raise RuntimeError("HipAdam: parameters and gradients must be contiguous float32 tensors on one HIP device")
                if g is not None and not g.is_contiguous():
                    g = p.grad = g.contiguous()
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if torch.is_tensor(st["step"]):          # a state_dict written by torch.optim.Adam keeps `step` as a tensor
                    st["step"] = int(st["step"].item())
                st["step"] += 1
                if self.skip_nonfinite:
                    self._guarded[p] = self._guarded.get(p, 0) + 1
                n = p.numel()
                if n == 0:
                    continue
                img = ws.plain_image(p) if ws is not None else None
                if img is not None and (img.numel() != n or img.device != p.device):
                    img = None
                if img is not None:
                    imaged.append(p)
                rows.append((p.data_ptr(), g.data_ptr() if g is not None else 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             img.data_ptr() if img is not None else 0, n, st["step"], first))
                first += (n + 4095) // 4096
                if dev is not None and p.device != dev:
                    raise RuntimeError("HipAdam: the parameters of one group must live on one device")
                dev = p.device
            if not rows:
                continue
            if group.get("amsgrad") or group.get("maximize"):
                raise RuntimeError("HipAdam implements torch.optim.Adam without amsgrad / maximize (a loaded state_dict asked for them)")
            # ATen's fused Adam (ATen/native/cuda/fused_adam_utils.cuh:130-137, torch 2.10): both corrections AND the square root
            # are formed in double (`std::pair<double, double>`), then narrowed to the float arguments of adam_math -- checked bit
            # for bit over 40 steps by tests/test_gpu_hardening.py (rounding to float before the root, as ADVICE r3 suggested, breaks it)
            bias = lambda k: (1.0 - beta1 ** k, math.sqrt(1.0 - beta2 ** k))
            uniform = all(r[6] == rows[0][6] for r in rows)
            # the table holds pointers (and per-tensor bias corrections only when the step counts differ): with gradients that keep
            # their addresses -- FlatGradSync's flat buffer, or the caching allocator handing the same blocks back every step -- it
            # is uploaded once; otherwise through pinned memory, asynchronously (no host sync in the training loop)
            # (the moments' addresses are part of the signature: `load_state_dict` / a rollback that replaces `exp_avg` while the
            # parameters and the flat gradient buffer stay put must not leave the kernel updating the old, freed tensors)
            sig = tuple((r[0], r[1], r[2], r[3], r[4], r[5], 0 if uniform else r[6]) for r in rows)
            hit = self._tables.get(gi)
            if hit is None or hit[0] != sig:
                tab = []
                for (pp, gp, mp, vp, sp, n, k, fb) in rows:
                    bits = 0
                    if not uniform:
                        b1, b2 = bias(k)
                        bits = struct.unpack("<I", struct.pack("<f", b1))[0] | (struct.unpack("<I", struct.pack("<f", b2))[0] << 32)
                        if bits >= 1 << 63:
                            bits -= 1 << 64
                    tab.append([pp, gp, mp, vp, sp, n, bits, fb])
                tab.append([0, 0, 0, 0, 0, 0, 0, first])
                hit = self._tables[gi] = (sig, torch.tensor(tab, dtype=torch.int64).pin_memory().to(dev, non_blocking=True), len(rows), first)
            work.append((group, hit[1], hit[2], hit[3], bias(rows[0][6]), imaged, ws))
        if fused and work:
            self._clip_record(lib, work, grad_scale)
        for group, table, n_jobs, blocks, (b1, b2), imaged, ws in work:
            beta1, beta2 = group["betas"]
            with torch.cuda.device(table.device):      # the launch goes to the parameters' device whatever the caller's current device is
                args = (_stream(table), table.data_ptr(), n_jobs, blocks, float(group["lr"]), float(beta1), float(beta2),
                        float(group["weight_decay"]), float(group["eps"]), b1, b2)
                if fused:
                    _lib.check(lib.pangu_adam_step_multi_scaled(*args, self._clip_state[1].data_ptr()), "adam_step_multi_scaled")
                else:
                    _lib.check(lib.pangu_adam_step_multi(*args), "adam_step_multi")
            for p in imaged:       # (a skipped step re-wrote the image from the unchanged parameter: fresh either way)
                ws.mark_fresh(p)
        return loss

    def _clip_record(self, lib, work, grad_scale):
        """The launches in front of a clipped / scaled / guarded step: the sum of squares of every group's gradients into one
        partial buffer, then the device record (csrc/adam.hip ClipState) the scaled Adam launches read."""
        from . import _lib
        from .ops import _stream
        dev = work[0][1].device
        if any(w[1].device != dev for w in work):
            raise RuntimeError("HipAdam: max_grad_norm / skip_nonfinite / grad_scale take ONE norm over all groups: every group must "
                               "live on one device")
        if self._clip_state is None or self._clip_state[0] != dev:
            self._clip_state = (dev, torch.zeros(6, dtype=torch.int32, device=dev))
            self._skips_seen = 0
        total = sum(w[3] for w in work)
        if self._partials is None or self._partials[0] != total or self._partials[1].device != dev:
            self._partials = (total, torch.empty(total, dtype=torch.float64, device=dev))
        partials, state = self._partials[1], self._clip_state[1]
        with torch.cuda.device(dev):
            stream, first = _stream(partials), 0
            for _, table, n_jobs, blocks, _, _, _ in work:
                _lib.check(lib.pangu_grad_sumsq_multi(stream, table.data_ptr(), n_jobs, blocks, partials.data_ptr() + 8 * first),
                           "grad_sumsq_multi")
                first += blocks
            clip = self.max_grad_norm is not None
            _lib.check(lib.pangu_grad_clip_state(stream, partials.data_ptr(), total, state.data_ptr(), int(clip),
                                                 self.max_grad_norm if clip else 0.0, grad_scale, int(self.skip_nonfinite)),
                       "grad_clip_state")


def make_optimizer(model, lr=5e-6, weight_decay=3e-6, max_grad_norm=None, skip_nonfinite=False):
    """The reference's optimiser (finetune_fully.py:121: Adam(lr=5e-6, weight_decay=3e-6)).  Parameters on a HIP device: the
    one-launch HipAdam above (bit-identical to torch's fused Adam); CPU parameters (host-side tests): torch.optim.Adam.
    max_grad_norm / skip_nonfinite: HipAdam's fused global-norm clipping and non-finite-step guard; torch's Adam has neither, so
    asking for them where HipAdam cannot be used is a ValueError."""
    params = [p for p in model.parameters() if p.requires_grad]
    on_gpu = all(p.is_cuda for p in params)
    if on_gpu and all(p.dtype == torch.float32 and p.is_contiguous() for p in params):
        return HipAdam(params, lr=lr, weight_decay=weight_decay, shadow_of=model, max_grad_norm=max_grad_norm,
                       skip_nonfinite=skip_nonfinite)
    if max_grad_norm is not None or skip_nonfinite:
        raise ValueError("make_optimizer: max_grad_norm / skip_nonfinite are HipAdam's (contiguous fp32 parameters on a HIP device); "
                         "these parameters get torch.optim.Adam, which would ignore them")
    return torch.optim.Adam(params, lr=lr, weight_decay=weight_decay, fused=on_gpu)


class GraphedTrainStep:
    """OPT-IN: forward + loss + backward of one fixed-shape batch captured in a hipGraph, Adam stepped eagerly after each replay
    (its bias corrections are host scalars that change every step; it is ONE launch).  For a model WITHOUT active stochastic depth
    only (model.eval(), or every DropPath at rate 0): a captured step cannot skip a dropped branch -- it would have to compute it
    and scale it by a zero read from device memory, as the reference does, which costs the ~10 % of block work that not computing
    dropped branches saves.  Measured (tools/profile_train.py <dtype> <steps> <warmup> graph): the eager step is
    not host-bound, so replaying it from a graph recovers next to nothing -- this class exists to make that a number.
    The bf16 weight shadows the graph reads are re-made IN PLACE after every optimizer step (WeightShadow.refresh_in_place)."""

    def __init__(self, model, optimizer, batch, statistics, maps, const_h, stats_last=None, warmup=2):
        from .layers import DropPath, LoraLinear
        if any(type(m) is LoraLinear for m in model.modules()):
            raise RuntimeError("GraphedTrainStep: the model carries LoRA adapters, whose W_eff = W + s*B@A would go stale inside the "
                               "replayed graph; use train.train_step (or merge_lora() first)")
        if model.training and any(isinstance(m, DropPath) and m.drop_prob > 0.0 for m in model.modules()):
            raise RuntimeError("GraphedTrainStep: stochastic depth is active (model.train() with DropPath rates > 0): a captured step "
                               "cannot skip dropped branches; call model.eval() or use train.train_step")
        self.model, self.optimizer = model, optimizer
        self.batch = [t.clone() for t in batch]
        self.consts, self.stats_last = (statistics, maps, const_h), stats_last
        dev = self.batch[0].device
        with torch.cuda.device(dev):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):            # outside capture: weight shadows, loss weights, allocator, lazy LDS attributes
                    optimizer.zero_grad(set_to_none=True)
                    self._fwd_bwd()
            torch.cuda.current_stream().wait_stream(side)
            optimizer.zero_grad(set_to_none=True)      # the gradients are (re-)allocated INSIDE the capture: static addresses
            from . import ops
            ops.reset_pass_arenas()                    # never a zero buffer filled outside the capture (e.g. left by a failed backward)
            ops.release_stream_workspaces()            # the capture allocates its own weight-gradient scratch, inside its own pool
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                self.loss = self._fwd_bwd()
            ops.release_stream_workspaces()            # ... which stays this graph's: nothing else may be handed a pointer into the pool
        # the graph writes THESE gradient tensors; `optimizer.zero_grad(set_to_none=True)` between replays (the usual loop idiom)
        # detaches them from the parameters, and HipAdam would then skip every parameter silently: step() re-attaches them
        self._grads = [(p, p.grad) for group in optimizer.param_groups for p in group["params"] if p.grad is not None]

    def _fwd_bwd(self):
        inp, inp_s, tgt, tgt_s = self.batch
        # every forward here IS followed by its backward: the activation-saving forward at once, not inference kernels + a recompute
        # (PanguModel.eval_grad_mode; this class needs stochastic depth off, i.e. usually model.eval())
        mode, self.model.eval_grad_mode = getattr(self.model, "eval_grad_mode", "save"), "save"
        try:
            out, out_s = self.model(inp, inp_s, *self.consts)
        finally:
            self.model.eval_grad_mode = mode
        loss = weighted_l1_loss(out, out_s, tgt, tgt_s, stats_last=self.stats_last)      # normData folded into the loss passes
        loss.backward()
        return loss.detach()

    def step(self, batch=None):
        """Replay fwd + loss + bwd on `batch` (copied into the static buffers; None = the captured batch again), then one optimizer
        step; returns the (static) loss tensor."""
        if batch is not None:
            for dst, src in zip(self.batch, batch):
                dst.copy_(src)
        self.graph.replay()
        for p, g in self._grads:            # (see __init__: a zero_grad(set_to_none=True) in the caller's loop detached them)
            if p.grad is not g:
                p.grad = g
        self.optimizer.step()
        sh = getattr(self.model, "_shadow", None)
        if sh is not None and sh.cache:
            sh.refresh_in_place()
        return self.loss


def _owns_dropped_branches(grad_sync):
    """True when `grad_sync` is a bound method of dist.FlatGradSync (its flat buffer holds a zero for every parameter whose
    branch was dropped, and every rank launches every bucket whatever it drew)."""
    from .dist import FlatGradSync
    return isinstance(getattr(grad_sync, "__self__", None), FlatGradSync)


def _optimizer_tail(optimizer, grad_sync, grad_scale=1.0):
    """What follows the backward in train_step / rollout_train_step: the gradient sync, then the optimizer step in which parameters
    without a gradient (DropPath-dropped branches) get the reference's zero-gradient update.  grad_scale != 1 (accumulated
    backward passes): HipAdam scales inside its kernel; any other optimizer gets its gradients scaled with torch ops first."""
    hip = isinstance(optimizer, HipAdam)
    kw = {"grad_scale": grad_scale} if hip and grad_scale != 1.0 else {}
    if grad_sync is not None:
        grad_sync()
        _scale_grads(optimizer, 1.0 if hip else grad_scale)
        optimizer.step(**kw)
    elif hip:
        # a DropPath-dropped branch is not computed here, so its parameters come back without a gradient; the reference
        # computes the branch, multiplies by zero and hands Adam ZERO gradients (moments decay, weight decay applies)
        optimizer.step(missing_as_zero=True, **kw)
    else:
        for group in optimizer.param_groups:
            for p in group["params"]:
                if p.requires_grad and p.grad is None:
                    p.grad = torch.zeros_like(p)
        _scale_grads(optimizer, grad_scale)
        optimizer.step()


def _scale_grads(optimizer, grad_scale):
    if grad_scale != 1.0:
        grads = [p.grad for group in optimizer.param_groups for p in group["params"] if p.grad is not None]
        if grads:
            torch._foreach_mul_(grads, grad_scale)


def train_step(model, optimizer, batch, statistics, maps, const_h, stats_last=None, grad_sync=None, levels_reversed=False):
    """One optimisation step (reference pangu_sample.py:45-77). batch = (input, input_surface, target, target_surface).
    `grad_sync` (optional callable) runs between backward and optimizer.step(): the data-parallel gradient
    all-reduce (the reference's intended `gather_grad`, era5_data/utils_dist.py:125-134).
    `stats_last`: the targets are in physical units (`normData`, :57, folded into the loss kernel).
    `levels_reversed`: input and target carry their level axis as on disk (ascending); the reader's reversal
    (era5_data/utils_data.py:117) is done by the first / last kernel's addressing (data.DevicePrefetcher(fuse_flip=True)).

    Dropped-branch contract: a DropPath-dropped branch is not computed here, so the backward leaves its parameters WITHOUT a
    gradient and the arm that steps the optimizer hands them the reference's zero-gradient step (moments decay, weight decay
    applies).  That holds for grad_sync=None and for a dist.FlatGradSync method (flat buffer: zeros are already there, every rank
    launches every bucket).  Any OTHER grad_sync callable (e.g. dist.gather_grad, which all-reduces parameter by parameter and
    skips `p.grad is None`) sees materialised ZERO gradients instead: ranks that drew different DropPath patterns would
    otherwise issue different numbers of collectives (a hang) and the optimizer would skip those parameters."""
    inp, inp_s, tgt, tgt_s = batch
    optimizer.zero_grad(set_to_none=True)
    out, out_s = model(inp, inp_s, statistics, maps, const_h, levels_reversed=levels_reversed)
    loss = weighted_l1_loss(out, out_s, tgt, tgt_s, target_levels_reversed=levels_reversed, stats_last=stats_last)
    from . import ops
    lean = grad_sync is None or _owns_dropped_branches(grad_sync)
    with ops.dropped_branch_grads("none" if lean else "zeros"):
        loss.backward()
    _optimizer_tail(optimizer, grad_sync)
    return loss.detach()


def accumulated_train_step(model, optimizer, batches, statistics, maps, const_h, stats_last=None, grad_sync=None,
                           levels_reversed=False):
    """One optimisation step on the MEAN gradient of n batches (gradient accumulation: the per-rank batch is one sample, as in the
    reference, so this is how one GPU reaches the reference's effective batch of 8).  batches: a sequence of n train_step batches.
    zero_grad once; n forward / loss / backward passes under train_step's dropped-branch policy, autograd accumulating; `grad_sync`
    once, after the last backward; then train_step's optimizer tail with grad_scale = 1/n -- inside HipAdam's kernel (the
    gradients are not rewritten; a `max_grad_norm` clips the norm of the mean gradient), with torch ops for any other optimizer.
    A parameter is without a gradient only if its branch was dropped in all n passes.  Returns the mean of the n detached losses;
    nothing in here waits for the device.  n = 1 is train_step, bit for bit.
    Not with a dist.FlatGradSync method and n > 1 (its per-parameter hooks would fire, and launch its buckets, n times):
    RuntimeError, as rollout_train_step(checkpoint=True)."""
    batches = list(batches)
    n = len(batches)
    if n == 0:
        raise ValueError("accumulated_train_step: `batches` is empty")
    if n > 1 and grad_sync is not None and _owns_dropped_branches(grad_sync):
        raise RuntimeError(f"accumulated_train_step runs {n} backward passes, and a dist.FlatGradSync's per-parameter hooks would fire "
                           "(and launch its buckets) once per pass: use another grad_sync, or one batch per step")
    from . import ops
    lean = grad_sync is None or _owns_dropped_branches(grad_sync)
    optimizer.zero_grad(set_to_none=True)
    total = None
    for inp, inp_s, tgt, tgt_s in batches:
        out, out_s = model(inp, inp_s, statistics, maps, const_h, levels_reversed=levels_reversed)
        loss = weighted_l1_loss(out, out_s, tgt, tgt_s, target_levels_reversed=levels_reversed, stats_last=stats_last)
        with ops.dropped_branch_grads("none" if lean else "zeros"):
            loss.backward()
        total = loss.detach() if total is None else total + loss.detach()
        del out, out_s, loss
    _optimizer_tail(optimizer, grad_sync, 1.0 / n)
    return total if n == 1 else total / n


# ---- multi-step (rollout) fine-tuning ---------------------------------------------------------------------------------------


def _rollout_seed_torch(output, output_surface, target, target_surface, grad, d_next, d_next_surface, stats_last,
                        target_levels_reversed=False):
    """Torch form of `pangu_rollout_l1_seed_bwd` (what RolloutStepFn falls back to for tensors the HIP loss does not take): the
    gradient entering the model's output at one step of a chain = autograd's gradient of grad * weighted_l1_loss PLUS the next
    step's input gradient taken back through `rollout.norm_back` (out * std + mean: a multiply by std; one rounding, then the add)."""
    o, o_s = output.detach().requires_grad_(True), output_surface.detach().requires_grad_(True)
    with torch.enable_grad():
        loss = _weighted_l1_loss_torch(o, o_s, target, target_surface, target_levels_reversed, stats_last)
    d_o, d_os = torch.autograd.grad(loss, (o, o_s), grad.to(loss.dtype))
    if d_next is not None:
        _, s_std, _, u_std = stats_last
        d_o, d_os = d_o + d_next * u_std, d_os + d_next_surface * s_std
    return d_o, d_os


class RolloutStepFn(torch.autograd.Function):
    """One lead time of a K-step fine-tune, after the model: (out, out_surface) -> (loss_k, next_upper, next_surface).
    next_upper / next_surface are the PHYSICAL fields the forward's last kernel wrote under `ops.scatter_denorm` (the next step's
    input; None at the last step); they enter as plain buffers and leave as outputs of this node, so that the gradient the next
    step's input receives arrives HERE.  The backward is one launch (csrc/loss.hip `pangu_rollout_l1_seed_bwd`):
    d_out = d loss_k + d_next * std, written over the incoming d_next buffer.  The last step gets d_next = None
    (`set_materialize_grads(False)`) and runs the loss backward's own kernel."""

    @staticmethod
    def forward(ctx, output, output_surface, target, target_surface, next_upper, next_surface, target_levels_reversed, stats_last):
        ctx.set_materialize_grads(False)
        if stats_last is None:
            raise ValueError("RolloutStepFn: stats_last is required (the fed-back fields are de-normalised with it)")
        rev = bool(target_levels_reversed)
        nxt = (None, None) if next_upper is None else (next_upper.detach(), next_surface.detach())
        ctx.hip = _hip_loss_ok(output, output_surface, target, target_surface)
        if not ctx.hip:
            ctx.save_for_backward(output, output_surface, target, target_surface)
            ctx.rev, ctx.stats_last = rev, stats_last
            return (_weighted_l1_loss_torch(output, output_surface, target, target_surface, rev, stats_last),) + nxt
        from . import _lib
        wu, ws = _weights_on(output.device, torch.float32)
        with torch.cuda.device(output.device):
            loss = WeightedL1LossFn._forward(ctx, _lib.load(), wu, ws, output, output_surface, target, target_surface, rev, stats_last)
        return (loss,) + nxt

    @staticmethod
    def backward(ctx, g, d_next, d_next_surface):
        if not ctx.hip:
            output, output_surface, target, target_surface = ctx.saved_tensors
        else:
            output, output_surface, target, target_surface, u_mean, u_std, s_mean, s_std = ctx.saved_tensors
        if g is None:
            g = torch.zeros((), dtype=torch.float32, device=output.device)
        if (d_next is None) != (d_next_surface is None):        # one field of the next step's input was never read
            if d_next is None:
                d_next = torch.zeros_like(output)
            else:
                d_next_surface = torch.zeros_like(output_surface)
        if not ctx.hip:
            return _rollout_seed_torch(output, output_surface, target, target_surface, g, d_next, d_next_surface, ctx.stats_last,
                                       ctx.rev) + (None,) * 6
        from . import _lib
        from .ops import _stream
        wu, ws = _weights_on(output.device, torch.float32)
        g = g.to(torch.float32).contiguous()
        if d_next is None:
            d_o, d_os = torch.empty_like(output), torch.empty_like(output_surface)
            np_ = (None, None)
        else:
            # in place: the incoming buffers are this node's alone (the gradient of a tensor only the next step's model read)
            d_o, d_os = (t if t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
                         else t.to(torch.float32).clone(memory_format=torch.contiguous_format) for t in (d_next, d_next_surface))
            if d_o.shape != output.shape or d_os.shape != output_surface.shape:
                raise RuntimeError(f"rollout step: next-step input gradients {tuple(d_o.shape)} / {tuple(d_os.shape)} for outputs "
                                   f"{tuple(output.shape)} / {tuple(output_surface.shape)}")
            np_ = (d_o.data_ptr(), d_os.data_ptr())
        with torch.cuda.device(output.device):
            _lib.check(_lib.load().pangu_rollout_l1_seed_bwd(
                _stream(output), output.data_ptr(), target.data_ptr(), output_surface.data_ptr(), target_surface.data_ptr(),
                wu.data_ptr(), ws.data_ptr(), g.data_ptr(), *np_, u_std.data_ptr(), s_std.data_ptr(), d_o.data_ptr(), d_os.data_ptr(),
                *ctx.geom, int(ctx.rev), u_mean.data_ptr(), u_std.data_ptr(), s_mean.data_ptr(), s_std.data_ptr()),
                "rollout_l1_seed_bwd")
        return d_o, d_os, None, None, None, None, None, None


def _check_rollout_batch(batch, stats_last, lead_weights):
    batch = tuple(batch)
    if len(batch) < 4 or len(batch) % 2:
        raise ValueError("rollout_train_step: batch = (input, input_surface, target_1, target_surface_1, ..., target_K, "
                         f"target_surface_K): got {len(batch)} tensors (the target list is empty or odd)")
    K = len(batch) // 2 - 1
    if stats_last is None or len(stats_last) != 4:
        raise ValueError("rollout_train_step: stats_last = (s_mean, s_std, u_mean, u_std) is required: the fed-back fields are "
                         "de-normalised with it, and the targets are in physical units")
    lam = [1.0 / K] * K if lead_weights is None else [float(w) for w in lead_weights]
    if len(lam) != K:
        raise ValueError(f"rollout_train_step: {len(lam)} lead_weights for K = {K} lead times")
    inp, inp_s = batch[0], batch[1]
    if inp.dim() != 5 or inp_s.dim() != 4 or inp_s.shape[0] != inp.shape[0] or inp_s.shape[-2:] != inp.shape[-2:]:
        raise ValueError(f"rollout_train_step: input {tuple(inp.shape)} / input_surface {tuple(inp_s.shape)}: expected "
                         "(1, 5, 13, LAT, LON) / (1, 4, LAT, LON)")
    if inp.shape[0] != 1:
        raise ValueError(f"rollout_train_step: the per-rank batch is one sample (as in the reference), got B = {inp.shape[0]}")
    for k in range(K):
        t, t_s = batch[2 + 2 * k], batch[3 + 2 * k]
        if t.shape != inp.shape or t_s.shape != inp_s.shape:
            raise ValueError(f"rollout_train_step: target {k + 1} is {tuple(t.shape)} / {tuple(t_s.shape)}, the fields are "
                             f"{tuple(inp.shape)} / {tuple(inp_s.shape)}")
    if not all(t.is_cuda for t in batch):
        raise RuntimeError("rollout_train_step: the batch must live on the model's HIP device (got CPU tensors); there is no CPU "
                           "fallback")
    if any(t.device != inp.device for t in batch):
        raise RuntimeError("rollout_train_step: the batch tensors are on different devices")
    return batch, K, lam


def _weighted_total(losses, lam):
    total = losses[0] * lam[0]
    for l, w in zip(losses[1:], lam[1:]):
        total = total + l * w
    return total


def rollout_train_step(model, optimizer, batch, statistics, maps, const_h, stats_last, *, lead_weights=None, checkpoint=False,
                       grad_sync=None, levels_reversed=False):
    """One optimisation step on a loss summed over K autoregressive 24 h steps, gradients flowing back through the fed-back state.
    batch = (input, input_surface, target_1, target_surface_1, ..., target_K, target_surface_K), targets in PHYSICAL units, one
    sample (what data.DevicePrefetcher yields with extra `*rest` tensors; K = 1 is train_step's batch and train_step's result).
    total = sum_k lead_weights[k] * loss_k (default 1/K each).  Returns (total, per_step): detached device tensors of shape () and
    (K,); nothing in here waits for the device.

    Step k runs the model inside `ops.scatter_denorm`, so its last kernel also writes the physical fields of step k+1 (the two
    roundings of rollout.norm_back, no extra pass); the loss is `pangu_weighted_l1_loss_fwd`; and the backward of each step starts
    with ONE launch that forms d loss_k + (gradient of step k+1's input) * std (RolloutStepFn).
    `levels_reversed` applies to step 0's input and to every target; fed-back fields are in the model's level order.

    checkpoint=False: one autograd graph over all K steps, one backward (memory grows by one step's activations per lead time);
    works with a dist.FlatGradSync method as `grad_sync` (its hooks fire once per parameter).
    checkpoint=True: pass 1 runs the K forwards keeping only each step's two input fields (0.6 GB per lead time) and the host RNG
    state in front of it; then, last step first, each step is re-run with gradients under that RNG state (the same DropPath draws),
    its loss and backward run with the d_next of the step after it, and its input gradient is kept for the step before it.  Peak
    memory is one step's.  The host RNG ends where pass 1 left it, as with checkpoint=False.  The DropPath counters (`n_dropped`,
    `n_dropped_branch`) count the recomputed forwards too: the branches of every step but the last are counted twice.  Not with a FlatGradSync method
    (its per-parameter hooks would fire K times): RuntimeError; any other `grad_sync` callable runs after the last backward.

    Dropped-branch contract and optimizer tail: train_step's; a parameter is without a gradient only if its branch was dropped in
    all K steps."""
    batch, K, lam = _check_rollout_batch(batch, stats_last, lead_weights)
    if checkpoint and grad_sync is not None and _owns_dropped_branches(grad_sync):
        raise RuntimeError("rollout_train_step(checkpoint=True) runs K backward passes, and a dist.FlatGradSync's per-parameter hooks "
                           "would fire (and launch its buckets) K times: use checkpoint=False with FlatGradSync, or another grad_sync")
    from . import ops
    inp, inp_s = batch[0], batch[1]
    targets = [(batch[2 + 2 * k], batch[3 + 2 * k]) for k in range(K)]
    consts = (statistics, maps, const_h)
    lean = grad_sync is None or _owns_dropped_branches(grad_sync)
    policy = "none" if lean else "zeros"
    optimizer.zero_grad(set_to_none=True)

    def forward_step(k, cur, cur_s, feed):
        """(out, out_surface, next_upper, next_surface): the model on step k's input; with `feed`, its last kernel also writes the
        next step's physical input fields."""
        rev = levels_reversed and k == 0
        if not feed:
            return model(cur, cur_s, *consts, levels_reversed=rev) + (None, None)
        nxt, nxt_s = torch.empty_like(inp), torch.empty_like(inp_s)
        with ops.scatter_denorm(nxt, nxt_s, stats_last):
            return model(cur, cur_s, *consts, levels_reversed=rev) + (nxt, nxt_s)

    if not checkpoint:
        cur, cur_s, losses = inp, inp_s, []
        for k in range(K):
            out, out_s, nxt, nxt_s = forward_step(k, cur, cur_s, k + 1 < K)
            loss_k, cur, cur_s = RolloutStepFn.apply(out, out_s, *targets[k], nxt, nxt_s, levels_reversed, stats_last)
            losses.append(loss_k)
        total = _weighted_total(losses, lam)
        with ops.dropped_branch_grads(policy):
            total.backward()
        _optimizer_tail(optimizer, grad_sync)
        return total.detach(), torch.stack([l.detach() for l in losses])

    # pass 1: the same forwards (same kernels: the fed-back fields and every out_k are those of the other mode, bit for bit); each
    # step's graph dies with its outputs, only the step's input fields and the RNG state in front of it are kept
    fields, rng = [(inp, inp_s)], []
    for k in range(K - 1):
        rng.append(torch.get_rng_state())
        out, out_s, nxt, nxt_s = forward_step(k, *fields[k], True)
        del out, out_s
        fields.append((nxt, nxt_s))
    rng.append(torch.get_rng_state())
    losses, d_next, rng_end = [None] * K, (None, None), None
    for k in range(K - 1, -1, -1):
        if k < K - 1:
            torch.set_rng_state(rng[k])
        cur, cur_s = fields[k]
        if k > 0:                                     # a fed-back state: its gradient is the d_next of the step before
            cur.requires_grad_(True)
            cur_s.requires_grad_(True)
        out, out_s, _, _ = forward_step(k, cur, cur_s, False)
        if k == K - 1:
            rng_end = torch.get_rng_state()           # where one pass over all K steps leaves the generator
        nxt, nxt_s = fields[k + 1] if k + 1 < K else (None, None)
        loss_k, nxt, nxt_s = RolloutStepFn.apply(out, out_s, *targets[k], nxt, nxt_s, levels_reversed, stats_last)
        losses[k] = loss_k.detach()
        roots, seeds = [loss_k], [torch.full((), lam[k], dtype=loss_k.dtype, device=loss_k.device)]
        if d_next[0] is not None:
            roots += [nxt, nxt_s]
            seeds += list(d_next)
        del out, out_s
        with ops.dropped_branch_grads(policy):
            torch.autograd.backward(roots, seeds)
        d_next = (cur.grad, cur_s.grad) if k > 0 else (None, None)
        if k + 1 < K:
            fields[k + 1] = None
    torch.set_rng_state(rng_end)
    _optimizer_tail(optimizer, grad_sync)
    return _weighted_total(losses, lam), torch.stack(losses)


# ---- fair-CRPS ensemble fine-tuning -------------------------------------------------------------------------------------------

CRPS_MIN_MEMBERS, CRPS_MAX_MEMBERS = 2, 16      # csrc/crps_loss.hip keeps the E values of an element in registers

_crps_lat = {}      # (H, device) -> max(score.latitude_weights(H), 0), fp32 on the device


def _crps_lat_weights(H, device):
    """The latitude weights of the fair-CRPS loss: score.latitude_weights clamped at zero (see fair_crps_loss)."""
    key = (int(H), str(device))
    a = _crps_lat.get(key)
    if a is None:
        from . import score
        a = _crps_lat[key] = score.latitude_weights(H, device).clamp_min(0.0).contiguous()
    return a


def _check_member_count(E, who):
    if not CRPS_MIN_MEMBERS <= E <= CRPS_MAX_MEMBERS:
        raise ValueError(f"{who}: {CRPS_MIN_MEMBERS} <= members <= {CRPS_MAX_MEMBERS}, got {E}")


def _fair_crps_loss_torch(outputs, outputs_surface, target, target_surface, target_levels_reversed=False, stats_last=None,
                          lat_weighted=True):
    """The definition of fair_crps_loss as torch ops (any device, any floating dtype; the reference of the tests): O(E^2) passes
    over the fields."""
    E = len(outputs)
    if target_levels_reversed:
        target = target.flip(-3)
    if stats_last is not None:
        target, target_surface = norm_data(target, target_surface, stats_last)
    dev, dt = outputs[0].device, outputs[0].dtype
    wu, ws = _weights_on(dev, dt)
    a = _crps_lat_weights(outputs[0].shape[-2], dev).to(dt).view(-1, 1) if lat_weighted else None

    def mean_crps(xs, t, w):
        s1 = sum((x - t).abs() for x in xs)
        s2 = sum((xs[e] - xs[f]).abs() for e in range(1, E) for f in range(e))       # every pair once: 2 / (2E(E-1))
        c = (s1 / E - s2 / (E * (E - 1))) * w
        return torch.mean(c if a is None else c * a)

    return mean_crps(outputs, target, wu) + mean_crps(outputs_surface, target_surface, ws) * 0.25


def _crps_geom(upper, surface):
    return (upper.shape[0], upper.shape[1], upper.shape[2], surface.shape[1], upper.shape[-2], upper.shape[-1])


def _crps_pointers(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _fair_crps_launch_fwd(outputs, outputs_surface, target, target_surface, rev, st, lat):
    """The forward launch pair on contiguous fp32 device fields -> loss (3,) = (total, upper mean, surface mean)."""
    from . import _lib
    from .ops import _stream
    lib = _lib.load()
    E, o = len(outputs), outputs[0]
    geom = _crps_geom(o, outputs_surface[0])
    nblk = lib.pangu_fair_crps_loss_blocks(E, *geom)
    if nblk <= 0:
        raise RuntimeError(f"fair_crps_loss: unsupported shapes {tuple(o.shape)} {tuple(outputs_surface[0].shape)} x {E} members")
    wu, ws = _weights_on(o.device, torch.float32)
    sp = tuple(t.data_ptr() for t in st) if st else (None,) * 4
    partial = torch.empty((nblk,), dtype=torch.float32, device=o.device)
    loss = torch.empty((3,), dtype=torch.float32, device=o.device)
    with torch.cuda.device(o.device):
        _lib.check(lib.pangu_fair_crps_loss_fwd(
            _stream(o), _crps_pointers(outputs), _crps_pointers(outputs_surface), E, target.data_ptr(), target_surface.data_ptr(),
            wu.data_ptr(), ws.data_ptr(), None if lat is None else lat.data_ptr(), partial.data_ptr(), loss.data_ptr(), *geom,
            int(rev), *sp), "fair_crps_loss_fwd")
    return loss


def _fair_crps_launch_bwd(outputs, outputs_surface, target, target_surface, rev, st, lat, g, d_outputs, d_outputs_surface):
    """The backward launch: d_outputs[e] / d_outputs_surface[e] may be outputs[e] / outputs_surface[e] themselves."""
    from . import _lib
    from .ops import _stream
    E, o = len(outputs), outputs[0]
    wu, ws = _weights_on(o.device, torch.float32)
    sp = tuple(t.data_ptr() for t in st) if st else (None,) * 4
    with torch.cuda.device(o.device):
        _lib.check(_lib.load().pangu_fair_crps_loss_bwd(
            _stream(o), _crps_pointers(outputs), _crps_pointers(outputs_surface), E, target.data_ptr(), target_surface.data_ptr(),
            wu.data_ptr(), ws.data_ptr(), None if lat is None else lat.data_ptr(), g.data_ptr(), _crps_pointers(d_outputs),
            _crps_pointers(d_outputs_surface), *_crps_geom(o, outputs_surface[0]), int(rev), *sp), "fair_crps_loss_bwd")


class FairCrpsLossFn(torch.autograd.Function):
    """fair_crps_loss on the device: one forward launch pair (block partials, fp64 final sum) and one backward launch that writes
    all 2E gradient fields (csrc/crps_loss.hip).  apply(target, target_surface, target_levels_reversed, stats_last, lat_weighted,
    *outputs, *outputs_surface)."""

    @staticmethod
    def forward(ctx, target, target_surface, target_levels_reversed, stats_last, lat_weighted, *fields):
        E = len(fields) // 2
        outputs, outputs_surface = fields[:E], fields[E:]
        o = outputs[0]
        st = _flat_stats(stats_last, o.device, o.shape[1], o.shape[2], outputs_surface[0].shape[1]) if stats_last is not None else ()
        lat = _crps_lat_weights(o.shape[-2], o.device) if lat_weighted else None
        loss = _fair_crps_launch_fwd(outputs, outputs_surface, target, target_surface, target_levels_reversed, st, lat)
        ctx.save_for_backward(target, target_surface, *fields, *st)
        ctx.E, ctx.rev, ctx.lat = E, bool(target_levels_reversed), lat
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        E = ctx.E
        target, target_surface, *rest = ctx.saved_tensors
        outputs, outputs_surface, st = rest[:E], rest[E:2 * E], rest[2 * E:]
        d_o, d_os = [torch.empty_like(t) for t in outputs], [torch.empty_like(t) for t in outputs_surface]
        _fair_crps_launch_bwd(outputs, outputs_surface, target, target_surface, ctx.rev, st, ctx.lat,
                              g.to(torch.float32).contiguous(), d_o, d_os)
        return (None,) * 5 + tuple(d_o) + tuple(d_os)


def _hip_crps_ok(outputs, outputs_surface, target, target_surface):
    o, o_s = outputs[0], outputs_surface[0]
    return (all(_hip_loss_ok(x, x_s, target, target_surface) for x, x_s in zip(outputs, outputs_surface))
            and all(x.device == o.device and x.shape == o.shape for x in outputs)
            and all(x.shape == o_s.shape for x in outputs_surface) and o.shape[-2:] == o_s.shape[-2:])


def fair_crps_loss(outputs, outputs_surface, target, target_surface, target_levels_reversed=False, stats_last=None,
                   lat_weighted=True):
    """The fair (unbiased-in-E) CRPS of E member forecasts against one target, in weighted_l1_loss's shape -- the score
    score.ensemble_scores reports, as a differentiable training loss.  outputs / outputs_surface: sequences of E (2..16) member
    fields, normalised, (1,5,13,H,W) / (1,4,H,W); target / target_surface, target_levels_reversed, stats_last: as weighted_l1_loss.
    Per grid point
        c = (1/E) sum_e |x_e - t|  -  1/(2E(E-1)) sum_e sum_f |x_e - x_f|
        loss = mean(w_upper[var] * a[h] * c) + 0.25 * mean(w_surface[var] * a[h] * c_surface)
    lat_weighted: a[h] = max(score.latitude_weights(H)[h], 0), else a = 1.  The clamp: the reference's `3.1416` literal for pi makes
    the weight of the last latitude row -7.5e-6, and a loss must not reward error there; the effect on the value is about 1e-8
    relative.  With identical members and lat_weighted=False this is weighted_l1_loss.
    Contiguous fp32 fields on one HIP device take the HIP form (FairCrpsLossFn: the fields are read once per direction, where the
    torch expression makes O(E^2) passes); anything else (other dtypes, CPU tensors, targets that need gradients) the torch
    expression `_fair_crps_loss_torch`."""
    outputs, outputs_surface = tuple(outputs), tuple(outputs_surface)
    _check_member_count(len(outputs), "fair_crps_loss")
    if len(outputs_surface) != len(outputs):
        raise ValueError(f"fair_crps_loss: {len(outputs)} upper-air and {len(outputs_surface)} surface member fields")
    if _hip_crps_ok(outputs, outputs_surface, target, target_surface):
        return FairCrpsLossFn.apply(target, target_surface, bool(target_levels_reversed), stats_last, bool(lat_weighted),
                                    *outputs, *outputs_surface)
    return _fair_crps_loss_torch(outputs, outputs_surface, target, target_surface, target_levels_reversed, stats_last, lat_weighted)


def _check_ensemble_batch(batch, stats_last, members, amplitude, octaves, period):
    from . import ensemble
    if not isinstance(members, int) or isinstance(members, bool):
        raise ValueError(f"ensemble_train_step: members must be an int, got {members!r}")
    _check_member_count(members, "ensemble_train_step")
    ensemble._amplitude9(amplitude)
    batch = tuple(batch)
    if len(batch) != 4:
        raise ValueError(f"ensemble_train_step: batch = (input, input_surface, target, target_surface): got {len(batch)} tensors")
    if stats_last is None or len(stats_last) != 4:
        raise ValueError("ensemble_train_step: stats_last = (s_mean, s_std, u_mean, u_std) is required: the perturbations are scaled "
                         "with it, and the targets are in physical units")
    inp, inp_s, tgt, tgt_s = batch
    if inp.dim() != 5 or inp_s.dim() != 4 or inp_s.shape[0] != inp.shape[0] or inp_s.shape[-2:] != inp.shape[-2:]:
        raise ValueError(f"ensemble_train_step: input {tuple(inp.shape)} / input_surface {tuple(inp_s.shape)}: expected "
                         "(1, 5, 13, LAT, LON) / (1, 4, LAT, LON)")
    if inp.shape[0] != 1:
        raise ValueError(f"ensemble_train_step: the per-rank batch is one sample (as in the reference), got B = {inp.shape[0]}")
    if tgt.shape != inp.shape or tgt_s.shape != inp_s.shape:
        raise ValueError(f"ensemble_train_step: the target is {tuple(tgt.shape)} / {tuple(tgt_s.shape)}, the fields are "
                         f"{tuple(inp.shape)} / {tuple(inp_s.shape)}")
    ensemble._check_lattice(inp.shape[-1], octaves, period)
    return batch


def ensemble_train_step(model, optimizer, batch, statistics, maps, const_h, stats_last, *, members, amplitude, seed,
                        checkpoint=True, lat_weighted=True, grad_sync=None, octaves=3, period=12, persistence=0.5, control=True):
    """One optimisation step on the fair CRPS (fair_crps_loss) of `members` perturbed forecasts of one sample: the model is
    fine-tuned on the score its ensembles are judged by (score.ensemble_scores).  batch = train_step's (input, input_surface,
    target, target_surface): one sample in the model's level order, targets in PHYSICAL units, on the device.  The member inputs
    are the sample under ensemble.perturb_(amplitude, seed, octaves, period, persistence, control) -- amplitude is required, the
    project has no calibrated default.  Returns the detached loss; nothing in here waits for the device.

    checkpoint=True: pass 1 runs the E forwards keeping only each member's two output fields (0.3 GB) and the host RNG state in
    front of it -- with the kernels of the training forward, so that the recomputed outputs are the ones the loss saw, bit for
    bit; one loss forward and one loss backward launch then write every member's output gradient over the kept outputs; then each
    member is re-run with gradients under its RNG state (the same DropPath draws) and back-propagated from those gradients,
    parameter gradients accumulating over the members.  Peak memory is one step's activations plus the member fields.  The host
    RNG ends where pass 1 left it; the DropPath counters count every forward twice.  Not with a dist.FlatGradSync method (its
    per-parameter hooks would fire E times): RuntimeError, as rollout_train_step(checkpoint=True); any other `grad_sync` callable
    runs after the last backward.
    checkpoint=False: one autograd graph over the E forwards and FairCrpsLossFn, one backward (memory grows by one step's
    activations per member); works with a dist.FlatGradSync method.

    zero_grad once; dropped-branch contract and optimizer tail: train_step's; a parameter is without a gradient only if its branch
    was dropped in all E forwards."""
    inp, inp_s, tgt, tgt_s = _check_ensemble_batch(batch, stats_last, members, amplitude, octaves, period)
    if checkpoint and grad_sync is not None and _owns_dropped_branches(grad_sync):
        raise RuntimeError("ensemble_train_step(checkpoint=True) runs E backward passes, and a dist.FlatGradSync's per-parameter hooks "
                           "would fire (and launch its buckets) E times: use checkpoint=False with FlatGradSync, or another grad_sync")
    if not all(t.is_cuda for t in (inp, inp_s, tgt, tgt_s)):
        raise RuntimeError("ensemble_train_step: the batch must live on the model's HIP device (got CPU tensors); there is no CPU "
                           "fallback")
    if any(t.device != inp.device for t in (inp_s, tgt, tgt_s)):
        raise RuntimeError("ensemble_train_step: the batch tensors are on different devices")
    from . import ensemble, ops
    E = members
    consts = (statistics, maps, const_h)
    policy = "none" if grad_sync is None or _owns_dropped_branches(grad_sync) else "zeros"
    up = inp.to(torch.float32).expand(E, *inp.shape[1:]).contiguous()
    sf = inp_s.to(torch.float32).expand(E, *inp_s.shape[1:]).contiguous()
    ensemble.perturb_(up, sf, stats_last, amplitude, seed, octaves=octaves, period=period, persistence=persistence, control=control)
    optimizer.zero_grad(set_to_none=True)

    if not checkpoint:
        outs = [model(up[e:e + 1], sf[e:e + 1], *consts) for e in range(E)]
        loss = fair_crps_loss([o for o, _ in outs], [o_s for _, o_s in outs], tgt, tgt_s, stats_last=stats_last,
                              lat_weighted=lat_weighted)
        del outs
        with ops.dropped_branch_grads(policy):
            loss.backward()
        _optimizer_tail(optimizer, grad_sync)
        return loss.detach()

    # pass 1: each member's graph dies with its outputs; only the two output fields and the RNG state in front of the forward stay
    rng, kept, kept_s = [], [], []
    for e in range(E):
        rng.append(torch.get_rng_state())
        out, out_s = model(up[e:e + 1], sf[e:e + 1], *consts)
        kept.append(out.detach())
        kept_s.append(out_s.detach())
        del out, out_s
    rng_end = torch.get_rng_state()
    if not _hip_crps_ok(kept, kept_s, tgt, tgt_s):
        raise RuntimeError("ensemble_train_step: model outputs and targets must be contiguous float32 fields of one shape on one "
                           "HIP device")
    st = _flat_stats(stats_last, inp.device, kept[0].shape[1], kept[0].shape[2], kept_s[0].shape[1])
    lat = _crps_lat_weights(kept[0].shape[-2], inp.device) if lat_weighted else None
    loss = _fair_crps_launch_fwd(kept, kept_s, tgt, tgt_s, False, st, lat)[0]
    one = torch.ones((), dtype=torch.float32, device=inp.device)
    _fair_crps_launch_bwd(kept, kept_s, tgt, tgt_s, False, st, lat, one, kept, kept_s)       # in place: kept now holds d loss / d out
    for e in range(E):
        torch.set_rng_state(rng[e])
        out, out_s = model(up[e:e + 1], sf[e:e + 1], *consts)
        with ops.dropped_branch_grads(policy):
            torch.autograd.backward([out, out_s], [kept[e], kept_s[e]])
        del out, out_s
        kept[e] = kept_s[e] = None
    torch.set_rng_state(rng_end)
    _optimizer_tail(optimizer, grad_sync)
    return loss
