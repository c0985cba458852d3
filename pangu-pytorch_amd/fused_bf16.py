"""bf16 precision of the whole model (BASELINE configs[2]/[4]): bf16 activations + bf16 weight shadows, fp32 LayerNorm /
softmax / accumulation, fp32 output fields.  `WeightShadow` keeps the bf16 images of the fp32 parameters; the forward, training
and inference, is the driver of fused.py run with the model's WeightShadow."""
import torch

from . import ops, ops_bf16 as ob


class WeightShadow:
    """bf16 copies of the projection weights and bias tables (and the transposed / packed weight images of the backward GEMMs
    and the fused MLP kernel), re-made when a parameter's stamp changes (ops.param_stamp).  Never pickled / deep-copied with
    the model (PanguModel.__getstate__).

    After an optimizer step EVERY copy is stale.  Each copy made from contiguous fp32 parameters is also recorded as a job
    (cast / transposed cast / gather through the MLP pack index) of `pangu_shadow_refresh_bf16`; the first lookup of a new
    optimizer epoch re-makes all recorded copies IN PLACE with one launch over a device-resident job table (1.56 GB of HBM
    traffic, ~0.3 ms) instead of ~240 small torch launches (1.6 ms of GPU time, 10 ms of host time per training step)."""

    def __init__(self):
        ops.require_epoch_hook()
        self.cache = {}          # key -> (stamp, tensor)
        self.jobs = {}           # key -> (mode, params, dst, idx, n0, n1, blocks, signature of the params)
        self.table = None        # (device int64 job table, keys in table order, total blocks, keys left out)
        self.bulk_epoch = ops._weights_epoch[0]
        self.makers = {}         # key -> (params, make) of the copies that are NOT bulk-refresh jobs (padded casts): refresh_in_place
        self.fresh = {}          # key -> (epoch, param _version, param address) when an optimizer wrote that copy itself (train.HipAdam): skipped by the next refresh

    def clear(self):
        self.cache.clear()
        self.jobs.clear()
        self.makers.clear()
        self.fresh.clear()
        self.table = None

    def plain_image(self, p):
        """The recorded plain bf16 cast of parameter `p` (None when there is none or it no longer matches `p`): an optimizer that
        updates `p` may write this image in the same pass (train.HipAdam) and call `mark_fresh(p)`."""
        j = self.jobs.get(id(p))
        if j is None or j[0] != 0 or self._sig(j[1]) != j[7] or self.cache.get(id(p), (None, None))[1] is not j[2]:
            return None
        return j[2]

    def mark_fresh(self, p):
        """`plain_image(p)` was just re-written from the updated `p` by the optimizer step in progress (epoch = the current one;
        the post-step hook advances it): the refresh of the NEXT epoch -- and only that one -- leaves it out."""
        # (the parameter's `_version` and address at this moment: HipAdam's raw-pointer kernel bumps neither, so an in-place edit
        # before the next forward -- load_state_dict(best), an EMA swap, a weight clamp -- is what changes them, and the image
        # written here is then stale like every other copy)
        self.fresh[id(p)] = (ops._weights_epoch[0], p._version, p.data_ptr())

    @staticmethod
    def _sig(params):
        return tuple((p.data_ptr(), tuple(p.shape), p.device, p.dtype) for p in params)

    def _record(self, key, mode, params, dst, idx=None):
        """Remember how `dst` derives from `params` (all contiguous fp32 on dst's device), for the bulk refresh."""
        if not dst.is_cuda or not dst.is_contiguous() or dst.dtype != torch.bfloat16:
            return
        if any(p.dtype != torch.float32 or not p.is_contiguous() or p.device != dst.device for p in params):
            return
        if mode == 0:
            n0, n1 = params[0].numel(), 0
            blocks = (n0 + 4095) // 4096
        elif mode == 1:
            n0 = params[0].shape[0]
            n1 = params[0].numel() // n0
            blocks = ((n0 + 63) // 64) * ((n1 + 63) // 64)
        else:
            n0, n1 = params[0].numel(), dst.numel()
            blocks = (n1 + 4095) // 4096
        if blocks == 0 or dst.numel() != (n1 if mode == 2 else params[0].numel()):
            return
        self.jobs[key] = (mode, params, dst, idx, n0, n1, blocks, self._sig(params))
        self.table = None

    def _bulk_refresh(self):
        """One launch re-makes every recorded copy whose parameters still live where they did; the others are dropped and
        re-made lazily by their next lookup."""
        for key in [k for k, j in self.jobs.items() if self._sig(j[1]) != j[7] or self.cache.get(k, (None, None))[1] is not j[2]]:
            del self.jobs[key]
            self.cache.pop(key, None)
            self.table = None
        if not self.jobs:
            return
        from . import _lib
        # copies an optimizer wrote itself during the ONE step since the last epoch (exactly one: any other optimizer step in
        # between could have touched the parameter again)
        ep = ops._weights_epoch[0]
        skip = frozenset(k for k, (e, ver, ptr) in self.fresh.items()
                         if e == ep - 1 and k in self.jobs and self.jobs[k][1][0]._version == ver and self.jobs[k][1][0].data_ptr() == ptr)
        self.fresh.clear()
        if self.table is None or self.table[3] != skip:
            rows, keys, first = [], [], 0
            for key, (mode, params, dst, idx, n0, n1, blocks, _) in self.jobs.items():
                if key in skip:
                    continue
                rows.append([params[0].data_ptr(), params[1].data_ptr() if len(params) > 1 else 0, dst.data_ptr(),
                             idx.data_ptr() if idx is not None else 0, n0, n1, mode, first])
                keys.append(key)
                first += blocks
            rows.append([0, 0, 0, 0, 0, 0, 0, first])
            dev = next(iter(self.jobs.values()))[2].device
            self.table = (torch.tensor(rows, dtype=torch.int64).to(dev), keys, first, skip)
        table, keys, total, _ = self.table
        if keys:
            _lib.check(_lib.load().pangu_shadow_refresh_bf16(ob._stream(table), table.data_ptr(), len(keys), total), "shadow_refresh_bf16")
        for key in list(keys) + list(skip):
            self.cache[key] = (tuple(ops.param_stamp(p) for p in self.jobs[key][1]), self.jobs[key][2])

    def _lookup(self, key, params, make, mode=None, idx=None):
        ep = ops._weights_epoch[0]
        if self.bulk_epoch != ep:
            self.bulk_epoch = ep
            if self.jobs:
                self._bulk_refresh()
        stamp = tuple(ops.param_stamp(p) for p in params)
        hit = self.cache.get(key)
        if hit is not None and hit[0] == stamp:
            return hit[1]
        w = make()
        self.cache[key] = (stamp, w)
        if self.jobs.pop(key, None) is not None:
            self.table = None
        if mode is not None:
            self._record(key, mode, params, w, idx() if callable(idx) else idx)
        if key not in self.jobs:
            self.makers[key] = (params, make)
        else:
            self.makers.pop(key, None)
        return w

    def refresh_in_place(self):
        """Re-make EVERY cached copy now, INTO the tensors it already lives in -- for a captured training step
        (train.GraphedTrainStep), whose graph holds the shadows' addresses and runs no Python that could notice a new optimizer
        epoch: call after `optimizer.step()`.  The recorded jobs take the one-launch bulk refresh, the few others (padded casts)
        an in-place copy."""
        self.bulk_epoch = ops._weights_epoch[0]
        if self.jobs:
            self._bulk_refresh()
        with torch.no_grad():
            for key, (params, make) in list(self.makers.items()):
                hit = self.cache.get(key)
                if hit is None or key in self.jobs:
                    continue
                hit[1].copy_(make())
                self.cache[key] = (tuple(ops.param_stamp(p) for p in params), hit[1])

    @staticmethod
    def _lora_owner(p):
        """The LoraLinear whose W_eff the tensor `p` is (layers.LoraLinear.effective_weight tags it with a weak reference), or None:
        a parameter, or a W_eff whose module is gone."""
        ref = getattr(p, "_lora_owner", None)
        return ref() if ref is not None else None

    def _lora_lookup(self, kind, lin, p, cast):
        """The `kind` image of the adapted projection `lin`, asked for through its W_eff tensor `p` (the layer Functions of the
        training path hold that tensor, not the module).  W_eff is a fresh tensor per refresh, so the image is keyed by the MODULE
        and stamped by (W, A, B), like get_lin -- keyed by id(p), every optimizer step would leave a dead entry behind -- and made
        lazily, never as a bulk-refresh job (those run before W_eff is current).  A `p` that its module has replaced since (a
        backward that outlived an optimizer step) gets a one-off cast that is not cached."""
        if p is not lin._w_eff or lin._w_eff_stamp != lin._stamp():
            return cast(p.detach())
        return self._lookup((kind, id(lin)), (lin.weight, lin.lora_A, lin.lora_B), lambda: cast(lin.effective_weight()))

    def get(self, p, pad_k=None):
        lin = self._lora_owner(p)
        if lin is not None:
            return self._lora_lookup("lora", lin, p, lambda w: w.to(torch.bfloat16).contiguous())

        def make():
            w = p.detach().reshape(p.shape[0], -1) if p.dim() == 3 else p.detach()
            if p.dim() == 5:
                w = w[0]
            if pad_k is not None and w.shape[1] < pad_k:
                w = torch.nn.functional.pad(w, (0, pad_k - w.shape[1]))
            return w.to(torch.bfloat16).contiguous()
        padded = pad_k is not None and p.dim() >= 2 and p.numel() // p.shape[0] < pad_k
        return self._lookup(id(p), (p,), make, mode=None if padded else 0)

    def get_lin(self, lin):
        """bf16 shadow of a projection's weight: `get(lin.weight)` for a plain nn.Linear; for a LoraLinear the cast of its W_eff,
        keyed by the stamps of W, A and B (made lazily, never a bulk-refresh job: those run before W_eff is current)."""
        from .layers import eff_weight
        return self.get(eff_weight(lin))

    def get_mlp_lin(self, l1, l2):
        """`get_mlp` of an Mlp's two projections, on W_eff where they carry adapters."""
        from .layers import eff_weight
        return self.get_mlp(eff_weight(l1), eff_weight(l2))

    def get_t(self, p):
        """Transposed bf16 shadow (in, out): the `W` operand of the input-gradient GEMM dA = dC @ W."""
        lin = self._lora_owner(p)
        if lin is not None:
            return self._lora_lookup("lora-t", lin, p, lambda w: w.t().to(torch.bfloat16).contiguous())
        return self._lookup(("t", id(p)), (p,),
                            lambda: p.detach().reshape(p.shape[0], -1).t().to(torch.bfloat16).contiguous(), mode=1)

    def get_mlp(self, w1, w2):
        """Packed chunk image of an Mlp's two weights for the fused MLP kernel (ops_bf16.pack_mlp_weights).  Where a weight is the
        W_eff of an adapted projection the image is keyed by that module and stamped by its (W, A, B), as in _lora_lookup."""
        lins = (self._lora_owner(w1), self._lora_owner(w2))
        if lins[0] is None and lins[1] is None:
            return self._lookup(("mlp", id(w1), id(w2)), (w1, w2), lambda: ob.pack_mlp_weights(w1.detach(), w2.detach()),
                                mode=2, idx=lambda: ob.mlp_pack_index32(w1.shape[1], w1.device))
        if any(l is not None and (w is not l._w_eff or l._w_eff_stamp != l._stamp()) for l, w in zip(lins, (w1, w2))):
            return ob.pack_mlp_weights(w1.detach(), w2.detach())
        src = tuple((lambda l=l: l.effective_weight()) if l is not None else (lambda w=w: w.detach()) for l, w in zip(lins, (w1, w2)))
        params = tuple(q for l, w in zip(lins, (w1, w2)) for q in ((l.weight, l.lora_A, l.lora_B) if l is not None else (w,)))
        return self._lookup(("mlp-lora",) + tuple(id(l) if l is not None else id(w) for l, w in zip(lins, (w1, w2))), params,
                            lambda: ob.pack_mlp_weights(src[0](), src[1]()))
