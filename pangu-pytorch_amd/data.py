"""Input pipeline: keep the GPU fed once a step takes tens of milliseconds.

The reference's loop moves four pageable tensors per step with `.to(device)` (models/pangu_sample.py:41-43: 573 MB, on the
training thread, each copy staged through the runtime's own bounce buffers) and synchronises every step (`loss.item()`, :77);
its reader reverses the level axis on the host (`[::-1]`, era5_data/utils_data.py:117).  `DevicePrefetcher` is the idea of the
reference's (unused) DataPrefetcher (era5_data/utils_data.py:16-51) done for batches of that size:

  * a WORKER THREAD pulls the next batch from the loader, stages it into page-locked buffers that are allocated once
    (`pangu_host_copy`: the 573 MB split over a few host threads -- one thread copies at 2-3 GB/s, a 43 ms step needs 13.4 GB/s)
    and queues the host->device copies on a side stream; the training thread never touches host memory;
  * `depth` batches are staged AHEAD of the consumer, so a per-step `loss.item()` does not expose the copy of the next batch;
  * loaders that can write into a given buffer skip the staging copy altogether (`fill_pinned` protocol below);
  * the level reversal costs nothing: with `fuse_flip=True` the fields stay in file order and the first kernel that reads them
    (patch_embed_gather) / the loss kernel address level 12 - l (`levels_reversed=True` of PanguModel.forward / train.train_step).

`HostDrain` is the mirror image for the OUTPUT side of a forecast loop (the reference pulls every step's de-normalised output to the
host, models/pangu_sample.py:204-226 and :141-158): a pack (int16 planes with a per-plane scale / offset, ERA5 NetCDF's storage) or
stage (fp32) kernel on the forecast stream, the device->host copy on a side stream into page-locked buffers allocated once, and a
worker thread that hands each lead time to a sink; the forecast thread never waits on host I/O unless the ring is full.
"""
import os
import queue
import threading
import time

import torch


class PinnedFiller:
    """Protocol (duck-typed; subclassing is optional) of a loader that writes each batch straight into page-locked memory:

        spec          list of (shape, dtype), one per tensor of a batch (input, input_surface, target, target_surface, ...)
        fill_pinned(buffers) -> bool     write the next batch into `buffers` (CPU tensors of `spec`, page-locked); False = exhausted
        reset()       optional: rewind for another epoch (called at the start of every iteration)
        __len__()     optional

    A reader that decodes its file format into the buffers it is handed (numpy views of them: `buf.numpy()`) removes the only
    host-side copy of the pipeline."""
    spec = ()

    def fill_pinned(self, buffers):
        raise NotImplementedError


def default_copy_threads():
    """Host threads of one staging copy: up to 8, and never more than half of this rank's share of the host's cores."""
    world = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")) or 1)
    return max(1, min(8, (os.cpu_count() or 1) // (2 * max(world, 1))))


def host_copy(dst, src, threads):
    """dst (page-locked CPU tensor) <- src (CPU tensor): the multi-threaded C-ABI copy for plain contiguous same-dtype tensors,
    `Tensor.copy_` (dtype conversion / strides) otherwise."""
    if (src.device.type == "cpu" and src.dtype == dst.dtype and src.shape == dst.shape and src.is_contiguous()
            and dst.is_contiguous()):
        from . import _lib
        _lib.check(_lib.load().pangu_host_copy(dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(), int(threads)),
                   "host_copy")
    else:
        dst.copy_(src)


_END = object()


class DevicePrefetcher:
    """Wrap an iterable of (input, input_surface, target, target_surface, *rest) CPU batches -- or a PinnedFiller.

    flip_levels   the reader delivers ascending levels: reverse the pressure-level axis (dim -3) of input / target.
    fuse_flip     with flip_levels: do NOT move any data; batches are yielded in file order and `self.levels_reversed` is True --
                  pass it on (`train_step(..., levels_reversed=pf.levels_reversed)`).  False: a device-side `flip` per field.
                  The device-side flip touches batch elements 0 and 2 only, so a multi-target feed (train.rollout_train_step:
                  target_2, target_3, ... ride in `*rest`) uses fuse_flip=True, which reverses every target by addressing.
    depth         batches staged ahead of the consumer (>= 1; 2 hides the copy behind a per-step host sync).
    threaded      False: stage on the consumer's thread (the pre-round-6 behaviour; for debugging / comparison).
    copy_threads  host threads of one staging copy (default_copy_threads()).
    reuse_device_buffers   True: the device tensors of a batch are `depth + 3` STATIC buffer sets filled in turn (no allocator traffic
                  in the loop: a fresh 270 MB block per field and step can mean a synchronous hipMalloc when the caching allocator's
                  pool is fragmented) -- a yielded batch is valid until the consumer asks for the NEXT one (an event recorded then
                  orders the buffer's refill behind the consumer's work on it -- work enqueued on the stream that is CURRENT when the next
                  batch is requested); keep nothing from a batch across iterations.
                  False (default): every batch is freshly allocated and stays valid as long as it is referenced."""

    def __init__(self, loader, device, flip_levels=False, depth=2, fuse_flip=False, threaded=True, copy_threads=None,
                 reuse_device_buffers=False):
        self.loader, self.device = loader, torch.device(device)
        self.flip = bool(flip_levels) and not fuse_flip
        self.levels_reversed = bool(flip_levels) and bool(fuse_flip)
        self.depth = max(1, int(depth))
        self.threaded = bool(threaded)
        self.copy_threads = int(copy_threads) if copy_threads else default_copy_threads()
        # (high priority: the uploads are tiny next to a step's kernels and must not queue behind them)
        self.stream = torch.cuda.Stream(device=self.device, priority=-1)
        self._nslots = self.depth + 1          # `depth` queued + the one being staged
        self._pinned = [None] * self._nslots   # per slot: list of page-locked host buffers
        self._busy = [None] * self._nslots     # per slot: event of the last host->device copy that read those buffers
        self._slot = 0
        self.reuse = bool(reuse_device_buffers)
        self._ndev = self.depth + 3            # queued + being staged + held by the consumer + one whose release was just recorded
        self._dev = [None] * self._ndev        # per device slot: list of static device tensors
        self._consumed = [None] * self._ndev   # per device slot: event on the consumer's stream after its last use of that slot
        self._dslot = 0
        self._filler = hasattr(loader, "fill_pinned")
        # what the pipeline did, for bench.py: seconds in the staging copy / bytes staged / seconds the consumer waited for a batch
        self.stats = {"host_copy_s": 0.0, "bytes": 0, "batches": 0, "consumer_wait_s": 0.0, "h2d_events": []}

    def __len__(self):
        return len(self.loader)

    # ---- staging (worker thread, or the consumer's when threaded=False)
    def _slot_buffers(self, slot, spec):
        pins = self._pinned[slot]
        if pins is None or len(pins) != len(spec) or any(tuple(p.shape) != tuple(sh) or p.dtype != dt for p, (sh, dt) in zip(pins, spec)):
            pins = self._pinned[slot] = [torch.empty(tuple(sh), dtype=dt, pin_memory=True) for sh, dt in spec]
        return pins

    def _next_slot(self):
        slot = self._slot
        self._slot = (slot + 1) % self._nslots
        if self._busy[slot] is not None:
            self._busy[slot].synchronize()      # the async copy that last read this slot's buffers must be done (blocks the stager only)
        return slot

    def _upload(self, slot, pins, layout):
        """pins: the slot's page-locked tensors; layout: per batch element either an index into pins or ('obj', value)."""
        out, dslot = [], -1
        with torch.cuda.device(self.device), torch.cuda.stream(self.stream):
            if self.reuse:
                dslot = self._dslot
                self._dslot = (dslot + 1) % self._ndev
                dev = self._dev[dslot]
                if dev is None or len(dev) != len(pins) or any(d.shape != p.shape or d.dtype != p.dtype for d, p in zip(dev, pins)):
                    dev = self._dev[dslot] = [torch.empty(p.shape, dtype=p.dtype, device=self.device) for p in pins]
                if self._consumed[dslot] is not None:
                    self.stream.wait_event(self._consumed[dslot])      # the consumer's last kernels on this buffer set come first
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(self.stream)
            for i, item in enumerate(layout):
                if isinstance(item, tuple):
                    out.append(item[1])
                    continue
                if self.reuse:
                    d = dev[item]
                    d.copy_(pins[item], non_blocking=True)
                else:
                    d = pins[item].to(self.device, non_blocking=True)
                if self.flip and i in (0, 2) and d.dim() >= 4:
                    d = d.flip(-3)
                out.append(d)
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(self.stream)
        self._busy[slot] = ev
        st = self.stats
        st["h2d_events"].append((e0, ev, sum(p.numel() * p.element_size() for p in pins)))
        del st["h2d_events"][:-16]
        return out, ev, dslot

    def _stage(self, batch):
        tensors = [t for t in batch if torch.is_tensor(t)]
        slot = self._next_slot()
        pins = self._slot_buffers(slot, [(t.shape, t.dtype) for t in tensors])
        t0 = time.perf_counter()
        for pin, t in zip(pins, tensors):
            host_copy(pin, t, self.copy_threads)              # host -> page-locked (the only host-side copy)
        st = self.stats
        st["host_copy_s"] += time.perf_counter() - t0
        st["bytes"] += sum(p.numel() * p.element_size() for p in pins)
        st["batches"] += 1
        layout, k = [], 0
        for t in batch:
            if torch.is_tensor(t):
                layout.append(k)
                k += 1
            else:
                layout.append(("obj", t))
        return self._upload(slot, pins, layout)

    def _stage_filled(self):
        slot = self._next_slot()
        pins = self._slot_buffers(slot, list(self.loader.spec))
        t0 = time.perf_counter()
        if not self.loader.fill_pinned(pins):
            return None
        st = self.stats
        st["host_copy_s"] += time.perf_counter() - t0          # (here: the loader's own decode-into-buffer time)
        st["bytes"] += sum(p.numel() * p.element_size() for p in pins)
        st["batches"] += 1
        return self._upload(slot, pins, list(range(len(pins))))

    def _staged(self):
        """Generator of staged (batch, event) pairs, in the calling thread."""
        if self._filler:
            if hasattr(self.loader, "reset"):
                self.loader.reset()
            while True:
                item = self._stage_filled()
                if item is None:
                    return
                yield item
        else:
            for batch in self.loader:
                yield self._stage(batch)

    def _worker(self, q, stop):
        try:
            for item in self._staged():
                while not stop.is_set():
                    try:
                        q.put(item, timeout=0.1)
                        break
                    except queue.Full:
                        continue
                if stop.is_set():
                    return
            q.put(_END)
        except BaseException as e:       # delivered to the consumer, which re-raises it
            q.put(e)

    def _hand_over(self, batch, ev, dslot=-1):
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        if dslot < 0:
            for t in batch:
                if torch.is_tensor(t):
                    t.record_stream(cur)
        return tuple(batch)

    def _release(self, dslot):
        """The consumer asked for the next batch: everything it enqueued on the batch in device slot `dslot` precedes this event."""
        if dslot >= 0:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._consumed[dslot] = ev

    def __iter__(self):
        if not self.threaded:
            # one batch staged ahead, on this thread (its host copy overlaps nothing but the GPU's queue)
            gen = self._staged()
            pending = next(gen, None)
            while pending is not None:
                batch, ev, dslot = pending
                pending = next(gen, None)
                yield self._hand_over(batch, ev, dslot)
                self._release(dslot)
            return
        q = queue.Queue(maxsize=self.depth)
        stop = threading.Event()
        th = threading.Thread(target=self._worker, args=(q, stop), name="pangu-prefetch", daemon=True)
        th.start()
        try:
            while True:
                t0 = time.perf_counter()
                while True:                   # never block forever on a worker that died without posting its end marker
                    try:
                        item = q.get(timeout=1.0)
                        break
                    except queue.Empty:
                        if not th.is_alive():
                            try:
                                item = q.get_nowait()
                                break
                            except queue.Empty:
                                raise RuntimeError("DevicePrefetcher: the staging thread ended without delivering a batch or its end marker")
                self.stats["consumer_wait_s"] += time.perf_counter() - t0
                if item is _END:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield self._hand_over(*item)
                self._release(item[2])
        finally:
            stop.set()
            while th.is_alive():          # unblock a worker stuck on a full queue (the consumer left early)
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                th.join(timeout=0.05)

    def summary(self):
        """Rates of the pipeline so far (call after a synchronize): staging copy GB/s (host), host->device GB/s (copy engine,
        over the last batches), seconds the consumer waited for batches."""
        st = self.stats
        h2d_ms = h2d_b = 0.0
        for e0, e1, nbytes in st["h2d_events"]:
            if e1.query():
                h2d_ms += e0.elapsed_time(e1)
                h2d_b += nbytes
        return {"batches": st["batches"], "bytes_per_batch": st["bytes"] / max(st["batches"], 1),
                "host_stage_GBps": st["bytes"] / st["host_copy_s"] / 1e9 if st["host_copy_s"] > 0 else None,
                "host_stage_ms_per_batch": st["host_copy_s"] / max(st["batches"], 1) * 1e3,
                "h2d_GBps": h2d_b / (h2d_ms * 1e-3) / 1e9 if h2d_ms > 0 else None,
                "consumer_wait_ms_per_batch": st["consumer_wait_s"] / max(st["batches"], 1) * 1e3,
                "copy_threads": self.copy_threads, "depth": self.depth, "threaded": self.threaded,
                "direct_fill": self._filler, "levels_reversed_fused": self.levels_reversed, "static_device_buffers": self.reuse}


class DrainedField:
    """One tensor of a drained item: numpy views into the item's page-locked slot (valid until the item is released).

        packed        int16, shaped like the submitted tensor (mode "int16"), -32768 = non-finite; None in mode "float32"
        values        float32, shaped like the submitted tensor (mode "float32"); None in mode "int16"
        scale_offset  (planes, 2) float32 (scale, offset) per (.., H, W) plane; value = packed * scale + offset.  None in "float32"
        nonfinite     (planes,) int32: non-finite values per plane.  None in "float32" """

    def __init__(self, packed, values, scale_offset, nonfinite, threads):
        self.packed, self.values, self.scale_offset, self.nonfinite, self._threads = packed, values, scale_offset, nonfinite, threads

    def to_float32(self, out=None):
        """The field as float32 (a copy that outlives the item; `out`: a C-contiguous float32 array of the same shape to fill)."""
        import numpy as np
        src = self.values if self.packed is None else self.packed
        if out is None:
            out = np.empty(src.shape, dtype=np.float32)
        if out.shape != src.shape or out.dtype != np.float32 or not out.flags.c_contiguous:
            raise ValueError("to_float32: `out` must be a C-contiguous float32 array shaped like the field")
        if self.packed is None:
            np.copyto(out, src)
            return out
        from . import _lib
        planes = self.scale_offset.shape[0]
        _lib.check(_lib.load().pangu_unpack_i16_host(out.ctypes.data, src.ctypes.data, self.scale_offset.ctypes.data, planes,
                                                     src.size // planes, int(self._threads)), "unpack_i16_host")
        return out


class DrainedItem:
    """What one `HostDrain.submit` delivers: `fields` (one DrainedField per submitted tensor) and `tag`.  Valid until `release()`;
    `get()` of the next item releases this one unless `keep()` was called (then the caller releases it)."""

    def __init__(self, drain, slot, tag, fields):
        self._drain, self._slot, self.tag, self.fields, self._kept = drain, slot, tag, fields, False

    def to_float32(self):
        return [f.to_float32() for f in self.fields]

    def keep(self):
        self._kept = True
        return self

    def release(self):
        if self._slot is not None:
            slot, self._slot = self._slot, None
            self.fields = []
            self._drain._free_slot(slot)


class HostDrain:
    """Deliver device fields to the host without stalling the loop that produces them.

        drain = HostDrain(device, mode="int16", sink=write_one_lead_time)
        for k in range(steps): ...; drain.submit([upper, surface], tag=k)
        drain.close()

    mode          "int16": each (.., H, W) plane is packed on the device (pangu_pack_planes_i16: per-plane scale / offset, half the
                  bytes over the link); "float32": staged unpacked (pangu_stage_planes_f32).
    depth         items that may be in flight behind the producer; the ring has depth + 1 slots (device staging + page-locked host
                  buffers), allocated once for the shapes of the first submit.  A full ring blocks `submit` (back-pressure).
    stats_last    the 4-tuple of rollout.norm_back (s_mean (1,4,1,1), s_std, u_mean (1,5,13,1,1), u_std): the submitted tensors are
                  NORMALISED model outputs -- 5-D ones take the upper-air pair, 4-D ones the surface pair -- and are de-normalised
                  by the kernel.  None: the fields are physical already.
    flip_levels   reverse the level axis (dim -3) of 5-D tensors, by addressing.
    sink          callable(item) run on a worker thread for every item, in order; the item is released when it returns.  An
                  exception ends the sink's service (later items are dropped) and is re-raised by the next submit() or close().
                  None: fetch items with get() / iteration -- at least once every depth + 1 submits, or from another thread: a
                  full ring blocks submit until an item is released.
    copy_threads  host threads of DrainedField.to_float32 (default_copy_threads()).
    regrid        None, a score.RegridPlan, or an (H_out, W_out) pair from which the plan is built at the first submit: every
                  submitted tensor, on the plan's input grid, is remapped conservatively to the coarser grid on the device
                  (pangu_regrid_planes_f32, with stats_last and flip_levels folded into that launch) and delivered as
                  (.., H_out, W_out) -- 36x fewer bytes over the link at 721 x 1440 -> 121 x 240.  "float32": the coarse field is
                  the staging buffer; "int16": it is then packed (pangu_pack_planes_i16 on the coarse planes).

    submit() works on the CURRENT stream and does not synchronise the host: the kernel reads the tensors in stream order, so they
    may be overwritten as soon as submit returns."""

    def __init__(self, device, mode="int16", depth=2, stats_last=None, flip_levels=False, sink=None, copy_threads=None,
                 regrid=None):
        if mode not in ("int16", "float32"):
            raise ValueError(f"HostDrain: mode must be 'int16' or 'float32', not {mode!r}")
        self.device, self.mode = torch.device(device), mode
        self.depth = max(1, int(depth))
        self.stats_last, self.flip = stats_last, bool(flip_levels)
        self.sink = sink
        self.regrid = regrid                   # None, a score.RegridPlan or (H_out, W_out); the plan once allocated
        self.copy_threads = int(copy_threads) if copy_threads else default_copy_threads()
        self.stream = torch.cuda.Stream(device=self.device, priority=-1)     # (high priority: the copy must not queue behind kernels)
        self._nslots = self.depth + 1
        self._spec = None                      # per tensor: (shape, planes, plane_elems, levels, mul, add, ws, delivered shape)
        self._dev = None                       # per slot, per tensor: dict of device staging tensors
        self._pin = None                       # per slot, per tensor: dict of page-locked host tensors
        self._free = [True] * self._nslots
        self._cv = threading.Condition()
        self._next = 0
        self._q = queue.Queue()                # (slot, tag, event) in submit order
        self._pending = 0                      # submitted, not yet fetched by get()
        self._last = None                      # the item get() handed out last
        self._error, self._failed = None, False
        self._closed = False
        self._thread = None
        self.stats = {"bytes": 0, "items": 0, "producer_wait_s": 0.0, "d2h_events": []}
        if sink is not None:
            self._thread = threading.Thread(target=self._worker, name="pangu-drain", daemon=True)
            self._thread.start()

    # ---- ring
    def _free_slot(self, slot):
        with self._cv:
            self._free[slot] = True
            self._cv.notify_all()

    def _take_slot(self):
        slot = self._next
        with self._cv:
            if not self._free[slot]:
                t0 = time.perf_counter()
                while not self._free[slot]:
                    self._cv.wait(timeout=0.5)
                    if self._thread is not None and not self._thread.is_alive() and not self._free[slot]:
                        raise RuntimeError("HostDrain: the sink thread ended with items outstanding")
                self.stats["producer_wait_s"] += time.perf_counter() - t0
            self._free[slot] = False
        self._next = (slot + 1) % self._nslots
        return slot

    def _plane_stats(self, t):
        """(mul, add) per SOURCE plane of tensor t, or (None, None)."""
        if self.stats_last is None:
            return None, None
        if t.dim() not in (4, 5):
            raise ValueError("HostDrain: stats_last serves 5-D (B,5,13,H,W) and 4-D (B,4,H,W) tensors only")
        from . import score
        return score.plane_affine(t, self.stats_last, self.device)

    def _allocate(self, tensors):
        spec, int16 = [], self.mode == "int16"
        from . import _lib, score
        for t in tensors:
            if t.dim() < 2:
                raise ValueError("HostDrain: tensors are (..., H, W)")
            out_shape = tuple(t.shape)
            if self.regrid is not None:
                self.regrid = score._as_plan(self.regrid, t.shape[-2], t.shape[-1], "HostDrain")
                out_shape = out_shape[:-2] + self.regrid.out_grid
            elems = out_shape[-1] * out_shape[-2]           # of a DELIVERED plane
            planes = t.numel() // max(t.shape[-1] * t.shape[-2], 1)
            if planes <= 0 or elems <= 0:
                raise ValueError("HostDrain: empty tensor")
            levels = t.shape[-3] if (self.flip and t.dim() == 5) else 0
            mul, add = self._plane_stats(t)
            ws = _lib.load().pangu_pack_i16_ws_bytes(planes, elems) if int16 else 0
            if ws < 0:
                _lib.check(int(ws), "pack_i16_ws_bytes")
            spec.append((tuple(t.shape), planes, elems, int(levels), mul, add, int(ws), out_shape))
        dev, pin = [], []
        for _ in range(self._nslots):
            d, h = [], []
            for _, planes, elems, _, _, _, ws, shape in spec:
                if int16:
                    d.append({"data": torch.empty(shape, dtype=torch.int16, device=self.device),
                              "so": torch.empty((planes, 2), dtype=torch.float32, device=self.device),
                              "nf": torch.empty((planes,), dtype=torch.int32, device=self.device),
                              "ws": torch.empty((ws + 3) // 4, dtype=torch.float32, device=self.device)})
                    if self.regrid is not None:              # the coarse fp32 field the pack launches read (stays on the device)
                        d[-1]["coarse"] = torch.empty(shape, dtype=torch.float32, device=self.device)
                    h.append({"data": torch.empty(shape, dtype=torch.int16, pin_memory=True),
                              "so": torch.empty((planes, 2), dtype=torch.float32, pin_memory=True),
                              "nf": torch.empty((planes,), dtype=torch.int32, pin_memory=True)})
                else:
                    d.append({"data": torch.empty(shape, dtype=torch.float32, device=self.device)})
                    h.append({"data": torch.empty(shape, dtype=torch.float32, pin_memory=True)})
            dev.append(d)
            pin.append(h)
        self._spec, self._dev, self._pin = spec, dev, pin

    # ---- producer
    def submit(self, tensors, tag=None):
        """Queue `tensors` (a list of contiguous fp32 CUDA tensors (..., H, W), the same shapes on every call) for delivery."""
        if self._closed:
            raise RuntimeError("HostDrain: submit after close")
        self._raise_pending()
        tensors = list(tensors)
        for t in tensors:
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError("HostDrain.submit: contiguous float32 CUDA tensors only")
        if self._spec is None:
            with torch.cuda.device(self.device):
                self._allocate(tensors)
        if [tuple(t.shape) for t in tensors] != [sp[0] for sp in self._spec]:
            raise ValueError("HostDrain.submit: the shapes differ from those of the first submit")
        slot = self._take_slot()
        self._raise_pending()
        from . import _lib, score
        lib = _lib.load()
        int16 = self.mode == "int16"
        nbytes = 0
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            for t, (_, planes, elems, levels, mul, add, ws, _), d in zip(tensors, self._spec, self._dev[slot]):
                pm, pa = (mul.data_ptr(), add.data_ptr()) if mul is not None else (None, None)
                src = t.data_ptr()
                if self.regrid is not None:     # de-normalise, flip and remap in one launch; what follows sees a physical field
                    coarse = d["coarse" if int16 else "data"]
                    score._regrid_launch(cur.cuda_stream, src, mul, add, coarse.data_ptr(), planes, self.regrid, levels,
                                         self.device)
                    if not int16:
                        continue
                    src, pm, pa, levels = coarse.data_ptr(), None, None, 0
                if int16:
                    _lib.check(lib.pangu_pack_planes_i16(cur.cuda_stream, src, pm, pa, d["data"].data_ptr(),
                                                         d["so"].data_ptr(), d["nf"].data_ptr(), d["ws"].data_ptr(), ws, planes, elems,
                                                         levels), "pack_planes_i16")
                else:
                    _lib.check(lib.pangu_stage_planes_f32(cur.cuda_stream, src, pm, pa, d["data"].data_ptr(), planes, elems,
                                                          levels), "stage_planes_f32")
            ready = torch.cuda.Event()
            ready.record(cur)
            self.stream.wait_event(ready)
            with torch.cuda.stream(self.stream):
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(self.stream)
                for d, h in zip(self._dev[slot], self._pin[slot]):
                    for k, buf in h.items():
                        buf.copy_(d[k], non_blocking=True)
                        nbytes += buf.numel() * buf.element_size()
                ev = torch.cuda.Event(enable_timing=True)
                ev.record(self.stream)
        st = self.stats
        st["bytes"] += nbytes
        st["items"] += 1
        st["d2h_events"].append((e0, ev, nbytes))
        del st["d2h_events"][:-16]
        self._pending += 1
        self._q.put((slot, tag, ev))

    # ---- consumer
    def _item(self, slot, tag, ev):
        ev.synchronize()
        fields = []
        for h in self._pin[slot]:
            if self.mode == "int16":
                fields.append(DrainedField(h["data"].numpy(), None, h["so"].numpy(), h["nf"].numpy(), self.copy_threads))
            else:
                fields.append(DrainedField(None, h["data"].numpy(), None, None, self.copy_threads))
        return DrainedItem(self, slot, tag, fields)

    def get(self):
        """The next item in submit order (blocks until its copy has landed), or None when nothing is outstanding.  Releases the item
        handed out before unless it was kept.  Not available with a sink."""
        if self._thread is not None:
            raise RuntimeError("HostDrain.get: items go to the sink")
        if self._last is not None and not self._last._kept:
            self._last.release()
        self._last = None
        if self._pending == 0:
            return None
        slot, tag, ev = self._q.get()
        self._pending -= 1
        self._last = self._item(slot, tag, ev)
        return self._last

    def __iter__(self):
        while True:
            item = self.get()
            if item is None:
                return
            yield item

    def _worker(self):
        while True:
            job = self._q.get()
            if job is _END:
                return
            slot, tag, ev = job
            item = None
            try:
                ev.synchronize()
                if self._failed:                    # after an error: drop the item, the ring keeps turning so that submit never hangs
                    self._free_slot(slot)
                    continue
                item = self._item(slot, tag, ev)
                try:
                    self.sink(item)
                finally:
                    item.release()
            except BaseException as e:              # delivered to the producer: the next submit() or close() re-raises it
                self._failed = True
                if self._error is None:
                    self._error = e
                if item is None:
                    self._free_slot(slot)

    def _raise_pending(self):
        if self._error is not None:
            e, self._error = self._error, None
            self._closed = True
            self._stop_worker()
            raise e

    def _stop_worker(self):
        if self._thread is not None and self._thread.is_alive():
            self._q.put(_END)
            self._thread.join()

    def close(self):
        """Deliver what is queued to the sink, join the worker and re-raise its exception, if any.  Without a sink: wait for the copies
        in flight; items not fetched are dropped."""
        if not self._closed:
            self._closed = True
            self._stop_worker()
            if self._thread is None:
                self.stream.synchronize()
        self._raise_pending()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                       # do not mask the caller's exception
            try:
                self.close()
            except BaseException:
                pass
        return False

    def summary(self):
        """Rates so far (call after close() or a synchronize): device->host GB/s over the last items, producer wait per item."""
        st = self.stats
        ms = b = 0.0
        for e0, e1, nbytes in st["d2h_events"]:
            if e1.query():
                ms += e0.elapsed_time(e1)
                b += nbytes
        return {"items": st["items"], "bytes_per_item": st["bytes"] / max(st["items"], 1),
                "d2h_GBps": b / (ms * 1e-3) / 1e9 if ms > 0 else None,
                "d2h_ms_per_item": ms / max(len(st["d2h_events"]), 1),
                "producer_wait_ms_per_item": st["producer_wait_s"] / max(st["items"], 1) * 1e3,
                "mode": self.mode, "depth": self.depth, "sink": self.sink is not None}
