"""Ensemble forecasts: perturbed initial states, a graph-captured rollout of every member, and on-device ensemble scores.

The Pangu-Weather paper (Bi et al., Nature 2023) makes its ensembles by perturbing the initial state with Perlin noise, one
member left unperturbed.  Here the noise is made in place on the device (`pangu_ensemble_perturb_f32`, the definition is pinned
in csrc/ensemble.hip), the members run as B = 1 forwards inside hipGraphs over chunks of members that feed their physical
fields back into one (E, ...) state tensor (the `scatter_denorm` feed-back of rollout.GraphedStep), and the ensemble mean,
spread and CRPS come from one HIP pass over the members (score.ensemble_scores).
"""
import numbers

import torch

from . import _lib, score
from .ops import _stream

EP_MAX_NODES = 1024     # csrc/ensemble.hip: lattice columns (plus one per octave) over all octaves
EP_MAX_OCTAVES = 8


def _check_lattice(W, octaves, period):
    if not 1 <= octaves <= EP_MAX_OCTAVES:
        raise ValueError(f"octaves must be in 1..{EP_MAX_OCTAVES}, got {octaves}")
    if period < 1:
        raise ValueError(f"period must be >= 1, got {period}")
    if W % 4:
        raise ValueError(f"W % 4 != 0 (W = {W})")
    nodes = 0
    for o in range(octaves):
        L = period << o
        if W % L:
            raise ValueError(f"octave {o}: {L} lattice cells do not divide W = {W} (W % L != 0)")
        nodes += L + 1
    if nodes > EP_MAX_NODES:
        raise ValueError(f"the lattice of {octaves} octaves at period {period} has {nodes} columns, more than {EP_MAX_NODES}")


def _amplitude9(amplitude):
    if amplitude is None:
        raise ValueError("amplitude is required (a scalar or 9 per-variable values): the project has no calibrated default")
    if isinstance(amplitude, numbers.Real):
        return [float(amplitude)] * 9
    vals = [float(a) for a in (amplitude.reshape(-1).tolist() if isinstance(amplitude, torch.Tensor) else amplitude)]
    if len(vals) != 9:
        raise ValueError(f"amplitude: a scalar or 9 values (z, q, t, u, v, msl, u10, v10, t2m), got {len(vals)}")
    return vals


_amp_on = {}      # (device, the 9 amplitudes) -> the fp32 device tensor


def _amplitudes_on(device, amp):
    """Uploaded once per (device, values): torch.tensor(list, device=cuda) is a synchronous host-to-device copy (it waits for
    whatever the stream holds), which a training step that perturbs every step must not pay (train.ensemble_train_step)."""
    key = (str(device), tuple(amp))
    t = _amp_on.get(key)
    if t is None:
        if len(_amp_on) > 8:
            _amp_on.clear()
        t = _amp_on[key] = torch.tensor(amp, dtype=torch.float32).to(device)
    return t


def perturb_(upper, surface, stats_last, amplitude, seed, octaves=3, period=12, persistence=0.5, first_member=0, control=True):
    """Add amplitude[var] * std[plane] * Perlin noise, in place, to member states upper (E,5,13,H,W) and surface (E,4,H,W)
    (fp32, physical units, on the device); std comes from stats_last = (s_mean, s_std, u_mean, u_std).

    amplitude is required: a scalar or 9 per-variable values (the 5 upper variables, then the 4 surface ones), in units of the
    per-level standard deviation.  The project has no calibrated value, and the settings of the paper's ensembles cannot be
    checked from here.  octaves, period (lattice cells around the longitude circle at the coarsest octave) and persistence
    (weight ratio of successive octaves) are conventional Perlin settings, not tuned values.

    Member e is global member first_member + e; its noise depends on (seed, member, plane, position) only, so a member gets
    the same perturbation whatever chunk or batch it is made in.  With control=True member 0 stays unperturbed."""
    amp = _amplitude9(amplitude)
    if upper.dim() != 5 or surface.dim() != 4 or tuple(upper.shape[1:3]) != (5, 13) or surface.shape[1] != 4:
        raise ValueError("perturb_: expected upper (E,5,13,H,W) and surface (E,4,H,W)")
    E, H, W = upper.shape[0], upper.shape[-2], upper.shape[-1]
    if surface.shape[0] != E or tuple(surface.shape[-2:]) != (H, W):
        raise ValueError("perturb_: upper and surface disagree in E, H or W")
    if first_member < 0:
        raise ValueError("first_member must be >= 0")
    _check_lattice(W, octaves, period)
    for t, name in ((upper, "upper"), (surface, "surface")):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"perturb_: {name} must be a contiguous float32 tensor on an MI355X device (no CPU fallback)")
    _, s_std, _, u_std = stats_last
    dev = upper.device
    f = lambda t: t.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    amp_t = _amplitudes_on(dev, amp)
    us, ss = f(u_std), f(s_std)
    if us.numel() != 65 or ss.numel() != 4:
        raise ValueError("perturb_: stats_last must be (s_mean (1,4,1,1), s_std, u_mean (1,5,13,1,1), u_std)")
    _lib.check(_lib.load().pangu_ensemble_perturb_f32(
        _stream(upper), upper.data_ptr(), upper[0].numel(), surface.data_ptr(), surface[0].numel(), E, first_member, H, W,
        amp_t.data_ptr(), us.data_ptr(), ss.data_ptr(), int(seed) & 0xFFFFFFFF, octaves, period, float(persistence),
        1 if control else 0), "ensemble_perturb_f32")
    return upper, surface


class EnsembleRollout:
    """E perturbed members of one initial state, advanced together one model step per .step().

    The state is one (E,5,13,H,W) / (E,4,H,W) pair of tensors.  Each chunk of members is captured once as a hipGraph that
    runs every member of the chunk as its own B = 1 forward whose last kernel writes the member's physical fields back into
    its slice of the state (ops.scatter_denorm, as in rollout.GraphedStep): a step is one replay per chunk, with no host sync
    and no copy of member states.  A member's arithmetic is that of a B = 1 rollout, whatever the chunk size.

    The model's compute dtype at construction is the one captured.  perturbation settings: see perturb_."""

    def __init__(self, model, inp, inp_surface, statistics, maps, const_h, stats_last, members, amplitude, seed=0, chunk=None,
                 octaves=3, period=12, persistence=0.5, control=True, warmup=2):
        if members < 2:
            raise ValueError(f"an ensemble needs at least 2 members, got {members}")
        _amplitude9(amplitude)
        if inp.dim() != 5 or inp.shape[0] != 1 or inp_surface.dim() != 4 or inp_surface.shape[0] != 1:
            raise ValueError("EnsembleRollout: inp (1,5,13,H,W) and inp_surface (1,4,H,W)")
        _check_lattice(inp.shape[-1], octaves, period)
        chunk = members if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be >= 1")
        if not inp.is_cuda:
            raise RuntimeError("EnsembleRollout needs the inputs on an MI355X device (no CPU fallback)")
        self.model = model
        self.members = members
        self.consts = (statistics, maps, const_h)
        self.stats_last = stats_last
        self.seed = seed
        self.perturb_args = dict(amplitude=amplitude, octaves=octaves, period=period, persistence=persistence, control=control)
        self.upper = torch.empty((members,) + tuple(inp.shape[1:]), dtype=torch.float32, device=inp.device)
        self.surface = torch.empty((members,) + tuple(inp_surface.shape[1:]), dtype=torch.float32, device=inp.device)
        self.reset(inp, inp_surface)
        with torch.no_grad():
            # warm-up outside capture (weight shadows, attribute calls, allocator) on a scratch copy of one member: the
            # state itself is not advanced
            wu, ws = self.upper[:1].clone(), self.surface[:1].clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    self._member(wu, ws)
            torch.cuda.current_stream().wait_stream(side)
            del wu, ws
            pool = torch.cuda.graph_pool_handle()
            self.graphs = []
            for e0 in range(0, members, chunk):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                    for e in range(e0, min(members, e0 + chunk)):
                        self._member(self.upper[e:e + 1], self.surface[e:e + 1])
                self.graphs.append(g)

    def _member(self, up, sf):
        from . import ops
        with ops.scatter_denorm(up, sf, self.stats_last):
            self.model(up, sf, *self.consts)

    def reset(self, inp, inp_surface, seed=None):
        """Start again from the initial state (inp (1,5,13,H,W), inp_surface (1,4,H,W)), perturbed with `seed` (default:
        the constructor's); the captured graphs are kept."""
        if seed is not None:
            self.seed = seed
        self.upper.copy_(inp.expand_as(self.upper))
        self.surface.copy_(inp_surface.expand_as(self.surface))
        perturb_(self.upper, self.surface, self.stats_last, seed=self.seed, **self.perturb_args)

    def step(self):
        """Advance every member by one model step (one graph replay per chunk)."""
        for g in self.graphs:
            g.replay()

    def state(self):
        """The live member state (upper (E,5,13,H,W), surface (E,4,H,W)), physical units; clone it to keep a step."""
        return self.upper, self.surface

    def scores(self, target, target_surface, regrid=None):
        """score.ensemble_scores of the current state against one target.  regrid: a score.RegridPlan or an (H_out, W_out) pair:
        the members and the target are first remapped conservatively to that coarser grid (score.regrid_fields) and scored
        there, e.g. (121, 240) for WeatherBench-style 1.5 degree scores."""
        upper, surface = self.upper, self.surface
        if regrid is not None:
            upper, surface = score.regrid_fields(upper, surface, regrid)
            target, target_surface = score.regrid_fields(target.reshape((1,) + tuple(self.upper.shape[1:])).contiguous(),
                                                         target_surface.reshape((1,) + tuple(self.surface.shape[1:])).contiguous(),
                                                         regrid)
        return score.ensemble_scores(upper, surface, target, target_surface, self.stats_last)

    def mean_std(self):
        """((mean_upper, mean_surface), (std_upper, std_surface)): ensemble mean and the square root of the unbiased
        member variance, shaped like one member."""
        su, ss = score.ensemble_scores(self.upper, self.surface, None, None, self.stats_last, want_fields=True)
        return (su["mean"], ss["mean"]), (su["std"], ss["std"])

    def reliability(self, target, target_surface, thresholds=None, seed=0):
        """score.ensemble_reliability of the current state against one target: (upper, surface) ReliabilityTables (rank
        histogram, and the reliability tables of the events x > thresholds)."""
        return score.ensemble_reliability(self.upper, self.surface, target, target_surface, thresholds=thresholds, seed=seed)

    def exceedance(self, thresholds):
        """(prob_upper (T,5,13,H,W), prob_surface (T,4,H,W)): the share of members above each threshold at every grid point
        of the current state (forecast mode, no target); fields a data.HostDrain can ship like those of mean_std()."""
        ru, rs = score.ensemble_reliability(self.upper, self.surface, None, None, thresholds=thresholds, want_fields=True)
        return ru.prob, rs.prob

    def quantiles(self, q):
        """(fields_upper (Q,5,13,H,W), fields_surface (Q,4,H,W)): the quantile fields of the current state at the levels q
        (score.ensemble_quantiles; forecast mode, no target)."""
        ru, rs = score.ensemble_quantiles(self.upper, self.surface, q)
        return ru.fields, rs.fields

    def quantile_scores(self, target, target_surface, q):
        """(upper, surface) score.QuantileResult of the current state against one target: pinball score and coverage per level,
        without the fields."""
        return score.ensemble_quantiles(self.upper, self.surface, q, target, target_surface, want_fields=False)

    def spectra(self, target=None, target_surface=None, bands=None, kmax=None):
        """Zonal power spectra of the current state (score.zonal_spectrum; bands and kmax as there): a dict of (upper, surface)
        score.SpectrumResult pairs with N = 1,
          "members"  the member spectra averaged over the members,
          "mean"     the spectrum of the ensemble mean of mean_std(),
        and with one target ((1,)5,13,H,W / (1,)4,H,W) also
          "target"   the target's spectrum,
          "error"    the spectrum of mean - target.
        members / mean at small scales is the spectral face of the spread: the mean cannot carry more anomaly power than the
        members do on average."""
        if (target is None) != (target_surface is None):
            raise ValueError("EnsembleRollout.spectra: give both targets or neither")
        kw = dict(bands=bands, kmax=kmax)
        out = {"members": tuple(r.mean_over_items() for r in score.zonal_spectrum(self.upper, self.surface, **kw))}
        (mu, ms), _ = self.mean_std()
        mu, ms = mu.unsqueeze(0), ms.unsqueeze(0)
        out["mean"] = score.zonal_spectrum(mu, ms, **kw)
        if target is not None:
            out["target"] = score.zonal_spectrum(target.reshape(mu.shape), target_surface.reshape(ms.shape), **kw)
            out["error"] = score.zonal_spectrum(mu, ms, target, target_surface, **kw)
        return out

    def update_lead_stats(self, agg, lead):
        """Fold the current member state into the lead windows of agg (a score.LeadWindowStats built without stats_last) at `lead`:
        per-member window means, extremes and spell lengths, leading dimension E.  score.ensemble_scores, ensemble_quantiles and
        ensemble_reliability(want_fields=True) of agg.result(w)'s fields give their probabilities."""
        agg.update(lead, self.upper, self.surface)

    @staticmethod
    def product_names(mean_std=True, quantiles=None, thresholds=None):
        """The names of the tensors products() returns for the same arguments, in its order."""
        names = ["mean_upper", "mean_surface", "std_upper", "std_surface"] if mean_std else []
        if quantiles is not None:
            names += ["quantiles_upper", "quantiles_surface"]
        if thresholds is not None:
            names += ["exceedance_upper", "exceedance_surface"]
        if not names:
            raise ValueError("EnsembleRollout.products: nothing requested")
        return names

    def products(self, mean_std=True, quantiles=None, thresholds=None):
        """The forecast products of the current state as an ordered list of contiguous fp32 tensors, physical units: mean upper,
        mean surface, std upper, std surface (mean_std), the quantile fields (Q,5,13,H,W), (Q,4,H,W) at the levels `quantiles`,
        the exceedance probabilities (T,5,13,H,W), (T,4,H,W) of `thresholds` (see exceedance) -- only the requested ones.  The
        list is what a data.HostDrain built without stats_last accepts, with the same shapes every step; product_names gives the
        matching names."""
        self.product_names(mean_std, quantiles, thresholds)
        out = []
        if mean_std:
            (mu, ms), (su, ss) = self.mean_std()
            out += [mu, ms, su, ss]
        if quantiles is not None:
            out += list(self.quantiles(quantiles))
        if thresholds is not None:
            out += list(self.exceedance(thresholds))
        return out


def ensemble_rollout(model, inp, inp_surface, statistics, maps, const_h, stats_last, members, amplitude, steps=7, seed=0,
                     chunk=None, targets=None, reliability=None, thresholds=None, drain=None, products=None, quantile_levels=None,
                     *, lead_stats=None, **perturb_kw):
    """`steps` steps of an EnsembleRollout.  Returns the final member state (upper, surface); with targets (a list of
    (target, target_surface) per step) also the list of per-step score dicts.  With reliability (a score.ReliabilityAccumulator
    of at least `steps` leads; needs targets) step k's reliability tables against targets[k], for the events x > thresholds,
    are added to it at lead k (rank ties broken with `seed`); the return value is unchanged.

    drain: a data.HostDrain (built WITHOUT stats_last: the products are physical already).  After every step the step's
    EnsembleRollout.products(**products) (products: a dict of its arguments, default the mean and std) are submitted with tag =
    the step index; the pack launches follow the replays on the same stream, with no host synchronisation here.  A drain built
    with regrid=(H_out, W_out) delivers the products on that coarser grid (remapped on the device), with no change here.
    quantile_levels (needs targets): step k's history entry becomes (upper_scores, surface_scores, upper_quantiles,
    surface_quantiles), the last two the score.QuantileResult of quantile_scores against targets[k].
    lead_stats: a score.LeadWindowStats (built WITHOUT stats_last) whose windows all end within `steps`: after step k the member
    state is folded into every window that holds lead k (EnsembleRollout.update_lead_stats); the statistics are per member, their
    leading dimension is E.  The return value is unchanged."""
    from .rollout import check_lead_stats
    check_lead_stats(lead_stats, steps, "ensemble_rollout")
    if reliability is not None and targets is None:
        raise ValueError("ensemble_rollout: reliability needs targets")
    if reliability is None and thresholds is not None:
        raise ValueError("ensemble_rollout: thresholds are used only with reliability")
    if products is not None and drain is None:
        raise ValueError("ensemble_rollout: products are delivered through a drain")
    if drain is not None and getattr(drain, "stats_last", None) is not None:
        raise ValueError("ensemble_rollout: the drain must be built without stats_last (the products are physical already)")
    if quantile_levels is not None and targets is None:
        raise ValueError("ensemble_rollout: quantile_levels needs targets")
    if quantile_levels is not None:
        quantile_levels = score._check_levels(quantile_levels, "ensemble_rollout")
    product_kw = dict(products or {})
    if drain is not None:
        EnsembleRollout.product_names(**product_kw)
        if product_kw.get("quantiles") is not None:
            score._check_levels(product_kw["quantiles"], "ensemble_rollout")
    with torch.no_grad():
        ens = EnsembleRollout(model, inp, inp_surface, statistics, maps, const_h, stats_last, members, amplitude, seed=seed,
                              chunk=chunk, **perturb_kw)
        history = []
        for k in range(steps):
            ens.step()
            if targets is not None:
                entry = ens.scores(*targets[k])
                if quantile_levels is not None:
                    entry = entry + ens.quantile_scores(*targets[k], quantile_levels)
                history.append(entry)
            if reliability is not None:
                reliability.add(k, *ens.reliability(*targets[k], thresholds=thresholds, seed=seed))
            if drain is not None:
                drain.submit(ens.products(**product_kw), tag=k)
            if lead_stats is not None:
                ens.update_lead_stats(lead_stats, k)
        up, sf = ens.state()
    return (up, sf, history) if targets is not None else (up, sf)
