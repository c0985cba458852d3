"""Autoregressive rollout (BASELINE configs[4]: 7 x 24 h) with the forward step captured in a hipGraph.

Shape of the loop: reference inference/inference_singleOutput.py:97-105 (the output of one 24 h step is the input of
the next).  The torch model returns NORMALISED fields (reference models/layers.py:531,542 leave the de-normalisation
commented out), so each step is followed by `normBackData` (reference era5_data/utils_data.py:324-330) before the
fields are fed back; here that de-normalisation is folded into the forward's last kernel (`pangu_patch_recover_scatter_denorm`
writes the physical fields straight into the step's static input buffers), inside the same captured graph, so the 286 MB state
never leaves the device, costs no extra pass, and one rollout step is ONE graph launch.
"""
import torch


def norm_back(upper, surface, stats_last):
    """reference era5_data/utils_data.py:324-330; stats_last = (s_mean(1,4,1,1), s_std, u_mean(1,5,13,1,1), u_std)."""
    s_mean, s_std, u_mean, u_std = stats_last
    return upper * u_std + u_mean, surface * s_std + s_mean


def norm_back_into(upper, surface, stats_last, dst_upper, dst_surface):
    """norm_back written straight into existing buffers (the rollout's next-step inputs): the same two roundings
    (multiply, then add) as the reference expression, without the temporaries and the copy pass."""
    s_mean, s_std, u_mean, u_std = stats_last
    torch.mul(upper, u_std, out=dst_upper).add_(u_mean)
    torch.mul(surface, s_std, out=dst_surface).add_(s_mean)


class GraphedStep:
    """One model step captured as a hipGraph (static shapes, B fixed, no host syncs inside the path).

    step(): input buffers -> model -> (optionally) de-normalised outputs copied back into the input buffers.
    """

    def __init__(self, model, inp, inp_surface, statistics, maps, const_h, stats_last=None, feed_back=False, warmup=2):
        assert inp.is_cuda and not any(p.requires_grad and torch.is_grad_enabled() for p in ())
        self.model = model
        self.inp = inp.clone()
        self.inp_surface = inp_surface.clone()
        self.consts = (statistics, maps, const_h)
        self.stats_last = stats_last
        self.feed_back = feed_back
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):                 # warm-up outside capture: weight shadows, attribute calls, allocator
                self._body()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.out, self.out_surface = self._body()
        # warm-up advanced the state when feed_back is on: restore the caller's initial fields
        self.inp.copy_(inp)
        self.inp_surface.copy_(inp_surface)

    def _body(self):
        if self.feed_back:
            # normBackData folded into the forward's last kernel: the scatter writes the physical fields straight into the
            # input buffers (read by the first kernel of this same forward, long finished by then)
            from . import ops
            with ops.scatter_denorm(self.inp, self.inp_surface, self.stats_last):
                return self.model(self.inp, self.inp_surface, *self.consts)
        return self.model(self.inp, self.inp_surface, *self.consts)

    def load(self, inp, inp_surface):
        self.inp.copy_(inp)
        self.inp_surface.copy_(inp_surface)

    def step(self):
        """Replay the graph once; returns the (static) normalised output tensors of this step."""
        self.graph.replay()
        return self.out, self.out_surface


def check_lead_stats(lead_stats, steps, who):
    """What rollout(lead_stats=) and ensemble.ensemble_rollout(lead_stats=) ask of a score.LeadWindowStats, before the first step."""
    if lead_stats is None:
        return
    if getattr(lead_stats, "stats_last", None) is not None:
        raise ValueError(f"{who}: lead_stats must be built without stats_last (it is handed physical fields)")
    end = max(b for _, b in lead_stats.windows)
    if steps < end:
        raise ValueError(f"{who}: {steps} steps do not reach the end of every lead window (the last ends at lead {end})")


def rollout(model, inp, inp_surface, statistics, maps, const_h, stats_last, steps=7, graph=True, keep=False, drain=None,
            scorecard=None, targets=None, events=None, *, lead_stats=None, sites=None, observations=None, obs=None):
    """`steps` chained forwards. Returns the last step's physical-unit fields (and, with keep=True, a list of the
    normalised outputs of every step, cloned).

    drain: a data.HostDrain (built WITHOUT stats_last: it is handed physical fields).  After every step the step's physical-unit
    fields are submitted to it with the step index as the tag -- the forecast of every lead time reaches the host while the next
    steps run.  The pack / stage launches follow each graph replay on the same stream (they are not part of the captured graph)
    and read the static input buffers the scatter-denorm has just written; the returned values are unchanged.  A drain built
    with regrid=(H_out, W_out) (or a score.RegridPlan) delivers every lead time on that coarser grid, e.g. (121, 240) for 1.5
    degrees: the remap runs on the device and 36x fewer bytes cross the link; nothing else changes here.

    scorecard: a score.ScoreAccumulator with at least `steps` leads, and targets: a sequence of `steps` entries, each a pair
    (target_upper, target_surface) of device tensors in physical units or None (no analysis for that lead).  After step k the
    step's physical-unit fields are scored against targets[k] and pooled at lead k (scorecard.score): two launches per tensor
    that follow the graph replay on the same stream, outside the captured graph, while the host goes on to the next step; no
    host sync, and the returned values are unchanged.

    events: a score.EventAccumulator with at least `steps` leads, scored against the same `targets` at the same place
    (events.score: contingency tables and Fractions Skill Score sums, two more launches per tensor), with or without a scorecard.

    lead_stats: a score.LeadWindowStats (built WITHOUT stats_last: it is handed physical fields) whose windows all end within
    `steps`.  After step k the step's physical-unit fields are folded into every window that holds lead k (lead_stats.update: one
    launch per tensor and window, behind the graph replay on the same stream, outside the captured graph, no host sync); the
    window means, extremes and spell lengths are then read from lead_stats.result(w) (lead_stats.reset() before the next rollout).
    The returned values are unchanged.

    sites: a score.PointSeries with at least `steps` leads.  After step k the step's physical-unit fields are interpolated to the
    series' points into its row k (sites.record: one launch per tensor), the forecast at a user's sites without draining a field.

    observations: a score.ObservationAccumulator with at least `steps` leads, and obs: a sequence of `steps` entries, each a pair
    (obs_upper (.., 5, 13, N), obs_surface (.., 4, N)) of device tensors in physical units, NaN where there is no report, or None (no
    observations for that lead).  After step k the step's fields are scored against obs[k] at the points and pooled at lead k
    (observations.score: two launches per tensor).  Both hooks follow the graph replay on the same stream, outside the captured
    graph, with no host sync; the returned values are unchanged."""
    who = "rollout"

    def per_step(seq, what):
        seq = list(seq)
        if len(seq) != steps:
            raise ValueError(f"{who}: {len(seq)} {what} for {steps} steps")
        return seq

    def holds(hook, what):
        if hook is not None and hook.leads < steps:
            raise ValueError(f"{who}: the {what} holds {hook.leads} leads, the rollout makes {steps} steps")

    def pairs(seq, what):
        for p in seq:
            if p is not None and len(p) != 2:
                raise ValueError(f"{who}: {what} or None")

    check_lead_stats(lead_stats, steps, who)
    holds(sites, "point series")
    if (observations is None) != (obs is None):
        raise ValueError(f"{who}: observations and obs go together (a score.ObservationAccumulator and one pair (obs_upper, "
                         "obs_surface) or None per step)")
    if obs is not None:
        obs = per_step(obs, "obs entries")
        holds(observations, "observation accumulator")
        pairs(obs, "an obs entry is a pair (obs_upper, obs_surface)")
    if (scorecard is not None and targets is None) or (targets is not None and scorecard is None and events is None):
        raise ValueError(f"{who}: scorecard and targets go together (a score.ScoreAccumulator and one target pair or None per step)")
    if events is not None and targets is None:
        raise ValueError(f"{who}: events needs targets (a score.EventAccumulator and one target pair or None per step)")
    if targets is not None:
        targets = per_step(targets, "targets")
        holds(scorecard, "scorecard")
        holds(events, "event accumulator")
        pairs(targets, "a target is a pair (target_upper, target_surface)")

    def hooks(k, upper, surface):
        """Step k's physical-unit fields meet the hooks, in the documented order; all launches, no host sync."""
        target, ob = None if targets is None else targets[k], None if obs is None else obs[k]
        if drain is not None:
            drain.submit([upper, surface], tag=k)
        if scorecard is not None and target is not None:
            scorecard.score(k, upper, surface, *target)
        if events is not None and target is not None:
            events.score(k, upper, surface, *target)
        if lead_stats is not None:
            lead_stats.update(k, upper, surface)
        if sites is not None:
            sites.record(k, upper, surface)
        if observations is not None and ob is not None:
            observations.score(k, upper, surface, *ob)

    history = []
    with torch.no_grad():
        if graph:
            g = GraphedStep(model, inp, inp_surface, statistics, maps, const_h, stats_last, feed_back=True)
            for k in range(steps):
                out, out_s = g.step()
                if keep:
                    history.append((out.clone(), out_s.clone()))
                hooks(k, g.inp, g.inp_surface)
            up, sf = g.inp.clone(), g.inp_surface.clone()
        else:
            up, sf = inp, inp_surface
            for k in range(steps):
                out, out_s = model(up, sf, statistics, maps, const_h)
                if keep:
                    history.append((out.clone(), out_s.clone()))
                up, sf = norm_back(out, out_s, stats_last)
                hooks(k, up, sf)
    return (up, sf, history) if keep else (up, sf)
