"""Latitude-weighted RMSE / ACC on the device (reference era5_data/score.py:80-135).

The 286 MB prediction/target fields never leave HBM: one HIP reduction pass (`pangu_lat_weighted_sums`) produces the
four weighted sums per (sample, channel) plane, from which both scores follow.  The weights reproduce the reference's
torch versions, including its `3.1416` literal for pi (score.py:89,98 — the numpy versions use np.pi)."""
import torch

from . import _lib
from .ops import _chk, _stream


def latitude_weights(num_lat, device):
    """reference score.py:82-88: num_lat * cos(3.1416/180 * lat_j) / sum_j cos(...), lat_j = 90 - j*180/(num_lat-1)."""
    j = torch.arange(0, num_lat, device=device)
    lat = 90.0 - j * 180.0 / float(num_lat - 1)
    c = torch.cos(3.1416 / 180.0 * lat)
    return (num_lat * c / torch.sum(c)).to(torch.float32).contiguous()


def _sums(pred, target):
    if pred.shape != target.shape or pred.dim() not in (3, 4, 5):
        raise RuntimeError("pred/target must have equal shape (.., H, W)")
    H, W = pred.shape[-2], pred.shape[-1]
    planes = pred.numel() // (H * W)
    out = torch.zeros((planes, 4), dtype=torch.float32, device=pred.device)
    w = latitude_weights(H, pred.device)
    lib = _lib.load()
    _lib.check(lib.pangu_lat_weighted_sums(_stream(pred), _chk(pred.contiguous(), "pred"), _chk(target.contiguous(), "target"),
                                           w.data_ptr(), out.data_ptr(), planes, H, W), "lat_weighted_sums")
    return out.view(pred.shape[:-2] + (4,)), H * W


def weighted_rmse_channels(pred, target):
    """reference weighted_rmse_torch_channels (score.py:92-105): sqrt(mean_{h,w} w_h (p-t)^2) per leading index."""
    s, n = _sums(pred, target)
    return torch.sqrt(s[..., 0] / n)


def weighted_acc_channels(pred, target):
    """reference weighted_acc_torch_channels (score.py:123-135)."""
    s, _ = _sums(pred, target)
    return s[..., 1] / torch.sqrt(s[..., 2] * s[..., 3])


def weighted_rmse(pred, target):
    return weighted_rmse_channels(pred, target).mean(dim=0)


def weighted_acc(pred, target):
    return weighted_acc_channels(pred, target).mean(dim=0)


# ---- what the wrappers below share: pointers, cached latitude weights, the (upper, surface) contract, per-plane vectors, lead pools

_LAT_WEIGHTS = {}                     # (H, device) -> latitude_weights(H, device)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _lat_weights(H, device):
    """latitude_weights(H, device), built once per (H, device): half a dozen small torch launches otherwise, per tensor and call."""
    key = (H, str(device))
    if key not in _LAT_WEIGHTS:
        _LAT_WEIGHTS[key] = latitude_weights(H, device)
    return _LAT_WEIGHTS[key]


def _no_cpu(who, device):
    raise RuntimeError(f"{who}: the Pangu HIP path needs tensors on an MI355X device (got {device}); there is no CPU fallback")


def _check_members(who, upper, surface, target_upper, target_surface):
    """The member form of the pair: upper (E,5,13,H,W) and surface (E,4,H,W) on one grid, 2 <= E <= 128, W % 4 == 0, and both
    targets or neither."""
    us, ss = upper.shape, surface.shape
    E = us[0]
    if len(us) != 5 or len(ss) != 4 or ss[0] != E or us[1:3] != (5, 13) or ss[1] != 4:
        raise ValueError(f"{who}: expected upper (E,5,13,H,W) and surface (E,4,H,W)")
    if us[-2:] != ss[-2:]:
        raise ValueError(f"{who}: upper and surface on different grids")
    if not 2 <= E <= 128:
        raise ValueError(f"{who}: 2 <= E <= 128 members, got {E}")
    if us[-1] % 4:
        raise ValueError(f"{who}: W % 4 != 0")
    if (target_upper is None) != (target_surface is None):
        raise ValueError(f"{who}: give both targets or neither")


def _check_cases(who, upper, surface, targets=None, w4=False, max_w=None, dense=False):
    """The case form of the pair: upper (.., 5, 13, H, W) and surface (.., 4, H, W) with the same leading dimensions and grid.
    targets: the (target_upper, target_surface) pair of an entry that needs both, one value per forecast value; w4: W % 4 == 0,
    and with max_w also W <= max_w; dense: contiguous fp32 tensors on one device, not empty.  Returns (H, W)."""
    if dense:
        for t, name in ((upper, "upper"), (surface, "surface")):
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"{who}: {name} must be a contiguous float32 tensor")
    us, ss = upper.shape, surface.shape                 # read once: every .shape builds a new torch.Size
    if len(us) < 4 or len(ss) < 3 or us[-4:-2] != (5, 13) or ss[-3] != 4:
        raise ValueError(f"{who}: expected upper (.., 5, 13, H, W) and surface (.., 4, H, W)")
    if us[:-4] != ss[:-3] or us[-2:] != ss[-2:]:
        raise ValueError(f"{who}: upper and surface disagree in their leading dimensions or grids")
    H, W = us[-2:]
    if w4 and (W % 4 or (max_w is not None and W > max_w)):
        raise ValueError(f"{who}: W % 4 != 0" + ("" if max_w is None else f" or W > {max_w}"))
    if targets is not None:
        target_upper, target_surface = targets
        if target_upper is None or target_surface is None:
            raise ValueError(f"{who}: both targets are required")
        if target_upper.numel() != upper.numel() or target_surface.numel() != surface.numel():
            raise ValueError(f"{who}: the targets must hold one value per forecast value, got {tuple(target_upper.shape)} and "
                             f"{tuple(target_surface.shape)} for {tuple(upper.shape)} and {tuple(surface.shape)}")
    if dense and (upper.numel() == 0 or upper.device != surface.device):
        raise ValueError(f"{who}: empty tensors, or upper and surface on different devices")
    return H, W


def _per_plane(values, t, device):
    """fp32 (planes,) on `device`: the statistic `values` ((.., 5, 13, 1, 1), (.., 4, 1, 1) or flat, one value per plane of one
    case) for every plane of t, whose last dimensions are one case's planes and the grid; leading cases repeat the values."""
    v = values.to(device=device, dtype=torch.float32).reshape(-1)
    planes = t.numel() // (t.shape[-2] * t.shape[-1])
    return v.expand(planes // v.numel(), v.numel()).contiguous().view(planes)      # view: refuses values that do not fill the planes


def _stats_affine(t, stats_last, upper, device):
    """(mul, add) per plane of a NORMALISED t, so that t * mul + add is rollout.norm_back with stats_last = (s_mean, s_std, u_mean,
    u_std); (None, None) without stats_last.  upper: t is the upper-air tensor and takes the u_ pair."""
    if stats_last is None:
        return None, None
    s_mean, s_std, u_mean, u_std = stats_last
    mean, std = (u_mean, u_std) if upper else (s_mean, s_std)
    return _per_plane(std, t, device), _per_plane(mean, t, device)


def _per_plane_thresholds(thr, T, planes, device):
    """fp32 (T, cases, per_case) on `device`: the thresholds thr (T, 5, 13) or (T, 4) for `planes` planes, cases outermost."""
    per_case = thr[0].numel()
    return thr.to(device=device, dtype=torch.float32).reshape(T, 1, per_case).expand(T, planes // per_case, per_case).contiguous()


class _LeadPool:
    """What the per-lead accumulators share: `leads` slots that start empty, the lead check, cases(lead), the refusal to read an
    empty slot, and the region plans of score() per (H, W, device)."""

    _verb = "scored"

    def __init__(self, leads):
        self.leads = int(leads)
        if self.leads < 1:
            raise ValueError(f"{type(self).__name__}: leads must be >= 1")
        self._pool = [None] * self.leads
        self._plans = {}

    def _check_lead(self, lead):
        if not 0 <= lead < self.leads:
            raise IndexError(f"lead {lead} outside 0..{self.leads - 1}")

    def cases(self, lead):
        self._check_lead(lead)
        return 0 if self._pool[lead] is None else self._pool[lead][0].cases

    def _pooled(self, lead):
        self._check_lead(lead)
        if self._pool[lead] is None:
            raise ValueError(f"{type(self).__name__}: nothing {self._verb} at lead {lead}")
        return self._pool[lead]

    def _region_plan(self, regions, upper):
        """The RegionPlan of `regions` (a mapping as for region_bits, or None for the global region) on upper's grid and device."""
        if isinstance(regions, RegionPlan):
            return regions
        key = (upper.shape[-2], upper.shape[-1], str(upper.device))
        if key not in self._plans:
            self._plans[key] = region_bits(key[0], key[1], regions, upper.device)
        return self._plans[key]


ENSEMBLE_KEYS = ("rmse_mean", "acc_mean", "spread", "crps")


def _ens_stats(x, target, clim, want_fields, what):
    """One pangu_ensemble_stats_f32 call over x (E, *plane_shape, H, W); returns ({key: (*plane_shape) tensor}, mean, std)."""
    E, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    pshape = tuple(x.shape[1:-2])
    planes = x[0].numel() // (H * W)
    _chk(x, what)
    if target is not None:
        target = target.reshape(x.shape[1:])
        _chk(target, what + " target")
    slabs = (H + 3) // 4
    ws = torch.empty(planes * slabs * 8, dtype=torch.float32, device=x.device)
    out = torch.empty((planes, 4), dtype=torch.float32, device=x.device)
    mean = torch.empty(x.shape[1:], dtype=torch.float32, device=x.device) if want_fields else None
    std = torch.empty(x.shape[1:], dtype=torch.float32, device=x.device) if want_fields else None
    _lib.check(_lib.load().pangu_ensemble_stats_f32(
        _stream(x), x.data_ptr(), x[0].numel(), E, _ptr(target), _ptr(clim), _lat_weights(H, x.device).data_ptr(), out.data_ptr(),
        _ptr(mean), _ptr(std), ws.data_ptr(), ws.numel() * 4, planes, H, W), "ensemble_stats_f32")
    return {k: out[:, i].reshape(pshape) for i, k in enumerate(ENSEMBLE_KEYS)}, mean, std


def ensemble_scores(upper, surface, target_upper, target_surface, stats_last, want_fields=False):
    """Latitude-weighted ensemble scores of E members upper (E,5,13,H,W) / surface (E,4,H,W) against one target
    ((1,)5,13,H,W / (1,)4,H,W), one HIP pass per tensor (pangu_ensemble_stats_f32), no host sync.

    Returns (upper_scores, surface_scores): dicts of device tensors, (5,13) and (4,), with the keys
      rmse_mean  RMSE of the ensemble mean (reference weighted_rmse_torch_channels, score.py:92-105),
      acc_mean   ACC of the ensemble mean against the stats_last means as climatology (reference pangu_sample.py:252-256),
      spread     sqrt(weighted mean of the unbiased member variance),
      crps       weighted mean of the fair CRPS, (1/E) sum|x_i - y| - 1/(2E(E-1)) sum_ij |x_i - x_j|.
    want_fields=True adds "mean" and "std" (the ensemble mean and the square root of the unbiased variance), shaped like one
    member.  Targets may be None: then only spread (and the fields) are computed, the other keys are NaN."""
    _check_members("ensemble_scores", upper, surface, target_upper, target_surface)
    s_mean, _, u_mean, _ = stats_last
    su, mu, sdu = _ens_stats(upper, target_upper, _per_plane(u_mean, upper[0], upper.device), want_fields, "ensemble upper")
    ss, ms, sds = _ens_stats(surface, target_surface, _per_plane(s_mean, surface[0], upper.device), want_fields, "ensemble surface")
    if want_fields:
        su.update(mean=mu, std=sdu)
        ss.update(mean=ms, std=sds)
    return su, ss


# ---- ensemble reliability: verification rank histogram, reliability tables of threshold events, exceedance probabilities ------

RELIABILITY_MAX_T = 4      # csrc/reliability.hip


def reliability_workspace_bytes(planes, H, E, T):
    """Workspace of pangu_ensemble_reliability_f32 (include/pangu_hip.h): per (plane, slab of 4 rows) one uint32 count and one
    float partial for each of the (1 + 2T) * (E + 1) bins."""
    return planes * ((H + 3) // 4) * (1 + 2 * T) * (E + 1) * 8


class ReliabilityTables:
    """The tables of one ensemble_reliability call, or a pool of `cases` of them (ReliabilityAccumulator), for planes shaped
    `rank_counts.shape[:-1]` ((5, 13) or (4,)):
      rank_counts / rank_freq          (..., E+1)     points per verification rank (Talagrand histogram),
      event_counts / event_freq        (T, ..., E+1)  points at which k of the E members exceed threshold t (N_t),
      observed_counts / observed_freq  (T, ..., E+1)  those of them at which the target exceeds it too (O_t),
      prob                             (T, ..., H, W) k / E per grid point, or None.
    *_counts are int64 point counts; *_freq weight each point by its latitude weight and divide by H*W, so rank_freq and each N_t
    sum to about `cases` per plane.  The derived quantities are torch ops on these small tables (float64) and work on any device."""

    def __init__(self, E, T, rank_counts, rank_freq, event_counts, event_freq, observed_counts, observed_freq, prob=None, cases=1):
        self.E, self.T, self.cases = int(E), int(T), cases
        self.rank_counts, self.rank_freq = rank_counts, rank_freq
        self.event_counts, self.event_freq = event_counts, event_freq
        self.observed_counts, self.observed_freq = observed_counts, observed_freq
        self.prob = prob

    @classmethod
    def from_raw(cls, counts, freq, E, T, plane_shape, prob=None):
        """From the kernel's layout: counts / freq (planes, 1 + 2T, E+1), prob (T, planes, H, W) or None."""
        ps = tuple(plane_shape)
        rank = lambda a: a[:, 0].reshape(ps + (E + 1,))
        tabs = lambda a, first: a[:, first::2].transpose(0, 1).reshape((T,) + ps + (E + 1,))
        counts = counts.to(torch.int64)
        if prob is not None:
            prob = prob.reshape((T,) + ps + tuple(prob.shape[-2:]))
        return cls(E, T, rank(counts), rank(freq), tabs(counts, 1), tabs(freq, 1), tabs(counts, 2), tabs(freq, 2), prob)

    def _p(self):
        return torch.arange(self.E + 1, dtype=torch.float64, device=self.rank_freq.device) / self.E

    def brier(self):
        """Latitude-weighted Brier score per (t, plane), (T, ...): mean of (k/E - o)^2 = sum_k [N_k (k/E)^2 - 2 O_k (k/E) + O_k]."""
        p, n, o = self._p(), self.event_freq.double(), self.observed_freq.double()
        return (n * p * p - 2.0 * o * p + o).sum(-1) / self.cases

    def reliability_curve(self):
        """(forecast probability k/E (E+1,), observed frequency O_k / N_k (T, ..., E+1; NaN where no point forecast k/E),
        forecast share N_k (T, ..., E+1; sums to about 1))."""
        n, o = self.event_freq.double(), self.observed_freq.double()
        return self._p(), o / n, n / self.cases

    def rank_frequencies(self):
        """The weighted rank histogram normalised to sum 1 per plane (..., E+1): flat at 1 / (E+1) for a calibrated ensemble."""
        f = self.rank_freq.double()
        return f / f.sum(-1, keepdim=True)


def spread_skill_ratio(scores, E):
    """sqrt((E+1)/E) * spread / rmse_mean of an ensemble_scores dict: 1 where the spread matches the error of the ensemble mean
    (the factor accounts for the finite ensemble), below 1 for an under-dispersive ensemble."""
    return ((E + 1.0) / E) ** 0.5 * scores["spread"] / scores["rmse_mean"]


def _check_thresholds(thresholds, who):
    if thresholds is None:
        return None, None, 0
    tu, ts = thresholds
    if tu.dim() != 3 or tuple(tu.shape[1:]) != (5, 13) or ts.dim() != 2 or ts.shape[1] != 4 or ts.shape[0] != tu.shape[0]:
        raise ValueError(f"{who}: thresholds must be a pair of tensors (T, 5, 13) and (T, 4)")
    if tu.shape[0] > RELIABILITY_MAX_T:
        raise ValueError(f"{who}: at most {RELIABILITY_MAX_T} thresholds, got {tu.shape[0]}")
    return tu, ts, int(tu.shape[0])


def _reliability(x, target, thr, T, seed, first_plane, want_fields, what):
    """One pangu_ensemble_reliability_f32 call over x (E, *plane_shape, H, W); thr (T, *plane_shape) or None."""
    E, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    pshape = tuple(x.shape[1:-2])
    planes = x[0].numel() // (H * W)
    _chk(x, what)
    dev = x.device
    if target is not None:
        target = target.reshape(x.shape[1:])
        _chk(target, what + " target")
    thr = _per_plane_thresholds(thr, T, planes, dev) if T else None
    counts = torch.empty((planes, 1 + 2 * T, E + 1), dtype=torch.int32, device=dev)      # the entry's uint32, all < 2^31
    freq = torch.empty((planes, 1 + 2 * T, E + 1), dtype=torch.float32, device=dev)
    prob = torch.empty((T, planes, H, W), dtype=torch.float32, device=dev) if want_fields and T else None
    ws = torch.empty(reliability_workspace_bytes(planes, H, E, T), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().pangu_ensemble_reliability_f32(
        _stream(x), x.data_ptr(), x[0].numel(), E, _ptr(target), _ptr(thr), T, _lat_weights(H, dev).data_ptr(),
        int(seed) & 0xFFFFFFFF, first_plane, counts.data_ptr(), freq.data_ptr(), _ptr(prob), ws.data_ptr(), ws.numel(), planes, H, W),
        "ensemble_reliability_f32")
    return ReliabilityTables.from_raw(counts, freq, E, T, pshape, prob)


def ensemble_reliability(upper, surface, target_upper, target_surface, thresholds=None, seed=0, want_fields=False):
    """Reliability tables of E members upper (E,5,13,H,W) / surface (E,4,H,W) against one target ((1,)5,13,H,W / (1,)4,H,W),
    one HIP pass per tensor (pangu_ensemble_reliability_f32, definitions pinned in csrc/reliability.hip), no host sync.

    thresholds: None, or a pair of tensors (T, 5, 13) and (T, 4) in physical units, T <= 4, for the events x > threshold; +inf
    means "no event on this plane".  Device tensors avoid an upload.  seed breaks ties between members and the target in the
    rank (uniformly; the surface planes hash as planes 65..68, the numbering of ensemble.perturb_).  Targets may be None
    (forecast mode, needs thresholds): the rank and observed tables are then zero.  want_fields=True adds the exceedance
    probabilities k / E as .prob.  Returns (upper_result, surface_result), two ReliabilityTables."""
    who = "ensemble_reliability"
    _check_members(who, upper, surface, target_upper, target_surface)
    thr_u, thr_s, T = _check_thresholds(thresholds, who)
    if T == 0 and target_upper is None:
        raise ValueError(f"{who}: nothing to compute without a target and without thresholds")
    ru = _reliability(upper, target_upper, thr_u, T, seed, 0, want_fields, "ensemble upper")
    rs = _reliability(surface, target_surface, thr_s, T, seed, 65, want_fields, "ensemble surface")
    return ru, rs


class ReliabilityAccumulator(_LeadPool):
    """Pools ReliabilityTables over cases, per lead: the tables add exactly (counts in int64, frequencies in float64, on the
    tables' device, no host sync).  leads: the number of leads (0 .. leads-1).  One rank histogram from one case says little;
    this and spread_skill_ratio are the instruments for calibrating the perturbation amplitude."""

    _FIELDS = ("rank_counts", "rank_freq", "event_counts", "event_freq", "observed_counts", "observed_freq")
    _verb = "added"

    def __init__(self, leads):
        super().__init__(leads)
        self.E = self.T = None

    def add(self, lead, upper_result, surface_result):
        self._check_lead(lead)
        for r in (upper_result, surface_result):
            if self.E is None:
                self.E, self.T = r.E, r.T
            if (r.E, r.T) != (self.E, self.T):
                raise ValueError(f"ReliabilityAccumulator: tables of E = {r.E}, T = {r.T} added to a pool of E = {self.E}, "
                                 f"T = {self.T}")
        wide = lambda t: t.to(torch.int64 if not t.is_floating_point() else torch.float64)
        if self._pool[lead] is None:
            self._pool[lead] = tuple(ReliabilityTables(r.E, r.T, *(wide(getattr(r, f)).clone() for f in self._FIELDS), cases=r.cases)
                                     for r in (upper_result, surface_result))
            return
        for pooled, r in zip(self._pool[lead], (upper_result, surface_result)):
            for f in self._FIELDS:
                getattr(pooled, f).add_(wide(getattr(r, f)))
            pooled.cases += r.cases

    def tables(self, lead):
        """(upper, surface) pooled ReliabilityTables of a lead."""
        return self._pooled(lead)

    def brier(self, lead):
        return tuple(t.brier() for t in self.tables(lead))

    def reliability_curve(self, lead):
        return tuple(t.reliability_curve() for t in self.tables(lead))

    def rank_frequencies(self, lead):
        return tuple(t.rank_frequencies() for t in self.tables(lead))


# ---- ensemble quantile fields, the quantile (pinball) score and quantile coverage ----------------------------------------------

QUANTILES_MAX_Q = 8      # csrc/quantile.hip


def quantiles_workspace_bytes(planes, H, Q):
    """Workspace of pangu_ensemble_quantiles_f32 (include/pangu_hip.h): per (plane, slab of 4 rows) 3Q + 1 32-bit words."""
    return planes * ((H + 3) // 4) * (3 * Q + 1) * 4


def _check_levels(q, who):
    try:
        levels = [float(v) for v in q]
    except TypeError:
        raise ValueError(f"{who}: q must be a sequence of 1..{QUANTILES_MAX_Q} levels in [0, 1]") from None
    if not 1 <= len(levels) <= QUANTILES_MAX_Q:
        raise ValueError(f"{who}: 1 <= Q <= {QUANTILES_MAX_Q} quantile levels, got {len(levels)}")
    for v in levels:
        if not 0.0 <= v <= 1.0:      # NaN included
            raise ValueError(f"{who}: quantile levels must lie in [0, 1], got {v}")
    return tuple(levels)


class QuantileResult:
    """The outputs of one ensemble_quantiles call for planes shaped `plane_shape` ((5, 13) or (4,)):
      q                the Q levels (a tuple of floats),
      fields           (Q, ..., H, W) quantile fields, or None,
      pinball          (Q, ...) latitude-weighted quantile score, mean of rho_q(y - x_q); None without targets,
      coverage_counts  (Q, ...) int64 points with y <= x_q; None without targets,
      coverage_freq    (Q, ...) the same points weighted by latitude over H*W (near q when calibrated); None without targets,
      nonfinite        (...) int64 points per plane left out because a member is NaN (their fields are NaN).
    The definitions are pinned in csrc/quantile.hip."""

    def __init__(self, q, fields, pinball, coverage_counts, coverage_freq, nonfinite):
        self.q = tuple(q)
        self.fields, self.pinball = fields, pinball
        self.coverage_counts, self.coverage_freq, self.nonfinite = coverage_counts, coverage_freq, nonfinite

    def interval(self, lo_index, hi_index):
        """The central interval between levels q[lo_index] <= q[hi_index] as a dict of per-plane tensors (float64):
          nominal   q[hi] - q[lo] (a float),
          coverage  coverage_freq[hi] - coverage_freq[lo]: the weighted share of points with x_lo < y <= x_hi (needs targets),
          width     the latitude-weighted mean of fields[hi] - fields[lo] (needs fields; points with a NaN member make it NaN).
        Entries whose inputs are missing are None."""
        Q = len(self.q)
        if not (0 <= lo_index < Q and 0 <= hi_index < Q):
            raise IndexError(f"QuantileResult.interval: level indices within 0..{Q - 1}")
        if self.q[lo_index] > self.q[hi_index]:
            raise ValueError("QuantileResult.interval: q[lo_index] must not exceed q[hi_index]")
        out = {"nominal": self.q[hi_index] - self.q[lo_index], "coverage": None, "width": None}
        if self.coverage_freq is not None:
            out["coverage"] = self.coverage_freq[hi_index].double() - self.coverage_freq[lo_index].double()
        if self.fields is not None:
            d = self.fields[hi_index] - self.fields[lo_index]
            w = latitude_weights(d.shape[-2], d.device).double()
            out["width"] = (d.double() * w[:, None]).mean(dim=(-2, -1))
        return out


def _quantiles(x, target, levels, want_fields, what):
    """One pangu_ensemble_quantiles_f32 call over x (E, *plane_shape, H, W)."""
    import ctypes
    E, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    pshape = tuple(x.shape[1:-2])
    planes = x[0].numel() // (H * W)
    Q = len(levels)
    _chk(x, what)
    dev = x.device
    if target is not None:
        target = target.reshape(x.shape[1:])
        _chk(target, what + " target")
    fields = torch.empty((Q, planes, H, W), dtype=torch.float32, device=dev) if want_fields else None
    nonfinite = torch.empty((planes,), dtype=torch.int32, device=dev)      # the entry's uint32, all < 2^31
    pin = cov = cnt = w = None
    if target is not None:
        pin = torch.empty((Q, planes), dtype=torch.float32, device=dev)
        cov = torch.empty((Q, planes), dtype=torch.float32, device=dev)
        cnt = torch.empty((Q, planes), dtype=torch.int32, device=dev)
        w = _lat_weights(H, dev)
    ws = torch.empty(quantiles_workspace_bytes(planes, H, Q), dtype=torch.uint8, device=dev)
    lv = (ctypes.c_double * Q)(*levels)
    _lib.check(_lib.load().pangu_ensemble_quantiles_f32(
        _stream(x), x.data_ptr(), x[0].numel(), E, ctypes.addressof(lv), Q, _ptr(target), _ptr(w), _ptr(fields), _ptr(pin), _ptr(cnt),
        _ptr(cov), nonfinite.data_ptr(), ws.data_ptr(), ws.numel(), planes, H, W), "ensemble_quantiles_f32")
    shaped = lambda t: None if t is None else t.reshape((Q,) + pshape)
    return QuantileResult(levels, None if fields is None else fields.reshape((Q,) + pshape + (H, W)), shaped(pin),
                          None if cnt is None else shaped(cnt.to(torch.int64)), shaped(cov),
                          nonfinite.to(torch.int64).reshape(pshape))


def ensemble_quantiles(upper, surface, q, target_upper=None, target_surface=None, want_fields=True):
    """Quantile fields of E members upper (E,5,13,H,W) / surface (E,4,H,W) at the levels q (a sequence of 1..8 floats in [0, 1]),
    and with one target ((1,)5,13,H,W / (1,)4,H,W) their quantile (pinball) score and coverage; one HIP pass per tensor
    (pangu_ensemble_quantiles_f32, definitions pinned in csrc/quantile.hip: numpy's "linear" method clamped into its bracket,
    exact member values where q * (E - 1) is an integer), no host sync.

    want_fields=False skips the (Q, ..., H, W) fields (scores only; needs targets).  Returns (upper_result, surface_result), two
    QuantileResult."""
    who = "ensemble_quantiles"
    _check_members(who, upper, surface, target_upper, target_surface)
    levels = _check_levels(q, who)
    if not want_fields and target_upper is None:
        raise ValueError(f"{who}: nothing to compute without fields and without a target")
    ru = _quantiles(upper, target_upper, levels, want_fields, "ensemble upper")
    rs = _quantiles(surface, target_surface, levels, want_fields, "ensemble surface")
    return ru, rs


# ---- zonal power spectra: power per zonal wavenumber along each latitude circle, averaged over latitude bands -------------------

SPECTRUM_MAX_B = 4                    # csrc/spectrum.hip
SPECTRUM_WS_LIMIT = 256 << 20         # bytes of workspace per launch: zonal_spectrum splits N above it

_BASIS = {}                           # (W, K, device) -> (cos, sin) fp32 device tensors
_BAND_WEIGHTS = {}                    # (H, bands, device) -> the (B, H) weights of named bands, as zonal_spectrum uses them


def spectrum_basis(W, K):
    """The two basis tables of pangu_zonal_spectrum_f32 as float64 numpy arrays (W/2 + 1, K + 1): cos and sin of
    2 pi r / W with r = (j k) mod W taken in integers, so the argument never exceeds 2 pi; exact 0 and +-1 where the angle is
    a multiple of pi / 2.  The kernel reads them rounded once to fp32."""
    import numpy as np
    if W < 8 or W % 4 or not 1 <= K <= W // 2:
        raise ValueError(f"spectrum_basis: W % 4 == 0, W >= 8 and 1 <= K <= W/2, got W = {W}, K = {K}")
    j = np.arange(W // 2 + 1, dtype=np.int64)[:, None]
    k = np.arange(K + 1, dtype=np.int64)[None, :]
    r = (j * k) % W
    ang = 2.0 * np.pi * r.astype(np.float64) / W
    c, s = np.cos(ang), np.sin(ang)
    quarter = (4 * r) % W == 0
    q = (4 * r) // W                 # the quadrant where the angle is a multiple of pi / 2
    c[quarter] = np.array([1.0, 0.0, -1.0, 0.0])[q[quarter]]
    s[quarter] = np.array([0.0, 1.0, 0.0, -1.0])[q[quarter]]
    return c, s


def _device_basis(W, K, device):
    key = (W, K, str(device))
    if key not in _BASIS:
        c, s = spectrum_basis(W, K)
        up = lambda a: torch.from_numpy(a).to(torch.float32).to(device).contiguous()      # float64 -> fp32: the one rounding
        _BASIS[key] = (up(c), up(s))
    return _BASIS[key]


def spectrum_band_weights(H, bands=None, device=None):
    """(B, H) fp32 band weights for zonal_spectrum.  bands: a sequence of up to 4 (lat_south, lat_north) pairs in degrees on the
    grid lat_j = 90 - j * 180 / (H - 1) (both ends included); default: the one global band (-90, 90).  Each row is
    latitude_weights(H) restricted to the band and normalised to sum 1, so the global row is latitude_weights(H) / H and, with
    kmax = W/2, the global spectrum sums over k to the sum w p^2 / (H W) of pangu_lat_weighted_sums."""
    bands = [(-90.0, 90.0)] if bands is None else list(bands)
    if not 1 <= len(bands) <= SPECTRUM_MAX_B:
        raise ValueError(f"spectrum_band_weights: 1 <= B <= {SPECTRUM_MAX_B} bands, got {len(bands)}")
    device = torch.device("cpu") if device is None else device
    w = latitude_weights(H, device).double()
    lat = 90.0 - torch.arange(H, device=device, dtype=torch.float64) * 180.0 / float(H - 1)
    rows = []
    for band in bands:
        try:
            south, north = (float(v) for v in band)
        except (TypeError, ValueError):
            raise ValueError("spectrum_band_weights: a band is a (lat_south, lat_north) pair") from None
        if not south <= north:      # NaN included
            raise ValueError(f"spectrum_band_weights: lat_south <= lat_north, got ({south}, {north})")
        inside = (lat >= south) & (lat <= north)
        row = torch.where(inside, w, torch.zeros_like(w))
        total = float(row.sum())
        if not bool(inside.any()) or not total > 0.0:
            raise ValueError(f"spectrum_band_weights: the band ({south}, {north}) holds no latitude row of weight")
        rows.append(row / total)
    return torch.stack(rows).to(torch.float32).contiguous()


class SpectrumResult:
    """The zonal power spectra of one zonal_spectrum call for planes shaped (5, 13) or (4,):
      power  (N, B, ..., K + 1) band-averaged power per wavenumber, on the device; fp32 from the kernel, float64 after
             mean_over_items,
      k      the wavenumbers 0..K (int64),
      bands  what the call was given: None (global), the (lat_south, lat_north) pairs, or the (B, H) weight tensor.
    The definitions are pinned in csrc/spectrum.hip.  The derived quantities are torch ops on these small tables (float64) and
    work on any device."""

    def __init__(self, power, k, bands):
        self.power, self.k, self.bands = power, k, bands

    def variance(self):
        """(N, B, ...) anomaly power: the sum over k >= 1, in float64."""
        return self.power[..., 1:].double().sum(-1)

    def mean_over_items(self):
        """A result with N = 1: the items' spectra added in float64 and divided by N."""
        return SpectrumResult(self.power.double().mean(dim=0, keepdim=True), self.k, self.bands)

    def ratio(self, reference):
        """power / reference.power in float64 (a reference with N = 1 serves every item)."""
        return self.power.double() / reference.power.double()

    def effective_resolution(self, reference, threshold=0.5):
        """Per (item, band, plane) the smallest k >= 1 from which ratio(reference) stays below `threshold` up to K, K + 1 where
        the ratio at K is not below it (int64): from which scale on this forecast is blurred."""
        below = (self.ratio(reference)[..., 1:] < threshold).to(torch.int64)
        tail = torch.flip(torch.cumprod(torch.flip(below, dims=(-1,)), dim=-1), dims=(-1,))      # 1 where all of k..K are below
        return below.shape[-1] + 1 - tail.sum(-1)


def _spectrum(x, minus, bw, K, bands, what):
    """pangu_zonal_spectrum_f32 over x (N, *plane_shape, H, W), N split so that the workspace stays under SPECTRUM_WS_LIMIT."""
    N, H, W = x.shape[0], x.shape[-2], x.shape[-1]
    pshape = tuple(x.shape[1:-2])
    item = x[0].numel()
    planes = item // (H * W)
    B = bw.shape[0]
    dev = x.device
    if not x.is_cuda:
        _no_cpu(what, dev)
    if x.dtype != torch.float32:
        raise RuntimeError(f"{what}: expected float32, got {x.dtype}")
    stride = x.stride(0) if N > 1 else item
    if not x[0].is_contiguous() or stride < item or stride % 4:
        raise RuntimeError(f"{what}: expected contiguous items with an item stride that is a multiple of 4")
    if minus is not None:
        minus = minus.reshape(x.shape[1:])
        _chk(minus, what + " minus")
    cos_t, sin_t = _device_basis(W, K, dev)
    lib = _lib.load()
    per_item = lib.pangu_zonal_spectrum_ws_bytes(1, planes, H, B, K)
    if per_item < 0:
        _lib.check(per_item, "zonal_spectrum_ws_bytes")
    step = max(1, min(N, SPECTRUM_WS_LIMIT // per_item))
    ws = torch.empty(step * per_item, dtype=torch.uint8, device=dev)
    outs = []
    for n0 in range(0, N, step):
        n = min(step, N - n0)
        out = torch.empty((n, B, planes, K + 1), dtype=torch.float32, device=dev)
        _lib.check(lib.pangu_zonal_spectrum_f32(
            _stream(x), x[n0].data_ptr(), stride, n, _ptr(minus), bw.data_ptr(), B,
            cos_t.data_ptr(), sin_t.data_ptr(), K, out.data_ptr(), ws.data_ptr(), ws.numel(), planes, H, W), "zonal_spectrum_f32")
        outs.append(out)
    power = outs[0] if len(outs) == 1 else torch.cat(outs)
    return SpectrumResult(power.reshape((N, B) + pshape + (K + 1,)), torch.arange(K + 1, device=dev), bands)


def zonal_spectrum(upper, surface, minus_upper=None, minus_surface=None, bands=None, kmax=None):
    """Zonal power spectra of N states upper (N,5,13,H,W) / surface (N,4,H,W), N >= 1 (items may be strided: members of a
    larger buffer), optionally of their difference to one state minus_upper ((1,)5,13,H,W) / minus_surface ((1,)4,H,W), per
    latitude band and wavenumber 0..kmax (default W/2); one HIP pass per tensor (pangu_zonal_spectrum_f32, definitions pinned in
    csrc/spectrum.hip: a pivot-subtracted folded real DFT on the f32-input MFMA), no host sync once the basis tables of
    (W, kmax, device) are cached.

    bands: None (the global band), a sequence of up to 4 (lat_south, lat_north) pairs (spectrum_band_weights), or a (B, H) fp32
    tensor of explicit row weights.  Returns (upper_result, surface_result), two SpectrumResult."""
    who = "zonal_spectrum"
    if upper.dim() != 5 or surface.dim() != 4 or surface.shape[0] != upper.shape[0] or upper.shape[0] < 1:
        raise ValueError(f"{who}: expected upper (N,5,13,H,W) and surface (N,4,H,W), N >= 1")
    H, W = upper.shape[-2], upper.shape[-1]
    if tuple(surface.shape[-2:]) != (H, W):
        raise ValueError(f"{who}: upper and surface on different grids")
    if W % 4 or W < 8:
        raise ValueError(f"{who}: W % 4 == 0 and W >= 8, got {W}")
    if (minus_upper is None) != (minus_surface is None):
        raise ValueError(f"{who}: give both minus tensors or neither")
    if minus_upper is not None and (minus_upper.numel() != upper[0].numel() or minus_surface.numel() != surface[0].numel()):
        raise ValueError(f"{who}: minus tensors must be one state, ((1,)5,13,H,W) and ((1,)4,H,W)")
    K = W // 2 if kmax is None else int(kmax)
    if not 1 <= K <= W // 2:
        raise ValueError(f"{who}: 1 <= kmax <= W/2 = {W // 2}, got {kmax}")
    if isinstance(bands, torch.Tensor):
        if bands.dim() != 2 or bands.shape[1] != H or not 1 <= bands.shape[0] <= SPECTRUM_MAX_B:
            raise ValueError(f"{who}: band weights must be (B, H) with 1 <= B <= {SPECTRUM_MAX_B}")
        bw = bands.to(device=upper.device, dtype=torch.float32).contiguous()
    else:
        bands = None if bands is None else list(bands)
        try:
            key = (H, None if bands is None else tuple((float(s), float(n)) for s, n in bands), str(upper.device))
        except (TypeError, ValueError):
            key = None                        # not pairs of numbers: spectrum_band_weights says what is wrong
        if key not in _BAND_WEIGHTS:          # a dozen small torch launches otherwise, a fifth of one state's transform
            bw = spectrum_band_weights(H, bands, upper.device)
            if key is None:
                raise ValueError(f"{who}: bands must be (lat_south, lat_north) pairs")
            _BAND_WEIGHTS[key] = bw
        bw = _BAND_WEIGHTS[key]
        bands = key[1]
    ru = _spectrum(upper, minus_upper, bw, K, bands, "spectrum upper")
    rs = _spectrum(surface, minus_surface, bw, K, bands, "spectrum surface")
    return ru, rs


# ---- conservative regridding to a coarser lat-lon grid of the same family ---------------------------------------------------------

REGRID_MAX_TAPS = 16                  # csrc/regrid.hip
REGRID_DROP = 1e-12                   # an overlap below this share of the output cell is a coinciding edge, not a tap


def _band(dense, who):
    """Band tables of the rows of `dense` (n_out, columns), whose non-zeros are contiguous: start / count int32 (n_out,), weights
    fp32 (n_out, T) zero-padded, T the largest count."""
    import numpy as np
    nz = dense > 0.0
    start = nz.argmax(axis=1).astype(np.int32)
    last = dense.shape[1] - 1 - nz[:, ::-1].argmax(axis=1)
    count = (last - start + 1).astype(np.int32)
    T = int(count.max())
    if T > REGRID_MAX_TAPS:
        raise ValueError(f"regrid_plan: {who} needs {T} taps per output cell, the kernel serves at most {REGRID_MAX_TAPS}")
    w = np.zeros((dense.shape[0], T), np.float32)
    for r in range(dense.shape[0]):
        w[r, :count[r]] = dense[r, start[r]:start[r] + count[r]]
    return start, count, w


class RegridPlan:
    """The first-order conservative remap of regrid_plan: per axis `*_start`, `*_count` (int32 per output index; lon_start may be
    negative, longitudes are read modulo W_in) and `*_weights` (fp32 (n_out, T), zero-padded), as pangu_regrid_planes_f32 reads
    them, and the float64 matrices they were rounded from (dense()).  The device copies of the tables are cached per device."""

    def __init__(self, H_in, W_in, H_out, W_out, r_lat, r_lon, lat, lon):
        self.H_in, self.W_in, self.H_out, self.W_out = H_in, W_in, H_out, W_out
        self._dense = (r_lat, r_lon)
        self.lat_start, self.lat_count, self.lat_weights = lat
        self.lon_start, self.lon_count, self.lon_weights = lon
        self._dev = {}

    @property
    def lat_taps(self):
        return self.lat_weights.shape[1]

    @property
    def lon_taps(self):
        return self.lon_weights.shape[1]

    @property
    def in_grid(self):
        return (self.H_in, self.W_in)

    @property
    def out_grid(self):
        return (self.H_out, self.W_out)

    def dense(self):
        """(R_lat (H_out, H_in), R_lon (W_out, W_in)) in float64: out = R_lat @ x @ R_lon.T per plane."""
        return self._dense

    def _device_tables(self, device):
        key = str(device)
        if key not in self._dev:
            up = lambda a: torch.from_numpy(a).to(device).contiguous()
            self._dev[key] = tuple(up(a) for a in (self.lat_start, self.lat_count, self.lat_weights, self.lon_start,
                                                   self.lon_count, self.lon_weights))
        return self._dev[key]


def regrid_plan(H_in, W_in, H_out, W_out):
    """The conservative remap from the grid (H_in, W_in) to the coarser (H_out, W_out), both of the project's family: latitudes
    lat_j = 90 - j * 180 / (H - 1) with the poles, longitudes lon_i = i * 360 / W.  Cell j spans lat_j +- 90 / (H - 1) clipped to
    [-90, 90] (the polar rows are half-height caps), cell i spans (i +- 1/2) * 360 / W, periodic.  In float64:
      R_lat[J, j]  the overlap of output cell J with input cell j in sin(latitude), divided by the row sum,
      R_lon[I, i]  the overlap in longitude divided by the output cell's width,
    overlaps below 1e-12 of the output cell dropped.  Rows sum to 1 and area_out^T R = area_in^T (area means are preserved).  The
    cell edges are compared as integers (in units of 90 / ((H_in - 1)(H_out - 1)) degrees and 180 / (W_in W_out) degrees), so edges
    that coincide give exactly no overlap.  Returns a RegridPlan; the same grid in and out gives the identity (one tap of weight 1)."""
    import numpy as np
    H_in, W_in, H_out, W_out = int(H_in), int(W_in), int(H_out), int(W_out)
    if not 2 <= H_out <= H_in:
        raise ValueError(f"regrid_plan: 2 <= H_out <= H_in, got H_in = {H_in}, H_out = {H_out} (no refinement, poles included)")
    if not 1 <= W_out <= W_in:
        raise ValueError(f"regrid_plan: 1 <= W_out <= W_in, got W_in = {W_in}, W_out = {W_out} (no refinement)")
    # latitude: colatitude of the edges as integers m, angle = pi * m / (2 M), M = (H_in - 1)(H_out - 1)
    M = (H_in - 1) * (H_out - 1)

    def edges(H, other):
        k = np.arange(H + 1, dtype=np.int64)
        return np.clip((2 * k - 1) * (other - 1), 0, 2 * M)

    e_in, e_out = edges(H_in, H_out), edges(H_out, H_in)
    top = np.maximum(e_out[:-1, None], e_in[None, :-1])              # the northern edge of the overlap (smaller colatitude)
    bot = np.minimum(e_out[1:, None], e_in[None, 1:])
    s = lambda m: np.cos(np.pi * m.astype(np.float64) / (2.0 * M))   # sin(latitude)
    ov = np.where(bot > top, s(top) - s(np.maximum(bot, top)), 0.0)
    cell = (s(e_out[:-1]) - s(e_out[1:]))[:, None]
    ov[ov < REGRID_DROP * cell] = 0.0
    r_lat = ov / ov.sum(axis=1, keepdims=True)
    lat = _band(r_lat, "latitude")
    # longitude: edges in units of 180 / (W_in W_out) degrees, output cell I = [(2I - 1) W_in, (2I + 1) W_in]
    i0 = np.arange(W_out, dtype=np.int64)
    lo, hi = (2 * i0 - 1) * W_in, (2 * i0 + 1) * W_in
    first = -((-(lo - W_out)) // (2 * W_out)) - 1                    # ceil((lo - W_out) / (2 W_out)) - 1: one cell of margin
    span = int((2 * W_in) // (2 * W_out)) + 4
    i = first[:, None] + np.arange(span, dtype=np.int64)[None, :]    # unwrapped input cells
    o = np.minimum(hi[:, None], (2 * i + 1) * W_out) - np.maximum(lo[:, None], (2 * i - 1) * W_out)
    wl = np.where(o > 0, o, 0).astype(np.float64) / (2.0 * W_in)
    wl[wl < REGRID_DROP] = 0.0
    start, count, w = _band(wl, "longitude")
    lon_start = (first + start).astype(np.int32)
    lon_start = np.where(lon_start >= W_in, lon_start - W_in, lon_start).astype(np.int32)
    r_lon = np.zeros((W_out, W_in), np.float64)
    for r in range(W_out):
        for t in range(count[r]):
            r_lon[r, (first[r] + start[r] + t) % W_in] += wl[r, start[r] + t]
    return RegridPlan(H_in, W_in, H_out, W_out, r_lat, r_lon, lat, (lon_start, count, w))


def _as_plan(plan, H_in, W_in, who):
    """A RegridPlan, or an (H_out, W_out) pair from which the plan for the grid (H_in, W_in) is built."""
    if not isinstance(plan, RegridPlan):
        try:
            H_out, W_out = (int(v) for v in plan)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: regrid is a score.RegridPlan or an (H_out, W_out) pair") from None
        key = (H_in, W_in, H_out, W_out)
        if key not in _PLANS:
            _PLANS[key] = regrid_plan(*key)
        plan = _PLANS[key]
    if plan.in_grid != (H_in, W_in):
        raise ValueError(f"{who}: the plan regrids {plan.in_grid} fields, got one on {(H_in, W_in)}")
    return plan


_PLANS = {}                           # (H_in, W_in, H_out, W_out) -> the plan built from an (H_out, W_out) pair


def _regrid_launch(stream, src_ptr, mul, add, dst_ptr, planes, plan, levels, device):
    """pangu_regrid_planes_f32 with the plan's device tables; mul / add device tensors or None."""
    ls, lc, lw, os_, oc, ow = plan._device_tables(device)
    _lib.check(_lib.load().pangu_regrid_planes_f32(
        stream, src_ptr, _ptr(mul), _ptr(add), dst_ptr, planes, plan.H_in, plan.W_in, plan.H_out, plan.W_out, ls.data_ptr(),
        lc.data_ptr(), lw.data_ptr(), plan.lat_taps, os_.data_ptr(), oc.data_ptr(), ow.data_ptr(), plan.lon_taps, levels),
        "regrid_planes_f32")


def regrid(x, plan, mul=None, add=None, flip_levels=False, out=None):
    """x (.., H_in, W_in), a contiguous fp32 CUDA tensor, remapped conservatively to (.., H_out, W_out) by `plan`
    (regrid_plan), one HIP launch on the current stream (pangu_regrid_planes_f32), no host sync.  mul / add: fp32 tensors with one
    value per plane of x, both or neither: the remap is taken of x * mul + add (two roundings).  flip_levels reverses dim -3 by
    addressing (mul / add stay indexed by the plane of x).  out: the fp32 result tensor to write.  Non-finite values propagate to
    every output cell they touch."""
    who = "regrid"
    if not isinstance(plan, RegridPlan):
        raise ValueError(f"{who}: plan must be a score.RegridPlan")
    if not (torch.is_tensor(x) and x.dim() >= 2 and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError(f"{who}: x must be a contiguous float32 tensor (.., H, W)")
    if not x.is_cuda:
        _no_cpu(who, x.device)
    if tuple(x.shape[-2:]) != plan.in_grid:
        raise ValueError(f"{who}: the plan regrids {plan.in_grid} fields, got one on {tuple(x.shape[-2:])}")
    planes = x.numel() // (plan.H_in * plan.W_in)
    if planes < 1:
        raise ValueError(f"{who}: empty tensor")
    if (mul is None) != (add is None):
        raise ValueError(f"{who}: give both mul and add or neither")
    if mul is not None:
        for name, t in (("mul", mul), ("add", add)):
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() == planes):
                raise ValueError(f"{who}: {name} must be a float32 tensor of {planes} values, one per plane")
        mul = mul.to(x.device).contiguous().view(-1)
        add = add.to(x.device).contiguous().view(-1)
    levels = 0
    if flip_levels:
        if x.dim() < 3:
            raise ValueError(f"{who}: flip_levels needs a level axis (dim -3)")
        levels = x.shape[-3]
    shape = tuple(x.shape[:-2]) + plan.out_grid
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif not (torch.is_tensor(out) and out.dtype == torch.float32 and out.is_contiguous() and out.device == x.device
              and tuple(out.shape) == shape):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor {shape} on {x.device}")
    _regrid_launch(_stream(x), x.data_ptr(), mul, add, out.data_ptr(), planes, plan, levels, x.device)
    return out


def plane_affine(t, stats_last, device):
    """(mul, add) per plane of a NORMALISED model output t, flat fp32 device tensors: t * mul + add is rollout.norm_back.  stats_last
    = (s_mean (1,4,1,1), s_std, u_mean (1,5,13,1,1), u_std); 5-D tensors take the upper-air pair, 4-D ones the surface pair."""
    if t.dim() not in (4, 5):
        raise ValueError("stats_last serves 5-D (B,5,13,H,W) and 4-D (B,4,H,W) tensors only")
    return _stats_affine(t, stats_last, t.dim() == 5, device)


def regrid_fields(upper, surface, plan, stats_last=None):
    """(upper, surface) on the plan's coarse grid: upper (B,5,13,H,W) and surface (B,4,H,W) through regrid(), two launches.  With
    stats_last (the 4-tuple of rollout.norm_back) the inputs are NORMALISED model outputs and the de-normalisation is folded into
    the pass.  plan: a RegridPlan or an (H_out, W_out) pair.  The results feed the scores as they are, e.g. WeatherBench-style
    1.5 degree scores of a forecast and of an ensemble:

        plan = score.regrid_plan(721, 1440, 121, 240)
        up, sf = score.regrid_fields(out_upper, out_surface, plan, stats_last)       # normalised model outputs
        tu, ts = score.regrid_fields(target_upper, target_surface, plan)             # physical targets
        rmse = score.weighted_rmse_channels(up, tu)                                  # (B, 5, 13)
        eu, es = score.regrid_fields(ens.upper, ens.surface, plan)                   # E members
        su, ss = score.ensemble_scores(eu, es, tu, ts, stats_last)
        qu, qs = score.ensemble_quantiles(eu, es, (0.1, 0.5, 0.9), tu, ts)"""
    if upper.dim() != 5 or surface.dim() != 4:
        raise ValueError("regrid_fields: expected upper (B,5,13,H,W) and surface (B,4,H,W)")
    if tuple(upper.shape[-2:]) != tuple(surface.shape[-2:]):
        raise ValueError("regrid_fields: upper and surface on different grids")
    plan = _as_plan(plan, upper.shape[-2], upper.shape[-1], "regrid_fields")
    return tuple(regrid(t, plan, *_stats_affine(t, stats_last, t is upper, t.device)) for t in (upper, surface))


# ---- regional scorecard of a deterministic forecast: bias, MAE, RMSE, ACC, activity per (plane, region) ---------------------------

SCORECARD_MAX_R = 8                   # csrc/scorecard.hip
SCORECARD_SUMS = 10

# name -> ((lat_south, lat_north), (lon_west, lon_east)) in degrees; latitude ends closed, longitude half-open and wrapping
REGION_PRESETS = {
    "global": ((-90.0, 90.0), (0.0, 360.0)),
    "nh_extratropics": ((20.0, 90.0), (0.0, 360.0)),
    "tropics": ((-20.0, 20.0), (0.0, 360.0)),
    "sh_extratropics": ((-90.0, -20.0), (0.0, 360.0)),
    "arctic": ((65.0, 90.0), (0.0, 360.0)),
    "antarctic": ((-90.0, -65.0), (0.0, 360.0)),
    "europe": ((35.0, 75.0), (-12.5, 42.5)),
    "north_america": ((25.0, 60.0), (-120.0, -75.0)),
    "north_atlantic": ((25.0, 65.0), (-70.0, -10.0)),
    "north_pacific": ((25.0, 60.0), (145.0, -130.0)),
    "east_asia": ((25.0, 60.0), (102.5, 150.0)),
    "ausnz": ((-45.0, -12.5), (120.0, 175.0)),
}

_REGION_PLANS = {}                    # (H, W, regions, device) -> RegionPlan, for region sets without a mask tensor


class RegionPlan:
    """The regions of one scorecard on one grid: `names` (a tuple), `bits` (the uint8 (H, W) device tensor that
    pangu_scorecard_sums_f32 reads: bit r of a point's byte says that the point lies in region r), R = len(names) and
    `everywhere` (the plan is one region of every point: the entry is then called without a mask)."""

    def __init__(self, names, bits, everywhere=False):
        self.names, self.bits = tuple(names), bits
        self.R = len(self.names)
        self.H, self.W = int(bits.shape[0]), int(bits.shape[1])
        self.everywhere = bool(everywhere) and self.R == 1      # one region of every point: the kernel needs no mask


def _box_limits(lat, lon, who):
    """(south, north, west, width) of a box in degrees: the width lon[1] - lon[0] taken into (0, 360], so that a box may cross the
    date line or the prime meridian."""
    try:
        (south, north), (west, east) = (float(v) for v in lat), (float(v) for v in lon)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: lat and lon are (lo, hi) pairs in degrees") from None
    if not south <= north:      # NaN included
        raise ValueError(f"{who}: lat_lo <= lat_hi, got ({south}, {north})")
    width = east - west
    if not abs(width) <= 360.0:      # NaN included
        raise ValueError(f"{who}: a longitude range spans at most 360 degrees, got ({west}, {east})")
    if width <= 0.0:
        width += 360.0
    return south, north, west, width


def _in_box(lat, lon, limits):
    """bool numpy, the broadcast of lat and lon (float64, degrees): lat in [south, north] and (lon - west) mod 360 below the width."""
    import numpy as np
    south, north, west, width = limits
    return ((lat >= south) & (lat <= north)) & (np.mod(lon - west, 360.0) < width)


def _region_box(H, W, lat, lon, who):
    """bool numpy (H, W): rows with lat[0] <= 90 - 180 j / (H - 1) <= lat[1], columns with (360 i / W - lon[0]) mod 360 below the
    box's width (lon[1] - lon[0] taken into (0, 360]: a box may cross the date line or the prime meridian)."""
    import numpy as np
    limits = _box_limits(lat, lon, who)
    rows = 90.0 - 180.0 * np.arange(H, dtype=np.float64) / float(max(H - 1, 1))
    cols = 360.0 * np.arange(W, dtype=np.float64) / float(W)
    return _in_box(rows[:, None], cols[None, :], limits)


def _region_specs(regions, H, W, who):
    """The regions of a region_bits mapping as a list of (name, lat, lon, mask), checked; None stands for {"global": "global"}."""
    regions = {"global": "global"} if regions is None else regions
    if not hasattr(regions, "items"):
        raise ValueError(f"{who}: regions is a mapping from a name to a preset name or a dict(lat=, lon=, mask=)")
    if not 1 <= len(regions) <= SCORECARD_MAX_R:
        raise ValueError(f"{who}: 1 <= R <= {SCORECARD_MAX_R} regions, got {len(regions)}")
    specs = []
    for name, spec in regions.items():
        if isinstance(spec, str):
            if spec not in REGION_PRESETS:
                raise ValueError(f"{who}: no preset region {spec!r}; presets: {', '.join(REGION_PRESETS)}")
            lat, lon = REGION_PRESETS[spec]
            mask = None
        elif isinstance(spec, dict):
            unknown = set(spec) - {"lat", "lon", "mask"}
            if unknown:
                raise ValueError(f"{who}: region {name!r} has unknown keys {sorted(unknown)}")
            lat, lon, mask = spec.get("lat", (-90.0, 90.0)), spec.get("lon", (0.0, 360.0)), spec.get("mask")
        else:
            raise ValueError(f"{who}: region {name!r} is a preset name or a dict(lat=, lon=, mask=)")
        if mask is not None and not (torch.is_tensor(mask) and mask.dtype == torch.bool and tuple(mask.shape) == (H, W)):
            raise ValueError(f"{who}: the mask of region {name!r} must be a bool tensor ({H}, {W})")
        specs.append((name, lat, lon, mask))
    return specs


def region_bits(H, W, regions=None, device=None):
    """The RegionPlan of up to 8 named regions on the grid (H, W): latitudes 90 - 180 j / (H - 1), longitudes 360 i / W.

    regions: an ordered mapping name -> a preset name (REGION_PRESETS) or dict(lat=(lo, hi), lon=(lo, hi), mask=None); None gives
    {"global": "global"}.  lat: both ends closed (default (-90, 90)); lon: half-open and wrapping, (lon - lo) mod 360 < hi - lo with
    the width taken into (0, 360] (default (0, 360): every column); mask: a bool (H, W) tensor that is ANDed in, e.g. land_mask >
    0.5.  Regions may overlap.  Plans without a mask tensor are cached per (H, W, regions, device)."""
    import numpy as np
    who = "region_bits"
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"{who}: a positive grid size, got ({H}, {W})")
    device = torch.device("cpu") if device is None else torch.device(device)
    specs = _region_specs(regions, H, W, who)
    key = []
    for name, lat, lon, mask in specs:
        if key is not None and mask is None:
            try:
                key.append((name, tuple(float(v) for v in lat), tuple(float(v) for v in lon)))
            except (TypeError, ValueError):
                key = None                    # _region_box says what is wrong
        else:
            key = None
    key = None if key is None else (H, W, tuple(key), str(device))
    if key is not None and key in _REGION_PLANS:
        return _REGION_PLANS[key]
    bits = np.zeros((H, W), np.uint8)
    for r, (name, lat, lon, mask) in enumerate(specs):
        inside = _region_box(H, W, lat, lon, f"{who}: region {name!r}")
        if mask is not None:
            inside = inside & mask.detach().cpu().numpy()
        bits |= (inside.astype(np.uint8) << r).astype(np.uint8)
    plan = RegionPlan([s[0] for s in specs], torch.from_numpy(bits).to(device).contiguous(), everywhere=bool((bits == 1).all()))
    if key is not None:
        _REGION_PLANS[key] = plan
    return plan


class ScoreSums:
    """The ten sums of pangu_scorecard_sums_f32 per (plane, region), of one deterministic_scores call or of a pool of `cases`
    of them (ScoreAccumulator): `sums` float64 (..., R, 10) on the device, the planes shaped (.., 5, 13) or (.., 4); `names` the
    regions.  With d = pred - target, a = pred - clim, b = target - clim and the latitude weight w, over a region's points:
      [0] sum w   [1] sum w d   [2] sum w |d|   [3] sum w d^2   [4] sum w a   [5] sum w b   [6] sum w a b   [7] sum w a^2
      [8] sum w b^2   [9] the number of points.
    The derived quantities are torch float64 ops on this small table, shaped (..., R), and work on any device.  They are
    normalised by the region's own sum of weights; for the global region that is H * W up to the rounding of the weights."""

    def __init__(self, sums, names, cases=1):
        self.sums, self.names, self.cases = sums, tuple(names), cases
        if sums.shape[-1] != SCORECARD_SUMS or sums.shape[-2] != len(self.names):
            raise ValueError("ScoreSums: sums must be (..., R, 10) with one name per region")

    def _s(self, k):
        return self.sums[..., k].double()

    @property
    def bias(self):
        return self._s(1) / self._s(0)

    @property
    def mae(self):
        return self._s(2) / self._s(0)

    @property
    def mse(self):
        return self._s(3) / self._s(0)

    @property
    def rmse(self):
        return torch.sqrt(self.mse)

    @property
    def acc(self):
        """Uncentred anomaly correlation, the reference's (era5_data/score.py:123-135) and WeatherBench 2's form."""
        return self._s(6) / torch.sqrt(self._s(7) * self._s(8))

    @property
    def acc_centred(self):
        """The anomaly correlation with the region's weighted mean anomalies removed from all three moments."""
        ma, mb = self._s(4) / self._s(0), self._s(5) / self._s(0)
        cov = self._s(6) / self._s(0) - ma * mb
        return cov / torch.sqrt((self._s(7) / self._s(0) - ma * ma) * (self._s(8) / self._s(0) - mb * mb))

    @property
    def activity_forecast(self):
        """Standard deviation of the forecast anomaly over the region: falls below activity_target where a forecast is blurred."""
        m = self._s(4) / self._s(0)
        return torch.sqrt(self._s(7) / self._s(0) - m * m)

    @property
    def activity_target(self):
        m = self._s(5) / self._s(0)
        return torch.sqrt(self._s(8) / self._s(0) - m * m)

    @property
    def counts(self):
        return self.sums[..., 9].to(torch.int64)

    def wind_rmse(self):
        """sqrt((sum w du^2 + sum w dv^2) / sum w): of variables 3 and 4 of an upper-air table (.., 5, 13, R, 10), per level
        (.., 13, R), or of variables 1 and 2 of a surface table (.., 4, R, 10), (.., R)."""
        s = self.sums
        if s.dim() >= 4 and tuple(s.shape[-4:-2]) == (5, 13):
            u, v = s[..., 3, :, :, :].double(), s[..., 4, :, :, :].double()
        elif s.dim() >= 3 and s.shape[-3] == 4:
            u, v = s[..., 1, :, :].double(), s[..., 2, :, :].double()
        else:
            raise ValueError("ScoreSums.wind_rmse: needs a table of planes (.., 5, 13) or (.., 4)")
        return torch.sqrt((u[..., 3] + v[..., 3]) / u[..., 0])

    def skill(self, reference):
        """1 - rmse / reference.rmse against the ScoreSums of a persistence or climatology forecast of the same targets."""
        if self.names != reference.names:
            raise ValueError(f"ScoreSums.skill: regions {self.names} against {reference.names}")
        return 1.0 - self.rmse / reference.rmse

    def region(self, name):
        """The table of one region, as a ScoreSums with R = 1."""
        if name not in self.names:
            raise KeyError(f"ScoreSums.region: no region {name!r} among {self.names}")
        i = self.names.index(name)
        return ScoreSums(self.sums[..., i:i + 1, :], (name,), self.cases)


def scorecard_workspace_bytes(planes, H, R):
    """Workspace of pangu_scorecard_sums_f32 (include/pangu_hip.h): per (plane, slab of 32 rows, region) ten 32-bit words."""
    return planes * ((H + 31) // 32) * R * SCORECARD_SUMS * 4


def _scorecard(pred, target, target_levels, clim, clim_kind, plan, what):
    """pangu_scorecard_sums_f32 over pred / target (cases.., *plane_shape, H, W); clim: None, a flat fp32 tensor with one value per
    plane of one case, or a field shaped like one case.  Returns the float64 (cases.., *plane_shape, R, 10) sums."""
    H, W = pred.shape[-2], pred.shape[-1]
    if target.shape != pred.shape:
        raise ValueError(f"{what}: the target is {tuple(target.shape)}, the forecast {tuple(pred.shape)}")
    if (plan.H, plan.W) != (H, W) or plan.bits.device != pred.device:
        raise ValueError(f"{what}: the region plan is for a {(plan.H, plan.W)} grid on {plan.bits.device}, the fields are "
                         f"{(H, W)} on {pred.device}")
    planes = pred.numel() // (H * W)
    R = plan.R
    stream = _stream(pred)
    p_ptr, t_ptr = _chk(pred, what), _chk(target, what + " target")
    dev = pred.device
    sums = torch.empty(tuple(pred.shape[:-2]) + (R, SCORECARD_SUMS), dtype=torch.float64, device=dev)
    w = _lat_weights(H, dev)
    lib = _lib.load()

    def launch(first, n, clim_ptr):
        ws = torch.empty(scorecard_workspace_bytes(n, H, R), dtype=torch.uint8, device=dev)
        _lib.check(lib.pangu_scorecard_sums_f32(
            stream, p_ptr + 4 * first * H * W, t_ptr + 4 * first * H * W, target_levels, clim_ptr, clim_kind, w.data_ptr(),
            None if plan.everywhere else plan.bits.data_ptr(), R, sums.data_ptr() + 8 * first * R * SCORECARD_SUMS, ws.data_ptr(), ws.numel(), n, H, W),
            "scorecard_sums_f32")

    if clim_kind == 0:
        launch(0, planes, None)
    elif clim_kind == 1:
        c = _per_plane(clim, pred, dev)      # named: it must outlive the launch's own allocation
        launch(0, planes, c.data_ptr())
    else:
        per_case = clim.numel() // (H * W)      # the field serves every case: one launch per case, none of them copies it
        c_ptr = _chk(clim, what + " climatology")
        for first in range(0, planes, per_case):
            launch(first, per_case, c_ptr)
    return sums


def deterministic_scores(upper, surface, target_upper, target_surface, regions=None, clim=None, target_levels_reversed=False):
    """The regional scorecard sums of forecasts upper (.., 5, 13, H, W) / surface (.., 4, H, W) against targets of the same shapes,
    all fp32 in physical units (what rollout() holds after a step); leading dimensions are separate cases.  One HIP pass per tensor
    (pangu_scorecard_sums_f32, definitions pinned in csrc/scorecard.hip), no host sync, bit-identical from run to run.

    regions: None (the global region), a mapping as for region_bits, or a RegionPlan.  clim: None (anomalies are the fields
    themselves), stats_last (s_mean, s_std, u_mean, u_std: the means serve as one climatological value per plane, as
    ensemble_scores uses them), or a pair (clim_upper, clim_surface) of fields shaped like one case (a day-of-year climatology;
    with several cases one launch per case).  target_levels_reversed: the upper-air target is stored with its level axis reversed.
    Returns (upper_sums, surface_sums), two ScoreSums with sums (.., 5, 13, R, 10) and (.., 4, R, 10)."""
    who = "deterministic_scores"
    H, W = _check_cases(who, upper, surface, targets=(target_upper, target_surface), w4=True)
    plan = regions if isinstance(regions, RegionPlan) else region_bits(H, W, regions, upper.device)
    cu = cs = None
    kind = 0
    if clim is not None:
        clim = tuple(clim)
        if len(clim) == 4:
            kind, cs, cu = 1, clim[0], clim[2]
            if cu.numel() != 65 or cs.numel() != 4:
                raise ValueError(f"{who}: stats_last means must hold 5 x 13 and 4 values")
        elif len(clim) == 2:
            kind, (cu, cs) = 2, clim
            if cu.numel() != 65 * H * W or cs.numel() != 4 * H * W:
                raise ValueError(f"{who}: climatology fields must be shaped like one case, (5, 13, H, W) and (4, H, W)")
        else:
            raise ValueError(f"{who}: clim is None, stats_last or a pair of fields")
    su = _scorecard(upper, target_upper.reshape(upper.shape), 13 if target_levels_reversed else 0, cu, kind, plan, "scorecard upper")
    ss = _scorecard(surface, target_surface.reshape(surface.shape), 0, cs, kind, plan, "scorecard surface")
    return ScoreSums(su, plan.names), ScoreSums(ss, plan.names)


SCORECARD_METRICS = ("bias", "mae", "rmse", "acc", "acc_centred", "activity_forecast", "activity_target")


class ScoreAccumulator(_LeadPool):
    """Pools ScoreSums over cases, per lead: the float64 sums are added on their device (no host sync), so pooled scores are the
    scores over all cases' points.  leads: the number of leads (0 .. leads-1); regions, clim and
    target_levels_reversed as for deterministic_scores, which score() calls.  The twin of ReliabilityAccumulator, and what
    rollout(scorecard=) feeds."""

    def __init__(self, leads, regions=None, clim=None, target_levels_reversed=False):
        super().__init__(leads)
        self.regions, self.clim, self.target_levels_reversed = regions, clim, bool(target_levels_reversed)
        self.names = None

    def score(self, lead, upper, surface, target_upper, target_surface):
        """deterministic_scores of these fields, pooled at `lead`; returns the two ScoreSums of this call."""
        self._check_lead(lead)
        plan = self._region_plan(self.regions, upper)
        su, ss = deterministic_scores(upper, surface, target_upper, target_surface, plan, self.clim, self.target_levels_reversed)
        self.add(lead, su, ss)
        return su, ss

    def add(self, lead, upper_sums, surface_sums):
        """Pools sums computed elsewhere; leading case dimensions are summed, each counting `cases` per entry."""
        self._check_lead(lead)
        for s in (upper_sums, surface_sums):
            if self.names is None:
                self.names = s.names
            if s.names != self.names:
                raise ValueError(f"ScoreAccumulator: sums of the regions {s.names} added to a pool of {self.names}")
        flat_u = upper_sums.sums.double().reshape((-1,) + tuple(upper_sums.sums.shape[-4:]))
        flat_s = surface_sums.sums.double().reshape((-1,) + tuple(surface_sums.sums.shape[-3:]))
        if flat_u.shape[0] != flat_s.shape[0]:
            raise ValueError("ScoreAccumulator: upper and surface sums of different numbers of cases")
        n = flat_u.shape[0] * upper_sums.cases
        if self._pool[lead] is None:
            self._pool[lead] = (ScoreSums(flat_u.sum(0), self.names, n), ScoreSums(flat_s.sum(0), self.names, n))
            return
        for pooled, flat in zip(self._pool[lead], (flat_u, flat_s)):
            pooled.sums.add_(flat.sum(0))
            pooled.cases += n

    def sums(self, lead):
        """(upper, surface) pooled ScoreSums of a lead, sums (5, 13, R, 10) and (4, R, 10)."""
        return self._pooled(lead)

    def table(self, lead, metrics=SCORECARD_METRICS):
        """The scorecard of a lead on the host: {"regions": names, "cases": n, metric: float64 numpy (69, R), ...}, the 65
        upper-air planes (variable-major) followed by the 4 surface planes.  One device-to-host copy: the only sync."""
        up, sf = self.sums(lead)
        rows = [torch.cat((getattr(up, m).reshape(65, -1), getattr(sf, m).reshape(4, -1))) for m in metrics]
        host = torch.stack(rows).cpu().numpy()
        out = {"regions": self.names, "cases": up.cases}
        out.update({m: host[i] for i, m in enumerate(metrics)})
        return out


# ---- event verification of deterministic forecasts: contingency scores and the Fractions Skill Score (csrc/events.hip)

EVENT_MAX_T = 4                       # csrc/events.hip
EVENT_MAX_N = 4
EVENT_MAX_RADIUS = 32
EVENT_MAX_W = 4096
EVENT_SLAB_ROWS = 32                  # EV_ROWS: the rows one workgroup owns


def event_scores_workspace_bytes(planes, H, T, N):
    """Workspace of pangu_event_scores_f32 (include/pangu_hip.h): per (plane, row) 1 + 3 T + 2 T N 64-bit integers."""
    return planes * H * (1 + 3 * T + 2 * T * N) * 8


def _ratio(num, den):
    """num / den in float64, NaN where den == 0."""
    num, den = num.double(), den.double()
    return torch.where(den == 0, torch.full_like(den, float("nan")), num / torch.where(den == 0, torch.ones_like(den), den))


def _check_radii(radii, W, who):
    try:
        radii = tuple(int(r) for r in radii)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: radii is a sequence of integers") from None
    if not 1 <= len(radii) <= EVENT_MAX_N:
        raise ValueError(f"{who}: 1 <= N <= {EVENT_MAX_N} radii, got {len(radii)}")
    for i, r in enumerate(radii):
        if not 0 <= r <= EVENT_MAX_RADIUS:
            raise ValueError(f"{who}: 0 <= radius <= {EVENT_MAX_RADIUS}, got {r}")
        if i and r <= radii[i - 1]:
            raise ValueError(f"{who}: radii must be strictly increasing, got {radii}")
        if W is not None and 2 * r + 1 > W:
            raise ValueError(f"{who}: the box of radius {r} is wider than the {W} columns")
    return radii


class EventScores:
    """The raw event sums of pangu_event_scores_f32 for T thresholds and N radii, of one event_scores call or of a pool of `cases`
    of them (EventAccumulator), the planes shaped (.., 5, 13) or (.., 4):
      counts    int64 (.., T, planes.., 4): hits, false alarms, misses, correct negatives over the domain's points;
      wsums     float64, the same four with every point weighted by its latitude weight;
      fss_sums  float64 (.., T, planes.., N, 2): numerator and denominator of the Fractions Skill Score per radius;
      radii     the N box radii in grid points.
    The derived scores are float64 torch ops on these small tables, on their device and without a sync; a score whose denominator
    is 0 is NaN."""

    def __init__(self, counts, wsums, fss_sums, radii, cases=1):
        self.counts, self.wsums, self.fss_sums, self.radii, self.cases = counts, wsums, fss_sums, tuple(int(r) for r in radii), cases
        if counts.shape[-1] != 4 or tuple(wsums.shape) != tuple(counts.shape):
            raise ValueError("EventScores: counts and wsums must be (..., 4) of one shape")
        if tuple(fss_sums.shape) != tuple(counts.shape[:-1]) + (len(self.radii), 2):
            raise ValueError("EventScores: fss_sums must be (..., N, 2) over the planes of counts, with one radius per N")

    def _w(self, k):
        return self.wsums[..., k].double()

    def pod(self):
        """Probability of detection (hit rate): hits / (hits + misses)."""
        return _ratio(self._w(0), self._w(0) + self._w(2))

    def far(self):
        """False alarm ratio: false alarms / (hits + false alarms)."""
        return _ratio(self._w(1), self._w(0) + self._w(1))

    def csi(self):
        """Critical success index (threat score): hits / (hits + false alarms + misses)."""
        return _ratio(self._w(0), self._w(0) + self._w(1) + self._w(2))

    def frequency_bias(self):
        """(hits + false alarms) / (hits + misses): forecast events per observed event."""
        return _ratio(self._w(0) + self._w(1), self._w(0) + self._w(2))

    def ets(self):
        """Equitable threat score: (hits - r) / (hits + false alarms + misses - r) with the hits of a random forecast of the same
        frequencies, r = (hits + false alarms)(hits + misses) / total."""
        a, b, c = self._w(0), self._w(1), self._w(2)
        n = a + b + c + self._w(3)
        r = _ratio((a + b) * (a + c), n)
        return _ratio(a - r, a + b + c - r)

    def base_rate(self):
        """The weighted observed frequency: (hits + misses) / total."""
        return _ratio(self._w(0) + self._w(2), self._w(0) + self._w(1) + self._w(2) + self._w(3))

    def fss(self):
        """The Fractions Skill Score 1 - num / den per radius, (.., T, planes.., N)."""
        return 1.0 - _ratio(self.fss_sums[..., 0], self.fss_sums[..., 1])

    def fss_useful(self):
        """0.5 + base_rate / 2: the FSS from which a forecast counts as useful (Roberts & Lean 2008)."""
        return 0.5 + 0.5 * self.base_rate()

    def useful_radius(self):
        """int64 (.., T, planes..): the smallest requested radius whose FSS reaches fss_useful, or -1 (none does, or NaN)."""
        ok = self.fss() >= self.fss_useful().unsqueeze(-1)
        r = torch.tensor(self.radii, dtype=torch.int64, device=ok.device)
        big = EVENT_MAX_RADIUS + 1
        first = torch.where(ok, r, torch.full_like(r, big)).amin(-1)
        return torch.where(first == big, torch.full_like(first, -1), first)


def _events(pred, target, target_levels, thr, T, radii, bits, bit, what):
    """pangu_event_scores_f32 over pred / target (cases.., *plane_shape, H, W), thr (T, *plane_shape).  Returns counts, wsums
    (cases.., T, *plane_shape, 4) and fss sums (cases.., T, *plane_shape, N, 2)."""
    import ctypes
    H, W = pred.shape[-2], pred.shape[-1]
    if target.shape != pred.shape:
        raise ValueError(f"{what}: the target is {tuple(target.shape)}, the forecast {tuple(pred.shape)}")
    nplane = len(thr.shape) - 1
    case_shape, plane_shape = tuple(pred.shape[:-2 - nplane]), tuple(pred.shape[-2 - nplane:-2])
    planes = pred.numel() // (H * W)
    stream = _stream(pred)
    p_ptr, t_ptr = _chk(pred, what), _chk(target, what + " target")
    dev = pred.device
    N = len(radii)
    thr = _per_plane_thresholds(thr, T, planes, dev)
    counts = torch.empty((T, planes, 4), dtype=torch.int64, device=dev)
    wsums = torch.empty((T, planes, 4), dtype=torch.float64, device=dev)
    fss = torch.empty((T, planes, N, 2), dtype=torch.float64, device=dev)
    ws = torch.empty(event_scores_workspace_bytes(planes, H, T, N), dtype=torch.uint8, device=dev)
    host_radii = (ctypes.c_int * N)(*radii)
    _lib.check(_lib.load().pangu_event_scores_f32(
        stream, p_ptr, t_ptr, target_levels, thr.data_ptr(), T, host_radii, N, _lat_weights(H, dev).data_ptr(), _ptr(bits), bit,
        counts.data_ptr(), wsums.data_ptr(), fss.data_ptr(), ws.data_ptr(), ws.numel(), planes, H, W), "event_scores_f32")
    nc = len(case_shape)
    shape = (T,) + case_shape + plane_shape
    return (counts.reshape(shape + (4,)).movedim(0, nc), wsums.reshape(shape + (4,)).movedim(0, nc),
            fss.reshape(shape + (N, 2)).movedim(0, nc))


def _event_domain(H, W, regions, region, device, who):
    """(bits, bit) of the one region to score: (None, 0) for the whole grid."""
    if regions is None:
        if region is not None:
            raise ValueError(f"{who}: region {region!r} named without regions")
        return None, 0
    plan = regions if isinstance(regions, RegionPlan) else region_bits(H, W, regions, device)
    if region is None or region not in plan.names:
        raise ValueError(f"{who}: region names the one region to score, one of {plan.names}; got {region!r}")
    if (plan.H, plan.W) != (H, W) or plan.bits.device != torch.device(device):
        raise ValueError(f"{who}: the region plan is for a {(plan.H, plan.W)} grid on {plan.bits.device}, the fields are "
                         f"{(H, W)} on {device}")
    if plan.everywhere:
        return None, 0
    return plan.bits, plan.names.index(region)


def event_scores(upper, surface, target_upper, target_surface, thresholds, radii=(0,), regions=None, region=None,
                 target_levels_reversed=False):
    """Event verification of forecasts upper (.., 5, 13, H, W) / surface (.., 4, H, W) against targets of the same shapes, all fp32
    in physical units; leading dimensions are separate cases.  The events are x > threshold for the pair `thresholds` (T, 5, 13) /
    (T, 4), T <= 4 (+inf: no event on that plane).  One HIP pass per tensor (pangu_event_scores_f32, definitions pinned in
    csrc/events.hip), no host sync, bit-identical from run to run.

    radii: up to 4 strictly increasing box radii in grid points, 0 <= r <= 32: the neighbourhoods of the Fractions Skill Score
    (radius 0 is the point-wise score).  regions / region: None scores the whole grid; else a mapping as for region_bits or a
    RegionPlan, and the name of the ONE region whose points are scored (every grid point still feeds the neighbourhoods).
    target_levels_reversed: the upper-air target is stored with its level axis reversed.
    Returns (upper_scores, surface_scores), two EventScores."""
    who = "event_scores"
    H, W = _check_cases(who, upper, surface, targets=(target_upper, target_surface), w4=True, max_w=EVENT_MAX_W)
    thr_u, thr_s, T = _check_thresholds(thresholds, who)
    if T == 0:
        raise ValueError(f"{who}: thresholds are required: a pair of tensors (T, 5, 13) and (T, 4)")
    radii = _check_radii(radii, W, who)
    bits, bit = _event_domain(H, W, regions, region, upper.device, who)
    cu, wu, fu = _events(upper, target_upper.reshape(upper.shape), 13 if target_levels_reversed else 0, thr_u, T, radii, bits, bit,
                         "events upper")
    cs, wsf, fs = _events(surface, target_surface.reshape(surface.shape), 0, thr_s, T, radii, bits, bit, "events surface")
    return EventScores(cu, wu, fu, radii), EventScores(cs, wsf, fs, radii)


EVENT_METRICS = ("pod", "far", "csi", "frequency_bias", "ets", "base_rate")


class EventAccumulator(_LeadPool):
    """Pools EventScores over cases, per lead: counts add in int64 and the weighted sums in float64 on their device (no host
    sync), so pooled scores are the scores over all cases' points and the pooled FSS is 1 - sum num / sum den.  leads: the number
    of leads (0 .. leads-1); thresholds, radii, regions, region and target_levels_reversed as for event_scores, which score()
    calls.  The twin of ScoreAccumulator, and what rollout(events=) feeds."""

    def __init__(self, leads, thresholds, radii, regions=None, region=None, target_levels_reversed=False):
        super().__init__(leads)
        _, _, T = _check_thresholds(thresholds, "EventAccumulator")
        if T == 0:
            raise ValueError("EventAccumulator: thresholds are required: a pair of tensors (T, 5, 13) and (T, 4)")
        self.thresholds, self.T = thresholds, T
        self.radii = _check_radii(radii, None, "EventAccumulator")
        if regions is None and region is not None:
            raise ValueError(f"EventAccumulator: region {region!r} named without regions")
        self.regions, self.region, self.target_levels_reversed = regions, region, bool(target_levels_reversed)

    def score(self, lead, upper, surface, target_upper, target_surface):
        """event_scores of these fields, pooled at `lead`; returns the two EventScores of this call."""
        self._check_lead(lead)
        plan = None if self.regions is None else self._region_plan(self.regions, upper)
        eu, es = event_scores(upper, surface, target_upper, target_surface, self.thresholds, self.radii, plan, self.region,
                              self.target_levels_reversed)
        self.add(lead, eu, es)
        return eu, es

    def add(self, lead, upper_scores, surface_scores):
        """Pools sums computed elsewhere; leading case dimensions are summed, each counting `cases` per entry."""
        self._check_lead(lead)
        N = len(self.radii)
        flat = []
        for e, pshape in ((upper_scores, (5, 13)), (surface_scores, (4,))):
            if e.radii != self.radii:
                raise ValueError(f"EventAccumulator: scores of the radii {e.radii} added to a pool of {self.radii}")
            tail = (self.T,) + pshape
            if tuple(e.counts.shape[-len(tail) - 1:-1]) != tail:
                raise ValueError(f"EventAccumulator: expected counts (.., {', '.join(map(str, tail))}, 4), got {tuple(e.counts.shape)}")
            flat.append((e.counts.to(torch.int64).reshape((-1,) + tail + (4,)), e.wsums.double().reshape((-1,) + tail + (4,)),
                         e.fss_sums.double().reshape((-1,) + tail + (N, 2))))
        if flat[0][0].shape[0] != flat[1][0].shape[0]:
            raise ValueError("EventAccumulator: upper and surface scores of different numbers of cases")
        n = flat[0][0].shape[0] * upper_scores.cases
        if self._pool[lead] is None:
            self._pool[lead] = tuple(EventScores(c.sum(0), w.sum(0), f.sum(0), self.radii, n) for c, w, f in flat)
            return
        for pooled, (c, w, f) in zip(self._pool[lead], flat):
            pooled.counts.add_(c.sum(0))
            pooled.wsums.add_(w.sum(0))
            pooled.fss_sums.add_(f.sum(0))
            pooled.cases += n

    def sums(self, lead):
        """(upper, surface) pooled EventScores of a lead, counts (T, 5, 13, 4) and (T, 4, 4)."""
        return self._pooled(lead)

    def table(self, lead, metrics=EVENT_METRICS):
        """The event scores of a lead on the host: {"cases": n, "radii": radii, metric: float64 numpy (T, 69), ..., "fss": (T, 69, N),
        "fss_useful": (T, 69), "useful_radius": int64 (T, 69)}, the 65 upper-air planes (variable-major) followed by the 4 surface
        planes.  One device-to-host copy: the only sync."""
        up, sf = self.sums(lead)
        T, N = self.T, len(self.radii)
        both = lambda f: torch.cat((f(up).reshape(T, 65, -1), f(sf).reshape(T, 4, -1)), 1).double()
        names = tuple(metrics) + ("fss_useful", "useful_radius")
        cols = [both(lambda e, m=m: getattr(e, m)()) for m in names] + [both(lambda e: e.fss())]
        host = torch.cat(cols, -1).cpu().numpy()
        out = {"cases": up.cases, "radii": self.radii}
        out.update({m: host[..., i] for i, m in enumerate(names)})
        out["useful_radius"] = out["useful_radius"].astype("int64")
        out["fss"] = host[..., len(names):]
        return out


# ---- statistics across the leads of a rollout: window means, extremes and their leads, exceedance counts, spell lengths ----------

LEAD_MAX_WINDOWS = 4
LEAD_MAX_LEADS = 255                  # csrc/leadstats.hip: the byte counters and when_* hold 0..255
LEAD_STATS = ("mean", "min", "max", "when_min", "when_max", "count", "longest_spell")


class LeadWindowResult:
    """The statistics of one complete lead window [a, b), every entry an (upper, surface) pair shaped like the submitted fields, or
    None where that statistic was not kept:
      window          (a, b), and n = b - a, the number of leads;
      sum, mean       fp32: the left-to-right fp32 sum in lead order, and sum / n;
      min, max        fp32 (a NaN at any lead gives NaN);
      when_min/_max   uint8: the absolute lead of the extreme (the earliest on a tie);
      count           uint8 (.., T, 5, 13, H, W) / (.., T, 4, H, W): the leads with x > threshold, T placed as in EventScores;
      longest_spell   uint8, the same shape: the longest run of consecutive such leads."""

    def __init__(self, window, **pairs):
        self.window = tuple(window)
        self.n = self.window[1] - self.window[0]
        for name in ("sum", "mean", "min", "max", "when_min", "when_max", "count", "longest_spell"):
            setattr(self, name, pairs.get(name))


def _lead_stats_launch(stream, src_ptr, mul, add, fields, thr, T, planes, plane_elems, levels, lead, first):
    """pangu_lead_stats_update_f32; fields: a dict of the kept device tensors among sum, min, max, when_min, when_max, count, run,
    longest; mul / add / thr device tensors or None."""
    f = lambda k: _ptr(fields.get(k))
    _lib.check(_lib.load().pangu_lead_stats_update_f32(
        stream, src_ptr, _ptr(mul), _ptr(add), f("sum"), f("min"), f("max"), f("when_min"), f("when_max"), _ptr(thr) if T else None, T,
        f("count"), f("run"), f("longest"), planes, plane_elems, levels, lead, 1 if first else 0), "lead_stats_update_f32")


class LeadWindowStats:
    """Statistics across the leads of a rollout, kept on the device: per window of leads the mean field, the minimum and maximum
    with the leads at which they occur, the number of leads above a threshold and the longest run of consecutive such leads.

        agg = LeadWindowStats(windows=[(0, 7), (0, 3), (3, 7)], stats=("mean", "max", "when_max", "count", "longest_spell"),
                              thresholds=(thr_upper (T,5,13), thr_surface (T,4)))
        for k in range(7): ...; agg.update(k, upper, surface)          # or rollout(..., lead_stats=agg)
        week = agg.result(0); week.mean, week.max, week.when_max, week.count, week.longest_spell

    windows          up to 4 half-open lead ranges [a, b), 0 <= a < b <= 255; they may overlap and need not start at 0.
    stats            a subset of mean, min, max, when_min, when_max, count, longest_spell; when_* keeps its extreme too.
    thresholds       for count / longest_spell (and only with one of them): the events x > threshold, a pair (T, 5, 13) / (T, 4) in
                     physical units in the model's level order, T <= 4, +inf: no event on that plane.
    stats_last       the 4-tuple of rollout.norm_back: the submitted fields are NORMALISED model outputs and are de-normalised by the
                     kernel (per stored plane, as data.HostDrain(stats_last=) does).  None: they are physical already.
    levels_reversed  the upper-air tensor is stored with ascending levels (an analysis read from disk); reversed by addressing.

    update(lead, upper, surface) takes upper (.., 5, 13, H, W) and surface (.., 4, H, W), contiguous fp32 device tensors; leading
    dimensions (ensemble members, cases) are simply more planes, with statistics of their own.  It issues one launch per tensor per
    window that holds `lead` (pangu_lead_stats_update_f32, definitions pinned in csrc/leadstats.hip) on the current stream, with no
    host sync; a lead in no window issues none.  Leads arrive in strictly increasing order and every lead of a window must arrive.

    Storage is allocated at the first update, per window and element: 4 B each for mean (its sum), min and max, 1 B each for
    when_min and when_max, and per threshold 1 B for count and 2 B for longest_spell (the current run and the longest).  bytes()
    gives the total.  It is what an ensemble pays: E = 50 members x (mean, min, max) x one window is 50 x 69 x 721 x 1440 x 12 B,
    about 43 GB -- keep per-member statistics of few windows, or reduce the members first.

    The results compose with what exists: deterministic_scores of two window means is the weekly-mean scorecard, ensemble_scores /
    ensemble_quantiles / ensemble_reliability(want_fields=True) of per-member results give the probabilistic products, and
    data.HostDrain ships products(w)."""

    def __init__(self, windows, stats=("mean",), thresholds=None, stats_last=None, levels_reversed=False):
        who = "LeadWindowStats"
        try:
            self.windows = tuple((int(a), int(b)) for a, b in windows)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: windows is a sequence of (first lead, end lead) pairs") from None
        if not 1 <= len(self.windows) <= LEAD_MAX_WINDOWS:
            raise ValueError(f"{who}: 1..{LEAD_MAX_WINDOWS} windows, got {len(self.windows)}")
        for a, b in self.windows:
            if not 0 <= a < b <= LEAD_MAX_LEADS:
                raise ValueError(f"{who}: a window [a, b) needs 0 <= a < b <= {LEAD_MAX_LEADS}, got ({a}, {b})")
        stats = (stats,) if isinstance(stats, str) else tuple(stats)
        for s in stats:
            if s not in LEAD_STATS:
                raise ValueError(f"{who}: unknown statistic {s!r}; the statistics are {LEAD_STATS}")
        if not stats:
            raise ValueError(f"{who}: no statistic requested")
        self.stats = tuple(s for s in LEAD_STATS if s in stats)
        thr_u, thr_s, T = _check_thresholds(thresholds, who)
        events = "count" in self.stats or "longest_spell" in self.stats
        if events and T == 0:
            raise ValueError(f"{who}: count and longest_spell need thresholds, a pair of tensors (T, 5, 13) and (T, 4)")
        if T and not events:
            raise ValueError(f"{who}: thresholds are used only by count and longest_spell")
        self.thresholds, self.T = ((thr_u, thr_s) if T else None), T
        self.stats_last, self.levels_reversed = stats_last, bool(levels_reversed)
        kept = []                                       # the kernel's fields, in its argument order
        if "mean" in self.stats:
            kept.append("sum")
        for ext in ("min", "max"):
            if ext in self.stats or "when_" + ext in self.stats:
                kept.append(ext)
        kept += [w for w in ("when_min", "when_max") if w in self.stats]
        if "count" in self.stats:
            kept.append("count")
        if "longest_spell" in self.stats:
            kept += ["run", "longest"]
        self._kept = tuple(kept)
        self._shapes = None                             # (upper shape, surface shape, device) of the first update
        self._acc = None                                # per window: (upper fields, surface fields), dicts of device tensors
        self._aux = None                                # per tensor: (mul, add, thr) device tensors or None
        self.reset()

    def reset(self):
        """Forget every lead (a new rollout); the accumulators stay allocated and need no clearing."""
        self._last = -1
        self._seen = [0] * len(self.windows)

    def _check_window(self, w):
        if not 0 <= w < len(self.windows):
            raise IndexError(f"window {w} outside 0..{len(self.windows) - 1}")

    def complete(self, w):
        """True once every lead of window w has arrived."""
        self._check_window(w)
        a, b = self.windows[w]
        return self._seen[w] == b - a

    def bytes(self):
        """The accumulators' footprint on the device (0 before the first update)."""
        if self._acc is None:
            return 0
        return sum(t.numel() * t.element_size() for pair in self._acc for fields in pair for t in fields.values())

    def _field_shape(self, key, shape):
        return ((self.T,) if key in ("count", "run", "longest") else ()) + tuple(shape)

    def _allocate(self, upper, surface):
        dev = upper.device
        self._aux = []
        for t, thr in zip((upper, surface), self.thresholds if self.T else (None, None)):
            if thr is not None:
                thr = _per_plane_thresholds(thr, self.T, t.numel() // (t.shape[-1] * t.shape[-2]), dev)
            self._aux.append(_stats_affine(t, self.stats_last, t is upper, dev) + (thr,))
        dtype = lambda k: torch.float32 if k in ("sum", "min", "max") else torch.uint8
        self._acc = [tuple({k: torch.empty(self._field_shape(k, t.shape), dtype=dtype(k), device=dev) for k in self._kept}
                           for t in (upper, surface)) for _ in self.windows]

    def update(self, lead, upper, surface):
        """Fold the fields of `lead` into every window that holds it."""
        lead = int(lead)
        shapes = self._check_update(lead, upper, surface)
        self._fold(lead, upper, surface)
        self._shapes = shapes
        for w, (a, b) in enumerate(self.windows):
            if a <= lead < b:
                self._seen[w] += 1
        self._last = lead

    def _check_update(self, lead, upper, surface):
        """Everything update() refuses before a device call; returns (upper shape, surface shape, device)."""
        who = "LeadWindowStats.update"
        if not 0 <= lead < LEAD_MAX_LEADS:
            raise IndexError(f"{who}: lead {lead} outside 0..{LEAD_MAX_LEADS - 1}")
        if lead <= self._last:
            raise ValueError(f"{who}: leads must arrive in strictly increasing order, got {lead} after {self._last}")
        for (a, b), seen in zip(self.windows, self._seen):
            if seen < b - a and lead >= a and lead != a + seen:
                raise ValueError(f"{who}: window ({a}, {b}) expects lead {a + seen} next, got {lead}: every lead of a window must arrive")
        _check_cases(who, upper, surface, dense=True)
        shapes = (tuple(upper.shape), tuple(surface.shape), upper.device)
        if self._shapes is not None and shapes != self._shapes:
            raise ValueError(f"{who}: shapes and device must stay those of the first update, {self._shapes}; got {shapes}")
        return shapes

    def _fold(self, lead, upper, surface):
        """The device side of update(): the accumulators (at the first call) and one launch per tensor and window that holds lead."""
        if not upper.is_cuda:
            _no_cpu("LeadWindowStats.update", upper.device)
        stream = _stream(upper)
        if self._acc is None:
            self._allocate(upper, surface)
        elems = upper.shape[-1] * upper.shape[-2]
        for w, (a, b) in enumerate(self.windows):
            if not a <= lead < b:
                continue
            for t, fields, (mul, add, thr), levels in zip((upper, surface), self._acc[w], self._aux,
                                                          (13 if self.levels_reversed else 0, 0)):
                _lead_stats_launch(stream, t.data_ptr(), mul, add, fields, thr, self.T, t.numel() // elems, elems, levels, lead,
                                   lead == a)

    def _stat_pair(self, w, stat):
        key = {"mean": "sum", "longest_spell": "longest"}.get(stat, stat)
        pair = tuple(fields[key] for fields in self._acc[w])
        if stat == "mean":
            n = self.windows[w][1] - self.windows[w][0]
            return tuple(t / float(n) for t in pair)
        if stat in ("count", "longest_spell"):          # (T, cases.., planes.., H, W) -> T behind the cases, as in EventScores
            return tuple(t.movedim(0, t.dim() - 1 - nplane - 2) for t, nplane in zip(pair, (2, 1)))
        return pair

    def result(self, w):
        """The LeadWindowResult of window w, once it is complete.  The tensors are the live accumulators (or views of them): clone
        what must outlive the next reset() and update()."""
        if not self.complete(w):
            a, b = self.windows[w]
            raise ValueError(f"LeadWindowStats: window ({a}, {b}) is incomplete: {self._seen[w]} of {b - a} leads have arrived")
        pairs = {s: self._stat_pair(w, s) for s in self.stats}
        for ext in ("min", "max"):
            if ext in self._kept:
                pairs[ext] = self._stat_pair(w, ext)
        if "sum" in self._kept:
            pairs["sum"] = self._stat_pair(w, "sum")
        return LeadWindowResult(self.windows[w], **pairs)

    def product_names(self, w):
        """The names of the tensors products(w) returns, in its order: <statistic>_upper, <statistic>_surface per statistic."""
        self._check_window(w)
        return [f"{s}_{part}" for s in self.stats for part in ("upper", "surface")]

    def products(self, w):
        """The statistics of the complete window w as an ordered list of contiguous fp32 tensors (the byte fields converted), in the
        order of `stats`: what a data.HostDrain built without stats_last accepts; product_names(w) names the entries."""
        r = self.result(w)
        return [t.to(torch.float32).contiguous() for s in self.stats for t in getattr(r, s)]


# ---- verification against point observations, and forecasts at sites: the observation operator (csrc/points.hip) ------------------

POINT_CHUNK = 1024                    # csrc/points.hip PT_CHUNK: the points of one workspace partial


class PointPlan:
    """N points on the grid (H, W) as pangu_sample_points_f32 reads them, in the caller's order: `row`, `col` (int32 (N,)) the grid
    node north-west of a point, `wy`, `wx` (fp32 (N,)) the weights of the next row and the next column (columns wrap), `bits` (uint8
    (N,): bit r says that the point lies in region r); `names`, R = len(names), and `everywhere` (one region that holds every point:
    the scores entry is then called without region bits).  0 <= wy, wx < 1 always, and wy == 0 where row == H - 1."""

    def __init__(self, H, W, row, col, wy, wx, bits, names, everywhere=False):
        self.H, self.W, self.N = int(H), int(W), int(row.shape[0])
        self.row, self.col, self.wy, self.wx, self.bits = row, col, wy, wx, bits
        self.names = tuple(names)
        self.R = len(self.names)
        self.everywhere = bool(everywhere) and self.R == 1

    @property
    def device(self):
        return self.row.device


def _point_cells(H, W, lat, lon):
    """row, col (int64) and wy, wx (fp32) of point_plan for float64 coordinate arrays that passed its checks."""
    import numpy as np
    y = (90.0 - lat) * (H - 1) / 180.0
    row = np.minimum(np.floor(y), H - 1)
    wy = (y - row).astype(np.float32)
    x = np.mod(lon, 360.0) * W / 360.0
    col = np.floor(x)
    wx = (x - col).astype(np.float32)
    row, col = row.astype(np.int64), col.astype(np.int64)
    over = col >= W                                    # (lon mod 360) rounded up to 360: the first column
    col[over], wx[over] = 0, 0.0
    up = wy == np.float32(1.0)                         # a weight that rounds up to 1 in fp32: the next node, weight 0
    row[up] += 1
    wy[up] = 0.0
    up = wx == np.float32(1.0)
    col[up] = (col[up] + 1) % W
    wx[up] = 0.0
    return row, col, wy, wx


def point_plan(H, W, lat, lon, regions=None, device=None):
    """The PointPlan of the points (lat[i], lon[i]) in degrees on the grid (H, W): latitudes 90 - 180 j / (H - 1), longitudes
    360 i / W.  In float64, y = (90 - lat)(H - 1) / 180, row = min(floor(y), H - 1), wy = y - row; x = (lon mod 360) W / 360, col =
    floor(x), wx = x - col; the weights are then rounded to fp32.  A col that reaches W becomes column 0 with wx = 0, and a weight
    that rounds up to 1.0 moves the point to the next node with weight 0 (the column wrapping), so that the kernel never sees a
    weight of 1.  Longitudes may be any finite value; lat outside [-90, 90], a non-finite coordinate, no point at all or lat and lon
    of different lengths raise ValueError.

    regions: a mapping as for region_bits (at most 8), evaluated at the points' own coordinates: lat in [lo, hi], (lon - lo) mod 360
    below the width; a `mask` (bool (H, W)) is read at the grid node nearest to the point, row + (wy >= 0.5) and (col + (wx >= 0.5))
    mod W.  None: one region that holds every point."""
    import numpy as np
    who = "point_plan"
    H, W = int(H), int(W)
    if H < 2 or W < 1:
        raise ValueError(f"{who}: a grid of at least 2 rows and 1 column, got ({H}, {W})")
    if H * W >= 2 ** 31:
        raise ValueError(f"{who}: H * W must stay below 2^31")
    as_array = lambda v: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(np.float64)
    try:
        lat, lon = as_array(lat), as_array(lon)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: lat and lon are sequences of numbers in degrees") from None
    if lat.ndim != 1 or lon.ndim != 1 or lat.shape != lon.shape:
        raise ValueError(f"{who}: lat and lon must be one-dimensional and of one length, got {lat.shape} and {lon.shape}")
    if lat.size == 0:
        raise ValueError(f"{who}: no points")
    if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
        raise ValueError(f"{who}: coordinates must be finite")
    if not ((lat >= -90.0) & (lat <= 90.0)).all():
        raise ValueError(f"{who}: latitudes must lie in [-90, 90]")
    device = torch.device("cpu") if device is None else torch.device(device)
    row, col, wy, wx = _point_cells(H, W, lat, lon)
    specs = _region_specs(regions, H, W, who)
    bits = np.zeros(lat.size, np.uint8)
    near_row, near_col = row + (wy >= np.float32(0.5)), (col + (wx >= np.float32(0.5))) % W
    for r, (name, blat, blon, mask) in enumerate(specs):
        inside = _in_box(lat, lon, _box_limits(blat, blon, f"{who}: region {name!r}"))
        if mask is not None:
            inside = inside & mask.detach().cpu().numpy()[near_row, near_col]
        bits |= (inside.astype(np.uint8) << r).astype(np.uint8)
    up = lambda a, dtype: torch.from_numpy(np.ascontiguousarray(a.astype(dtype))).to(device)
    return PointPlan(H, W, up(row, np.int32), up(col, np.int32), up(wy, np.float32), up(wx, np.float32), up(bits, np.uint8),
                     [s[0] for s in specs], everywhere=bool((bits == 1).all()))


def _check_point_fields(upper, surface, plan, who):
    if not isinstance(plan, PointPlan):
        raise ValueError(f"{who}: plan must be a score.PointPlan")
    _check_cases(who, upper, surface, dense=True)
    if tuple(upper.shape[-2:]) != (plan.H, plan.W) or plan.device != upper.device:
        raise ValueError(f"{who}: the point plan is for a {(plan.H, plan.W)} grid on {plan.device}, the fields are "
                         f"{tuple(upper.shape[-2:])} on {upper.device}")
    if not upper.is_cuda:
        _no_cpu(who, upper.device)


def _sample_launch(t, plan, mul, add, levels, out):
    planes = t.numel() // (plan.H * plan.W)
    _lib.check(_lib.load().pangu_sample_points_f32(
        _stream(t), t.data_ptr(), _ptr(mul), _ptr(add), plan.row.data_ptr(), plan.col.data_ptr(), plan.wy.data_ptr(),
        plan.wx.data_ptr(), out.data_ptr(), planes, plan.H, plan.W, plan.N, levels), "sample_points_f32")
    return out


def sample_points(upper, surface, plan, stats_last=None, levels_reversed=False, out=None):
    """upper (.., 5, 13, H, W) / surface (.., 4, H, W), contiguous fp32 device tensors, interpolated bilinearly to the plan's N points:
    (upper (.., 5, 13, N), surface (.., 4, N)), one HIP launch per tensor on the current stream (pangu_sample_points_f32, the
    arithmetic pinned in csrc/points.hip), no host sync.  Leading dimensions (ensemble members, cases) are simply more planes.
    stats_last: the 4-tuple of rollout.norm_back: the fields are NORMALISED model outputs and are de-normalised by the kernel (per
    stored plane).  levels_reversed: the upper-air tensor is stored with its level axis reversed; reversed by addressing.  out: a pair
    of contiguous fp32 tensors of the result's shapes to write.  A NaN at a grid node reaches the points that use the node."""
    who = "sample_points"
    _check_point_fields(upper, surface, plan, who)
    res = []
    for k, (t, levels) in enumerate(((upper, 13 if levels_reversed else 0), (surface, 0))):
        mul, add = _stats_affine(t, stats_last, k == 0, t.device)
        shape = tuple(t.shape[:-2]) + (plan.N,)
        if out is None:
            o = torch.empty(shape, dtype=torch.float32, device=t.device)
        else:
            o = out[k]
            if not (torch.is_tensor(o) and o.dtype == torch.float32 and o.is_contiguous() and o.device == t.device
                    and tuple(o.shape) == shape):
                raise ValueError(f"{who}: out[{k}] must be a contiguous float32 tensor {shape} on {t.device}")
        res.append(_sample_launch(t, plan, mul, add, levels, o))
    return tuple(res)


def point_scores_workspace_bytes(planes, N, R):
    """Workspace of pangu_point_scores_f32 (include/pangu_hip.h): per (plane, chunk of 1024 points, region) ten 32-bit words."""
    return planes * ((N + POINT_CHUNK - 1) // POINT_CHUNK) * R * SCORECARD_SUMS * 4


def _point_scores(t, obs, clim, plan, want_departures, what):
    planes = t.numel() // (plan.H * plan.W)
    shape = tuple(t.shape[:-2]) + (plan.N,)
    if not torch.is_tensor(obs) or tuple(obs.shape) != shape:
        raise ValueError(f"{what}: the observations must be {shape}, one value per plane and point (NaN: no report)")
    o_ptr = _chk(obs, what + " observations")
    dev = t.device
    sums = torch.empty(tuple(t.shape[:-2]) + (plan.R, SCORECARD_SUMS), dtype=torch.float64, device=dev)
    dep = torch.empty(shape, dtype=torch.float32, device=dev) if want_departures else None
    ws = torch.empty(point_scores_workspace_bytes(planes, plan.N, plan.R), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().pangu_point_scores_f32(
        _stream(t), t.data_ptr(), None, None, plan.row.data_ptr(), plan.col.data_ptr(), plan.wy.data_ptr(), plan.wx.data_ptr(),
        o_ptr, _ptr(clim), None if plan.everywhere else plan.bits.data_ptr(), plan.R, _ptr(dep), sums.data_ptr(), ws.data_ptr(),
        ws.numel(), planes, plan.H, plan.W, plan.N, 0), "point_scores_f32")
    return sums, dep


def observation_scores(upper, surface, obs_upper, obs_surface, plan, clim=None, want_departures=False):
    """The departure statistics of forecasts upper (.., 5, 13, H, W) / surface (.., 4, H, W), fp32 in physical units, against
    observations obs_upper (.., 5, 13, N) / obs_surface (.., 4, N) at the plan's N points, NaN where there is no report; leading
    dimensions are separate cases.  The forecast is interpolated bilinearly to the points and compared there, two HIP launches per
    tensor (pangu_point_scores_f32, definitions pinned in csrc/points.hip), no host sync, bit-identical from run to run.

    clim: None (anomalies are the values themselves) or stats_last (s_mean, s_std, u_mean, u_std: the means serve as one
    climatological value per plane, as in deterministic_scores).  Returns (upper_sums, surface_sums), two ScoreSums with sums
    (.., 5, 13, R, 10) and (.., 4, R, 10) over the plan's regions, every valid point with weight 1: bias, mae, rmse, acc and the
    others are those of the reports, `counts` their number (a plane and region without a report gives NaN scores).  wind_rmse() is
    meaningful where u and v are reported together: it divides the two sums of squares by the number of u reports.  With
    want_departures=True the departures forecast - observation follow, (.., 5, 13, N) and (.., 4, N), NaN where there is no report."""
    who = "observation_scores"
    _check_point_fields(upper, surface, plan, who)
    cu = cs = None
    if clim is not None:
        clim = tuple(clim)
        if len(clim) != 4 or clim[2].numel() != 65 or clim[0].numel() != 4:
            raise ValueError(f"{who}: clim is None or stats_last, whose means hold 5 x 13 and 4 values")
        cu, cs = _per_plane(clim[2], upper, upper.device), _per_plane(clim[0], surface, upper.device)
    su, du = _point_scores(upper, obs_upper, cu, plan, want_departures, who + ": upper")
    ss, ds = _point_scores(surface, obs_surface, cs, plan, want_departures, who + ": surface")
    res = (ScoreSums(su, plan.names), ScoreSums(ss, plan.names))
    return res + (du, ds) if want_departures else res


class ObservationAccumulator:
    """Pools observation_scores over cases, per lead: the float64 sums are added on their device (no host sync), so pooled scores
    are the scores over all cases' reports.  leads: the number of leads (0 .. leads-1); plan and clim as for observation_scores,
    which score() calls.  The twin of ScoreAccumulator for point observations, and what rollout(observations=) feeds."""

    def __init__(self, leads, plan, clim=None):
        if not isinstance(plan, PointPlan):
            raise ValueError("ObservationAccumulator: plan must be a score.PointPlan")
        try:
            self._pool = ScoreAccumulator(leads)
        except ValueError:
            raise ValueError("ObservationAccumulator: leads must be >= 1") from None
        self.leads, self.plan, self.clim = self._pool.leads, plan, clim

    def score(self, lead, upper, surface, obs_upper, obs_surface):
        """observation_scores of these fields and reports, pooled at `lead`; returns the two ScoreSums of this call."""
        self.cases(lead)                                # refuses a lead outside the pool before any launch
        su, ss = observation_scores(upper, surface, obs_upper, obs_surface, self.plan, self.clim)
        self._pool.add(lead, su, ss)
        return su, ss

    def cases(self, lead):
        return self._pool.cases(lead)

    def result(self, lead):
        """(upper, surface) pooled ScoreSums of a lead, sums (5, 13, R, 10) and (4, R, 10)."""
        if self.cases(lead) == 0:
            raise ValueError(f"ObservationAccumulator: nothing scored at lead {lead}")
        return self._pool.sums(lead)


class PointSeries:
    """The forecast at the plan's N sites for every lead of a rollout (a meteogram): `upper` (leads, .., 5, 13, N) and `surface`
    (leads, .., 4, N), fp32 on the device, allocated at the first record(); a lead that was not recorded holds NaN.
    record(lead, upper, surface) samples physical-unit fields (sample_points: one launch per tensor, no host sync) into row `lead`;
    rollout(sites=) calls it behind every step."""

    def __init__(self, plan, leads):
        if not isinstance(plan, PointPlan):
            raise ValueError("PointSeries: plan must be a score.PointPlan")
        self.plan, self.leads = plan, int(leads)
        if self.leads < 1:
            raise ValueError("PointSeries: leads must be >= 1")
        self.upper = self.surface = None

    def record(self, lead, upper, surface):
        lead = int(lead)
        if not 0 <= lead < self.leads:
            raise IndexError(f"PointSeries.record: lead {lead} outside 0..{self.leads - 1}")
        _check_point_fields(upper, surface, self.plan, "PointSeries.record")
        shapes = tuple((self.leads,) + tuple(t.shape[:-2]) + (self.plan.N,) for t in (upper, surface))
        if self.upper is None:
            self.upper, self.surface = (torch.full(s, float("nan"), dtype=torch.float32, device=upper.device) for s in shapes)
        elif (tuple(self.upper.shape), tuple(self.surface.shape)) != shapes:
            raise ValueError(f"PointSeries.record: shapes must stay those of the first record, {tuple(self.upper.shape[1:])} and "
                             f"{tuple(self.surface.shape[1:])} per lead")
        sample_points(upper, surface, self.plan, out=(self.upper[lead], self.surface[lead]))

    def _wind10(self):
        if self.surface is None:
            raise ValueError("PointSeries: nothing recorded")
        return self.surface[..., 1, :], self.surface[..., 2, :]

    def wind_speed10(self):
        """sqrt(u10^2 + v10^2) of the sampled components (surface variables 1 and 2), (leads, .., N)."""
        u, v = self._wind10()
        return torch.sqrt(u * u + v * v)

    def wind_direction10(self):
        """The meteorological direction in degrees in [0, 360), the direction the wind blows FROM, clockwise from north: 0 for a
        northerly (v10 < 0), 90 for an easterly (u10 < 0); 0 where the wind is calm (u10 = v10 = 0).  (leads, .., N)."""
        u, v = self._wind10()
        d = torch.remainder(torch.rad2deg(torch.atan2(-u, -v)), 360.0)
        d = torch.where(d >= 360.0, torch.zeros_like(d), d)
        return torch.where((u == 0) & (v == 0), torch.zeros_like(d), d)
