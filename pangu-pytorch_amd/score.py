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
    w = latitude_weights(H, x.device)
    ptr = lambda t: t.data_ptr() if t is not None else None
    _lib.check(_lib.load().pangu_ensemble_stats_f32(
        _stream(x), x.data_ptr(), x[0].numel(), E, ptr(target), ptr(clim), w.data_ptr(), out.data_ptr(), ptr(mean), ptr(std),
        ws.data_ptr(), ws.numel() * 4, planes, H, W), "ensemble_stats_f32")
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
    E = upper.shape[0]
    if upper.dim() != 5 or surface.dim() != 4 or surface.shape[0] != E:
        raise ValueError("ensemble_scores: expected upper (E,5,13,H,W) and surface (E,4,H,W)")
    if not 2 <= E <= 128:
        raise ValueError(f"ensemble_scores: 2 <= E <= 128 members, got {E}")
    if upper.shape[-1] % 4:
        raise ValueError("ensemble_scores: W % 4 != 0")
    if (target_upper is None) != (target_surface is None):
        raise ValueError("ensemble_scores: give both targets or neither")
    s_mean, _, u_mean, _ = stats_last
    clim = lambda t: t.to(device=upper.device, dtype=torch.float32).reshape(-1).contiguous()
    su, mu, sdu = _ens_stats(upper, target_upper, clim(u_mean), want_fields, "ensemble upper")
    ss, ms, sds = _ens_stats(surface, target_surface, clim(s_mean), want_fields, "ensemble surface")
    if want_fields:
        su.update(mean=mu, std=sdu)
        ss.update(mean=ms, std=sds)
    return su, ss
