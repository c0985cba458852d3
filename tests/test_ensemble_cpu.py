"""CPU-side checks of the ensemble surface: C-entry argument validation, Python refusals, and a float64 numpy restatement of
the perturbation noise (csrc/ensemble.hip pins the definition; tests/test_gpu_ensemble.py checks the kernel against this)."""
import os

import numpy as np
import pytest
import torch

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib


def lowbias32(x):
    x = np.array(x, dtype=np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def fade(t):
    return t * t * t * (t * (t * 6.0 - 15.0) + 10.0)


def lerp(a, b, t):
    return a + t * (b - a)


def noise_ref(seed, m, plane, rows, cols, W, octaves=3, period=12, persistence=0.5):
    """The noise of global member m on plane `plane` at rows x cols (any integers >= 0; cols may pass W), float64:
    sum_o persistence^o * Perlin_o with L = period * 2^o lattice cells around the longitude circle, cell width s = W / L,
    ix = w // s, fx = (w - ix s) / s (same for h), corner gradient (cos t, sin t), t = 2 pi h32 2^-32,
    h32 = lowbias32 chain over (seed, m, plane, o, j L + (i mod L)), fade t^3 (t (6t - 15) + 10), bilinear blend."""
    h = np.asarray(rows, dtype=np.int64)[:, None]
    w = np.asarray(cols, dtype=np.int64)[None, :]
    base = lowbias32(lowbias32(lowbias32(seed) ^ np.uint32(m)) ^ np.uint32(plane))
    total = np.zeros((h.shape[0], w.shape[1]))
    for o in range(octaves):
        L = period << o
        assert W % L == 0
        s = W // L
        ix, iy = w // s, h // s
        fx, fy = (w - ix * s) / s, (h - iy * s) / s
        ho = lowbias32(base ^ np.uint32(o))

        def dot(j, i, dx, dy):
            t = lowbias32(ho ^ (j * L + i % L).astype(np.uint32)).astype(np.float64) * 2.0 ** -32 * 2.0 * np.pi
            return np.cos(t) * dx + np.sin(t) * dy

        d00, d01 = dot(iy, ix, fx, fy), dot(iy, ix + 1, fx - 1.0, fy)
        d10, d11 = dot(iy + 1, ix, fx, fy - 1.0), dot(iy + 1, ix + 1, fx - 1.0, fy - 1.0)
        u, v = fade(fx), fade(fy)
        total += persistence ** o * lerp(lerp(d00, d01, u), lerp(d10, d11, u), v)
    return total


def perturb_ref(upper, surface, u_std, s_std, amplitude, seed, octaves=3, period=12, persistence=0.5, first_member=0,
                control=True, planes=None):
    """float64 restatement of ensemble.perturb_ on numpy arrays upper (E,5,13,H,W), surface (E,4,H,W) (copies); `planes`
    limits the planes computed (the rest are left as they are)."""
    up, sf = upper.astype(np.float64).copy(), surface.astype(np.float64).copy()
    E, H, W = up.shape[0], up.shape[-2], up.shape[-1]
    amp = np.broadcast_to(np.asarray(amplitude, dtype=np.float64), (9,))
    std = np.concatenate([np.asarray(u_std, np.float64).reshape(-1), np.asarray(s_std, np.float64).reshape(-1)])
    for e in range(E):
        m = first_member + e
        if control and m == 0:
            continue
        for p in (range(69) if planes is None else planes):
            var = p // 13 if p < 65 else 5 + p - 65
            n = amp[var] * std[p] * noise_ref(seed, m, p, np.arange(H), np.arange(W), W, octaves, period, persistence)
            if p < 65:
                up[e, p // 13, p % 13] += n
            else:
                sf[e, p - 65] += n
    return up, sf


def test_lowbias32_chain_is_uint32():
    assert int(lowbias32(0)) == 0
    assert lowbias32([1, 2**32 - 1]).dtype == np.uint32
    assert int(lowbias32(1)) != int(lowbias32(2))


def test_noise_is_periodic_in_longitude():
    """The lattice wraps at the dateline: noise(w = W) == noise(w = 0), and the step across the dateline is no larger than
    the steps between neighbours elsewhere (no seam)."""
    W, H = 96, 37
    for m, plane, oct_, per in ((1, 0, 3, 12), (7, 66, 2, 6), (3, 40, 1, 4)):
        n = noise_ref(11, m, plane, np.arange(H), np.arange(W + 1), W, oct_, per)
        assert np.allclose(n[:, W], n[:, 0], rtol=0, atol=1e-12)
        inner = np.abs(np.diff(n[:, :W], axis=1)).max()
        assert np.abs(n[:, W - 1] - n[:, 0]).max() <= inner + 1e-12
        assert np.abs(n).max() > 1e-2           # not trivially zero


def test_noise_vanishes_on_coarsest_lattice_nodes_of_one_octave():
    W, L = 96, 12
    s = W // L
    n = noise_ref(5, 2, 3, np.arange(0, 37, s), np.arange(0, W, s), W, octaves=1, period=L)
    assert np.abs(n).max() < 1e-12


def test_noise_independent_of_chunking():
    """A member's perturbation depends on its global index only: made alone or inside a batch at any offset, it is the same."""
    rng = np.random.default_rng(0)
    H, W = 13, 48
    up = rng.standard_normal((1, 5, 13, H, W))
    sf = rng.standard_normal((1, 4, H, W))
    u_std, s_std = rng.uniform(0.5, 2.0, 65), rng.uniform(0.5, 2.0, 4)
    kw = dict(octaves=2, period=6, planes=(0, 17, 64, 65, 68))
    batch_u, batch_s = perturb_ref(np.repeat(up, 4, 0), np.repeat(sf, 4, 0), u_std, s_std, 0.1, 9, first_member=2, **kw)
    for e in range(4):
        one_u, one_s = perturb_ref(up, sf, u_std, s_std, 0.1, 9, first_member=2 + e, **kw)
        assert np.array_equal(one_u[0], batch_u[e]) and np.array_equal(one_s[0], batch_s[e])
    ctl_u, _ = perturb_ref(np.repeat(up, 2, 0), np.repeat(sf, 2, 0), u_std, s_std, 0.1, 9, first_member=0, **kw)
    assert np.array_equal(ctl_u[0], up[0]) and not np.array_equal(ctl_u[1], up[0])


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libpangu_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_ensemble_entries_argument_validation_without_gpu():
    lib = _lib_or_skip()
    P8 = 8
    H, W = 37, 96
    su, ss = 65 * H * W, 4 * H * W
    perturb = lambda up, E, H_, W_, amp=P8, octaves=3, period=12, stride=su: lib.pangu_ensemble_perturb_f32(
        None, up, stride, P8, ss, E, 0, H_, W_, amp, P8, P8, 1, octaves, period, 0.5, 1)
    assert perturb(None, 3, H, W) == -2
    assert perturb(P8, 3, H, W, amp=None) == -2
    assert perturb(P8, 0, H, W) == -1                          # E
    assert perturb(P8, 3, H, 98, period=2, octaves=1) == -1      # W % 4
    assert perturb(P8, 3, H, 120, period=12) == -1             # octave 2: 48 cells do not divide 120
    assert perturb(P8, 3, H, W, octaves=0) == -1
    assert perturb(P8, 3, H, W, stride=su - 4) == -1           # member stride shorter than a member
    stats = lambda x, E, planes, H_, W_, out=P8, ws_bytes=1 << 30: lib.pangu_ensemble_stats_f32(
        None, x, planes * H_ * W_, E, P8, P8, P8, out, None, None, P8, ws_bytes, planes, H_, W_)
    assert stats(None, 3, 65, H, W) == -2
    assert stats(P8, 3, 65, H, W, out=None) == -2
    assert lib.pangu_ensemble_stats_f32(None, P8, 65 * H * W, 3, P8, None, P8, P8, None, None, P8, 1 << 30, 65, H, W) == -2   # clim
    assert stats(P8, 1, 65, H, W) == -1                        # E < 2
    assert stats(P8, 129, 65, H, W) == -1                      # E > 128
    assert stats(P8, 3, 65, H, 98) == -1                       # W % 4
    assert stats(P8, 3, 65, H, W, ws_bytes=16) == -4           # workspace too small


def test_python_refusals_before_any_launch():
    H, W = 8, 102
    up, sf = torch.zeros(2, 5, 13, H, W), torch.zeros(2, 4, H, W)
    sl = (torch.zeros(1, 4, 1, 1), torch.ones(1, 4, 1, 1), torch.zeros(1, 5, 13, 1, 1), torch.ones(1, 5, 13, 1, 1))
    with pytest.raises(ValueError, match="W % L"):
        P.ensemble.perturb_(torch.zeros(2, 5, 13, H, 120), torch.zeros(2, 4, H, 120), sl, 0.1, 0)
    with pytest.raises(ValueError, match="W % 4"):
        P.ensemble.perturb_(up, sf, sl, 0.1, 0)
    with pytest.raises(ValueError, match="amplitude"):
        P.ensemble.perturb_(torch.zeros(2, 5, 13, H, 96), torch.zeros(2, 4, H, 96), sl, None, 0)
    with pytest.raises(TypeError):
        P.ensemble.perturb_(torch.zeros(2, 5, 13, H, 96), torch.zeros(2, 4, H, 96), sl, seed=0)     # amplitude missing
    with pytest.raises(ValueError, match="9 values"):
        P.ensemble.perturb_(torch.zeros(2, 5, 13, H, 96), torch.zeros(2, 4, H, 96), sl, [0.1] * 5, 0)
    with pytest.raises(ValueError, match="2 <= E"):
        P.score.ensemble_scores(up[:1], sf[:1], up[0], sf[0], sl)
    with pytest.raises(ValueError, match="at least 2 members"):
        P.ensemble.EnsembleRollout(None, up[:1], sf[:1], None, None, None, sl, members=1, amplitude=0.1)
    with pytest.raises(TypeError):
        P.ensemble.EnsembleRollout(None, up[:1], sf[:1], None, None, None, sl, members=4)          # amplitude missing
    with pytest.raises(ValueError, match="W % L"):
        P.ensemble.EnsembleRollout(None, torch.zeros(1, 5, 13, H, 120), torch.zeros(1, 4, H, 120), None, None, None, sl,
                                   members=4, amplitude=0.1)
