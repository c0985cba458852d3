"""LoRA adapter dropout (PanguModel.enable_lora(lora_dropout=...), layers.lora_dropout_keep, LoraLinear's own forward, the new
C entries' argument checks): what can be checked without a GPU."""
import copy
import math
import pickle

import numpy as np
import pytest
import torch
from torch import nn

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib
from pangu_pytorch_amd.layers import LoraLinear, lora_dropout_keep

PS = (0.05, 0.1, 0.5)
SHAPES = ((4099, 192), (1024, 1536), (37, 384))
SEEDS = (0, 1, 2, 12345, 0xdeadbeef, 2 ** 32 - 1)


@pytest.fixture(scope="module")
def base():
    torch.manual_seed(0)
    return P.PanguModel(device="cpu")


@pytest.fixture(scope="module")
def adapted(base):
    m = copy.deepcopy(base)
    names = m.enable_lora(r=16, alpha=16, lora_dropout=0.1)
    return m, names


def test_enable_lora_accepts_lora_dropout(adapted):
    m, names = adapted
    lins = [x for x in m.modules() if type(x) is LoraLinear]
    assert len(names) == 67 and len(lins) == 67
    assert all(x.lora_dropout == 0.1 for x in lins)
    assert "lora_dropout=0.1" in repr(lins[0])
    assert m.has_lora_dropout()


def test_default_is_no_dropout(base):
    m = copy.deepcopy(base)
    m.enable_lora(r=8, alpha=8)
    assert all(x.lora_dropout == 0.0 for x in m.modules() if type(x) is LoraLinear)
    assert not m.has_lora_dropout()


def test_bad_values_raise(base):
    for p in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="lora_dropout"):
            copy.deepcopy(base).enable_lora(lora_dropout=p)
    with pytest.raises(ValueError, match="lora_dropout="):            # the old keyword still refuses, and names the new one
        copy.deepcopy(base).enable_lora(dropout=0.1)
    with pytest.raises(ValueError, match="bf16"):
        copy.deepcopy(base).enable_lora(lora_dropout=0.1, bf16_training=True)
    copy.deepcopy(base).enable_lora(lora_dropout=0.0, bf16_training=True)      # no dropout: as before
    with pytest.raises(ValueError, match="lora_dropout"):
        LoraLinear(8, 8, r=4, alpha=4, lora_dropout=1.0)


def test_deepcopy_and_pickle_keep_the_value(adapted):
    m, names = adapted
    lin = dict(m.named_modules())[names[0]]
    for clone in (copy.deepcopy(lin), pickle.loads(pickle.dumps(lin))):
        assert type(clone) is LoraLinear and clone.lora_dropout == 0.1 and clone.r == 16
    m2 = pickle.loads(pickle.dumps(m))
    assert all(x.lora_dropout == 0.1 for x in m2.modules() if type(x) is LoraLinear)


def test_state_dict_keys_unchanged(base, adapted):
    m, names = adapted
    plain = copy.deepcopy(base)
    plain.enable_lora(r=16, alpha=16)
    assert list(m.state_dict()) == list(plain.state_dict())
    assert list(m.lora_state_dict()) == list(plain.lora_state_dict())
    assert len(m.lora_state_dict()) == 2 * 67 + 4


# ---- the keep mask
def _lowbias32_np(x):
    x = x.astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    return x


def _keep_np(seed, M, K, p):
    """keep(seed, i, k) = lowbias32(lowbias32(lowbias32(seed) ^ i) ^ k) >= T, T = clamp(round(p 2^32), 1, 2^32 - 1)."""
    T = min(max(int(math.floor(p * 2.0 ** 32 + 0.5)), 1), 2 ** 32 - 1)
    hs = _lowbias32_np(np.array([seed], dtype=np.uint64))[0]
    hrow = _lowbias32_np(hs ^ np.arange(M, dtype=np.uint64))
    return _lowbias32_np(hrow[:, None] ^ np.arange(K, dtype=np.uint64)[None, :]) >= np.uint64(T)


def test_lowbias32_known_values():
    # csrc/common.h lowbias32 by hand: 0 -> 0 (every step keeps zero); 1 and 2^32 - 1 through plain Python integers
    def ref(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)
    for v in (0, 1, 12345, 0xdeadbeef, 2 ** 32 - 1):
        assert int(_lowbias32_np(np.array([v], dtype=np.uint64))[0]) == ref(v)
        assert int(P.layers._lowbias32(torch.tensor(v, dtype=torch.int64))) == ref(v)
    assert ref(0) == 0


@pytest.mark.parametrize("p", PS)
def test_keep_mask_equals_restatement_and_is_balanced(p):
    worst = 0.0
    for M, K in SHAPES:
        prev = None
        for seed in SEEDS:
            keep = lora_dropout_keep(seed, M, K, p)
            assert keep.dtype == torch.bool and tuple(keep.shape) == (M, K)
            k = keep.numpy()
            assert np.array_equal(k, _keep_np(seed, M, K, p)), (M, K, seed)
            n = M * K
            z = (k.mean() - (1 - p)) / math.sqrt(p * (1 - p) / n)
            assert abs(z) <= 5.0, ("fraction", M, K, seed, z)
            worst = max(worst, abs(z))
            c = k.astype(np.float64) - k.mean()
            var = (c * c).mean()
            for a, b, tag in ((c[:, :-1], c[:, 1:], "along a row"), (c[:-1], c[1:], "along a column")):
                zc = (a * b).mean() / var * math.sqrt(a.size)
                assert abs(zc) <= 5.0, ("lag-1", tag, M, K, seed, zc)
            if prev is not None:                        # two seeds agree like two independent masks
                q = (1 - p) ** 2 + p ** 2
                za = ((k == prev).mean() - q) / math.sqrt(q * (1 - q) / n)
                assert abs(za) <= 5.0, ("two seeds", M, K, seed, za)
            prev = k
    assert worst > 0.0


def test_keep_mask_threshold_edges():
    assert P.layers.lora_dropout_threshold(0.1) == 429496730
    assert P.layers.lora_dropout_threshold(1e-12) == 1 and P.layers.lora_dropout_threshold(1 - 1e-12) == 2 ** 32 - 1
    with pytest.raises(ValueError):
        lora_dropout_keep(2 ** 32, 4, 4, 0.1)


# ---- LoraLinear.forward on the CPU
def _module(p=0.1):
    torch.manual_seed(3)
    lin = LoraLinear.from_linear(nn.Linear(64, 48), r=8, alpha=16, lora_dropout=p)
    with torch.no_grad():
        lin.lora_B.copy_(torch.randn(48, 8) * 0.3)
    return lin


def test_forward_eval_ignores_dropout():
    lin, ref = _module(0.5).eval(), _module(0.0).eval()
    x = torch.randn(5, 7, 64)
    st = torch.get_rng_state()
    assert torch.equal(lin(x), ref(x))
    assert torch.equal(torch.get_rng_state(), st) and lin.last_dropout_seed is None      # no draw either


def test_forward_train_is_pefts_formula_with_the_restated_mask():
    lin = _module(0.1).train()
    x = torch.randn(5, 7, 64)
    y = lin(x)
    seed = lin.last_dropout_seed
    assert 0 <= seed < 2 ** 32
    keep = torch.from_numpy(_keep_np(seed, 35, 64, 0.1)).reshape(5, 7, 64)
    xd, W, b, A, B = (t.detach().double() for t in (x, lin.weight, lin.bias, lin.lora_A, lin.lora_B))
    ref = xd @ W.t() + b + lin.scaling * ((keep * xd / (1 - 0.1)) @ A.t()) @ B.t()
    assert ((y.double() - ref).norm() / ref.norm()).item() <= 1e-6
    assert not torch.equal(y, _module(0.0).train()(x))                 # the mask did something


def test_forward_train_follows_manual_seed():
    lin = _module(0.1).train()
    x = torch.randn(9, 64)
    torch.manual_seed(11)
    y1, s1 = lin(x), lin.last_dropout_seed
    y_other = lin(x)
    torch.manual_seed(11)
    y2, s2 = lin(x), lin.last_dropout_seed
    assert s1 == s2 and torch.equal(y1, y2)
    assert not torch.equal(y1, y_other)


def test_lora_args_carry_p_and_seed_only_when_active():
    lin, plain = _module(0.1), nn.Linear(64, 48)
    lin.eval()
    assert P.layers.lora_args(lin, plain) == ((lin.scaling, None), lin.lora_A, lin.lora_B, None, None)      # as without dropout
    lin.train()
    torch.manual_seed(5)
    lora, *ab = P.layers.lora_args(lin, plain)
    assert lora == ((lin.scaling, 0.1, lin.last_dropout_seed), None) and ab[0] is lin.lora_A and ab[1] is lin.lora_B
    torch.manual_seed(5)
    assert P.layers.lora_args(lin)[0][0][2] == lora[0][2]
    assert P.layers.dropout_active(lin) and not P.layers.dropout_active(plain, _module(0.0).train())


# ---- the C entries answer bad arguments before any launch
def test_dropout_entries_reject_bad_arguments_without_gpu():
    lib = _lib.load()
    P16 = 16          # any non-NULL, 16-B aligned address: the calls below return before touching memory
    for name in ("pangu_lora_dropout_fwd_f32", "pangu_lora_wgrad_dropout_f32", "pangu_lora_dropout_dx_f32"):
        assert name in _lib.SIGNATURES and name in _lib.header_functions() and hasattr(lib, name)

    def fwd(**kw):
        a = dict(x=P16, ldx=384, y=P16, ldy=384, A=P16, B=P16, M=1000, N=384, K=384, r=16, s=1.0, p=0.1, seed=1, act=0, h=None, ldh=0)
        a.update(kw)
        return lib.pangu_lora_dropout_fwd_f32(None, *a.values())

    for k in ("x", "y", "A", "B"):
        assert fwd(**{k: None}) == -2, k
    assert fwd(act=1) == -2                                  # GELU needs h
    assert fwd(act=1, h=P16, ldh=380) == -1
    assert fwd(act=2) == -4
    for r in (0, 2, 12, 64):
        assert fwd(r=r) == -1, r
    assert fwd(M=0) == -1 and fwd(K=200, ldx=200) == -1 and fwd(N=1600, ldy=1600) == -1
    assert fwd(ldx=380) == -1 and fwd(ldy=386) == -1
    assert fwd(x=P16 + 4) == -4 and fwd(y=P16 + 8) == -4
    for p in (0.0, 1.0, -0.5, float("nan")):
        assert fwd(p=p) == -4, p

    def wg(**kw):
        a = dict(dy=P16, lddy=384, x=P16, ldx=384, A=P16, B=P16, dA=P16, dB=P16, V=P16, M=1000, N=384, K=384, r=16, s=1.0, p=0.1,
                 seed=1, ws=P16, ws_bytes=1 << 20)
        a.update(kw)
        return lib.pangu_lora_wgrad_dropout_f32(None, *a.values())

    for k in ("dy", "x", "A", "B", "dA", "dB", "V", "ws"):
        assert wg(**{k: None}) == -2, k
    assert wg(r=12) == -1 and wg(M=0) == -1 and wg(K=200, ldx=200) == -1 and wg(ldx=380) == -1
    assert wg(p=0.0) == -4 and wg(p=1.0) == -4
    assert wg(x=P16 + 4) == -4 and wg(ws_bytes=16 * (384 + 384) * 4 - 4) == -4

    def dx(**kw):
        a = dict(dx=P16, lddx=384, V=P16, A=P16, M=1000, K=384, r=16, p=0.1, seed=1, pre=None, ldpre=0)
        a.update(kw)
        return lib.pangu_lora_dropout_dx_f32(None, *a.values())

    for k in ("dx", "V", "A"):
        assert dx(**{k: None}) == -2, k
    assert dx(r=24) == -1 and dx(M=0) == -1 and dx(K=200, lddx=200) == -1 and dx(lddx=380) == -1 and dx(lddx=386) == -1
    assert dx(pre=P16, ldpre=380) == -1
    assert dx(dx=P16 + 4) == -4 and dx(pre=P16 + 4, ldpre=384) == -4
    assert dx(p=1.0) == -4 and dx(p=0.0) == -4
