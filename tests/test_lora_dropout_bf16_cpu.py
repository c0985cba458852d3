"""LoRA adapter dropout on the bf16 training path (PanguModel.enable_lora(..., bf16_training=True, bf16_dropout=True), the three
entries of csrc/lora_dropout_bf16.hip / lora_bf16.hip): what can be checked without a GPU."""
import copy
import pickle

import pytest
import torch

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib

ENTRIES = ("pangu_lora_dropout_fwd_bf16", "pangu_lora_wgrad_dropout_bf16", "pangu_lora_dropout_dx_bf16")
E_SHAPE, E_NULL, E_ARG = -1, -2, -4
P16 = 16          # any non-NULL, 16-B aligned address: the calls below return before touching memory


@pytest.fixture(scope="module")
def base():
    torch.manual_seed(0)
    return P.PanguModel(device="cpu")


def test_bf16_dropout_flag_is_accepted_kept_and_cleared(base):
    m = copy.deepcopy(base)
    names = m.enable_lora(r=4, lora_dropout=0.1, bf16_training=True, bf16_dropout=True)
    assert len(names) == 67
    assert m._lora_bf16_dropout is True and m._lora_bf16_training is True
    assert "_lora_bf16_dropout" in m.__dict__
    assert m.has_lora_dropout()
    assert copy.deepcopy(m)._lora_bf16_dropout is True
    assert pickle.loads(pickle.dumps(m))._lora_bf16_dropout is True
    m.merge_lora()
    assert m._lora_bf16_dropout is False
    assert not m.has_lora()


def test_bf16_dropout_defaults_to_off_and_needs_bf16_training(base):
    m = copy.deepcopy(base)
    m.enable_lora(r=4, bf16_training=True)
    assert m._lora_bf16_dropout is False
    with pytest.raises(ValueError, match="bf16_training"):
        copy.deepcopy(base).enable_lora(r=4, lora_dropout=0.1, bf16_dropout=True)
    with pytest.raises(ValueError, match="bf16_training"):
        copy.deepcopy(base).enable_lora(r=4, bf16_dropout=True)
    # the pinned refusal stays, and now names the keyword that lifts it
    with pytest.raises(ValueError, match="bf16") as e:
        copy.deepcopy(base).enable_lora(lora_dropout=0.1, bf16_training=True)
    assert "bf16_dropout" in str(e.value)
    # the flag alone (no dropout) changes nothing else
    m = copy.deepcopy(base)
    m.enable_lora(r=4, bf16_training=True, bf16_dropout=True)
    assert m._lora_bf16_dropout is True and not m.has_lora_dropout()


def test_entries_are_declared():
    for name in ENTRIES:
        assert name in _lib.header_functions(), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["pangu_lora_dropout_fwd_bf16"] == _lib.SIGNATURES["pangu_lora_dropout_fwd_f32"]
    assert _lib.SIGNATURES["pangu_lora_wgrad_dropout_bf16"] == _lib.SIGNATURES["pangu_lora_wgrad_dropout_f32"]
    assert _lib.SIGNATURES["pangu_lora_dropout_dx_bf16"] == _lib.SIGNATURES["pangu_lora_dropout_dx_f32"]


def _caller(fn, ok, idx):
    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[idx[k]] = v
        return fn(*a)
    return call


def test_fwd_entry_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    # (stream, X, ldx, Y, ldy, A, B, M, N, K, r, scaling, p, seed, act, H, ldh)
    ok = (None, P16, 384, P16, 1536, P16, P16, 1000, 1536, 384, 16, 1.0, 0.1, 7, 0, None, 0)
    idx = {"x": 1, "ldx": 2, "y": 3, "ldy": 4, "A": 5, "B": 6, "M": 7, "N": 8, "K": 9, "r": 10, "p": 12, "act": 14, "h": 15, "ldh": 16}
    call = _caller(lib.pangu_lora_dropout_fwd_bf16, ok, idx)
    for k in ("x", "y", "A", "B"):
        assert call(**{k: None}) == E_NULL, k
    assert call(act=1, h=None, ldh=1536) == E_NULL            # GELU output asked for, no H
    for r in (0, 2, 12, 64):
        assert call(r=r) == E_SHAPE, r
    assert call(M=0) == E_SHAPE
    for p in (0.0, 1.0):
        assert call(p=p) == E_ARG, p
    assert call(K=200, ldx=200) == E_SHAPE                    # K % 64
    assert call(K=400, ldx=400) == E_SHAPE                    # a multiple of 16, not of 64
    assert call(N=1600, ldy=1600) == E_SHAPE                  # K + N = 1984 > 1920
    assert call(ldx=376) == E_SHAPE                           # ldx < K
    assert call(ldy=1532) == E_SHAPE                          # ldy < N
    assert call(ldx=388) == E_SHAPE                           # row stride not a multiple of 8
    assert call(ldy=1540) == E_SHAPE
    assert call(act=1, h=P16, ldh=1528) == E_SHAPE            # ldh < N
    assert call(act=1, h=P16, ldh=1540) == E_SHAPE
    for k in ("x", "y", "A", "B"):
        assert call(**{k: P16 + 2}) == E_ARG, k
    assert call(act=1, h=P16 + 2, ldh=1536) == E_ARG
    assert call(act=2) == E_ARG                               # neither NONE nor GELU


def test_wgrad_entry_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    ws = 1 << 20
    # (stream, dY, lddy, X, ldx, A, B, dA, dB, V, M, N, K, r, scaling, p, seed, workspace, workspace_bytes)
    ok = (None, P16, 384, P16, 384, P16, P16, P16, P16, P16, 1000, 384, 384, 16, 1.0, 0.1, 7, P16, ws)
    idx = {"dy": 1, "lddy": 2, "x": 3, "ldx": 4, "A": 5, "B": 6, "dA": 7, "dB": 8, "V": 9, "M": 10, "N": 11, "K": 12, "r": 13, "p": 15,
           "ws": 17, "ws_bytes": 18}
    call = _caller(lib.pangu_lora_wgrad_dropout_bf16, ok, idx)
    for k in ("dy", "x", "A", "B", "dA", "dB", "V", "ws"):
        assert call(**{k: None}) == E_NULL, k
    for r in (0, 2, 12, 64):
        assert call(r=r) == E_SHAPE, r
    assert call(M=0) == E_SHAPE
    for p in (0.0, 1.0):
        assert call(p=p) == E_ARG, p
    assert call(K=200, ldx=200) == E_SHAPE
    assert call(K=400, ldx=400) == E_SHAPE                    # a multiple of 16 (the plain entry's rule), not of 64
    assert call(N=1600, lddy=1600) == E_SHAPE                 # K + N = 1984 > 1920
    assert call(ldx=376) == E_SHAPE
    assert call(lddy=388) == E_SHAPE
    for k in ("dy", "x", "A", "B", "V", "ws"):
        assert call(**{k: P16 + 2}) == E_ARG, k
    assert call(ws_bytes=16 * (384 + 384) * 4 - 4) == E_ARG   # one element short of one partial


def test_dx_entry_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    # (stream, dX, lddx, V, A, M, K, r, p, seed, pre, ldpre)
    ok = (None, P16, 384, P16, P16, 1000, 384, 16, 0.1, 7, None, 0)
    idx = {"dx": 1, "lddx": 2, "V": 3, "A": 4, "M": 5, "K": 6, "r": 7, "p": 8, "pre": 10, "ldpre": 11}
    call = _caller(lib.pangu_lora_dropout_dx_bf16, ok, idx)
    for k in ("dx", "V", "A"):
        assert call(**{k: None}) == E_NULL, k
    for r in (0, 2, 12, 64):
        assert call(r=r) == E_SHAPE, r
    assert call(M=0) == E_SHAPE
    for p in (0.0, 1.0):
        assert call(p=p) == E_ARG, p
    assert call(K=200, lddx=200) == E_SHAPE
    assert call(K=1984, lddx=1984) == E_SHAPE                 # wider than any projection (K + N <= 1920)
    assert call(lddx=376) == E_SHAPE
    assert call(lddx=388) == E_SHAPE
    assert call(pre=P16, ldpre=376) == E_SHAPE
    assert call(pre=P16, ldpre=388) == E_SHAPE
    for k in ("dx", "V", "A"):
        assert call(**{k: P16 + 2}) == E_ARG, k
    assert call(pre=P16 + 2, ldpre=384) == E_ARG
