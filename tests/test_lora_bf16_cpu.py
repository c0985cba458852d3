"""bf16 LoRA training (PanguModel.enable_lora(bf16_training=True), pangu_lora_wgrad_bf16, the module-keyed bf16 images of W_eff):
what can be checked without a GPU."""
import copy
import pickle

import pytest
import torch

import pangu_pytorch_amd as P
from pangu_pytorch_amd import _lib, fused_bf16, ops
from pangu_pytorch_amd.layers import LoraLinear


@pytest.fixture(scope="module")
def base():
    torch.manual_seed(0)
    return P.PanguModel(device="cpu")


def test_bf16_training_flag_is_kept_and_cleared(base):
    m = copy.deepcopy(base)
    names = m.enable_lora(r=4, bf16_training=True)
    assert len(names) == 67
    assert m._lora_bf16_training is True
    assert "_lora_bf16_training" in m.__dict__
    assert copy.deepcopy(m)._lora_bf16_training is True
    assert pickle.loads(pickle.dumps(m))._lora_bf16_training is True
    m.merge_lora()
    assert m._lora_bf16_training is False
    assert not m.has_lora()


def test_bf16_training_defaults_to_off(base):
    m = copy.deepcopy(base)
    m.enable_lora(r=4)
    assert m._lora_bf16_training is False
    with pytest.raises(ValueError, match="lora_dropout"):
        copy.deepcopy(base).enable_lora(r=4, dropout=0.1, bf16_training=True)


def test_bf16_entry_is_declared():
    assert "pangu_lora_wgrad_bf16" in _lib.header_functions()
    assert "pangu_lora_wgrad_bf16" in _lib.SIGNATURES


def test_bf16_entry_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    P16 = 16          # any non-NULL, 16-B aligned address: the calls below return before touching memory
    ws = 1 << 20
    ok = (None, P16, 384, P16, 384, P16, P16, P16, P16, 1000, 384, 384, 16, 1.0, P16, ws)

    def call(**kw):
        a = list(ok)
        idx = {"dy": 1, "lddy": 2, "x": 3, "ldx": 4, "A": 5, "B": 6, "dA": 7, "dB": 8, "M": 9, "N": 10, "K": 11, "r": 12,
               "ws": 14, "ws_bytes": 15}
        for k, v in kw.items():
            a[idx[k]] = v
        return lib.pangu_lora_wgrad_bf16(*a)

    for k in ("dy", "x", "A", "B", "dA", "dB", "ws"):
        assert call(**{k: None}) == -2, k
    for r in (0, 2, 12, 24, 64):
        assert call(r=r) == -1, r
    assert call(M=0) == -1
    assert call(K=200, ldx=200) == -1                  # K % 16
    assert call(N=1552, lddy=1552) == -1               # K + N = 1936 > 1920
    assert call(ldx=376) == -1                         # ldx < K
    assert call(lddy=388) == -1                        # row stride not a multiple of 8
    assert call(x=P16 + 2) == -4                       # b128 loads need 16-B alignment
    assert call(ws_bytes=16 * (384 + 384) * 4 - 4) == -4  # one element short of one partial


def test_shadow_images_of_w_eff_are_keyed_by_the_module():
    """W_eff is a fresh tensor per refresh: its bf16 images must not be keyed by id() of that tensor, or every optimizer step
    leaves dead entries behind.  Plain cast, transposed cast: same cache size after every refresh, no bulk-refresh job."""
    torch.manual_seed(1)
    lin = LoraLinear(32, 48, r=4, alpha=8)
    with torch.no_grad():
        lin.lora_B.normal_()
    sh = fused_bf16.WeightShadow()
    sizes, seen = [], []
    for step in range(3):
        w = lin.effective_weight()
        seen.append(w)                                  # keep the old tensors alive: a recycled id() must not hide a leak
        img, img_t = sh.get(w), sh.get_t(w)
        assert img is sh.get_lin(lin)                   # the inference accessor shares the image
        assert torch.equal(img, w.to(torch.bfloat16)) and torch.equal(img_t, w.t().to(torch.bfloat16))
        assert sh.get(w) is img and sh.get_t(w) is img_t
        sizes.append((len(sh.cache), len(sh.jobs), len(sh.makers)))
        with torch.no_grad():
            lin.lora_A.mul_(1.5)                        # bumps the stamp: the next effective_weight() is a new tensor
        ops.bump_weights_epoch()
    assert seen[0] is not seen[1] and seen[1] is not seen[2]
    assert sizes[0] == sizes[1] == sizes[2] == (2, 0, 2)
    # a W_eff that its module has replaced since gets its own cast, uncached, and does not disturb the current image
    cur = lin.effective_weight()
    old = sh.get(seen[0])
    assert torch.equal(old, seen[0].to(torch.bfloat16)) and not torch.equal(old, sh.get(cur))
    assert (len(sh.cache), len(sh.jobs)) == (2, 0)
