"""Host side of HipAdam's fused gradient clipping / accumulation scale / non-finite-step guard (csrc/adam.hip): the three C entries
are declared, bound and validate their arguments before any launch; the Python options refuse where they cannot be honoured."""
import ctypes
import re

import pytest
import torch

from pangu_pytorch_amd import _lib, train

NEW = ("pangu_grad_sumsq_multi", "pangu_grad_clip_state", "pangu_adam_step_multi_scaled")
P8 = 8          # any non-NULL address: every call below returns before touching memory


def _header_argtypes(name):
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/pangu_hip.h"
    out = []
    for arg in m.group(1).split(","):
        if "*" in arg or "pangu_stream_t" in arg:
            out.append(ctypes.c_void_p)
        elif "long long" in arg:
            out.append(ctypes.c_longlong)
        elif "double" in arg:
            out.append(ctypes.c_double)
        elif "float" in arg:
            out.append(ctypes.c_float)
        else:
            assert re.search(r"\bint\b", arg), arg
            out.append(ctypes.c_int)
    return out


@pytest.mark.parametrize("name", NEW)
def test_header_matches_binding_table(name):
    assert name in _lib.header_functions()
    assert _lib.SIGNATURES[name] == _header_argtypes(name)
    assert name not in _lib._RESTYPES                        # int, like every entry that launches


def test_existing_adam_entry_and_abi_version_unchanged():
    assert _lib.SIGNATURES["pangu_adam_step_multi"] == _header_argtypes("pangu_adam_step_multi")
    assert len(_lib.SIGNATURES["pangu_adam_step_multi"]) == 11
    assert _lib.load().pangu_abi_version() == 1


ADAM = (1e-3, 0.9, 0.999, 0.0, 1e-8, 0.1, 0.03)          # lr, beta1, beta2, weight_decay, eps, bias corrections


def test_sumsq_rejections():
    f = _lib.load().pangu_grad_sumsq_multi
    assert f(None, None, 3, 10, P8) == -2
    assert f(None, P8, 3, 10, None) == -2
    assert f(None, P8, 0, 10, P8) == -1
    assert f(None, P8, 3, 0, P8) == -1
    assert f(None, P8, 3, -5, P8) == -1
    assert f(None, P8, 3, 1 << 31, P8) == -1                 # more blocks than a grid dimension holds


def test_clip_state_rejections():
    f = _lib.load().pangu_grad_clip_state
    assert f(None, None, 10, P8, 1, 1.0, 1.0, 0) == -2
    assert f(None, P8, 10, None, 1, 1.0, 1.0, 0) == -2
    assert f(None, P8, 0, P8, 1, 1.0, 1.0, 0) == -1
    assert f(None, P8, -1, P8, 1, 1.0, 1.0, 0) == -1
    assert f(None, P8, 1 << 31, P8, 1, 1.0, 1.0, 0) == -1
    for bad in (0.0, -1.0, float("nan")):                    # max_norm not > 0 (only looked at when clipping)
        assert f(None, P8, 10, P8, 1, bad, 1.0, 0) == -4
    for bad in (0.0, -0.5, float("inf"), float("nan")):      # grad_scale not finite and > 0
        assert f(None, P8, 10, P8, 0, 0.0, bad, 0) == -4
        assert f(None, P8, 10, P8, 1, 1.0, bad, 1) == -4


def test_scaled_step_rejections():
    f = _lib.load().pangu_adam_step_multi_scaled
    assert f(None, None, 3, 10, *ADAM, P8) == -2
    assert f(None, P8, 3, 10, *ADAM, None) == -2             # the state record is required
    assert f(None, P8, 0, 10, *ADAM, P8) == -1
    assert f(None, P8, 3, 0, *ADAM, P8) == -1
    assert f(None, P8, 3, 1 << 31, *ADAM, P8) == -1
    # the beta / eps / lr / weight_decay rules of pangu_adam_step_multi
    assert f(None, P8, 3, 10, 1e-3, 1.0, 0.999, 0.0, 1e-8, 0.1, 0.03, P8) == -4
    assert f(None, P8, 3, 10, 1e-3, 0.9, -0.1, 0.0, 1e-8, 0.1, 0.03, P8) == -4
    assert f(None, P8, 3, 10, 1e-3, 0.9, 0.999, 0.0, -1e-8, 0.1, 0.03, P8) == -4
    assert f(None, P8, 3, 10, -1e-3, 0.9, 0.999, 0.0, 1e-8, 0.1, 0.03, P8) == -4
    assert f(None, P8, 3, 10, 1e-3, 0.9, 0.999, -1.0, 1e-8, 0.1, 0.03, P8) == -4
    assert f(None, P8, 3, 10, float("nan"), 0.9, 0.999, 0.0, 1e-8, 0.1, 0.03, P8) == -4


def test_make_optimizer_refuses_options_it_would_ignore():
    cpu_model = torch.nn.Linear(3, 2)
    assert isinstance(train.make_optimizer(cpu_model), torch.optim.Adam)
    with pytest.raises(ValueError, match="max_grad_norm"):
        train.make_optimizer(cpu_model, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        train.make_optimizer(cpu_model, skip_nonfinite=True)


def test_hip_adam_option_validation():
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            train.HipAdam(p, max_grad_norm=bad)
    opt = train.HipAdam(p, max_grad_norm=2, skip_nonfinite=1)
    assert opt.max_grad_norm == 2.0 and opt.skip_nonfinite is True
    # nothing has run on a device yet: no record, nothing to reconcile, no synchronisation
    assert opt.last_grad_norm is None and opt.last_grad_multiplier is None and opt.skipped_steps is None
    assert opt.reconcile_skips() == 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="grad_scale"):
            opt.step(grad_scale=bad)


def test_accumulated_train_step_refusals(monkeypatch):
    calls = []
    monkeypatch.setattr(train, "_owns_dropped_branches", lambda sync: True)       # stands for a dist.FlatGradSync method
    batch = (None, None, None, None)
    with pytest.raises(RuntimeError, match="FlatGradSync"):
        train.accumulated_train_step(None, None, [batch, batch], None, None, None, grad_sync=lambda: calls.append(1))
    assert not calls
    with pytest.raises(ValueError, match="empty"):
        train.accumulated_train_step(None, None, [], None, None, None)


def test_optimizer_tail_scales_gradients_for_other_optimizers():
    """An optimizer that is not HipAdam has no grad_scale: the accumulated gradients are scaled with torch ops before step(), and
    grad_scale = 1 (train_step, rollout_train_step) leaves them alone."""
    lin = torch.nn.Linear(3, 2)
    opt = torch.optim.SGD(lin.parameters(), lr=1.0)
    w0 = lin.weight.detach().clone()
    lin.weight.grad = torch.full_like(lin.weight, 4.0)
    order = []
    train._optimizer_tail(opt, lambda: order.append("sync"), 0.25)            # bias: no gradient, sync given -> left alone
    assert order == ["sync"] and lin.bias.grad is None
    assert torch.equal(lin.weight.grad, torch.full_like(w0, 1.0)) and torch.equal(lin.weight.detach(), w0 - 1.0)
    lin.weight.grad = torch.full_like(lin.weight, 4.0)
    train._optimizer_tail(opt, None)                                          # no sync: the missing gradient becomes zeros
    assert torch.equal(lin.weight.grad, torch.full_like(w0, 4.0)) and torch.equal(lin.bias.grad, torch.zeros(2))
    assert torch.equal(lin.weight.detach(), w0 - 5.0)
