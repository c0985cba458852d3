"""The (upper, surface) contract of the score module, without a GPU: the seven entries that take a field pair refuse the same
malformed pair in the same way -- a ValueError under the entry's own name, raised by the shared validators (score._check_members,
score._check_cases) before any device call.  The tensors live on the CPU, where a pair that passes the validators ends in the
RuntimeError "no CPU fallback" instead, so a ValueError here is proof that nothing was launched."""
import pytest
import torch

from pangu_pytorch_amd import score

E, H, W = 2, 5, 8                                # two members or two cases, as the entry reads its leading dimension


def _thresholds():
    return torch.zeros(1, 5, 13), torch.zeros(1, 4)


def _stats_last():
    return torch.zeros(1, 4, 1, 1), torch.ones(1, 4, 1, 1), torch.zeros(1, 5, 13, 1, 1), torch.ones(1, 5, 13, 1, 1)


def _plan(up):
    return score.point_plan(up.shape[-2], up.shape[-1], [10.0, -20.0], [5.0, 300.0])


# who -> (call(upper, surface, target_upper, target_surface), takes targets, needs W % 4 == 0)
ENTRIES = {
    "ensemble_scores": (lambda up, sf, tu, ts: score.ensemble_scores(up, sf, tu, ts, _stats_last()), True, True),
    "ensemble_reliability": (lambda up, sf, tu, ts: score.ensemble_reliability(up, sf, tu, ts, _thresholds()), True, True),
    "ensemble_quantiles": (lambda up, sf, tu, ts: score.ensemble_quantiles(up, sf, (0.5,), tu, ts), True, True),
    "deterministic_scores": (lambda up, sf, tu, ts: score.deterministic_scores(up, sf, tu, ts), True, True),
    "event_scores": (lambda up, sf, tu, ts: score.event_scores(up, sf, tu, ts, _thresholds()), True, True),
    "sample_points": (lambda up, sf, tu, ts: score.sample_points(up, sf, _plan(up)), False, False),
    "LeadWindowStats.update": (lambda up, sf, tu, ts: score.LeadWindowStats([(0, 1)]).update(0, up, sf), False, False),
}


def _pair(upper=(E, 5, 13, H, W), surface=(E, 4, H, W)):
    return torch.zeros(upper), torch.zeros(surface)


@pytest.mark.parametrize("who", list(ENTRIES))
def test_every_entry_refuses_the_same_malformed_pair_alike(who):
    call, targets, w4 = ENTRIES[who]

    def refused(up, sf, tu=None, ts=None):
        if tu is None and targets:                               # member targets are one state, case targets one per case
            tu, ts = (up[0], sf[0]) if who.startswith("ensemble") else (up, sf)
        with pytest.raises(ValueError) as err:
            call(up, sf, tu, ts)
        assert str(err.value).startswith(who + ": "), str(err.value)
        return str(err.value)

    assert "expected upper" in refused(*_pair(upper=(E, 5, 12, H, W)))          # wrong plane dimensions
    assert "expected upper" in refused(*_pair(surface=(E, 3, H, W)))
    assert "grids" in refused(*_pair(surface=(E, 4, H, W + 4)))                 # disagreeing grids
    assert "grids" in refused(*_pair(surface=(E, 4, H + 1, W)))
    refused(*_pair(surface=(E + 1, 4, H, W)))                                   # disagreeing leading dimensions
    odd = _pair(upper=(E, 5, 13, H, W - 2), surface=(E, 4, H, W - 2))
    if w4:
        assert "W % 4" in refused(*odd)
    else:                                                                       # no such rule: the pair passes, the launch needs the device
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(*odd, None, None)
    if targets:                                                                 # one target of two
        up, sf = _pair()
        tu = up[0] if who.startswith("ensemble") else up
        assert "both targets" in refused(up, sf, tu, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # the well-formed pair passes every check
        up, sf = _pair()
        call(up, sf, *((up[0], sf[0]) if who.startswith("ensemble") else (up, sf)))
