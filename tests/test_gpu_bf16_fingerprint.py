"""The bf16 GEMMs (csrc/gemm_bf16.hip, csrc/gemm_ws_bf16.hip, csrc/gemm_ln_bf16.hip) compute the bits they computed before their
main loops, LayerNorm epilogue and patch traffic moved into shared headers (csrc/gemm_bf16_loop.h, csrc/ln_epilogue_bf16.h):
SHA-256 digests of everything `ops_bf16.linear`, `linear_gelu_bwd` and `linear_ln_residual` write over the case list of
tools/gemm_bf16_fingerprint.py, against the digests recorded from a build of the parent commit
(profiles/gemm_bf16_shared_fingerprint_parent.json).  Needs an MI355X: run with `-m gpu`."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gemm_bf16_fingerprint as F  # noqa: E402

pytestmark = pytest.mark.gpu
NCASES = 925


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "profiles", "gemm_bf16_shared_fingerprint_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    """key -> (digest of every buffer the case writes, everything behind and beside the written views still poisoned)"""
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    cache, out = {}, {}
    for case in F.cases():
        written = F.run(case, cache)
        out[F.key(case)] = (F.digest(*[buf for buf, _ in written]), all(F.untouched(buf, view) for buf, view in written))
    return out


def test_case_list_and_recorded_keys_are_the_same_set(recorded):
    keys = [F.key(c) for c in F.cases()]
    assert len(set(keys)) == len(keys) == NCASES
    assert set(keys) == set(recorded["cases"])


def test_every_digest_matches_the_parent(recorded, computed):
    got = F.record({k: d for k, (d, _) in computed.items()})
    assert set(got["cases"]) == set(recorded["cases"])
    assert [k for k in got["cases"] if got["cases"][k] != recorded["cases"][k]] == []
    assert got["all"] == recorded["all"]


def test_nothing_is_written_outside_the_view(computed):
    """Rows >= M (and the right half of a strided output) keep their poison at every cut of every tiling."""
    assert [k for k, (_, untouched) in sorted(computed.items()) if not untouched] == []
