"""The exact-split fp32 GEMMs (csrc/gemm_f32_split.hip, csrc/gemm_ln_f32_split.hip) compute the bits they computed under the
64 x 96 wave tiling: SHA-256 digests of `ops.linear_split` and `ops.linear_ln_residual_split` over the case lists of
tools/gemm_f32_fingerprint.py, against the digests recorded from a build of the commit before the row-owning tiling
(profiles/gemm_f32_shared_loops_fingerprint_new.json for the main list, profiles/split_rows_fingerprint_parent.json for the
edges of the tiling).  Needs an MI355X: run with `-m gpu`."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gemm_f32_fingerprint as F  # noqa: E402

pytestmark = pytest.mark.gpu
SPLIT = ("linear_split ", "linear_ln_residual_split ")


def _recorded(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        return {k: v for k, v in json.load(f).items() if k.startswith(SPLIT)}


@pytest.fixture(scope="module")
def edges():
    """key -> (digest of the whole poisoned buffer, the part behind and beside the written view still poisoned)"""
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    cache, out = {}, {}
    for case in F.edge_cases():
        buf, view = F.edge_run(case, cache)
        M, N = view.shape
        untouched = bool((buf[M:] == F.EDGE_POISON).all()) and bool((buf[:M, N:] == F.EDGE_POISON).all())
        out[F.edge_key(case)] = (F.digest(buf), untouched)
    return out


def test_main_list_matches_the_recorded_digests():
    want = _recorded("gemm_f32_shared_loops_fingerprint_new.json")
    assert len(want) == 240
    got = F.split_cases({})
    assert set(got) == set(want)
    assert [k for k in sorted(want) if got[k] != want[k]] == []


def test_edges_match_the_recorded_digests(edges):
    want = _recorded("split_rows_fingerprint_parent.json")
    assert set(want) == set(edges) and len(want) == len(F.edge_cases()) == 864 + 720
    assert [k for k in sorted(want) if edges[k][0] != want[k]] == []


def test_nothing_is_written_behind_row_M(edges):
    """Rows >= M of the tile (and the right half of a concat buffer) keep their poison at every cut of the wave tiling."""
    assert [k for k, (_, untouched) in sorted(edges.items()) if not untouched] == []
