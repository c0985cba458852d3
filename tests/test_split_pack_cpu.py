"""The layouts of the exact-split fp32 GEMM (csrc/gemm_f32_split.hip) as pangu_pytorch_amd/split_layout.py states them: the
weight image is a bijection, and under the gfx950 bank rules (tools/lds_banks.py) every ds_read_b128 fragment read of the
stage -- the fp32 A image and the three bf16 planes -- is conflict-free.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from lds_banks import conflict_free  # noqa: E402

from pangu_pytorch_amd import split_layout as L  # noqa: E402


@pytest.mark.parametrize("N,K", [(192, 16), (576, 192), (384, 400), (160, 384), (64, 384), (4, 16), (196, 48), (192, 32), (384, 16)])
def test_image_layout_is_a_bijection(N, K):
    """(plane, row 0 .. image_rows(N) - 1, k) -> every one of the 3 image_rows(N) K bf16 slots exactly once."""
    rows = L.image_rows(N)
    assert rows % 192 == 0 and rows - 192 < N <= rows and L.served(N, K)
    idx = [L.image_index(N, K, p, n, k) for p in range(3) for n in range(rows) for k in range(K)]
    assert sorted(idx) == list(range(3 * rows * K))
    # a lane's fragment (8 consecutive k of one row and plane) is one aligned 16-B chunk
    for p in range(3):
        for n in (0, 1, 191, N - 1):
            for k in range(0, K, 8):
                base = L.image_index(N, K, p, n, k)
                assert base % 8 == 0 and [L.image_index(N, K, p, n, k + j) - base for j in range(8)] == list(range(8))


def test_image_rows_and_refusals():
    assert [L.image_rows(n) for n in (4, 160, 192, 196, 384, 388)] == [192, 192, 192, 384, 384, 576]
    assert not L.served(6, 16) and not L.served(160, 24) and not L.served(0, 16)
    assert L.served(160, 384)
    # the rows of W have, in the image, the index they have in the image of the zero-extended weight
    assert L.image_index(160, 384, 2, 159, 383) == L.image_index(192, 384, 2, 159, 383)


def test_image_block_is_the_lds_stage_image():
    """The (n-tile, k-step) block of the image is copied linearly behind the A image of a stage: the byte a fragment read
    fetches is the byte the layout statement puts there."""
    N, K = 384, 48
    for nt in range(N // L.BN):
        for kt in range(K // L.BK):
            block = (nt * (K // L.BK) + kt) * L.B_BYTES
            for lane in range(64):
                lr, lh = lane & 31, lane >> 5
                for wn in range(2):
                    for j in range(3):
                        for p in range(3):
                            n, k = nt * L.BN + wn * 96 + j * 32 + lr, kt * L.BK + 8 * lh
                            assert block + L.w_fragment_address(lane, wn, j, p) - L.A_BYTES == 2 * L.image_index(N, K, p, n, k)
    assert L.STAGE % 1024 == 0 and L.A_BYTES % 1024 == 0
    dst = {L.dma_piece_destination(q, lane) for q in range(L.STAGE // 1024) for lane in range(64)}
    assert dst == set(range(0, L.STAGE, 16))


def test_a_image_is_a_bijection():
    offs = {L.a_chunk_offset(r, c) for r in range(L.BM) for c in range(4)}
    assert offs == set(range(0, L.A_BYTES, 16))


@pytest.mark.parametrize("wm", range(2))
@pytest.mark.parametrize("i", range(2))
@pytest.mark.parametrize("h", range(2))
def test_a_fragment_reads_conflict_free(wm, i, h):
    assert conflict_free("read_b128", lambda l: L.a_fragment_address(l, wm, i, h))


@pytest.mark.parametrize("wn", range(2))
@pytest.mark.parametrize("j", range(3))
@pytest.mark.parametrize("plane", range(3))
def test_w_fragment_reads_conflict_free(wn, j, plane):
    assert conflict_free("read_b128", lambda l: L.w_fragment_address(l, wn, j, plane))
    # ... in each ring slot (the stage size keeps the 256-byte bank phase)
    assert L.STAGE % 256 == 0
