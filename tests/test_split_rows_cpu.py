"""The fragment reads of the row-owning wave tiling of the exact-split fp32 GEMMs (split_main_loop<.., ROWS = true> in
csrc/split_f32.h), as pangu_pytorch_amd/split_layout.py states them: a wave reads the A rows 32 wm + lr of ONE row block and all
six column tiles of an n-tile block; the reads fetch the bytes the image layout puts there and stay conflict-free under the gfx950
bank rules (tools/lds_banks.py).  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from lds_banks import conflict_free  # noqa: E402

from pangu_pytorch_amd import split_layout as L  # noqa: E402

A_BYTES_64 = 64 * 64                 # the A image of the 64 x 384 tile (2 x 2 waves, two n-tile blocks per stage)


def test_a_rows_are_32_wm_plus_lr():
    """Every wave row reads its own 32 rows, both halves of the lane's 8 k; the four wave rows cover the 128-row image once."""
    seen = set()
    for wm in range(4):
        for lane in range(64):
            lr, lh = lane & 31, lane >> 5
            for h in range(2):
                addr = L.a_row_fragment_address(lane, wm, h)
                assert addr == L.a_chunk_offset(32 * wm + lr, 2 * lh + h)
                seen.add(addr)
    assert seen == set(range(0, L.A_BYTES, 16))


def test_row_tiling_reads_what_the_other_tiling_reads():
    """Row block (wm, i) and column block (wn, j) of the 64 x 96 wave are row block 2 wm + i and column tile 3 wn + j here."""
    for lane in range(64):
        for wm in range(2):
            for i in range(2):
                for h in range(2):
                    assert L.a_row_fragment_address(lane, 2 * wm + i, h) == L.a_fragment_address(lane, wm, i, h)
        for wn in range(2):
            for j in range(3):
                for p in range(3):
                    assert L.w_row_fragment_address(lane, 0, 3 * wn + j, p) == L.w_fragment_address(lane, wn, j, p)


@pytest.mark.parametrize("a_bytes,blocks", [(L.A_BYTES, 1), (A_BYTES_64, 2)])
def test_w_tiles_are_the_image_block(a_bytes, blocks):
    """Six column tiles x three planes of n-tile block wn: the byte a fragment read fetches is the byte the image layout puts
    there, the stage being the A image followed by the blocks copied linearly."""
    N, K = 192 * blocks, 32
    for kt in range(K // L.BK):
        for wn in range(blocks):
            block = (wn * (K // L.BK) + kt) * L.B_BYTES
            for lane in range(64):
                lr, lh = lane & 31, lane >> 5
                for j in range(6):
                    for p in range(3):
                        n, k = wn * L.BN + 32 * j + lr, kt * L.BK + 8 * lh
                        addr = L.w_row_fragment_address(lane, wn, j, p, a_bytes)
                        assert addr - a_bytes - wn * L.B_BYTES + block == 2 * L.image_index(N, K, p, n, k)
                        assert addr + 16 <= a_bytes + blocks * L.B_BYTES


@pytest.mark.parametrize("wm", range(4))
@pytest.mark.parametrize("h", range(2))
def test_a_row_fragment_reads_conflict_free(wm, h):
    assert conflict_free("read_b128", lambda l: L.a_row_fragment_address(l, wm, h))


@pytest.mark.parametrize("a_bytes,wn", [(L.A_BYTES, 0), (A_BYTES_64, 0), (A_BYTES_64, 1)])
@pytest.mark.parametrize("j", range(6))
@pytest.mark.parametrize("plane", range(3))
def test_w_row_fragment_reads_conflict_free(a_bytes, wn, j, plane):
    assert conflict_free("read_b128", lambda l: L.w_row_fragment_address(l, wn, j, plane, a_bytes))
    # ... in each ring slot of either tile (the stage sizes keep the 256-byte bank phase)
    assert (L.A_BYTES + L.B_BYTES) % 256 == 0 and (A_BYTES_64 + 2 * L.B_BYTES) % 256 == 0
