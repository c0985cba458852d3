"""The V^T image of the exact-split attention kernel (csrc/attn_f32_split.hip, vt128_off) in the LDS bank model of
tools/lds_banks.py: a bijection, conflict-free ds_read_b128 fragment reads, the closed-form fragment address the kernel uses, and
the (4-way) cost of the staging writes.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from lds_banks import conflict_free, cycles  # noqa: E402


def vt128_off(d, key):
    """csrc/attn_f32_split.hip: [32 d][128 keys] bf16, 256-byte rows, the 16-byte chunk (8 keys) XOR-ed with d & 15."""
    return d * 256 + ((((key >> 3) ^ d) & 15) << 4) + (key & 7) * 2


def test_image_is_a_bijection_onto_the_plane():
    offs = {vt128_off(d, k) for d in range(32) for k in range(128)}
    assert len(offs) == 32 * 128 and min(offs) == 0 and max(offs) == 32 * 256 - 2
    assert all(o % 2 == 0 for o in offs)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("u", [0, 1, 2, 3])
def test_fragment_reads_conflict_free_and_in_closed_form(dt, u):
    """PV k-step u, d-tile dt: lane (lq = l & 15, lg = l >> 4) reads V^T[d = 16dt + lq][keys 32u + 8lg .. +7]; the kernel forms the
    address as 256 lq + (16 ((lg ^ lq) & 15) ^ 64u) + 4096 dt."""
    addr = lambda l: vt128_off(16 * dt + (l & 15), 32 * u + 8 * (l >> 4))
    assert conflict_free("read_b128", addr)
    for l in range(64):
        lq, lg = l & 15, l >> 4
        assert addr(l) == 256 * lq + ((((lg ^ lq) & 15) << 4) ^ (64 * u)) + 4096 * dt
        assert addr(l) % 16 == 0 and addr(l) + 16 <= 32 * 256


def test_staging_writes_four_way():
    """Staging unit f of a wave's 64 threads: keys 2 (f >> 3), 2 (f >> 3) + 1 packed in one dword, dims 4 (f & 7) + e.  The eight
    dim quads of a key pair fall on four chunk swizzles, two of which share the 32 banks a write sees: each ds_write_b32 takes 4 x
    the conflict-free cycles.  Known and accepted: 36 such writes per thread against 114 MFMAs and 51 fragment reads per query
    tile; the reads are what the image is laid out for."""
    for first in range(0, 512, 64):
        for e in range(4):
            c, n = cycles("write_b32", lambda l: vt128_off(4 * ((first + l) & 7) + e, 2 * ((first + l) >> 3)))
            assert c == 4 * n
