"""The layouts of the exact-split fp32 GEMMs (the image written in csrc/gemm_f32_split.hip, the LDS stage of split_main_loop in
csrc/split_f32.h, its fp32 A part that of csrc/gemm_f32_dma_loop.h), stated in plain Python: the weight image written by
pangu_split_weight_bf16x3, and the LDS stage the kernel reads its MFMA fragments from, under both wave tilings of the loop: 2 x 2
waves of 64 x 96 (a_fragment_address, w_fragment_address: gemm_ln_f32_split.hip at N = 192) and row-owning waves of 32 x 192
(a_row_fragment_address, w_row_fragment_address: gemm_f32_split.hip, gemm_ln_f32_split.hip at N = 384 from K = 1536).  No torch, no GPU: the
tests un-permute an image and check the bank behaviour of the fragment reads with these.

The image of an (N, K) weight (N % 4 == 0, K % 16 == 0) has image_rows(N) rows, whole 192-row n-tile blocks: W's N rows, and behind
them zero rows (+0 in every plane)."""

BM, BN, BK = 128, 192, 16
A_BYTES = BM * 64                 # the fp32 A image of a stage: 128 rows of 64 B (16 floats), 16-B chunks XOR-swizzled
PLANE = 2 * BN * 16               # one bf16 plane of a stage: [k-half][row][8 bf16]
B_BYTES = 3 * PLANE               # hi, mid, lo
STAGE = A_BYTES + B_BYTES
PLANES = ("hi", "mid", "lo")
_F = (0, 2, 3, 1)


def served(N, K):
    return N > 0 and N % 4 == 0 and K % BK == 0


def image_rows(N):
    """Rows of the image of an N-row weight: the next multiple of 192."""
    return -(-N // BN) * BN


def image_index(N, K, plane, n, k):
    """Index (in bf16 elements) of plane `plane` (0 hi, 1 mid, 2 lo) of row n, column k of the image of an (N, K) weight, n in
    0 .. image_rows(N) - 1: [n // 192][k // 16][plane][(k // 8) & 1][n % 192][k % 8]."""
    nt, nl, kt, lh, j = n // BN, n % BN, k // BK, (k // 8) & 1, k % 8
    return (((((nt * (K // BK) + kt) * 3 + plane) * 2 + lh) * BN + nl) * 8) + j


def unpermute(image_u16, N, K):
    """image_u16: the image as a flat sequence of 3 image_rows(N) K bf16 bit patterns -> W's rows as three row-major
    lists-of-lists [plane][n][k]."""
    return [[[image_u16[image_index(N, K, p, n, k)] for k in range(K)] for n in range(N)] for p in range(3)]


def a_chunk_offset(row, chunk):
    """Byte offset in the stage of logical 16-B chunk `chunk` (4 floats: k = 4 chunk ..) of A row `row` (kswz64)."""
    return row * 64 + ((chunk ^ _F[(row >> 2) & 3]) << 4)


def a_fragment_address(lane, wm, i, h):
    """The ds_read_b128 of lane (lr = lane & 31, lh = lane >> 5) for row block i (0, 1) of wave row wm (0, 1): half h (0, 1) of
    its 8 consecutive k = 8 lh .. 8 lh + 7 of row 64 wm + 32 i + lr."""
    return a_chunk_offset(wm * 64 + i * 32 + (lane & 31), 2 * (lane >> 5) + h)


def w_fragment_address(lane, wn, j, plane):
    """The ds_read_b128 of the lane for column block j (0..2) of wave column wn (0, 1): the 8 bf16 k = 8 lh .. 8 lh + 7 of `plane`
    of tile row 96 wn + 32 j + lr."""
    return A_BYTES + plane * PLANE + ((lane >> 5) * BN + wn * 96 + j * 32 + (lane & 31)) * 16


def a_row_fragment_address(lane, wm, h):
    """Row-owning wave tiling (SplitTile<.., ROWS = true>): the ds_read_b128 of the lane for the ONE 32-row block of wave row wm
    (0..3 in the 128-row tile, 0..1 in the 64-row tile): half h of its 8 consecutive k of row 32 wm + lr."""
    return a_chunk_offset(wm * 32 + (lane & 31), 2 * (lane >> 5) + h)


def w_row_fragment_address(lane, wn, j, plane, a_bytes=A_BYTES):
    """Row-owning wave tiling: the ds_read_b128 of the lane for column tile j (0..5) of wave column wn, whose columns are the
    whole n-tile block wn of the stage (wn = 0 in the 128 x 192 tile; 0, 1 in the 64 x 384 tile, a_bytes = 64 * 64): the 8 bf16
    k = 8 lh .. 8 lh + 7 of `plane` of block row 32 j + lr."""
    return a_bytes + wn * B_BYTES + plane * PLANE + ((lane >> 5) * BN + j * 32 + (lane & 31)) * 16


def dma_piece_destination(q, lane):
    """LDS byte each lane of LDS-DMA piece q (0..25, 1 KB each) fills: linear."""
    return q * 1024 + lane * 16
