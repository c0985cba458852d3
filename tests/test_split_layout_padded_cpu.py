"""The padded statement of the exact-split weight image (split_layout.image_index_padded: the image written by
pangu_split_weight_bf16x3_padded) -- pure Python, no GPU."""
import pytest

from pangu_pytorch_amd import split_layout as L


@pytest.mark.parametrize("N,K", [(160, 384), (64, 384), (4, 16), (196, 48), (192, 32), (384, 16)])
def test_padded_index_is_a_bijection(N, K):
    """(plane, row 0 .. Npad-1, k) -> every one of the 6 Npad K / 2 bf16 slots exactly once."""
    Np = L.padded_rows(N)
    assert Np % 192 == 0 and Np - 192 < N <= Np and L.served_padded(N, K)
    slots = sorted(L.image_index_padded(N, K, p, n, k) for p in range(3) for n in range(Np) for k in range(K))
    assert slots == list(range(6 * Np * K // 2))


@pytest.mark.parametrize("N,K", [(192, 32), (384, 16), (576, 48)])
def test_padded_index_agrees_with_unpadded(N, K):
    assert L.padded_rows(N) == N and L.served(N, K) and L.served_padded(N, K)
    for p in range(3):
        for n in range(N):
            for k in range(K):
                assert L.image_index_padded(N, K, p, n, k) == L.image_index(N, K, p, n, k)


def test_padded_rows_and_refusals():
    assert [L.padded_rows(n) for n in (4, 160, 192, 196, 384, 388)] == [192, 192, 192, 384, 384, 576]
    assert not L.served_padded(6, 16) and not L.served_padded(160, 24) and not L.served_padded(0, 16)
    assert L.served_padded(160, 384) and not L.served(160, 384)
    # the rows of W keep, in the padded image, the index they have in the image of the zero-extended weight
    assert L.image_index_padded(160, 384, 2, 159, 383) == L.image_index(192, 384, 2, 159, 383)
