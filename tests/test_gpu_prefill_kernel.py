"""GPU: prefill_store_kernel alone (wb_prefill_store) on canary-filled caller arrays, at the three shapes of
prefill_ref.STORE_SHAPES (one row; a padded leading dimension with fewer active windows than slots; two 33-row windows in a
16-slot cache): K and V rows bit-exact at p * S + a, table entries exact in parity (n - 1) & 1, every other word of the three
arrays still its canary."""
import pytest

import prefill_ref as pf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", pf.STORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_store_kernel_against_canaries(shape):
    pf.check_store_case(shape)


def test_store_kernel_refuses_what_it_does_not_serve():
    import numpy as np
    import whisper_burn_amd as wb
    K, V, tabs = np.zeros((8, 64), np.float32), np.zeros((8, 64), np.float32), np.zeros((2, 1, 8), np.int32)
    for nA, n, ld in ((2, 1, 192), (1, 9, 192), (1, 1, 190), (1, 1, 128)):        # nA > S, n > Lmax, ld % 4, ld < 3 d
        with pytest.raises(wb.WbError) as e:
            wb.prefill_store(np.zeros((nA * n, ld), np.float32), nA, n, 64, 1, 8, K, V, tabs)
        assert e.value.status == -2
    assert not K.any() and not V.any() and not tabs.any()
