"""explainn_amd.strands without a device: the two argument checks against their exact texts, and the
[Fwd, Rev, Mean, Max] stack against numpy, bit for bit."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from explainn_amd.strands import as_codes_1d, check_strands, stack_strands  # noqa: E402


def test_as_codes_1d_takes_arrays_and_tensors_and_refuses_the_rest():
    codes = np.array([0, 1, 2, 3, 4, 0], dtype=np.uint8)
    for given in (codes, codes[::2], torch.from_numpy(codes)):
        got = as_codes_1d(given)
        assert torch.is_tensor(got) and got.dtype == torch.uint8 and got.dim() == 1
        assert np.array_equal(got.numpy(), np.asarray(given))
    t = torch.from_numpy(codes)
    assert as_codes_1d(t) is t
    for bad in (codes.astype(np.int64), codes.reshape(2, 3), torch.zeros(4), torch.zeros((2, 2), dtype=torch.uint8)):
        with pytest.raises(ValueError) as e:
            as_codes_1d(bad)
        assert str(e.value) == "codes must be a 1-D uint8 array of base codes"


def test_check_strands():
    check_strands("both")
    check_strands("fwd")
    for bad in ("rev", "Both", None, 2):
        with pytest.raises(ValueError) as e:
            check_strands(bad)
        assert str(e.value) == "strands must be 'both' or 'fwd' (got %r)" % (bad,)


@pytest.mark.parametrize("shape", [(3, 2), (3, 2, 2)])
def test_stack_strands_equals_numpy(shape):
    rng = np.random.default_rng(len(shape))
    a = (rng.standard_normal(shape) * 10).astype(np.float32)
    b = (rng.standard_normal(shape) * 10).astype(np.float32)
    b.flat[0] = a.flat[0]                               # a tie, and a pair whose sum rounds
    a.flat[1], b.flat[1] = np.float32(1.0), np.float32(2.0 ** -24)
    want = np.stack((a, b, (a + b) / np.float32(2), np.maximum(a, b)), axis=-1)
    assert want.dtype == np.float32
    got = stack_strands(torch.from_numpy(a), torch.from_numpy(b))
    assert got.dtype == torch.float32 and tuple(got.shape) == shape + (4,)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    mid = stack_strands(torch.from_numpy(a), torch.from_numpy(b), dim=1).numpy()
    assert np.array_equal(mid.view(np.uint32), np.stack((a, b, (a + b) / np.float32(2), np.maximum(a, b)),
                                                        axis=1).view(np.uint32))
