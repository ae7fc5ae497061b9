"""Host check of the transforms of the Δ+ΔΔ feature path (engine.check_delta_fmllr): what it refuses never reaches a kernel
that indexes the array by (speaker row, 3·dim, 3·dim+1) alone.  No device needed: the check runs before any launch."""
import numpy as np
import pytest
import torch

from montreal_forced_aligner_amd._lib import MfaHipError
from montreal_forced_aligner_amd.engine import check_delta_fmllr


@pytest.mark.parametrize("shape, dtype, utt2spk, why", [
    ((3, 40, 41), torch.float32, [0, 1, 2], "do not fit"),          # the LDA path's size
    ((3, 39, 39), torch.float32, [0, 1, 2], "do not fit"),          # no offset column
    ((39, 40), torch.float32, None, "do not fit"),                  # one matrix, not a stack
    ((2, 39, 40), torch.float32, [0, 2, 1], "2 fMLLR transforms for speaker rows up to 2"),
    ((0, 39, 40), torch.float32, None, "0 fMLLR transforms for speaker rows up to 0"),   # no utt2spk: row 0 is read
    ((3, 39, 40), torch.float64, [0, 1, 2], "float32"),
    ((3, 39, 40), torch.float32, [0, -1, 2], "negative speaker row"),
])
def test_refused(shape, dtype, utt2spk, why):
    with pytest.raises(MfaHipError, match=why):
        check_delta_fmllr(torch.zeros(shape, dtype=dtype), 13, None if utt2spk is None else np.asarray(utt2spk))


def test_refuses_numpy_and_strided_input():
    with pytest.raises(MfaHipError, match="float32 tensor"):
        check_delta_fmllr(np.zeros((3, 39, 40), np.float32), 13, None)
    with pytest.raises(MfaHipError, match="contiguous"):
        check_delta_fmllr(torch.zeros((3, 39, 80))[:, :, :40], 13, None)


def test_a_fitting_stack_passes_up_to_the_device_test():
    """Shape, dtype and rows in order: what is left to refuse is a tensor that is not on the device."""
    with pytest.raises(MfaHipError, match="on the device"):
        check_delta_fmllr(torch.zeros((3, 48, 49)), 16, np.array([2, 0, 1]))
