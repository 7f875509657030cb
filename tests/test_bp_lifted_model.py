"""The layered min-sum model (tests/bp_lnms_model.py) on the lifted BG2 codes:
the stream of tests/lifted_codes.py leaves both outcomes, so the GPU tests that
hold the kernels to the models on it (tests/test_gpu_lifted.py) see codewords
that stop early and codewords that use the whole budget."""
import numpy as np
import pytest

import lifted_codes as LC
from bp_lnms_model import lnms_model

# Z: (B, converged, blocks with a wrong info bit, mean sweeps): deterministic CPU results of the numpy model at
# snr -2.0 dB, 25 sweeps, alpha 0.75 (other values mean the stream or the contract was built differently)
EXPECTED = {128: (128, 84, 43, 18.5625), 288: (32, 26, 5, 17.9375)}


@pytest.mark.parametrize("Z", list(EXPECTED))
def test_stream_has_both_outcomes(data_dir, tmp_path, Z):
    B, conv_want, fail_want, sweeps_want = EXPECTED[Z]
    _, g = LC.graph(data_dir, Z, tmp_path)
    st = {}
    ret, uh, cch = lnms_model(g, LC.p0_stream(g.cc_len, B), LC.MAX_ITER, LC.MAX_ITER, 0.75, stats=st)
    conv, failed = int(st["converged"].sum()), int(uh.any(axis=1).sum())  # (the all-zero codeword was sent)
    print(f"Z = {Z}: {conv} of {B} converged, {failed} failed blocks, mean {st['iters'].mean():.2f} sweeps")
    assert conv >= 0.1 * B and failed >= 0.1 * B  # the conditions the stream was chosen for
    assert st["finite"]
    assert (conv, failed, float(st["iters"].mean())) == (conv_want, fail_want, sweeps_want)
