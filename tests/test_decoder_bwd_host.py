"""Where k = LSTM_BWD_K of test_gpu_decoder_bwd_ops.py comes from, without a GPU: the ConvLSTM pointwise backward (the formulas at the top
of csrc/pointwise.hip) evaluated in numpy float32 -- one rounding per operation, a correctly-rounded-to-1-ulp tanh -- against the same
expressions in float64, per element in units of 2^-24 * helpers.lstm_bwd_scales(..).  This is a condition on the REFERENCE and the bars
alone: if plain fp32 arithmetic needed more than 8 units the bars would be measuring the data, not the kernel.

Budget of k = 24: the fp32 evaluation itself stays below 8 here (about 5 observed); tanhf at 2 ulp instead of 1 moves tc by 2^-23 next
to 1, so tc^2 by 2^-22 and 1 - tc^2 -- charged at (|dh| + |dh2|) o <= M -- by up to ~8 units more; the rest is headroom for the order in
which a compiler contracts the products."""
import numpy as np
import pytest

from helpers import LSTM_BWD_OUTS, lstm_bwd_eval, lstm_bwd_inputs, lstm_bwd_ratios


@pytest.mark.parametrize("c_scale", [1.0, 4.0])
def test_fp32_evaluation_stays_within_8_units_of_the_float64_reference(c_scale):
    q = lstm_bwd_inputs(7 + int(c_scale), 8, 64, 4096, c_scale)            # 2 M samples
    worst = lstm_bwd_ratios(lstm_bwd_eval(q, np.float32), q)
    print("\nLSTM-BWD host fp32 vs float64, c scale %g: worst ratio per output %s" % (c_scale, {k: round(v, 2) for k, v in worst.items()}))
    assert set(worst) == set(LSTM_BWD_OUTS)
    assert max(worst.values()) <= 8.0, worst


@pytest.mark.parametrize("form", ["t0", "last"])
def test_absent_operands_and_non_finite_state_on_the_host(form):
    """the reference's own handling of what the GPU test feeds it: absent operands are zeros, c = +-inf / +-1e30 gives tanh = +-1 and
    1 - tanh^2 = 0, and every reference output stays finite"""
    q = lstm_bwd_inputs(11, 2, 4, 20, 4.0)
    for k in (("c_prev",) if form == "t0" else ("dh2", "dc_next")):
        q[k] = None
    q["c"].reshape(-1)[:4] = [np.inf, -np.inf, 1e30, -1e30]
    ref = lstm_bwd_eval(q)
    assert all(np.isfinite(v).all() for v in ref.values())
    if form == "t0":
        assert not ref["da_f"].any()
    else:
        assert not ref["dc_prev"].reshape(-1)[:4].any() and not ref["da_i"].reshape(-1)[:4].any()
    assert max(lstm_bwd_ratios(lstm_bwd_eval(q, np.float32), q).values()) <= 8.0
