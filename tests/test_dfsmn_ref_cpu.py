"""The float64 restatements of tests/_dfsmn_ref.py pinned to oracle.dfsmn with no device: the commuted seam of csrc/dfsmn_cfb.hip (y1 without
LayerNorm 1, the statistics applied behind the (3,1) conv) gives oracle.dfsmn.cfb in float64 within 1e-12 x the tensor's scale."""
import numpy as np
import pytest
import torch

import vadx  # noqa: F401
from vadx import weights
from oracle import dfsmn as od

import _dfsmn_ref as ref

TOL = 1e-12


@pytest.fixture(scope="module")
def w64():
    w = weights.dfsmn_synthetic(1234)
    return {k[len("iccrn."):]: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in w.items() if k.startswith("iccrn.")}


@pytest.fixture(scope="module")
def tb64():
    return od.CepsTables(torch.float64)


def block_input(cin, frames):
    g = torch.Generator().manual_seed(100 * cin + frames)
    x = torch.randn(1, cin, od.F_BINS, frames, generator=g, dtype=torch.float64)
    return x * torch.tensor([1.0, 0.1, 0.01], dtype=torch.float64)[torch.arange(frames) % 3] + 25.0 * (frames == 5)


@pytest.mark.parametrize("frames", [1, 5, 17])
@pytest.mark.parametrize("name,cin", [("cfb_e1", 20), ("cfb_d3", 40)])
def test_front_lstm_back_is_the_oracles_block(w64, tb64, name, cin, frames):
    x = block_input(cin, frames)
    with torch.no_grad():
        want = od.cfb(x, w64, name, tb64)
        fr = ref.cfb_front(x, w64, name, tb64)
        cu = name + ".ceps_unit"
        lo = od.ch_lstm_f(od.layer_norm(fr["S"], w64, cu + ".LN"), w64, cu + ".ch_lstm_f", 40, 20, 40, od.CEPS_F)
        got = ref.cfb_back(fr["S"], fr["y1"], fr["stats1"], w64, name, tb64, lo=lo)
        # the same through the hidden states, the tensor the device hands from lstm_f to cfb_back, with LayerNorm from the statistics rows
        hf = ref.lstm_f_hidden(fr["S"], fr["stats_li"], w64, cu)
        got_hf = ref.cfb_back(fr["S"], fr["y1"], fr["stats1"], w64, name, tb64, hf=hf)
    scale = float(want.abs().max())
    assert want.shape == got.shape == (1, 20, od.F_BINS, frames) and fr["S"].shape == (1, 40, od.CEPS_F, frames)
    assert float((got - want).abs().max()) <= TOL * scale
    assert float((got_hf - want).abs().max()) <= TOL * scale
    assert float((ref.lstm_f_linear(hf, w64, cu) - lo).abs().max()) <= TOL * float(lo.abs().max())


@pytest.mark.parametrize("frames", [1, 5, 17])
def test_statistics_rows_are_torchs_mean_and_std(w64, tb64, frames):
    x = block_input(20, frames)
    with torch.no_grad():
        fr = ref.cfb_front(x, w64, "cfb_e1", tb64)
    for key, src in (("stats1", "gx"), ("stats_li", "S")):
        t = fr[src][0].reshape(-1, frames)
        assert fr[key].shape == (frames, 2)
        torch.testing.assert_close(fr[key][:, 0], t.mean(0), rtol=1e-13, atol=0)
        torch.testing.assert_close(fr[key][:, 1], 1.0 / (t.std(0, unbiased=True) + 1e-6), rtol=1e-13, atol=0)
    # and LayerNorm from the rows is the oracle's LayerNorm
    p = "cfb_e1.ceps_unit.LN"
    ln = ref.layer_norm_from(fr["S"], fr["stats_li"], w64, p)
    assert float((ln - od.layer_norm(fr["S"], w64, p)).abs().max()) <= TOL * float(ln.abs().max())


def test_error_figures_show_a_quiet_frame():
    """`frame` is taken per frame against that frame's own maximum: an error of 1e-3 of a frame 100 times quieter than its neighbour is
    1e-5 in `all` and 1e-3 in `frame`; a frame whose reference is identically zero is left out of both and reported on its own."""
    y64 = torch.zeros(2, 3, 4, 3, dtype=torch.float64)
    y64[0, :, :, 0], y64[0, :, :, 1] = 1.0, 0.01
    y = y64.clone().float()
    y[0, 1, 2, 1] += 1e-5
    e_all, e_frame, scale, dead = ref.rel_errors(y, y64)
    assert scale == 1.0 and abs(e_all - 1e-5) < 1e-9 and abs(e_frame - 1e-3) < 1e-7 and dead == 0.0
    y[1, 0, 0, 2] = 0.5
    assert ref.rel_errors(y, y64) == (0.5, e_frame, 1.0, 0.5)
