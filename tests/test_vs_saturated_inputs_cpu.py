"""The input conditions of tests/test_gpu_vs_saturated.py, asserted on the float32 oracle alone (no GPU): for every
saturated problem of that file, at each of its three steps, every score is at least 10 err away from the decision
points of the clip masks (err = the oracle's own float32-against-float64 error of the scores), the planted values are
met exactly, all gradients are finite, and the shares of saturated and live candidates / units are what the GPU tests
rely on.  vs_reference / fs_reference raise an AssertionError on the first condition that does not hold."""
import numpy as np
import pytest

from tests import test_gpu_vs_saturated as S


@pytest.mark.parametrize('name', list(S.VS_SAT))
def test_saturated_vectorspace_inputs_are_decidable(name):
    r = S.vs_reference(name)
    assert len(r.steps) == S.STEPS == len(r.figures)
    for err, m15, mlo in r.figures:
        assert 0 < err < 1e-4 and m15 >= 10 * err and mlo >= 10 * err, (err, m15, mlo)
    sh = r.shares
    assert sh['above'] >= 0.05 and sh['below'] >= 0.05 and sh['inside'] >= 0.05 and sh['t_out'] >= 0.01 and sh['t_in'] >= 0.30
    print(name, 'sW %g sE %g' % (r.p['sW'], r.p['sE']), {k: round(v, 3) for k, v in sh.items()},
          ['err %.1e margins %.1e %.1e' % f for f in r.figures])


@pytest.mark.parametrize('name', list(S.FS_SAT))
def test_saturated_softmax_inputs_are_decidable(name):
    r = S.fs_reference(S.fs_key(name))
    for err, mlo, mhi in r.figures:
        assert 0 < err < 1e-3 and mlo >= 10 * err and mhi >= 10 * err, (err, mlo, mhi)
    assert r.shares['below'] >= 0.05 and r.shares['inside'] >= 0.05
    assert r.steps[0]['f']['py'][0] == np.float32(1.0)
    print(name, 'sW %g sE %g' % (r.p['sW'], r.p['sE']), {k: round(v, 3) for k, v in r.shares.items()},
          ['err %.1e margins %.1e %.1e' % f for f in r.figures])
