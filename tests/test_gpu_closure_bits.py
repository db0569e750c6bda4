"""The closure and the fit keep their bits: loss and gradient at four points (the start, a small step, a pose that drops both
priors, joints at exactly zero with bent elbows and knees) in the L2, GMM and VPoser modes, and one complete 4-stage L2 fit,
compared word for word with tests/golden/closure_bits.npz.

The file was recorded with tools/record_closure_bits.py at commit 0cdd649 ("Fit the persons of a scene together: frozen-field
collision term"), before the Rodrigues adjoint of E9 was rewritten with every product and sum stated.  A change that is MEANT
to alter result bits re-records the file with that tool and says so; anything else must leave it alone."""
import numpy as np
import pytest

from tests import closure_bits_cases as cb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(cb.GOLDEN))


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('mode', cb.MODES)
def test_closure_bits(golden, mode):
    loss, grad = cb.run_closures(golden, mode)
    for k in range(loss.shape[0]):
        dl = int((_words(loss[k]) != _words(golden['loss_' + mode][k])).sum())
        dg = int((_words(grad[k]) != _words(golden['grad_' + mode][k])).sum())
        print('%s point %d: loss words differing %d of %d, gradient words differing %d of %d'
              % (mode, k, dl, loss[k].size, dg, grad[k].size))
    assert np.array_equal(_words(loss), _words(golden['loss_' + mode]))
    assert np.array_equal(_words(grad), _words(golden['grad_' + mode]))


def test_fit_bits(golden):
    r = cb.run_fit(golden)
    print('closures', r['fit_n_closure'], 'iterations', r['fit_n_iter'], 'final', r['fit_final_loss'])
    assert np.array_equal(r['fit_n_closure'], golden['fit_n_closure'])
    assert np.array_equal(r['fit_n_iter'], golden['fit_n_iter'])
    assert np.array_equal(_words(r['fit_x']), _words(golden['fit_x']))
    assert np.array_equal(_words(r['fit_final_loss']), _words(golden['fit_final_loss']))
