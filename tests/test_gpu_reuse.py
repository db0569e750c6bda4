"""GPU: the opt-in MVFIT_F_REUSE_OUTER_VALUE (include/mvfit.h) - LBFGS.step() opens with a closure call
(lbfgs_ls.py:279-283) at the point the previous step() of the same stage ended on; with the flag the device optimiser
feeds the loss / gradient it still holds instead of evaluating again.  It must not change a single iterate: parameters
and final losses bit-identical to the default fit, only the closure count drops (by the number of skipped calls)."""
import numpy as np
import pytest

from mvsmplfitting_amd import _lib
from mvsmplfitting_amd import synthetic as syn
from mvsmplfitting_amd.engine import MvFit, stage_weights
from tests.test_gpu_async import _setup
from tests.test_gpu_vposer_service import _problems

pytestmark = pytest.mark.gpu


def _check_no_iterate_changes(eng, x0, base):
    xa, sa = eng.fit(x0, stage_weights(1536.0, flags=base))
    xb, sb = eng.fit(x0, stage_weights(1536.0, flags=base | _lib.F_REUSE_OUTER_VALUE))
    assert np.array_equal(xa.cpu().numpy(), xb.cpu().numpy())
    assert np.array_equal(sa['final_loss'].cpu().numpy(), sb['final_loss'].cpu().numpy())
    assert np.array_equal(sa['n_iter'].cpu().numpy(), sb['n_iter'].cpu().numpy())
    na, nb = sa['n_closure'].cpu().numpy(), sb['n_closure'].cpu().numpy()
    assert np.all(nb < na) and np.all(nb > 0.8 * na), (na, nb)          # 8-10 % of the calls are step-start re-evaluations


@pytest.mark.parametrize('sparse', [False, True])
def test_reuse_of_the_step_start_value_changes_no_iterate(sparse):
    eng, x0 = _setup(B=7)
    _check_no_iterate_changes(eng, x0, _lib.F_SPARSE_VERTS if sparse else 0)
    eng.close()


@pytest.mark.parametrize('prior', ['plain', 'gmm', 'vposer'])
def test_reuse_in_every_single_launch_kernel_that_has_it(prior):
    """The objective-vertices-only fit with the flag runs another instantiation of the single-launch kernel per prior
    (csrc/fit_plan.h: PV_REUSE_LEAN without a prior term, PV_REUSE with the GMM, PV_HELPERS_REUSE with the VPoser decoder on
    helper workgroups): each is launched here, on the synthetic body, and held to the same statement."""
    eng = MvFit(syn.make_body_model(0, skin_topk=4), vposer=syn.make_vposer_decoder() if prior == 'vposer' else None,
                gmm=syn.gmm_constants(syn.make_gmm(), np.float32) if prior == 'gmm' else None)
    x0 = _problems(eng, 3)[0]
    if prior == 'vposer':
        eng.set_options(vposer_helpers=1)
    _check_no_iterate_changes(eng, x0, _lib.F_SPARSE_VERTS | dict(plain=0, gmm=_lib.F_PRIOR_GMM, vposer=_lib.F_VPOSER)[prior])
    if prior == 'vposer':
        assert eng.decoder_stats()['launches'] == 1          # (the last fit: the helpers really rode on it)
    eng.close()
