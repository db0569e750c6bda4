"""Developer tool: record tests/golden/closure_bits.npz, the bit-exact closure and fit results that
tests/test_gpu_closure_bits.py compares against.  Run it on the GPU at the commit whose bits are to be kept:
    python tools/record_closure_bits.py [output.npz]
The inputs are made without the GPU (tests/closure_bits_cases.py) and stored with the results; the script asserts that the
third point drops both the pose prior (> 5e4) and the angle prior (> 1e4) in the L2 and GMM modes and that another keeps both."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from tests import closure_bits_cases as cb  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else cb.GOLDEN
inp = cb.make_inputs()
for mode in ('l2', 'gmm'):
    drops = [cb.prior_drops(inp, mode, k) for k in range(4)]
    print(mode, '(pose, angle) prior dropped, per point and problem:', drops)
    assert all(p and a for p, a in drops[2]), ('point 2 must drop both priors in every problem', mode, drops[2])
    assert any(not p and not a for d in drops for p, a in d), ('some point must keep both priors', mode, drops)
rec = dict(inp)
for mode in cb.MODES:
    rec['loss_' + mode], rec['grad_' + mode] = cb.run_closures(inp, mode)
    assert np.isfinite(rec['loss_' + mode]).all() and np.isfinite(rec['grad_' + mode]).all(), mode
rec.update(cb.run_fit(inp))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
np.savez_compressed(out_path, **rec)
print('wrote', out_path, os.path.getsize(out_path), 'bytes; fit closures', rec['fit_n_closure'], 'iterations', rec['fit_n_iter'],
      'final', rec['fit_final_loss'])
