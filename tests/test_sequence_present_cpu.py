"""CPU: fit_sequences(present=...) with a fake engine whose "fit" adds one to the betas and returns loss 1: which frames
are fitted, from which start, and that absent frames leave a sequence's carried state alone."""
import numpy as np
import torch

from mvsmplfitting_amd.engine import stage_weights
from mvsmplfitting_amd.sequence import fit_sequences


class FakeEngine:
    device = torch.device('cpu')

    def __init__(self):
        self.batches = []

    def set_problems(self, cams, gt_xy, w_conf):
        self.B = gt_xy.shape[0]

    def fit(self, x, stages):
        assert x.shape[0] == self.B
        self.batches.append((x.shape[0], len(stages)))
        out = x.clone()
        out[:, :10] += 1.0
        return out, dict(final_loss=torch.ones(self.B), n_closure=torch.full((self.B,), 7, dtype=torch.int32))


def _inputs(S, T):
    rng = np.random.default_rng(0)
    cams = (np.zeros((2, 3, 3), np.float32), np.zeros((2, 3), np.float32), np.ones(2, np.float32), np.zeros((2, 2), np.float32))
    x_init = rng.normal(0, 1, (S, T, 118)).astype(np.float32)
    return cams, np.zeros((S, T, 2, 17, 2), np.float32), np.ones((S, T, 2, 17), np.float32), x_init


def test_present_none_and_all_true_agree():
    cams, gt, wc, xi = _inputs(2, 3)
    st = stage_weights(1536.0)
    a, sa = fit_sequences(FakeEngine(), cams, gt, wc, xi, st)
    b, sb = fit_sequences(FakeEngine(), cams, gt, wc, xi, st, present=np.ones((2, 3), bool))
    assert torch.equal(a, b) and np.array_equal(sa['restarted'], sb['restarted'])
    assert torch.equal(sa['final_loss'], sb['final_loss']) and torch.equal(sa['n_closure'], sb['n_closure'])


def test_absent_frames_are_skipped_and_do_not_touch_the_chain():
    cams, gt, wc, xi = _inputs(3, 3)
    st = stage_weights(1536.0)
    present = np.array([[1, 1, 1], [0, 1, 1], [1, 0, 1]], bool)
    eng = FakeEngine()
    x, s = fit_sequences(eng, cams, gt, wc, xi, st, present=present)
    x = x.numpy()
    assert np.array_equal(np.isnan(x).all(2), ~present)
    assert np.array_equal(np.isnan(s['final_loss'].numpy()), ~present)
    assert np.array_equal(s['n_closure'].numpy(), np.where(present, 7, 0))
    # a sequence starts cold at its first present frame, warm afterwards - also across a gap
    assert np.array_equal(s['restarted'], np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0]], bool))
    # cold: the frame's own initial guess; warm: betas carried from the last PRESENT frame
    assert np.array_equal(x[1, 1, :10], xi[1, 1, :10] + 1)
    assert np.array_equal(x[1, 2, :10], x[1, 1, :10] + 1)
    assert np.array_equal(x[2, 2, :10], x[2, 0, :10] + 1)
    assert np.array_equal(x[2, 2, 13:82], xi[2, 2, 13:82])          # the body pose is not carried over
    # batches: t = 0 two cold; t = 1 one cold + one warm; t = 2 three warm
    assert [b for b, _ in eng.batches] == [2, 1, 1, 3]
    # sequence 0 is what it is alone
    alone, _ = fit_sequences(FakeEngine(), cams, gt[:1], wc[:1], xi[:1], st)
    assert np.array_equal(alone.numpy()[0], x[0])
