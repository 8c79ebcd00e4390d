"""mi355x_moe_route on the device against tests/moe_ref.py, by bits: the probabilities, the selected
experts (ties as ggml's exchange sort leaves them) and the normalised weights; random rows, two identical
router rows (tied probabilities) and a row with one dominant logit (a weight of 1.0, denormal others).
The words after each record stay untouched."""
import numpy as np
import pytest
import torch

import ggml_mi355x as g
from tests import moe_ref as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 0x5A5A5A5A
F32 = np.float32


def _inputs(n_embd, n_expert, T, seed):
    rng = np.random.default_rng([seed, n_embd, n_expert, T])
    gi = (rng.standard_normal((n_expert, n_embd)) * 2.0 / np.sqrt(n_embd)).astype(F32)
    x = rng.standard_normal((T, n_embd)).astype(F32)
    # two identical router rows: their probabilities tie bit for bit, in every row of x
    gi[n_expert - 1] = gi[0]
    if T > 1:
        # one dominant logit: the last row of x is along router row 1, its logit ~ 100 and the others' a few units
        # (the others' probabilities are float32 denormals or tiny; with 2 experts rows 0 and 1 are the tied pair)
        x[T - 1] = gi[1] * F32(100.0 / float((gi[1].astype(np.float64) ** 2).sum()))
    return gi, x


@pytest.mark.parametrize("n_embd", [256, 512])
@pytest.mark.parametrize("n_expert,n_used", [(2, 1), (2, 2), (8, 1), (8, 2), (8, 8), (64, 1), (64, 2), (64, 8)])
@pytest.mark.parametrize("T", [1, 3])
def test_route_matches_the_rule(n_embd, n_expert, n_used, T):
    gi, x = _inputs(n_embd, n_expert, T, 11)
    stride = 2 * n_used + 3  # three guard words after each record
    rec = torch.full((T, stride), GUARD, dtype=torch.int32, device=DEV)
    xd = torch.zeros((T, n_embd + 16), dtype=torch.float32, device=DEV)  # strided rows
    xd[:, :n_embd] = torch.from_numpy(x).to(DEV)
    _, probs = g.moe_route(torch.from_numpy(gi).to(DEV), xd[:, :n_embd], n_used, records=rec, probs=True)
    torch.cuda.synchronize()
    rec, probs = rec.cpu().numpy(), probs.cpu().numpy()
    saw_tie = False
    for t in range(T):
        ids, w, p = M.route(gi, x[t], n_used)
        assert (probs[t].view(np.uint32) == p.view(np.uint32)).all(), (t, probs[t], p)
        assert p[0].view(np.uint32) == p[n_expert - 1].view(np.uint32)
        saw_tie |= 0 in ids.tolist() or (n_expert - 1) in ids.tolist()
        assert rec[t, :n_used].tolist() == ids.tolist(), (t, rec[t], ids)
        assert (rec[t, n_used:2 * n_used].view(np.uint32) == w.view(np.uint32)).all(), (t, w)
        assert (rec[t, 2 * n_used:] == GUARD).all()
    if n_used == n_expert:
        assert saw_tie


def test_dominant_logit_and_ties_in_the_selection():
    """A row whose soft_max is 1.0 for one expert and denormal or zero for the rest (the weight is exactly
    1.0 at n_used 1; the rest tie at tiny values and come out in the exchange sort's order), and a row of
    all-equal logits (nothing swaps: ids 0 .. n_used - 1)."""
    n_embd, n_expert = 256, 8
    gi = np.zeros((n_expert, n_embd), F32)
    gi[:, 0] = [0.0, 0.0, 100.0, 1.0, 0.0, 1.0, 0.0, 0.0]
    x = np.zeros((3, n_embd), F32)
    x[0, 0] = 1.0    # logits 0 0 100 1 0 1 0 0: exp(-100), exp(-99) are denormal / tiny
    x[1, 0] = 1.03   # 103: exp(-103) is a float32 denormal
    x[2, 0] = 0.0    # all logits 0: all probabilities 0.125
    for n_used in (1, 2, 8):
        rec, probs = g.moe_route(torch.from_numpy(gi).to(DEV), torch.from_numpy(x).to(DEV), n_used, probs=True)
        torch.cuda.synchronize()
        rec, probs = rec.cpu().numpy(), probs.cpu().numpy()
        for t in range(3):
            ids, w, p = M.route(gi, x[t], n_used)
            assert (probs[t].view(np.uint32) == p.view(np.uint32)).all(), (t, probs[t], p)
            assert rec[t, :n_used].tolist() == ids.tolist(), (t, n_used, rec[t], ids)
            assert (rec[t, n_used:].view(np.uint32) == w.view(np.uint32)).all()
        assert probs[0, 2] == F32(1.0) and rec[0, 0] == 2
        assert 0 < M.route(gi, x[1], 1)[2][0] < np.finfo(F32).tiny  # the rule's own value: a denormal probability
        if n_used == 1:
            assert rec[0, 1:2].view(F32)[0] == F32(1.0)
        assert rec[2, :n_used].tolist() == list(range(n_used))
