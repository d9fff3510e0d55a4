"""The consensus of private tabular-Q agents (include/sgk.h: sgk_tabq_consensus) restated in numpy: agent e votes in state s iff it
may (mask[e] != 0) and its row has an entry != 0 (-0.0 is zero: an unlearnt row is no opinion); its vote is np.argmax of the row."""
import numpy as np


def vote(tables, mask=None):
    """tables float64 [A, S, 4], mask [A] or None -> (votes int64 [S, 4], voters int64 [S])."""
    t = np.asarray(tables, dtype=np.float64)
    may = np.ones(t.shape[0], dtype=bool) if mask is None else np.asarray(mask) != 0
    voting = (t != 0.0).any(axis=2) & may[:, None]
    action = t.argmax(axis=2)  # the first maximum
    votes = np.stack([((action == a) & voting).sum(axis=0) for a in range(4)], axis=1).astype(np.int64)
    return votes, voting.sum(axis=0).astype(np.int64)


def policy(votes):
    """uint8 [S]: the first action with the most votes, 0 where nobody voted."""
    return np.asarray(votes).argmax(axis=1).astype(np.uint8)
