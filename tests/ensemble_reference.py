"""The numpy reference of the ensemble's vote (include/sgk.h: sgk_members_vote), written from the header's contract and from nothing
else. tests/test_ensemble_abi.py checks it against hand-written cases; the library's host and device code is then compared with it,
exactly."""
import numpy as np


def vote(member_actions, members=None, live=None):
    """member_actions uint8 [M, N] -> (actions uint8 [N], votes uint16 [N, 4], dissent int64 [2]). votes[e][a] = the voters (all members,
    or those listed in `members`) whose action on env e is a; actions[e] = the first a with the largest count (np.argmax); dissent =
    (sum of voters - votes[action], sum of voters) over the envs with live[e] (default: all)."""
    a = np.asarray(member_actions, dtype=np.uint8)
    rows = a if members is None else a[np.asarray(list(members), dtype=np.int64)]
    votes = np.stack([(rows == k).sum(axis=0) for k in range(4)], axis=1).astype(np.uint16)
    actions = votes.argmax(axis=1).astype(np.uint8)
    live = np.ones(a.shape[1], dtype=bool) if live is None else np.asarray(live).astype(bool)
    total = votes.sum(axis=1, dtype=np.int64)
    won = votes[np.arange(a.shape[1]), actions].astype(np.int64)
    return actions, votes, np.array([((total - won) * live).sum(), (total * live).sum()], dtype=np.int64)
