"""PPOCRMDPAgent's corrupt-reward detection (reference spiky/agents.py:74-270) restated on integer keys and integer rewards with Python
dictionaries, sets and lists -- include/sgk.h's "detect" and "merge" of sgk_crmdp_filter, written for reading, not speed. It never calls
the product: the CPU tests hold it to the reference's recorded output (tests/golden/crmdp_plans.npz) and the library to it."""
import numpy as np

UNKNOWN, SAFE, CORRUPT = 0, 1, 2
NONE = -2 ** 31


def d_trans_boat(a, b, width, n_cells):
    """d_trans_boat (:41-63) on keys = prev cell * n_cells + cur cell."""
    (pa, ca), (pb, cb) = divmod(a, n_cells), divmod(b, n_cells)
    (par, pac), (car, cac) = divmod(pa, width), divmod(ca, width)
    (pbr, pbc), (cbr, cbc) = divmod(pb, width), divmod(cb, width)
    return abs(par - pbr) + abs(pac - pbc) + int(car - par != cbr - pbr) + int(cac - pac != cbc - pbc)


def tlv(idx, alive, keys, rewards, width, n_cells):
    """_get_TLV (:124-133): the violations of idx against the first occurrence of each key among the alive indices, ascending."""
    total, seen = 0, set()
    for j in alive:
        if keys[j] not in seen:
            seen.add(keys[j])
            total += max(0, abs(rewards[idx] - rewards[j]) - d_trans_boat(keys[j], keys[idx], width, n_cells))
    return total


def detect(keys, rewards, width, n_cells):
    """identify_corruption_in_trajectory (:168-206) without the memory -> (corrupt indices in marking order, safe index or None)."""
    L = len(keys)
    alive = list(range(L))
    tlv0 = [tlv(i, alive, keys, rewards, width, n_cells) for i in range(L)]
    walk = sorted(range(L), key=lambda i: (tlv0[i], i), reverse=True)  # np.argsort(TLV, kind="stable")[::-1]
    corrupt = []
    for idx in walk:
        value = tlv0[idx] if not corrupt else tlv(idx, alive, keys, rewards, width, n_cells)
        if value <= 0:
            return corrupt, idx
        corrupt.append(idx)
        alive.remove(idx)
    return corrupt, None


class Memory:
    """One agent's `states` ({key: [safe?, reward]}) and `rllb` ({key: bound}; a missing key and None are both "no bound")."""

    def __init__(self, width=5, n_cells=25):
        self.width, self.n_cells = width, n_cells
        self.states, self.rllb = {}, {}

    def filter(self, keys, rewards):
        """One trajectory: detect, merge, modified rewards -> (order, safe index or None, modified rewards with None for "no bound").
        A key outside the tables: nothing is marked, (None, None, the rewards)."""
        keys, rewards = [int(k) for k in keys], [int(r) for r in rewards]
        if any(k < 0 or k >= self.n_cells ** 2 for k in keys):
            return None, None, list(rewards)
        order, safe = detect(keys, rewards, self.width, self.n_cells)
        for i in order:
            self.states[keys[i]] = [False, rewards[i]]
        if safe is not None and self.states.get(keys[safe], [True])[0]:
            self.states[keys[safe]] = [True, rewards[safe]]
        if order:
            for c, (ok, _) in self.states.items():
                if ok:
                    continue
                bound = self.rllb.get(c)
                for s, (s_ok, s_reward) in self.states.items():
                    if s_ok:
                        b = s_reward - d_trans_boat(s, c, self.width, self.n_cells)
                        bound = b if bound is None or b > bound else bound
                self.rllb[c] = bound
        modified = [self.rllb.get(k) if (k in self.states and not self.states[k][0]) else r for k, r in zip(keys, rewards)]
        return order, safe, modified

    def tables(self):
        """(flag uint8, reward int32, rllb int32) [n_keys]: the memory as the library's tables hold it."""
        n = self.n_cells ** 2
        flag, reward, rllb = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.full(n, NONE, np.int32)
        for k, (ok, r) in self.states.items():
            flag[k], reward[k] = (SAFE if ok else CORRUPT), r
        for k, b in self.rllb.items():
            if b is not None:
                rllb[k] = b
        return flag, reward, rllb
