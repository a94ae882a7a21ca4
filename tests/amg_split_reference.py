"""numpy statement of the PARALLEL form of the C/F split of pgx_build_hierarchy (csrc/pgx_amg_build.hip: k_ab_split), next to the
serial greedy pass amg_reference.cf_split states.

TEST INFRASTRUCTURE ONLY.  The greedy pass is the lexicographically first maximal independent set of the strong edges between
vertices of one kind (Dirichlet - Dirichlet, interior - interior; the two kinds share no such edge, so their order does not matter).
Its parallel form, over the strong neighbours of a vertex's own kind with a LOWER index:

  an undecided vertex becomes F as soon as one of them is C,
  it becomes C as soon as all of them are F (at once if it has none).

A decision is final and rests on final decisions only, so every schedule that keeps deciding ends in the greedy split.
split_rounds applies the rule in synchronous rounds (every decision of a round reads the state the round began with) and counts
them; split_in_place sweeps the vertices in a given random order and lets every decision be seen at once, as a kernel that updates
its state array in place does."""
from __future__ import annotations

import numpy as np


def lower_edges(S, mask):
    """(i, j): the strong edges with j < i between vertices of one kind.  S: symmetrised strength pattern (amg_reference.strength)."""
    mask = np.asarray(mask, dtype=bool)
    i = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    j = S.indices
    keep = (j < i) & (mask[i] == mask[j])
    return i[keep], j[keep]


def split_rounds(S, mask):
    """(is_c [n] bool, rounds): synchronous rounds until no vertex is undecided."""
    n = S.shape[0]
    i, j = lower_edges(S, mask)
    deg = np.bincount(i, minlength=n)
    state = np.zeros(n, dtype=np.int8)  # 0 undecided, 1 C, 2 F
    rounds = 0
    while np.any(state == 0):
        n_c = np.bincount(i, weights=state[j] == 1, minlength=n)
        n_f = np.bincount(i, weights=state[j] == 2, minlength=n)
        open_ = state == 0
        to_f = open_ & (n_c > 0)
        to_c = open_ & ~to_f & (n_f == deg)
        assert np.any(to_f | to_c), "a round always decides the lowest undecided vertex"
        state[to_f], state[to_c] = 2, 1
        rounds += 1
    return state == 1, rounds


def split_in_place(S, mask, rng):
    """(is_c, sweeps): every sweep visits the vertices in a fresh random order and writes each decision where the next vertex reads."""
    n = S.shape[0]
    i, j = lower_edges(S, mask)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])  # i ascends: the edges of a vertex are contiguous
    state = np.zeros(n, dtype=np.int8)
    sweeps = 0
    while np.any(state == 0):
        for v in rng.permutation(np.flatnonzero(state == 0)):
            nb = state[j[ptr[v]:ptr[v + 1]]]
            if np.any(nb == 1):
                state[v] = 2
            elif np.all(nb == 2):
                state[v] = 1
        sweeps += 1
    return state == 1, sweeps
