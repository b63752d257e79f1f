"""Test infrastructure of the per-instance obstacle masks (mpc_set_obstacle_mask): mask draws and the cut of an instance's present obstacles out of
the arrays the solver reads, so that the oracle -- which knows one obstacle count per config -- can be asked about each group of equal masks."""
import numpy as np


def draw_masks(rng, B, no):
    """heterogeneous, non-prefix masks (B, no) whose counts cover 0 .. no across the batch: instance b keeps a random subset of (b mod (no + 1)) obstacles,
    so with B > no every count occurs; rows are shuffled"""
    act = np.zeros((B, no), bool)
    for b in range(B):
        act[b, rng.permutation(no)[: b % (no + 1)]] = True
    return act[rng.permutation(B)]


def active_columns(P, active_row):
    """the present obstacles of one instance: P (N + 1, no, 2) -> (N + 1, k, 2), obst (no, 4) -> (k, 4); the obstacles keep their order"""
    a = np.asarray(active_row, bool)
    P = np.asarray(P)
    if P.ndim == 3:
        return np.ascontiguousarray(P[:, a, :])
    return np.ascontiguousarray(P[a])


def groups(active):
    """{mask word: indices of the instances that carry it}, in order of first appearance"""
    out = {}
    for b, row in enumerate(np.asarray(active, bool)):
        out.setdefault(tuple(row.tolist()), []).append(b)
    return out


def poison(arr, active, value):
    """a copy of obst (B, no, 4) or P (B, N + 1, no, 2) with every entry of an absent obstacle set to `value`"""
    out = np.array(arr, dtype=np.float64, copy=True)
    absent = ~np.asarray(active, bool)
    if out.ndim == 3:
        out[absent] = value
    else:
        out[np.broadcast_to(absent[:, None, :], out.shape[:3])] = value
    return out
