"""Test infrastructure of the per-instance box bounds (mpc_set_instance_bounds): a menu of bound sets and the group of every instance, so that the
oracle -- which knows one set of bounds per config -- can be asked about each group of equal bounds."""
import numpy as np

# the handle's defaults (mpc_default_config): x, y in +-7, v, omega in +-10, u in +-8
DEFAULTS = dict(bx_lo=np.array([-7.0, -7.0, -10.0, -10.0]), bx_hi=np.array([7.0, 7.0, 10.0, 10.0]),
                bu_lo=np.array([-8.0, -8.0]), bu_hi=np.array([8.0, 8.0]))


def draw_bounds(rng, B, G=4):
    """(menu, group): menu[g] = dict(bx_lo (4,), bx_hi (4,), bu_lo (2,), bu_hi (2,)), group (B,) the menu entry of every instance.  Group 0 is the handle's
    defaults; the others draw every component and side on its own (asymmetric boxes): x, y limits +-U(6.5, 7.5), v +-U(0.8, 3.0), omega +-U(1.0, 4.0),
    u +-U(1.5, 6.0)"""
    menu = [{k: v.copy() for k, v in DEFAULTS.items()}]
    for _ in range(1, G):
        side = lambda: np.array([rng.uniform(6.5, 7.5), rng.uniform(6.5, 7.5), rng.uniform(0.8, 3.0), rng.uniform(1.0, 4.0)])
        bx_lo, bx_hi = -side(), side()
        bu_lo, bu_hi = -rng.uniform(1.5, 6.0, 2), rng.uniform(1.5, 6.0, 2)
        menu.append(dict(bx_lo=bx_lo, bx_hi=bx_hi, bu_lo=bu_lo, bu_hi=bu_hi))
    group = rng.permutation(np.arange(B) % G)
    return menu, group


def per_instance(menu, group):
    """the arrays of BatchedMpc.set_instance_bounds: dict(bx_lo (B, 4), bx_hi (B, 4), bu_lo (B, 2), bu_hi (B, 2))"""
    return {k: np.stack([menu[g][k] for g in group]) for k in ("bx_lo", "bx_hi", "bu_lo", "bu_hi")}


def as_cfg(entry):
    """one menu entry as config overrides (mpc_gpu.BatchedMpc(**...), oracle.config(**...))"""
    return {k: [float(x) for x in v] for k, v in entry.items()}
