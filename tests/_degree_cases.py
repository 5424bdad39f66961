"""What test_gpu_smoother_degrees.py and test_gpu_float_levels.py share: the hierarchies both run, and one numpy oracle build of
each per session (the product's numbering at max_brick=0 is a function of mesh and degree alone, so the oracle levels built
from one hierarchy's DoF keys serve every smoother degree and number type of that hierarchy)."""
import numpy as np

QUADRANT_HMG = ("quadrant", 3, 4, "HMG-global")  # hanging nodes, no fused bricks
HYPERCUBE_HMG = ("hypercube", 4, 2, "HMG-global")  # 17-point lattice bricks, fused transfers
QUADRANT_PMG = ("quadrant", 3, 4, "PMG")
# bricks next to other slots; of test_gpu_parity.FUSED_CASES' three such hierarchies the one whose numpy oracle builds fastest
# (measured on the CPU: quadrant 5 p=2 11.3 s, quadrant 6 p=1 12.9 s, quadrant 4 p=4 30.8 s)
MIXED_HMG = ("quadrant", 5, 2, "HMG-global")
HIER_CASES = [QUADRANT_HMG, HYPERCUBE_HMG, QUADRANT_PMG, MIXED_HMG]

_levels, _multigrids = {}, {}


def oracle_levels(oracle, case, h):
    """(levels, P) of the numpy oracle in the numbering of the product hierarchy h of that case"""
    if case not in _levels:
        _levels[case] = oracle.build_hierarchy(*case, numbering_keys=[d.keys() for d in h.dofs])
    levels, P = _levels[case]
    assert [lv.n for lv in levels] == [d.n_dofs for d in h.dofs]
    return levels, P


def oracle_multigrid(oracle, case, h, k):
    """oracle.Multigrid(levels, P, k, coarse="direct") of the case, built once per smoother degree"""
    if (case, k) not in _multigrids:
        levels, P = oracle_levels(oracle, case, h)
        _multigrids[(case, k)] = oracle.Multigrid(levels, P, k, coarse="direct")
    return _multigrids[(case, k)]


def n_fused(h):
    return sum(t.n_fused_bricks() for t in h.transfers[1:])


def round32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


class RenumberedLevel:
    """an oracle level in the numbering of another DoF handler of the same space (matched through the geometric DoF keys)"""

    def __init__(self, lv, keys):
        pos = {tuple(int(v) for v in k): i for i, k in enumerate(lv.keys)}
        perm = np.array([pos[tuple(int(v) for v in k)] for k in keys])
        assert len(perm) == lv.n and len(set(perm.tolist())) == lv.n
        self.n, self.A, self.inv_diag = lv.n, lv.A[perm][:, perm].tocsr(), lv.inv_diag[perm]


def float_cycle_reference(emu, mg, max_evs, r):
    """For the FP32 bound k * e_ref: the oracle mg with the product's eigenvalue estimates injected (so that the comparison
    is about the kernels alone), its float64 V-cycle of r, and e_ref, the distance of the float32 emulation from it."""
    mgp = emu.with_max_evs(mg, max_evs)
    ref = mgp.vcycle(r)
    z32 = emu.vcycle(mgp, r, np.float32)
    assert z32.dtype == np.float32
    e_ref = np.linalg.norm(z32 - ref) / np.linalg.norm(ref)
    return mgp, ref, e_ref
