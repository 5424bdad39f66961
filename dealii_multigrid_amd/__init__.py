"""MI355X-native matrix-free multigrid V-cycle -- Python host mirror of the reference's plugin surface.

Thin ctypes layer over the C ABI (`include/mgamd.h`, `lib/libmgamd.so`).  Class and method names
follow deal.II as the reference uses it:

  Triangulation            <-> parallel::distributed::Triangulation + GridGenerator  (ref:multigrid_throughput.cc:2041-2062)
  DoFs                     <-> DoFHandler + AffineConstraints + MatrixFree tables      (ref:multigrid_throughput.cc:1578-1595)
  Operator                 <-> Operator<3,1,Number>                                    (ref:include/operator.h:11-557)
  PreconditionChebyshev    <-> PreconditionChebyshev<Operator,Vector,DiagonalMatrix>   (ref:multigrid_throughput.cc:849-883)
  MGTwoLevelTransfer       <-> MGTwoLevelTransfer<3,Vector>                            (ref:multigrid_throughput.cc:1600-1604)
  PreconditionMG           <-> Multigrid + PreconditionMG + MGTransferGlobalCoarsening (ref:multigrid_throughput.cc:1093-1133)
  solve_cg                 <-> SolverCG + ReductionControl                             (ref:multigrid_throughput.cc:1140-1147)
  SparseMatrix             <-> Operator::get_trilinos_system_matrix on the device      (ref:include/operator.h:244-287)
  PreconditionAMG          <-> TrilinosWrappers::PreconditionAMG                       (ref:multigrid_throughput.cc:1907-1909)
  solve_with_global_coarsening  (ref:multigrid_throughput.cc:1443-1666)

There is no CPU fallback: every device call raises if the HIP library or a gfx950 GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

# MGAMD_LIBRARY: another build of the same library (development: the -DMGAMD_KERNEL_DEBUG build of `make debug`)
_LIB_PATH = os.environ.get("MGAMD_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmgamd.so")
F64, F32 = 8, 4
# levels of the sharded AMG with at most this many global rows are replicated (mgamd.h: a guess, unmeasured on multi-GPU hardware)
AMG_MIN_SHARDED_ROWS_DEFAULT = 20000
INVALID_DOF = 0xFFFFFFFF
# Triangulation.set_dirichlet_faces: every face of the cube is Dirichlet (the default, the reference's boundary id 0)
ALL_DIRICHLET = 0x3F


class MgamdError(RuntimeError):
    pass


class NoDeviceError(MgamdError):
    pass


def _load():
    if not os.path.exists(_LIB_PATH):
        raise MgamdError(
            f"{_LIB_PATH} is missing: build it with `make` (or __graft_entry__.build()); there is no fallback path"
        )
    lib = C.CDLL(_LIB_PATH)
    lib.mgamd_last_error.restype = C.c_char_p
    lib.mgamd_version.restype = C.c_char_p
    return lib


_lib = _load()


def _chk(status):
    if status != 0:
        msg = _lib.mgamd_last_error().decode()
        if status == 2:
            raise NoDeviceError(msg)
        raise MgamdError(msg)


class DofsInfo(C.Structure):
    _fields_ = [
        ("degree", C.c_uint32),
        ("n_cells", C.c_uint64),
        ("n_dofs", C.c_uint32),
        ("n_interior", C.c_uint32),
        ("n_tail", C.c_uint32),
        ("n_dirichlet", C.c_uint32),
        ("n_hanging", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("group_B", C.c_uint32 * 8),
        ("group_slots", C.c_uint64 * 8),
        ("n_tail_owned", C.c_uint32),
        ("n_dirichlet_owned", C.c_uint32),
        ("n_hanging_owned", C.c_uint32),
        ("n_peers", C.c_uint32),
        ("n_halo_send", C.c_uint32),
        ("n_edge", C.c_uint32),
        ("group_halo_slots", C.c_uint64 * 8),
    ]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Triangulation:
    def __init__(self, geometry="hypercube", n_ref_global=0, n_ref_local=0, _handle=None):
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            _chk(_lib.mgamd_tria_create(geometry.encode(), C.c_uint(n_ref_global), C.c_uint(n_ref_local), C.byref(self._h)))
        nc, nl, nh = C.c_uint64(), C.c_uint32(), C.c_uint64()
        _chk(_lib.mgamd_tria_info(self._h, C.byref(nc), C.byref(nl), C.byref(nh)))
        self.n_cells, self.n_levels, self.n_cells_hn = nc.value, nl.value, nh.value

    @classmethod
    def from_leaves(cls, level, i, j, k) -> "Triangulation":
        """a caller-built octree over one root cell (mgamd_tria_create_from_leaves): leaves (level, i, j, k) in any order; must
        tile the cube and be 2:1 balanced across faces, edges and corners, else MgamdError (status MGAMD_ERR_INVALID)"""
        level, i, j, k = (np.ascontiguousarray(level, np.uint8), np.ascontiguousarray(i, np.uint32), np.ascontiguousarray(j, np.uint32),
                          np.ascontiguousarray(k, np.uint32))
        if not (len(level) == len(i) == len(j) == len(k)):
            raise ValueError("from_leaves: arrays of different lengths")
        h = C.c_void_p()
        _chk(_lib.mgamd_tria_create_from_leaves(C.c_uint64(len(level)), _ptr(level), _ptr(i), _ptr(j), _ptr(k), C.byref(h)))
        return cls(_handle=h)

    def level_mesh(self, level: int) -> "Triangulation":
        """local smoothing: all cells of refinement level `level`, active or not (distribute_mg_dofs levels)"""
        h = C.c_void_p()
        _chk(_lib.mgamd_tria_level_mesh(self._h, level, C.byref(h)))
        return Triangulation(_handle=h)

    def coarsen(self) -> "Triangulation":
        h = C.c_void_p()
        _chk(_lib.mgamd_tria_coarsen(self._h, C.byref(h)))
        return Triangulation(_handle=h)

    def refine(self, flags, return_parent: bool = False):
        """flagged refinement (mgamd_tria_refine): every leaf with a non-zero flag (one per leaf, order of cells()) is replaced by its
        eight children, then the minimal ripple to the full 2:1 balance runs.  Children inherit the coefficient value of their
        parent; the dirichlet_faces mask and the Robin coefficients are copied.  With return_parent also the index, per new leaf,
        of the old leaf that is it or contains it.  MgamdError for flags None and for a flagged leaf at the deepest level."""
        h, par = C.c_void_p(), np.zeros(0, np.uint64)
        if flags is None:
            _chk(_lib.mgamd_tria_refine(self._h, None, C.byref(h), None))  # (refused by name)
            raise MgamdError("refine: flags is None")
        fl = np.ascontiguousarray(np.asarray(flags) != 0, np.uint8)
        if fl.shape != (self.n_cells,):
            raise ValueError(f"refine: {fl.shape} flags for {self.n_cells} cells")
        if return_parent:
            # (mgamd_tria_refine: at most 8 n_cells new cells, every leaf split once)
            par = np.zeros(8 * self.n_cells, np.uint64)
        _chk(_lib.mgamd_tria_refine(self._h, _ptr(fl), C.byref(h), _ptr(par) if return_parent else None))
        fine = Triangulation(_handle=h)
        return (fine, par[:fine.n_cells].copy()) if return_parent else fine

    def _face_neighbours(self):
        """the face-neighbour table of the error indicator (mgamd_debug_tria_face_neighbours): code (n_cells, 6), nbr (n_cells, 6, 4)"""
        code, nbr = np.zeros((self.n_cells, 6), np.uint8), np.zeros((self.n_cells, 6, 4), np.uint32)
        _chk(_lib.mgamd_debug_tria_face_neighbours(self._h, _ptr(code), _ptr(nbr)))
        return code, nbr

    def cells(self):
        n = self.n_cells
        lev = np.zeros(n, np.uint8)
        i, j, k = (np.zeros(n, np.uint32) for _ in range(3))
        mask = np.zeros(n, np.uint16)
        _chk(_lib.mgamd_tria_get_cells(self._h, _ptr(lev), _ptr(i), _ptr(j), _ptr(k), _ptr(mask)))
        return lev, i, j, k, mask

    def cell_centres(self):
        """the centres of the leaves in [-1, 1]^3, (n_cells, 3), in the order of cells()"""
        lev, i, j, k, _ = self.cells()
        h = 2.0 / (1 << lev.astype(np.int64))
        return np.stack([-1.0 + h * (c.astype(np.float64) + 0.5) for c in (i, j, k)], axis=1)

    def set_coefficient(self, values):
        """the diffusion coefficient a > 0 of -div(a grad u) + sigma u, one value per leaf in the order of cells(); None resets to
        a = 1.  coarsen() carries it down as the mean over each coarse leaf; DoFs copy it when they are built
        (mgamd_tria_set_coefficient).  MgamdError for a value that is <= 0, NaN or infinite."""
        if values is None:
            _chk(_lib.mgamd_tria_set_coefficient(self._h, None))
            return
        a = np.ascontiguousarray(values, np.float64)
        if a.shape != (self.n_cells,):
            raise ValueError(f"set_coefficient: {a.shape} values for {self.n_cells} cells")
        _chk(_lib.mgamd_tria_set_coefficient(self._h, _ptr(a)))

    def set_coefficient_function(self, f):
        """set_coefficient with f(x, y, z) evaluated at the leaf centres (arrays in, array out)"""
        c = self.cell_centres()
        self.set_coefficient(np.broadcast_to(np.asarray(f(c[:, 0], c[:, 1], c[:, 2]), np.float64), (self.n_cells,)))

    def coefficient(self):
        """one value per leaf (ones if none is set)"""
        a = np.zeros(self.n_cells, np.float64)
        _chk(_lib.mgamd_tria_get_coefficient(self._h, _ptr(a)))
        return a

    def has_coefficient(self) -> bool:
        has = C.c_int()
        _chk(_lib.mgamd_tria_has_coefficient(self._h, C.byref(has)))
        return bool(has.value)

    def set_dirichlet_faces(self, mask: int):
        """which faces of the cube [-1, 1]^3 are Dirichlet: bit f = 2 axis + side (0: x = -1, 1: x = +1, ... 5: z = +1); the other
        faces are natural (Neumann: zero flux unless rhs_boundary_flux adds one).  Default 0x3F.  coarsen() inherits the mask; DoFs
        copy it when they are built (mgamd_tria_set_dirichlet_faces).  MgamdError for a mask > 63."""
        if int(mask) < 0:
            raise MgamdError(f"dirichlet_faces mask {mask} refused: it is a 6-bit mask, 0 to 63")
        _chk(_lib.mgamd_tria_set_dirichlet_faces(self._h, C.c_uint(int(mask))))

    def dirichlet_faces(self) -> int:
        m = C.c_uint()
        _chk(_lib.mgamd_tria_get_dirichlet_faces(self._h, C.byref(m)))
        return m.value

    def set_robin_coefficients(self, beta):
        """convective (Robin) faces: a grad u . n + beta[f] (u - u_ext) = 0 on face f (numbered as for set_dirichlet_faces), beta[f]
        >= 0; 6 values or {face: value}, default 0.  The operator gains sum_f beta[f] B_f (surface mass matrices); the load of u_ext
        is rhs_boundary_flux with q[f] = beta[f] u_ext.  coarsen() inherits the values; DoFs copy them when they are built
        (mgamd_tria_set_robin_coefficients).  MgamdError for a negative or non-finite value and for beta[f] > 0 on a Dirichlet face."""
        beta = _flux_array(beta, "Robin coefficients")
        _chk(_lib.mgamd_tria_set_robin_coefficients(self._h, _ptr(beta)))

    def robin_coefficients(self):
        beta = np.zeros(6)
        _chk(_lib.mgamd_tria_get_robin_coefficients(self._h, _ptr(beta)))
        return beta

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_tria_destroy(self._h)
            self._h = None


def mark_maximum(eta, theta: float):
    """the maximum strategy: flag every leaf with eta_K >= theta max eta (uint8, one per leaf).  A threshold keeps the exact ties of
    a symmetric mesh together, which a fixed-number rule would cut by rounding.  An all-zero eta flags nothing."""
    eta = np.asarray(eta, np.float64)
    top = eta.max() if eta.size else 0.0
    if not top > 0.0:
        return np.zeros(eta.shape, np.uint8)
    return (eta >= theta * top).astype(np.uint8)


# the norms of Operator.integrate_difference (MGAMD_NORM_*)
NORM_L2, NORM_H1_SEMINORM, NORM_ENERGY, NORM_LINFTY = 0, 1, 2, 3


def compute_global_error(per_cell, norm: int) -> float:
    """VectorTools::compute_global_error: the global norm from the per-leaf values of Operator.integrate_difference, the l2 norm of
    the array for NORM_L2, NORM_H1_SEMINORM and NORM_ENERGY and its maximum for NORM_LINFTY"""
    e = np.asarray(per_cell, np.float64)
    if norm not in (NORM_L2, NORM_H1_SEMINORM, NORM_ENERGY, NORM_LINFTY):
        raise ValueError(f"compute_global_error: unknown norm {norm}")
    if norm == NORM_LINFTY:
        return float(e.max()) if e.size else 0.0
    return float(np.sqrt(np.sum(e * e)))


def create_geometric_coarsening_sequence(fine: Triangulation, coarse_coefficient=None):
    """MGTransferGlobalCoarseningTools::create_geometric_coarsening_sequence: coarsest first.  A diffusion coefficient on `fine`
    goes down mesh by mesh (Triangulation.coarsen: the mean over each coarse leaf); coarse_coefficient(tria) -> values, if given,
    overwrites every coarse mesh's values as soon as it exists (e.g. with a harmonic mean)."""
    seq = [fine]
    while seq[-1].n_cells > 1:
        seq.append(seq[-1].coarsen())
        if coarse_coefficient is not None:
            seq[-1].set_coefficient(coarse_coefficient(seq[-1]))
    return seq[::-1]


def _flux_array(q, what="boundary flux"):
    """six face values (fluxes, Robin coefficients) as a contiguous double array: a sequence of 6 values or {face: value}"""
    if isinstance(q, dict):
        a = np.zeros(6)
        for f, v in q.items():
            if not 0 <= int(f) <= 5:
                raise MgamdError(f"{what}: face {f} refused, the faces are 0 to 5")
            a[int(f)] = v
        return a
    a = np.ascontiguousarray(q, np.float64)
    if a.shape != (6,):
        raise ValueError(f"{what}: {a.shape} values for the 6 faces")
    return a


def _apply_dirichlet_faces(fine: Triangulation, mg_type: str, dirichlet_faces, robin=None):
    """Hierarchy(dirichlet_faces=..., robin=...): set on the mesh (the carrier, as for the coefficient) before anything is built from
    it, the mask first (a convective face must not be Dirichlet); the local-smoothing types refuse a positive Robin coefficient
    and another mask than 63 by name, in that order (a convective face implies another mask)"""
    if dirichlet_faces is not None:
        fine.set_dirichlet_faces(dirichlet_faces)
    if robin is not None:
        fine.set_robin_coefficients(robin)
    if mg_type in ("HMG-local", "HPMG-local") and np.any(fine.robin_coefficients() > 0):
        raise MgamdError(f"Type '{mg_type}' with the Robin coefficients {fine.robin_coefficients().tolist()}: not implemented (local "
                         "smoothing takes no convective faces)")
    if mg_type in ("HMG-local", "HPMG-local") and fine.dirichlet_faces() != ALL_DIRICHLET:
        raise MgamdError(f"Type '{mg_type}' with the dirichlet_faces mask {fine.dirichlet_faces()}: not implemented (local smoothing "
                         "takes the mask 63 only)")


def _apply_coefficient(fine: Triangulation, coefficient):
    """Hierarchy(coefficient=...): a function f(x, y, z) of the leaf centres or one value per leaf of the finest mesh"""
    if coefficient is None:
        return
    if callable(coefficient):
        fine.set_coefficient_function(coefficient)
    else:
        fine.set_coefficient(coefficient)


def create_polynomial_coarsening_sequence(degree: int):
    """...::create_polynomial_coarsening_sequence(degree, bisect): e.g. 4 -> [1, 2, 4] (the degrees of the PMG levels)."""
    return [p for _, p in _level_plan("PMG", 1, degree)[0]]


class Partition:
    """Domain decomposition of a level hierarchy over n_ranks GPUs."""

    def __init__(self, trias, n_ranks: int, hanging_weight: float = 2.0, min_root_cells: int = 0, group: int = 1,
                 min_sub_root_cells: int = 0):
        """group > 1: two tiers -- levels below the root level with >= min_sub_root_cells cells are cut into n_ranks / group
        parts, each held by `group` consecutive ranks (mgamd_partition_create_tiered)"""
        self.trias, self.n_ranks = list(trias), n_ranks
        arr = (C.c_void_p * len(self.trias))(*[t._h for t in self.trias])
        self._h = C.c_void_p()
        _chk(_lib.mgamd_partition_create_tiered(arr, len(self.trias), n_ranks, C.c_double(hanging_weight), C.c_uint64(min_root_cells),
                                                group, C.c_uint64(min_sub_root_cells), C.byref(self._h)))
        rl, sl, g = C.c_uint(), C.c_uint(), C.c_uint()
        _chk(_lib.mgamd_partition_info(self._h, C.byref(rl), None))
        _chk(_lib.mgamd_partition_tiers(self._h, C.byref(sl), C.byref(g)))
        self.root_level, self.sub_root_level, self.group = rl.value, sl.value, g.value

    def n_parts(self, level: int) -> int:
        """pieces the level is cut into: n_ranks, n_ranks / group on the subset levels, 1 on the replicated ones"""
        return self.n_ranks if level >= self.root_level else (self.n_ranks // self.group if level >= self.sub_root_level else 1)

    def statistics(self):
        """MGTools::print_multigrid_statistics (ref:include/mg_tools.h:267-512) for this partition"""
        st = (C.c_double * 5)()
        _chk(_lib.mgamd_partition_statistics(self._h, st))
        return dict(zip(("workload_eff", "workload_path_max", "vertical_eff", "horizontal_eff", "mem_total"), st))

    def owner(self, level: int):
        o = np.zeros(self.trias[level].n_cells, np.uint16)
        _chk(_lib.mgamd_partition_get_owner(self._h, level, _ptr(o)))
        return o

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_partition_destroy(self._h)
            self._h = None


class DoFs:
    def __init__(self, tria: Triangulation, degree: int, max_brick: int = 0, partition: "Partition" = None, level: int = 0, rank: int = 0,
                 local_smoothing_level: bool = False):
        """local_smoothing_level: `tria` is Triangulation.level_mesh(l); refinement-edge DoFs are numbered [I | T | E | D | H]"""
        self.tria = tria
        self._h = C.c_void_p()
        if local_smoothing_level:
            _chk(_lib.mgamd_dofs_create_level(tria._h, degree, max_brick, C.byref(self._h)))
        elif partition is None:
            _chk(_lib.mgamd_dofs_create(tria._h, degree, max_brick, C.byref(self._h)))
        else:
            _chk(_lib.mgamd_dofs_create_local(partition._h, level, rank, degree, max_brick, C.byref(self._h)))
        self.info = DofsInfo()
        _chk(_lib.mgamd_dofs_info(self._h, C.byref(self.info)))
        self.degree = degree
        self.n_dofs = self.info.n_dofs

    def set_mass_coefficient(self, sigma: float):
        """the mass term: operators, matrices and right-hand sides built from these DoFs AFTER the call represent K + sigma M
        (-Laplace u + sigma u).  sigma >= 0 and finite; local-smoothing levels only take 0 (mgamd_dofs_set_mass_coefficient)"""
        _chk(_lib.mgamd_dofs_set_mass_coefficient(self._h, C.c_double(sigma)))

    def mass_coefficient(self) -> float:
        s = C.c_double()
        _chk(_lib.mgamd_dofs_mass_coefficient(self._h, C.byref(s)))
        return s.value

    def coefficient_range(self):
        """(min, max) of the diffusion coefficient these DoFs were built with (their mesh's at that time)"""
        lo, hi = C.c_double(), C.c_double()
        _chk(_lib.mgamd_dofs_coefficient_range(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def dirichlet_faces(self) -> int:
        """the dirichlet_faces mask these DoFs were built with (their mesh's at that time)"""
        m = C.c_uint()
        _chk(_lib.mgamd_dofs_dirichlet_faces(self._h, C.byref(m)))
        return m.value

    def robin_coefficients(self):
        """the Robin coefficients these DoFs were built with (their mesh's at that time)"""
        beta = np.zeros(6)
        _chk(_lib.mgamd_dofs_robin_coefficients(self._h, _ptr(beta)))
        return beta

    def robin_faces(self):
        """the table of boundary cell faces on convective faces (this rank's cells): (idx [n, (p+1)^2] uint32 with INVALID_DOF on
        Dirichlet DoFs, flags [n] uint8, scale [n] = beta_f h^2); see mgamd_dofs_robin_faces"""
        n = C.c_uint64()
        _chk(_lib.mgamd_dofs_robin_faces(self._h, C.byref(n), None, None, None))
        n2 = (self.degree + 1) ** 2
        idx, flags, scale = np.zeros((n.value, n2), np.uint32), np.zeros(n.value, np.uint8), np.zeros(n.value)
        if n.value:
            _chk(_lib.mgamd_dofs_robin_faces(self._h, C.byref(n), _ptr(idx), _ptr(flags), _ptr(scale)))
        return idx, flags, scale

    def rhs_boundary_flux(self, q):
        """boundary load of one constant flux per face, host vector: sum_f q[f] int_{face f} phi_i, through the hanging-node
        constraints, constrained rows 0.  q: 6 values or {face: value}.  MgamdError for a non-zero flux on a Dirichlet face."""
        q, b = _flux_array(q), np.zeros(self.n_dofs)
        _chk(_lib.mgamd_dofs_rhs_boundary_flux(self._h, _ptr(q), _ptr(b)))
        return b

    def dirichlet_cells(self):
        """the table the lifting of Dirichlet data walks (this rank's cells, in Morton order, that gather a Dirichlet DoF):
        (idx [n, (p+1)^3] uint32 with the real index on Dirichlet DoFs, mask [n] uint16 the cell's hanging mask, scale [n, 2] =
        (a h, h)); see mgamd_dofs_dirichlet_cells"""
        n = C.c_uint64()
        _chk(_lib.mgamd_dofs_dirichlet_cells(self._h, C.byref(n), None, None, None))
        n3 = (self.degree + 1) ** 3
        idx, mask, scale = np.zeros((n.value, n3), np.uint32), np.zeros(n.value, np.uint16), np.zeros((n.value, 2))
        if n.value:
            _chk(_lib.mgamd_dofs_dirichlet_cells(self._h, C.byref(n), _ptr(idx), _ptr(mask), _ptr(scale)))
        return idx, mask, scale

    def rhs_dirichlet(self, g, include_mass: bool = True):
        """the lifting of the Dirichlet data g (n_dofs values, only those at Dirichlet DoFs are read), host vector:
        -[C^T (K_a + s sigma M) C g^] on free rows, 0 on constrained rows, s = include_mass; additive to rhs_function,
        rhs_boundary_flux and M f.  MgamdError where a convective face shares an edge with a Dirichlet face."""
        g, b = self._data_array(g, "rhs_dirichlet"), np.zeros(self.n_dofs)
        _chk(_lib.mgamd_dofs_rhs_dirichlet(self._h, _ptr(g), 1 if include_mass else 0, _ptr(b)))
        return b

    def distribute_values(self, x, g):
        """a copy of the host vector x with the Dirichlet DoFs set to the values of g and the hanging DoFs interpolated from
        their parents; free DoFs are untouched"""
        x, g = self._data_array(x, "distribute_values").copy(), self._data_array(g, "distribute_values")
        _chk(_lib.mgamd_dofs_distribute_values(self._h, _ptr(g), _ptr(x)))
        return x

    def dirichlet_face_values(self, v):
        """Dirichlet data of one constant per face: v[f] on the Dirichlet DoFs of face f (6 values or {face: value}; a DoF on
        several Dirichlet faces takes the lowest-numbered one), 0 elsewhere.  MgamdError for a non-zero value on a natural face."""
        v, g = _flux_array(v, "Dirichlet values"), np.zeros(self.n_dofs)
        _chk(_lib.mgamd_dofs_dirichlet_face_values(self._h, _ptr(v), _ptr(g)))
        return g

    def node_positions(self):
        """the support point of every DoF, (n_dofs, 3): g = f(*dofs.node_positions().T) is the nodal interpolant of f"""
        xyz = np.zeros((self.n_dofs, 3))
        _chk(_lib.mgamd_dofs_node_positions(self._h, _ptr(xyz)))
        return xyz

    def quadrature_points(self, n_q: int = 0):
        """the physical points of QGauss(n_q)^3 on every leaf (mgamd_dofs_quadrature_points), shape (n_cells, n_q, n_q, n_q, 3) indexed
        [cell, qz, qy, qx]: where Operator.integrate_difference expects caller data.  n_q: degree + 1 ... degree + 3, 0 for degree + 2.
        Host only."""
        nq = self.degree + 2 if n_q == 0 else int(n_q)
        valid = self.degree + 1 <= nq <= self.degree + 3
        xyz = np.zeros((self.info.n_cells, nq, nq, nq, 3) if valid else 1)
        _chk(_lib.mgamd_dofs_quadrature_points(self._h, C.c_int(n_q), _ptr(xyz)))  # (refuses n_q by name before it writes)
        return xyz

    def _points_array(self, a, per_point, n_q, who):
        """caller data at the quadrature points as a contiguous double array of the layout's size, None passed through"""
        if a is None:
            return None
        nq = self.degree + 2 if n_q == 0 else int(n_q)
        a = np.ascontiguousarray(a, dtype=np.float64)
        if self.degree + 1 <= nq <= self.degree + 3 and a.size != per_point * self.info.n_cells * nq ** 3:  # (another n_q is refused by name)
            raise ValueError(f"{who}: {a.size} values for {per_point} x {self.info.n_cells * nq ** 3} quadrature points")
        return a

    def integrate(self, values=None, gradients=None, n_q: int = 0):
        """the load of data at quadrature_points(n_q), host vector (mgamd_dofs_integrate; in deal.II: FEEvaluation::integrate,
        VectorTools::create_right_hand_side): b_i = sum_K sum_q w_q h_K^3 (values_q phi_i(x_q) + gradients_q . grad phi_i(x_q)) through
        the transposed hanging-node interpolation, constrained rows 0.  values [cell, qz, qy, qx], gradients [cell, component, qz, qy,
        qx]; either may be None, not both.  No coefficient and no sigma are applied."""
        v, g = self._points_array(values, 1, n_q, "integrate"), self._points_array(gradients, 3, n_q, "integrate")
        b = np.zeros(self.n_dofs)
        _chk(_lib.mgamd_dofs_integrate(self._h, None if v is None else _ptr(v), None if g is None else _ptr(g), C.c_int(n_q), _ptr(b)))
        return b

    def evaluate(self, u, n_q: int = 0, values: bool = True, gradients: bool = False):
        """u_h [cell, qz, qy, qx] and/or grad u_h [cell, component, qz, qy, qx] of the host vector u at quadrature_points(n_q)
        (mgamd_dofs_evaluate; in deal.II: FEEvaluation::evaluate): the values, the gradients, or the tuple of both.  Hanging entries of
        u are never read."""
        u = self._data_array(u, "evaluate")
        nq = self.degree + 2 if n_q == 0 else int(n_q)
        shape = (self.info.n_cells, nq, nq, nq) if self.degree + 1 <= nq <= self.degree + 3 else (1, 1, 1, 1)
        v = np.zeros(shape) if values else None
        g = np.zeros((shape[0], 3) + shape[1:]) if gradients else None
        _chk(_lib.mgamd_dofs_evaluate(self._h, _ptr(u), C.c_int(n_q), None if v is None else _ptr(v), None if g is None else _ptr(g)))
        return (v, g) if values and gradients else (v if values else g)

    @staticmethod
    def _points(points, who):
        """caller points as a contiguous double array [n, 3]"""
        xyz = np.ascontiguousarray(points, dtype=np.float64)
        if xyz.size == 0:
            return xyz.reshape(0, 3)
        if xyz.ndim == 1 and xyz.size == 3:
            xyz = xyz.reshape(1, 3)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f"{who}: points of shape {xyz.shape}, expected [n, 3]")
        return xyz

    def locate_points(self, points):
        """(cells [n] int32, -1: not found; reference_points [n, 3]) of points [n, 3] in [-1, 1]^3 (mgamd_dofs_locate_points; in deal.II:
        GridTools::find_active_cell_around_point).  A point on an interior face, edge or vertex belongs to the leaf on its upper side, a
        point on a face = +1 to the last leaf; no tolerance outside the cube."""
        xyz = self._points(points, "locate_points")
        cell, ref = np.full(len(xyz), -1, np.int32), np.zeros((len(xyz), 3))
        _chk(_lib.mgamd_dofs_locate_points(self._h, C.c_uint64(len(xyz)), _ptr(xyz), _ptr(cell), _ptr(ref)))
        return cell, ref

    def point_evaluate(self, points, u, values: bool = True, gradients: bool = False):
        """u_h [n] and/or grad u_h [3, n] of the host vector u at points [n, 3] (mgamd_dofs_point_evaluate; in deal.II:
        VectorTools::point_value / point_gradient): the values, the gradients, or the tuple of both.  Gradients are the one-sided
        gradients of the point's leaf; points that are not found get exactly 0 (locate_points tells); hanging entries of u are never read."""
        xyz = self._points(points, "point_evaluate")
        u = self._data_array(u, "point_evaluate")
        v = np.zeros(len(xyz)) if values else None
        g = np.zeros((3, len(xyz))) if gradients else None
        _chk(_lib.mgamd_dofs_point_evaluate(self._h, C.c_uint64(len(xyz)), _ptr(xyz), _ptr(u), None if v is None else _ptr(v),
                                            None if g is None else _ptr(g)))
        return (v, g) if values and gradients else (v if values else g)

    def point_integrate(self, points, values=None, gradients=None):
        """b_i = sum_k (values_k phi_i(x_k) + gradients_k . grad phi_i(x_k)) through the transposed hanging-node interpolation, host
        vector (mgamd_dofs_point_integrate; in deal.II: VectorTools::create_point_source_vector): point loads without quadrature weight
        or h^3, values [n] (Dirac), gradients [3, n] (dipole); either may be None, not both.  Constrained rows are 0, points that are
        not found add nothing."""
        xyz = self._points(points, "point_integrate")

        def data(a, per_point):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != per_point * len(xyz):
                raise ValueError(f"point_integrate: {a.size} values for {per_point} x {len(xyz)} points")
            return a

        v, g = data(values, 1), data(gradients, 3)
        b = np.zeros(self.n_dofs)
        _chk(_lib.mgamd_dofs_point_integrate(self._h, C.c_uint64(len(xyz)), _ptr(xyz), None if v is None else _ptr(v),
                                             None if g is None else _ptr(g), _ptr(b)))
        return b

    def _data_array(self, a, who):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.shape != (self.n_dofs,):
            raise ValueError(f"{who}: {a.shape} values for {self.n_dofs} DoFs")
        return a

    def keys(self):
        k = np.zeros((self.n_dofs, 5), np.int32)
        _chk(_lib.mgamd_dofs_get_keys(self._h, _ptr(k)))
        return k

    def cell_dofs(self):
        out = np.zeros((self.info.n_cells, (self.degree + 1) ** 3), np.uint32)
        _chk(_lib.mgamd_dofs_get_cell_dofs(self._h, _ptr(out)))
        return out

    def rhs_function(self, kind: int):
        """Operator::rhs for SimulationType kind (0 Constant, 1 Gaussian), host vector"""
        b = np.zeros(self.n_dofs)
        _chk(_lib.mgamd_dofs_rhs(self._h, kind, _ptr(b)))
        return b

    def distribute(self, x, kind: int):
        """AffineConstraints::distribute on a host vector (Dirichlet values of `kind`, hanging-node interpolation)"""
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        _chk(_lib.mgamd_dofs_distribute(self._h, kind, _ptr(x)))
        return x

    def rhs_constant(self):
        b = np.zeros(self.n_dofs)
        _chk(_lib.mgamd_dofs_rhs_constant(self._h, _ptr(b)))
        return b

    def groups(self):
        return [(self.info.group_B[g], self.info.group_slots[g]) for g in range(self.info.n_groups)]

    def matrix(self):
        """the assembled level matrix (Operator::get_trilinos_system_matrix) as (row_ptr, col, val), CSR with sorted columns"""
        nnz = C.c_uint64()
        _chk(_lib.mgamd_dofs_matrix(self._h, C.byref(nnz), None, None, None))
        ptr, col, val = np.zeros(self.n_dofs + 1, np.uint32), np.zeros(nnz.value, np.uint32), np.zeros(nnz.value)
        _chk(_lib.mgamd_dofs_matrix(self._h, C.byref(nnz), _ptr(ptr), _ptr(col), _ptr(val)))
        return ptr, col, val

    def amg_setup_info(self):
        """[(rows, nnz)] of the smoothed-aggregation hierarchy of the AMG coarse solver on this level, finest first"""
        n, rows, nnz = C.c_uint32(), (C.c_uint32 * 32)(), (C.c_uint64 * 32)()
        _chk(_lib.mgamd_dofs_amg_setup_info(self._h, C.byref(n), rows, nnz, 32))
        return [(rows[l], nnz[l]) for l in range(n.value)]

    def amg_hierarchy(self) -> "AmgHostHierarchy":
        """the host setup of the AMG coarse solver on this level, level by level (development entry, mgamd_dev.h)"""
        return AmgHostHierarchy(self)

    def cell_slots(self):
        grp, slot = np.zeros(self.info.n_cells, np.uint8), np.zeros(self.info.n_cells, np.uint32)
        _chk(_lib.mgamd_dofs_get_cell_slots(self._h, _ptr(grp), _ptr(slot)))
        return grp, slot

    def halo_plan(self):
        """host copy of the halo plan of a distributed level (see mgamd_dofs_halo_get)."""
        sz = (C.c_uint32 * 4)()
        _chk(_lib.mgamd_dofs_halo_sizes(self._h, sz))
        npeer, nsend, nsh, nc = (int(v) for v in sz)
        plan = dict(peers=np.zeros(npeer, np.int32), peer_offset=np.zeros(npeer + 1, np.uint32), pack_idx=np.zeros(nsend, np.uint32),
                    sh_tail=np.zeros(nsh, np.uint32), sh_ptr=np.zeros(nsh + 1, np.uint32), sh_src=np.zeros(nc, np.int32),
                    sh_owner_src=np.zeros(nsh, np.int32))
        if npeer:
            _chk(_lib.mgamd_dofs_halo_get(self._h, _ptr(plan["peers"]), _ptr(plan["peer_offset"]), _ptr(plan["pack_idx"]), _ptr(plan["sh_tail"]),
                                          _ptr(plan["sh_ptr"]), _ptr(plan["sh_src"]), _ptr(plan["sh_owner_src"])))
        return plan

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_dofs_destroy(self._h)
            self._h = None


def ls_copy_indices(active: DoFs, level_dofs: DoFs, level: int):
    """copy_to_mg / copy_from_mg index pairs (active-mesh index, level index) of refinement level `level`"""
    n = C.c_uint64()
    _chk(_lib.mgamd_ls_copy_indices(active._h, level_dofs._h, level, C.byref(n), None, None))
    g, l = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
    if n.value:
        _chk(_lib.mgamd_ls_copy_indices(active._h, level_dofs._h, level, C.byref(n), _ptr(g), _ptr(l)))
    return g, l


def transfer_tables(fine: DoFs, coarse: DoFs):
    """raw two-level tables for the CPU oracle: list of (kind, nf, coarse_idx, coarse_mask, fine_idx)."""
    npatch = (C.c_uint64 * 3)()
    nf = (C.c_uint32 * 3)()
    _chk(_lib.mgamd_transfer_tables_info(fine._h, coarse._h, npatch, nf))
    out = []
    nc3 = (coarse.degree + 1) ** 3
    for kind in range(3):
        n = npatch[kind]
        ci = np.zeros((n, nc3), np.uint32)
        cm = np.zeros(n, np.uint16)
        fi = np.zeros((n, nf[kind] ** 3), np.uint32)
        if n:
            _chk(_lib.mgamd_transfer_tables_get(fine._h, coarse._h, kind, _ptr(ci), _ptr(cm), _ptr(fi)))
        out.append((kind, int(nf[kind]), ci, cm, fi))
    return out


class Context:
    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        _chk(_lib.mgamd_ctx_create(device, C.byref(self._h)))

    def synchronize(self):
        _chk(_lib.mgamd_ctx_synchronize(self._h))

    def stream(self) -> int:
        s = C.c_void_p()
        _chk(_lib.mgamd_ctx_stream(self._h, C.byref(s)))
        return s.value

    def kernel_profile(self, enable: bool, brick_size: int = 0):
        _chk(_lib.mgamd_ctx_kernel_profile_brick(self._h, brick_size))
        _chk(_lib.mgamd_ctx_kernel_profile(self._h, 1 if enable else 0))

    def kernel_profile_read(self):
        ms, n, b = C.c_double(), C.c_uint64(), C.c_double()
        _chk(_lib.mgamd_ctx_kernel_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(b)))
        return ms.value, n.value, b.value

    def kernel_profile_bytes_moved(self):
        b = C.c_double()
        _chk(_lib.mgamd_ctx_kernel_profile_bytes_moved(self._h, C.byref(b)))
        return b.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_ctx_destroy(self._h)
            self._h = None


class SimGroup:
    """In-process simulation of n ranks on one GPU (every rank is a host thread); for tests."""

    def __init__(self, n_ranks: int):
        self.n_ranks = n_ranks
        self._h = C.c_void_p()
        _chk(_lib.mgamd_sim_group_create(n_ranks, C.byref(self._h)))

    def comm(self, rank: int) -> "Communicator":
        h = C.c_void_p()
        _chk(_lib.mgamd_comm_sim_create(self._h, rank, C.byref(h)))
        return Communicator(h, self.n_ranks, rank, self)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_sim_group_destroy(self._h)
            self._h = None


class Communicator:
    def __init__(self, handle, n_ranks, rank, keepalive=None):
        self._h, self.n_ranks, self.rank, self._keep = handle, n_ranks, rank, keepalive

    @staticmethod
    def rccl_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _chk(_lib.mgamd_comm_rccl_unique_id(buf))
        return buf.raw

    @staticmethod
    def rccl(ctx: "Context", n_ranks: int, rank: int, unique_id: bytes) -> "Communicator":
        h = C.c_void_p()
        _chk(_lib.mgamd_comm_rccl_create(ctx._h, n_ranks, rank, C.c_char_p(unique_id), C.byref(h)))
        return Communicator(h, n_ranks, rank)

    def subset(self, group: int) -> "Communicator":
        """communicator of a level that is cut into n_ranks / group parts (Partition tiers): rank = part"""
        if group == 1:
            return self
        h = C.c_void_p()
        _chk(_lib.mgamd_comm_subset(self._h, group, C.byref(h)))
        return Communicator(h, self.n_ranks // group, self.rank // group, self)

    def allreduce_sum(self, ctx: "Context", value: float) -> float:
        r = C.c_double()
        _chk(_lib.mgamd_comm_allreduce_sum(self._h, ctx._h, C.c_double(value), C.byref(r)))
        return r.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_comm_destroy(self._h)
            self._h = None


class Vector:
    """LinearAlgebra::distributed::Vector<Number>, device resident."""

    def __init__(self, ctx: Context, n: int, number_type: int = F64, _handle=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            _chk(_lib.mgamd_vec_create(ctx._h, C.c_uint64(n), number_type, C.byref(self._h)))
        sz = C.c_uint64()
        _chk(_lib.mgamd_vec_size(self._h, C.byref(sz)))
        self.n = sz.value

    def from_host(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.n
        _chk(_lib.mgamd_vec_from_host(self._h, _ptr(a)))
        return self

    def to_host(self):
        a = np.zeros(self.n)
        _chk(_lib.mgamd_vec_to_host(self._h, _ptr(a)))
        return a

    def set(self, value: float):
        _chk(_lib.mgamd_vec_set(self._h, C.c_double(value)))

    def copy_from(self, other: "Vector"):
        _chk(_lib.mgamd_vec_copy(self._h, other._h))

    def sadd(self, s: float, a: float, x: "Vector"):
        _chk(_lib.mgamd_vec_sadd(self._h, C.c_double(s), C.c_double(a), x._h))

    def dot(self, other: "Vector") -> float:
        r = C.c_double()
        _chk(_lib.mgamd_vec_dot(self._h, other._h, C.byref(r)))
        return r.value

    def l2_norm(self) -> float:
        r = C.c_double()
        _chk(_lib.mgamd_vec_norm2(self._h, C.byref(r)))
        return r.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_vec_destroy(self._h)
            self._h = None


class PointSet:
    """Located points of one Operator (Utilities::MPI::RemotePointEvaluation): built once, used for many vectors.  Location follows
    DoFs.locate_points bit for bit.  A point that is not found gets exactly 0 from evaluate and adds nothing in integrate, silently:
    check `found`."""

    def __init__(self, op: "Operator", points):
        self.op = op  # (the set belongs to the operator: keep it alive)
        self._h = C.c_void_p()
        xyz = DoFs._points(points, "point_set")
        _chk(_lib.mgamd_level_op_point_set_create(op._h, C.c_uint64(len(xyz)), _ptr(xyz), C.byref(self._h)))
        self.n = len(xyz)
        self.cells, self.reference_points = np.full(self.n, -1, np.int32), np.zeros((self.n, 3))
        _chk(_lib.mgamd_point_set_get(self._h, None, None, _ptr(self.cells), _ptr(self.reference_points)))
        self.found = self.cells >= 0

    def all_points_found(self) -> bool:
        return bool(self.found.all())

    def evaluate(self, u: "Vector", values: bool = True, gradients: bool = False):
        """u_h [n] and/or grad u_h [3, n] (flat, component by component) at the points, in the caller's point order, as device Vectors of
        the operator's number type (mgamd_point_set_evaluate; in deal.II: VectorTools::point_values, point_gradients): the values, the
        gradients, or the tuple of both.  Gradients are the one-sided gradients of the point's leaf.  Two calls give the same bits."""
        op = self.op
        v = Vector(op.ctx, self.n, op.number_type) if values else None
        g = Vector(op.ctx, 3 * self.n, op.number_type) if gradients else None
        _chk(_lib.mgamd_point_set_evaluate(self._h, op._h, u._h if u is not None else None, v._h if v is not None else None,
                                           g._h if g is not None else None))
        return (v, g) if values and gradients else (v if values else g)

    def integrate(self, b: "Vector", values=None, gradients=None):
        """b_i = sum_k (values_k phi_i(x_k) + gradients_k . grad phi_i(x_k)) through C^T on the device (mgamd_point_set_integrate; in
        deal.II: VectorTools::create_point_source_vector).  values [n] and gradients [3, n] are Vectors or arrays (uploaded); at least
        one is given.  b is overwritten, constrained rows are 0.  Not bit-reproducible across calls where occupied leaves share rows."""
        op = self.op

        def device(a, per_point):
            if a is None or isinstance(a, Vector):
                return a
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.size != per_point * self.n:
                raise ValueError(f"point_integrate: {a.size} values for {per_point} x {self.n} points")
            return Vector(op.ctx, a.size, op.number_type).from_host(a.ravel())

        v, g = device(values, 1), device(gradients, 3)
        _chk(_lib.mgamd_point_set_integrate(self._h, op._h, v._h if v is not None else None, g._h if g is not None else None,
                                            b._h if b is not None else None))

    def _info(self):
        """(device bytes of the set, host milliseconds of its build, device milliseconds of the locate kernel, of the last evaluate and
        of the last integrate; each time 0 before the first such call) (mgamd_debug_point_set_info)"""
        b, t = C.c_uint64(), [C.c_double() for _ in range(4)]
        _chk(_lib.mgamd_debug_point_set_info(None, self._h, None, None, C.byref(b), *[C.byref(x) for x in t]))
        return (b.value,) + tuple(x.value for x in t)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_point_set_destroy(self._h)
            self._h = None


class Operator:
    """Operator<3,1,Number> (ref:include/operator.h:11-557)."""

    def __init__(self, ctx: Context, dofs: DoFs, number_type: int = F64, comm: "Communicator" = None):
        self.ctx, self.dofs, self.number_type, self.comm = ctx, dofs, number_type, comm
        self._h = C.c_void_p()
        if comm is None:
            _chk(_lib.mgamd_level_op_create(ctx._h, dofs._h, number_type, C.byref(self._h)))
        else:
            _chk(_lib.mgamd_level_op_create_distributed(ctx._h, dofs._h, number_type, comm._h, C.byref(self._h)))

    def dot(self, x: "Vector", y: "Vector") -> float:
        r = C.c_double()
        _chk(_lib.mgamd_level_op_dot(self._h, x._h, y._h, C.byref(r)))
        return r.value

    def n_owned(self) -> int:
        n = C.c_uint64()
        _chk(_lib.mgamd_level_op_n_owned(self._h, C.byref(n)))
        return n.value

    def m(self) -> int:
        n = C.c_uint64()
        _chk(_lib.mgamd_level_op_m(self._h, C.byref(n)))
        return n.value

    def mass_coefficient(self) -> float:
        """the mass coefficient the operator was built with (DoFs.set_mass_coefficient before its construction)"""
        s = C.c_double()
        _chk(_lib.mgamd_level_op_mass_coefficient(self._h, C.byref(s)))
        return s.value

    def initialize_dof_vector(self) -> Vector:
        h = C.c_void_p()
        _chk(_lib.mgamd_level_op_init_vector(self._h, C.byref(h)))
        return Vector(self.ctx, 0, _handle=h)

    def vmult(self, dst: Vector, src: Vector):
        _chk(_lib.mgamd_level_op_vmult(self._h, dst._h, src._h))

    def vmult_mass(self, dst: Vector, src: Vector):
        """dst = C^T M C src: the mass matrix of this operator's space; rows and columns of constrained DoFs are zero, the
        mass coefficient plays no role (mgamd_level_op_vmult_mass)"""
        _chk(_lib.mgamd_level_op_vmult_mass(self._h, dst._h, src._h))

    def vmult_interface_up(self, dst: Vector, src: Vector):
        """local-smoothing level: the edge matrix, A with the refinement-edge DoFs unconstrained applied to src|edge"""
        _chk(_lib.mgamd_level_op_vmult_interface_up(self._h, dst._h, src._h))

    def exchange_add_tail(self, v: Vector):
        """distributed level: the shared entries of v become the sum over the sharing ranks (compress(add))"""
        _chk(_lib.mgamd_level_op_exchange_add_tail(self._h, v._h))

    def vmult_interface_down(self, dst: Vector, src: Vector):
        """Operator::vmult_interface_down: the plain cell loop (refinement-edge DoFs as ordinary DoFs), identity on the
        constrained rows -- the matrix of Multigrid's residual step (MGInterfaceOperator::vmult)"""
        _chk(_lib.mgamd_level_op_vmult_interface_down(self._h, dst._h, src._h))

    def compute_inverse_diagonal(self, diagonal: Vector):
        _chk(_lib.mgamd_level_op_inverse_diagonal(self._h, diagonal._h))

    def rhs(self, b: Vector, kind: int = 0):
        """Operator::rhs; kind = SimulationType (0 "Constant": f = 1, g = 0; 1 "Gaussian")"""
        _chk(_lib.mgamd_level_op_rhs_kind(self._h, kind, b._h))

    def rhs_boundary_flux(self, b: Vector, q):
        """b = boundary load of one constant flux per face (DoFs.rhs_boundary_flux), completed over the ranks like rhs"""
        q = _flux_array(q)
        _chk(_lib.mgamd_level_op_rhs_boundary_flux(self._h, _ptr(q), b._h))

    def distribute(self, x: Vector, kind: int = 0):
        """constraints.distribute(solution): Dirichlet values of `kind`, hanging nodes interpolated"""
        _chk(_lib.mgamd_level_op_distribute(self._h, kind, x._h))

    def rhs_dirichlet(self, b: Vector, g: Vector, include_mass: bool = True):
        """b = the lifting of the Dirichlet data g (DoFs.rhs_dirichlet) by the device kernel over the cells that gather a
        Dirichlet DoF; overwrites b, stream-ordered, completed over the ranks (mgamd_level_op_rhs_dirichlet)"""
        _chk(_lib.mgamd_level_op_rhs_dirichlet(self._h, g._h, 1 if include_mass else 0, b._h))

    def distribute_values(self, x: Vector, g: Vector):
        """x: Dirichlet DoFs from g, then hanging DoFs from their parents, on the device (mgamd_level_op_distribute_values)"""
        _chk(_lib.mgamd_level_op_distribute_values(self._h, x._h, g._h))

    def estimate_error(self, u: Vector, q=None):
        """the jump error indicator eta_K of u per leaf, in the order of Triangulation.cells() (mgamd_level_op_estimate_error):
        eta_K^2 = h_K / 24 sum over the faces of the integral of the squared jump of the normal flux a d_n u; q: the six boundary
        fluxes of rhs_boundary_flux (6 values or {face: value}) for the residual q - beta u - a d_n u on the natural and convective
        faces, None for no boundary term.  Only entries of u at free and Dirichlet DoFs are read.  Returns a host array."""
        eta = np.zeros(self.dofs.info.n_cells, np.float64)
        qa = None if q is None else _flux_array(q)
        _chk(_lib.mgamd_level_op_estimate_error(self._h, u._h, None if qa is None else _ptr(qa), _ptr(eta)))
        return eta

    def _estimator_info(self):
        """(bytes of the indicator's device tables and scratch, host milliseconds of their build, device milliseconds of the two
        kernels of the last call); zeros before the first estimate_error (mgamd_debug_level_op_estimator_info)"""
        b, t0, t1 = C.c_uint64(), C.c_double(), C.c_double()
        _chk(_lib.mgamd_debug_level_op_estimator_info(self._h, C.byref(b), C.byref(t0), C.byref(t1)))
        return b.value, t0.value, t1.value

    def integrate_difference(self, u: Vector, exact, norm: int, n_q: int = 0):
        """the error norm of u_h - w per leaf, in the order of Triangulation.cells() (mgamd_level_op_integrate_difference; in deal.II:
        VectorTools::integrate_difference): NORM_L2, NORM_H1_SEMINORM, NORM_ENERGY (a |grad e|^2 + sigma e^2 with the sigma the
        operator was built with; volume terms only) or NORM_LINFTY over QGauss(n_q)^3 per leaf, n_q = 0 for degree + 2.
        exact, the function w:
          * an int: the built-in kind, 0 for w = 0 (the norms of u_h), 1 for the Gaussian of SimulationType "Gaussian";
          * an array or Vector: the values of w at DoFs.quadrature_points(n_q), [cell, qz, qy, qx];
          * a tuple (values, gradients): gradients [cell, component, qz, qy, qx], read by the two gradient norms; values may be None
            for the H1 seminorm;
          * a callable f(x, y, z), or a tuple (f, grad_f) with grad_f(x, y, z) returning the three components: tabulated at the
            quadrature points on the host and uploaded.
        Only entries of u at free and Dirichlet DoFs are read.  Returns a host array; compute_global_error gives the global value."""
        out = np.zeros(self.dofs.info.n_cells, np.float64)
        if isinstance(exact, (int, np.integer)) and not isinstance(exact, bool):
            _chk(_lib.mgamd_level_op_integrate_difference(self._h, u._h, C.c_int(int(exact)), C.c_int(n_q), C.c_int(norm), _ptr(out)))
            return out
        values, gradients = exact if isinstance(exact, tuple) else (exact, None)
        v, g = self._quadrature_data(values, gradients, n_q)
        _chk(_lib.mgamd_level_op_integrate_difference_values(self._h, u._h, v._h if v is not None else None, g._h if g is not None else None,
                                                             C.c_int(n_q), C.c_int(norm), _ptr(out)))
        return out

    def _quadrature_data(self, values, gradients, n_q):
        """caller data at DoFs.quadrature_points(n_q) as device Vectors of the operator's number type (the rule of integrate_difference
        and integrate): each of values [cell, qz, qy, qx] and gradients [cell, component, qz, qy, qx] may be None, a Vector (passed
        through), an array (uploaded), or a callable of (x, y, z) tabulated at the points on the host (gradients: returning the three
        components) and uploaded"""
        points = None
        if callable(values) or callable(gradients):
            points = np.moveaxis(self.dofs.quadrature_points(n_q), -1, 0)  # (refuses n_q by name)

        def device(a, per_point):
            if a is None or isinstance(a, Vector):
                return a
            if callable(a):
                a = a(*points)
                if per_point == 3:
                    a = np.stack([np.broadcast_to(np.asarray(c, np.float64), points[0].shape) for c in a], axis=1)
                else:
                    a = np.broadcast_to(np.asarray(a, np.float64), points[0].shape)
            a = np.ascontiguousarray(a, dtype=np.float64)
            return Vector(self.ctx, a.size, self.number_type).from_host(a.ravel())

        return device(values, 1), device(gradients, 3)

    def evaluate(self, u: Vector, n_q: int = 0, values: bool = True, gradients: bool = False):
        """u_h and/or grad u_h at DoFs.quadrature_points(n_q) on the device (mgamd_level_op_evaluate; in deal.II:
        FEEvaluation::evaluate over a cell loop): device Vectors of the operator's number type, values laid out [cell, qz, qy, qx] and
        gradients [cell, component, qz, qy, qx].  Returns the values, the gradients, or the tuple (values, gradients) for both.  Only
        entries of u at free and Dirichlet DoFs are read; two calls give the same bits.  n_q = 0 for degree + 2."""
        nq = self.dofs.degree + 2 if n_q == 0 else int(n_q)
        n_points = self.dofs.info.n_cells * nq ** 3 if self.dofs.degree + 1 <= nq <= self.dofs.degree + 3 else 1  # (n_q is refused by name)
        v = Vector(self.ctx, n_points, self.number_type) if values else None
        g = Vector(self.ctx, 3 * n_points, self.number_type) if gradients else None
        _chk(_lib.mgamd_level_op_evaluate(self._h, u._h if u is not None else None, C.c_int(n_q), v._h if v is not None else None,
                                          g._h if g is not None else None))
        return (v, g) if values and gradients else (v if values else g)

    def integrate(self, b: Vector, values=None, gradients=None, n_q: int = 0):
        """b_i = sum_K sum_q w_q h_K^3 (values_q phi_i(x_q) + gradients_q . grad phi_i(x_q)) through C^T on the device
        (mgamd_level_op_integrate; in deal.II: FEEvaluation::integrate, VectorTools::create_right_hand_side): the load of a source
        (values = f), the divergence-form load (gradients = F) or both.  Each of values and gradients is a Vector, an array or a
        callable tabulated at DoFs.quadrature_points(n_q), by the rule of integrate_difference's `exact`; at least one is given.  b is
        overwritten, constrained rows are 0; no coefficient and no sigma are applied.  Not bit-reproducible across calls."""
        v, g = self._quadrature_data(values, gradients, n_q)
        _chk(_lib.mgamd_level_op_integrate(self._h, v._h if v is not None else None, g._h if g is not None else None, C.c_int(n_q),
                                           b._h if b is not None else None))

    def _cell_values_info(self):
        """(bytes of the device arrays evaluate and integrate use: the shared gather table; device milliseconds of the last evaluate
        and of the last integrate); zeros before the first call (mgamd_debug_level_op_cell_values_info)"""
        b, t0, t1 = C.c_uint64(), C.c_double(), C.c_double()
        _chk(_lib.mgamd_debug_level_op_cell_values_info(self._h, C.byref(b), C.byref(t0), C.byref(t1)))
        return b.value, t0.value, t1.value

    def point_set(self, points) -> "PointSet":
        """points [n, 3] of [-1, 1]^3 located on the operator's leaves on the device, once, for many vectors
        (mgamd_level_op_point_set_create; in deal.II: Utilities::MPI::RemotePointEvaluation::reinit)"""
        return PointSet(self, points)

    def _point_tables_bytes(self):
        """(bytes of the device arrays only the operator's point sets use, 0 before the first point set; bytes of the shared gather
        table, 0 until some call has built it) (mgamd_debug_point_set_info)"""
        b, g = C.c_uint64(), C.c_uint64()
        _chk(_lib.mgamd_debug_point_set_info(self._h, None, C.byref(b), C.byref(g), None, None, None, None, None))
        return b.value, g.value

    def _error_norm_info(self):
        """(bytes of the device arrays the error norms use, the shared gather table included; device milliseconds of the kernel of the
        last call; whether the indicator's neighbour table is built); zeros before the first integrate_difference
        (mgamd_debug_level_op_error_norm_info)"""
        b, t, nb = C.c_uint64(), C.c_double(), C.c_int()
        _chk(_lib.mgamd_debug_level_op_error_norm_info(self._h, C.byref(b), C.byref(t), C.byref(nb)))
        return b.value, t.value, bool(nb.value)

    def get_system_matrix(self) -> "SparseMatrix":
        """Operator::get_trilinos_system_matrix: the assembled matrix of this operator's DoFs on the device (FP64, one rank)"""
        if self.dofs.mass_coefficient() != self.mass_coefficient():  # the matrix is assembled from the DoFs' tables
            raise MgamdError(f"get_system_matrix: the mass coefficient of the DoFs ({self.dofs.mass_coefficient()}) was changed after this "
                             f"operator was built with {self.mass_coefficient()}; the assembled matrix would be another operator's")
        return SparseMatrix(self.ctx, self.dofs)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_level_op_destroy(self._h)
            self._h = None


class PreconditionChebyshev:
    def __init__(self, op: Operator, degree=3, smoothing_range=20.0, eig_cg_n_iterations=20):
        self.op = op
        self._h = C.c_void_p()
        _chk(_lib.mgamd_cheb_create(op._h, degree, C.c_double(smoothing_range), eig_cg_n_iterations, C.byref(self._h)))

    def vmult(self, dst: Vector, src: Vector):
        _chk(_lib.mgamd_cheb_vmult(self._h, dst._h, src._h))

    def step(self, dst: Vector, src: Vector):
        _chk(_lib.mgamd_cheb_step(self._h, dst._h, src._h))

    def eigenvalue_estimates(self):
        lo, hi = C.c_double(), C.c_double()
        _chk(_lib.mgamd_cheb_get_eigen_estimates(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_cheb_destroy(self._h)
            self._h = None


class MGTwoLevelTransfer:
    def __init__(self, fine: Operator, coarse: Operator):
        self.fine, self.coarse = fine, coarse
        self._h = C.c_void_p()
        _chk(_lib.mgamd_transfer2_create(fine._h, coarse._h, C.byref(self._h)))

    def prolongate_and_add(self, dst_fine: Vector, src_coarse: Vector):
        _chk(_lib.mgamd_transfer2_prolongate_and_add(self._h, dst_fine._h, src_coarse._h))

    def restrict_and_add(self, dst_coarse: Vector, src_fine: Vector):
        _chk(_lib.mgamd_transfer2_restrict_and_add(self._h, dst_coarse._h, src_fine._h))

    def n_fused_bricks(self):
        """fine bricks whose share of this transfer runs inside the operator passes of the V-cycle (0: none)"""
        n = C.c_uint64()
        _chk(_lib.mgamd_transfer2_n_fused_bricks(self._h, C.byref(n)))
        return n.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_transfer2_destroy(self._h)
            self._h = None


STAGE_NAMES = ["pre_smoother_step", "residual_step", "restriction", "coarse_solve", "prolongation", "edge_prolongation",
               "post_smoother_step", "transfer_to_mg", "transfer_to_global"]
_STAGE_CB = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_uint, C.c_void_p)


class PreconditionMG:
    """Multigrid<Vector> + PreconditionMG over MGTransferGlobalCoarsening."""

    def __init__(self, ctx: Context, levels, transfers, smoothers, coarse_solver="direct", nested: "PreconditionMG" = None,
                 n_cycles: int = 1, local_smoothing: "DoFs" = None, sharded_amg: "DoFs" = None,
                 amg_min_sharded_rows: int = AMG_MIN_SHARDED_ROWS_DEFAULT):
        """nested: geometric stand-in for the AMG coarse solvers on a large coarse level (an h-multigrid whose finest level
        is levels[0]), applied n_cycles times per coarse solve; see mgamd.h.
        local_smoothing: the DoFs of the ACTIVE mesh; `levels` are then operators on the refinement levels (HMG-local)
        sharded_amg: the GLOBAL DoFs of level 0's space; the AMG coarse solvers then run on the sharded level 0 (replicated setup,
        sharded cycle: mgamd_mg_create_sharded_amg), levels of at most amg_min_sharded_rows rows replicated"""
        self.ctx, self.levels, self.transfers, self.smoothers, self.nested = ctx, levels, transfers, smoothers, nested
        self.sharded_amg = sharded_amg
        n = len(levels)
        L = (C.c_void_p * n)(*[l._h for l in levels])
        T = (C.c_void_p * n)(*[(t._h if t is not None else None) for t in transfers])
        S = (C.c_void_p * n)(*[(s._h if s is not None else None) for s in smoothers])
        self._h = C.c_void_p()
        if sharded_amg is not None:
            if local_smoothing is not None or nested is not None:
                raise MgamdError("sharded_amg excludes local smoothing and a nested multigrid")
            _chk(_lib.mgamd_mg_create_sharded_amg(ctx._h, n, L, T, S, coarse_solver.encode(), sharded_amg._h, n_cycles,
                                                  C.c_uint32(amg_min_sharded_rows), C.byref(self._h)))
        elif local_smoothing is not None:
            _chk(_lib.mgamd_mg_create_local_smoothing(ctx._h, n, L, T, S, local_smoothing._h, coarse_solver.encode(), C.byref(self._h)))
        else:
            _chk(_lib.mgamd_mg_create_nested(ctx._h, n, L, T, S, coarse_solver.encode(), nested._h if nested is not None else None, n_cycles,
                                             C.byref(self._h)))
        self._cb = None

    def set_collapse(self, enable: bool) -> int:
        """switch the tabulated coarse levels off/on; returns the collapse level (0: none)"""
        l = C.c_uint()
        _chk(_lib.mgamd_mg_set_collapse(self._h, 1 if enable else 0, C.byref(l)))
        return l.value

    def coarse_solver_used(self) -> str:
        buf = C.create_string_buffer(32)
        _chk(_lib.mgamd_mg_coarse_solver_used(self._h, buf))
        return buf.value.decode()

    def coarse_iterations(self) -> int:
        """inner CG iterations of the coarse solver (cg, cg_with_chebyshev, cg_with_amg) since construction"""
        n = C.c_uint64()
        _chk(_lib.mgamd_mg_coarse_iterations(self._h, C.byref(n)))
        return n.value

    def amg_layout(self):
        """the levels of the algebraic coarse solver that runs, finest first: dicts of global_rows, owned_rows, ghosts, peers,
        replicated (mgamd_mg_amg_layout); empty if no AMG runs"""
        n, info = C.c_uint32(), (C.c_uint32 * (5 * 32))()
        _chk(_lib.mgamd_mg_amg_layout(self._h, C.byref(n), info, 32))
        return [dict(global_rows=info[5 * l], owned_rows=info[5 * l + 1], ghosts=info[5 * l + 2], peers=info[5 * l + 3],
                     replicated=bool(info[5 * l + 4])) for l in range(min(n.value, 32))]

    def vmult(self, z: Vector, r: Vector):
        _chk(_lib.mgamd_mg_vcycle(self._h, z._h, r._h))

    def connect_stages(self, fn):
        """fn(stage:int, start:bool, level:int) or None; see STAGE_NAMES."""
        if fn is None:
            self._cb = None
            _chk(_lib.mgamd_mg_set_stage_callback(self._h, None, None))
            return
        self._cb = _STAGE_CB(lambda s, st, lv, u: fn(s, bool(st), lv))
        _chk(_lib.mgamd_mg_set_stage_callback(self._h, self._cb, None))

    def stage_timing(self, enable: bool):
        """HIP-event stage timing of the unchanged cycle (no host synchronisation inside the cycle)"""
        _chk(_lib.mgamd_mg_stage_timing(self._h, 1 if enable else 0))

    def stage_times(self):
        """milliseconds accumulated per [stage, level] since the last call (see STAGE_NAMES)"""
        n = len(self.levels)
        ms = np.zeros((9, n))
        cnt = C.c_uint64()
        _chk(_lib.mgamd_mg_stage_times(self._h, _ptr(ms), n, C.byref(cnt)))
        return ms

    def time_vcycles(self, z: Vector, r: Vector, n: int, use_graph: bool = True) -> float:
        ms = C.c_double()
        _chk(_lib.mgamd_mg_time_vcycles(self._h, z._h, r._h, n, 1 if use_graph else 0, C.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_mg_destroy(self._h)
            self._h = None


class SparseMatrix:
    """The assembled system matrix on the device (mgamd_matrix_create): what Operator::get_trilinos_system_matrix returns and
    Type "AMG" runs CG on (ref:multigrid_throughput.cc:1877-1966).  FP64; refuses distributed and local-smoothing DoFs."""

    def __init__(self, ctx: Context, dofs: DoFs):
        self.ctx, self.dofs = ctx, dofs
        self._h = C.c_void_p()
        _chk(_lib.mgamd_matrix_create(ctx._h, dofs._h, C.byref(self._h)))
        n, nnz, lanes = C.c_uint64(), C.c_uint64(), C.c_int()
        _chk(_lib.mgamd_matrix_info(self._h, C.byref(n), C.byref(nnz), C.byref(lanes)))
        self.n_rows, self.nnz, self.lanes = n.value, nnz.value, lanes.value

    def m(self) -> int:
        return self.n_rows

    def vmult(self, dst: Vector, src: Vector):
        _chk(_lib.mgamd_matrix_vmult(self._h, dst._h, src._h))

    def time_spmv(self, mode: int, lanes: int, reps: int = 50) -> float:
        """measurement (tools/spmv_bench.py): milliseconds per launch of the product in `mode` (SPMV_PLAIN, SPMV_CHEB, SPMV_DOT)
        at `lanes` lanes per row, HIP events around `reps` launches"""
        ms = C.c_double()
        _chk(_lib.mgamd_debug_matrix_time_spmv(self._h, mode, lanes, reps, C.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_matrix_destroy(self._h)
            self._h = None


class PreconditionAMG:
    """TrilinosWrappers::PreconditionAMG on a SparseMatrix (mgamd_amg_create): n_cycles V-cycles of the library's
    smoothed-aggregation AMG; level 0 works on the matrix's own device arrays."""

    def __init__(self, matrix: SparseMatrix, n_cycles: int = 1):
        self.matrix, self.n_cycles = matrix, n_cycles
        self._h = C.c_void_p()
        _chk(_lib.mgamd_amg_create(matrix._h, n_cycles, C.byref(self._h)))

    def vmult(self, z: Vector, r: Vector):
        _chk(_lib.mgamd_amg_vmult(self._h, z._h, r._h))

    def layout(self):
        """rows of every AMG level, finest first"""
        n, rows = C.c_uint32(), (C.c_uint32 * 32)()
        _chk(_lib.mgamd_amg_layout(self._h, C.byref(n), rows, 32))
        return [rows[l] for l in range(min(n.value, 32))]

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_amg_destroy(self._h)
            self._h = None


def solve_cg(A, preconditioner, x: Vector, b: Vector, reltol=1e-4, abstol=1e-20, maxiter=10000):
    """SolverCG<Vector>(ReductionControl(maxiter, abstol, reltol)).solve(A, x, b, preconditioner) from x = 0.
    A: an Operator with a PreconditionMG (or None), or a SparseMatrix with a PreconditionAMG built on it (or None)."""
    it, res = C.c_uint(), C.c_double()
    ph = preconditioner._h if preconditioner is not None else None
    if isinstance(A, SparseMatrix):
        if preconditioner is not None and not isinstance(preconditioner, PreconditionAMG):
            raise MgamdError("solve_cg: a SparseMatrix takes a PreconditionAMG (or None)")
        _chk(_lib.mgamd_solve_cg_matrix(A._h, ph, x._h, b._h, C.c_double(reltol), C.c_double(abstol), maxiter, C.byref(it), C.byref(res)))
        return it.value, res.value
    if isinstance(preconditioner, PreconditionAMG):
        raise MgamdError("solve_cg: a PreconditionAMG goes with the SparseMatrix it was built on")
    _chk(_lib.mgamd_solve_cg(A._h, ph, x._h, b._h, C.c_double(reltol), C.c_double(abstol), maxiter, C.byref(it), C.byref(res)))
    return it.value, res.value


class TimeStepper:
    """theta-scheme for the heat equation M u' + K u = M f with constant step dt (mgamd_time_stepper).  op: the FP64 operator
    K + sigma M of a hierarchy built with mass_coefficient=TimeStepper.mass_coefficient(theta, dt) (Hierarchy.fine_operator,
    DistributedHierarchy.fine_operator), mg: its multigrid.  step() advances u in place, with u as the initial guess: the CG
    solves for the increment and reltol acts on the increment's residual."""

    def __init__(self, op: Operator, mg: "PreconditionMG", theta: float, dt: float):
        self.op, self.mg = op, mg  # (kept alive)
        self._h = C.c_void_p()
        _chk(_lib.mgamd_time_stepper_create(op._h, mg._h if mg is not None else None, C.c_double(theta), C.c_double(dt), C.byref(self._h)))

    @staticmethod
    def mass_coefficient(theta: float, dt: float) -> float:
        """sigma = 1 / (theta dt)"""
        return 1.0 / (theta * dt)

    def step(self, u: Vector, f_old: Vector = None, f_new: Vector = None, reltol=1e-4, abstol=1e-20, maxiter=10000, g_old: Vector = None,
             g_new: Vector = None, load: Vector = None):
        """one step; f_old / f_new: nodal source values at t and t + dt (both None: f = 0).  g_old / g_new: Dirichlet values at t and
        t + dt (both None: homogeneous data), load: a boundary load theta l_new + (1 - theta) l_old (Operator.rhs_boundary_flux);
        with one of the three the step is mgamd_time_stepper_step_data.  Returns the CG's iterations and final residual norm.
        Constrained entries of u are not read and are 0 on return: Operator.distribute_values(u, g_new) fills them for output."""
        it, res = C.c_uint(), C.c_double()
        h = lambda v: v._h if v is not None else None
        if g_old is None and g_new is None and load is None:
            _chk(_lib.mgamd_time_stepper_step(self._h, u._h, h(f_old), h(f_new), C.c_double(reltol), C.c_double(abstol), maxiter,
                                              C.byref(it), C.byref(res)))
        else:
            _chk(_lib.mgamd_time_stepper_step_data(self._h, u._h, h(f_old), h(f_new), h(g_old), h(g_new), h(load), C.c_double(reltol),
                                                   C.c_double(abstol), maxiter, C.byref(it), C.byref(res)))
        return it.value, res.value

    def time(self) -> float:
        t = C.c_double()
        _chk(_lib.mgamd_time_stepper_time(self._h, C.byref(t), None))
        return t.value

    def n_steps(self) -> int:
        n = C.c_uint64()
        _chk(_lib.mgamd_time_stepper_time(self._h, None, C.byref(n)))
        return n.value

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_time_stepper_destroy(self._h)
            self._h = None


class AmgHostHierarchy:
    """Smoothed-aggregation hierarchy of the "amg" coarse solvers as the host setup builds it (amg.hpp; mgamd_dev.h), finest level
    first: level(l) returns dict(A, P, agg, n_aggregates, lambda_max) with A, P as (row_ptr, col, val) CSR triples (P None on
    the coarsest level) and agg the aggregate of each row (-1: decoupled; None on the coarsest level)."""

    def __init__(self, dofs: DoFs):
        self._h = C.c_void_p()
        _chk(_lib.mgamd_debug_amg_host_create(dofs._h, C.byref(self._h)))
        n = C.c_uint32()
        _chk(_lib.mgamd_debug_amg_host_n_levels(self._h, C.byref(n)))
        self.n_levels = n.value

    def level(self, l: int):
        rows, nnz_a, cols_p, nnz_p, na, lam = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_double()
        _chk(_lib.mgamd_debug_amg_host_level_info(self._h, C.c_uint32(l), C.byref(rows), C.byref(nnz_a), C.byref(cols_p), C.byref(nnz_p),
                                                 C.byref(na), C.byref(lam)))
        n, coarsest = rows.value, l + 1 == self.n_levels
        A = (np.zeros(n + 1, np.uint32), np.zeros(nnz_a.value, np.uint32), np.zeros(nnz_a.value))
        P = (np.zeros(n + 1, np.uint32), np.zeros(nnz_p.value, np.uint32), np.zeros(nnz_p.value))
        agg = np.zeros(n, np.int32)
        _chk(_lib.mgamd_debug_amg_host_level_get(self._h, C.c_uint32(l), *[_ptr(a) for a in A], *([None] * 3 if coarsest else [_ptr(a) for a in P]),
                                                None if coarsest else _ptr(agg)))
        return dict(A=A, P=None if coarsest else P, n_cols_P=cols_p.value, agg=None if coarsest else agg, n_aggregates=na.value,
                    lambda_max=lam.value)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_debug_amg_host_destroy(self._h)
            self._h = None


class AmgShardPlans:
    """Host-only shard plans of the sharded AMG for every rank of a partition (amg_shard.hpp; mgamd_dev.h, no GPU needed): the AMG
    of multigrid level `level` (mesh index of the partition) at `degree`.  level(rank, l) returns a dict: replicated, n_global,
    n_rows, n_mirror, n_interior, n_ghost, n_recv, rows, ghost, peers, peer_offset, send_count, recv_count, send_idx and the local
    CSR triples A, P, R (None on replicated levels, which hold the global matrices of AmgHostHierarchy)."""

    def __init__(self, partition: "Partition", level: int, degree: int, max_brick: int = -1,
                 min_sharded_rows: int = AMG_MIN_SHARDED_ROWS_DEFAULT):
        self._h = C.c_void_p()
        _chk(_lib.mgamd_debug_amg_shard_create(partition._h, level, degree, max_brick, C.c_uint32(min_sharded_rows), C.byref(self._h)))
        n, ns = C.c_uint32(), C.c_uint32()
        _chk(_lib.mgamd_debug_amg_shard_n_levels(self._h, C.byref(n), C.byref(ns)))
        self.n_levels, self.n_sharded_levels, self.n_ranks = n.value, ns.value, partition.n_ranks

    def level(self, rank: int, l: int):
        info = (C.c_uint32 * 12)()
        _chk(_lib.mgamd_debug_amg_shard_level_info(self._h, rank, C.c_uint32(l), info))
        rep, ng, nr, nm, ni, ngh, nrecv, npeer, nza, nzp, nzr, rrows = (int(v) for v in info)
        out = dict(replicated=bool(rep), n_global=ng, n_rows=nr, n_mirror=nm, n_interior=ni, n_ghost=ngh, n_recv=nrecv, A=None, P=None, R=None)
        if rep:
            return out
        u32 = lambda n: np.zeros(n, np.uint32)  # noqa: E731
        out.update(rows=u32(nr), ghost=u32(nrecv), peers=np.zeros(npeer, np.int32), peer_offset=u32(npeer + 1), send_count=u32(npeer),
                   recv_count=u32(npeer), send_idx=u32(nrecv), A=(u32(nr + 1), u32(nza), np.zeros(nza)), P=(u32(nr + 1), u32(nzp), np.zeros(nzp)),
                   R=(u32(rrows + 1), u32(nzr), np.zeros(nzr)))
        _chk(_lib.mgamd_debug_amg_shard_level_get(self._h, rank, C.c_uint32(l), *[_ptr(out[k]) for k in ("rows", "ghost", "peers", "peer_offset",
                                                                                                      "send_count", "recv_count", "send_idx")],
                                                 *[_ptr(a) for a in out["A"]], *[_ptr(a) for a in out["P"]], *[_ptr(a) for a in out["R"]]))
        return out

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mgamd_debug_amg_shard_destroy(self._h)
            self._h = None


SPMV_PLAIN, SPMV_ADD, SPMV_RESID, SPMV_CHEB, SPMV_DOT = 0, 1, 2, 3, 4


def debug_csr_spmv(ctx: "Context", number_type, mode, lanes, ptr, col, val, x, y, b=None, xold=None, xold_is_y=False, dinv=None, f1=0.0,
                   f2=0.0):
    """one launch of the AMG cycle's CSR kernel (K7) through the production launcher (mgamd_debug_csr_spmv): returns (y, lanes used);
    y is the output's initial content (read by SPMV_ADD, and as xold when xold_is_y)"""
    ptr, col = np.ascontiguousarray(ptr, np.uint32), np.ascontiguousarray(col, np.uint32)
    val, x, y = (np.ascontiguousarray(a, np.float64) for a in (val, x, y))
    y = y.copy()
    opt = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (b, xold, dinv)]
    n_rows = len(ptr) - 1
    assert len(y) == n_rows and len(col) == len(val) == ptr[-1]
    used = C.c_int()
    _chk(_lib.mgamd_debug_csr_spmv(ctx._h, number_type, mode, lanes, C.c_uint32(n_rows), C.c_uint32(len(x)), _ptr(ptr), _ptr(col), _ptr(val),
                                   _ptr(x), _ptr(y), *[None if a is None else _ptr(a) for a in opt[:2]], 1 if xold_is_y else 0,
                                   None if opt[2] is None else _ptr(opt[2]), C.c_double(f1), C.c_double(f2), C.byref(used)))
    return y, used.value


def debug_csr_spmv_ex(ctx: "Context", mode, lanes, ptr, col, val, x, y, b=None, xold=None, xold_is_y=False, dinv=None, f1=0.0, f2=0.0,
                      max_blocks=0, number_type=F64):
    """debug_csr_spmv with what the assembled operator adds (mgamd_debug_csr_spmv_ex): lanes 64 (one wavefront per row) and
    SPMV_DOT; max_blocks > 0 caps the grid.  Returns (y, lanes used, blocks launched, x . y or 0.0)"""
    ptr, col = np.ascontiguousarray(ptr, np.uint32), np.ascontiguousarray(col, np.uint32)
    val, x, y = (np.ascontiguousarray(a, np.float64) for a in (val, x, y))
    y = y.copy()
    opt = [None if a is None else np.ascontiguousarray(a, np.float64) for a in (b, xold, dinv)]
    n_rows = len(ptr) - 1
    assert len(y) == n_rows and len(col) == len(val) == ptr[-1]
    used, blocks, dot = C.c_int(), C.c_int(), C.c_double()
    _chk(_lib.mgamd_debug_csr_spmv_ex(ctx._h, number_type, mode, lanes, C.c_uint32(n_rows), C.c_uint32(len(x)), _ptr(ptr), _ptr(col),
                                      _ptr(val), _ptr(x), _ptr(y), *[None if a is None else _ptr(a) for a in opt[:2]],
                                      1 if xold_is_y else 0, None if opt[2] is None else _ptr(opt[2]), C.c_double(f1), C.c_double(f2),
                                      max_blocks, C.byref(used), C.byref(blocks), C.byref(dot)))
    return y, used.value, blocks.value, dot.value


def csr_spmv_lanes_long(n_rows: int, nnz: int) -> int:
    """lanes per row the assembled operator and its AMG choose for a matrix of these sizes (64: one wavefront per row)"""
    lanes = C.c_int()
    _chk(_lib.mgamd_debug_csr_spmv_lanes_long(C.c_uint32(n_rows), C.c_uint64(nnz), C.byref(lanes)))
    return lanes.value


def amg_shard_match_rows(global_dofs: "DoFs", local_dofs: "DoFs"):
    """the first step of the sharded AMG's plans (development entry, mgamd_dev.h): the global row of every DoF of local_dofs in
    global_dofs; MgamdError if the two are not the same space (another degree, another mass coefficient)"""
    rows = np.zeros(local_dofs.n_dofs, np.uint32)
    _chk(_lib.mgamd_debug_amg_shard_match_rows(global_dofs._h, local_dofs._h, _ptr(rows)))
    return rows


def csr_row_pointers(row_counts):
    """the 32-bit row pointers assemble_level_matrix builds from 64-bit entry counts per row (host only); MgamdError when the
    matrix would need more than 2^32 - 1 entries"""
    counts = np.ascontiguousarray(row_counts, np.uint64)
    ptr = np.zeros(len(counts) + 1, np.uint32)
    _chk(_lib.mgamd_debug_csr_row_pointers(C.c_uint32(len(counts)), _ptr(counts), _ptr(ptr)))
    return ptr


COARSE_PLAIN, COARSE_NESTED, COARSE_SHARDED_AMG = 0, 1, 2  # mgamd_coarse_plan: what a coarse solver needs next to the levels


def _level_plan(mg_type: str, n_meshes: int, degree: int):
    """mgamd_level_plan: ([(mesh index, degree)] of the multigrid levels of `mg_type` over n_meshes meshes, coarse -> fine; whether
    they are local-smoothing levels).  MgamdError for a type without levels."""
    n, ls, mesh, deg = C.c_uint(), C.c_int(), (C.c_uint * 64)(), (C.c_uint * 64)()
    _chk(_lib.mgamd_level_plan(mg_type.encode(), n_meshes, degree, 64, C.byref(n), mesh, deg, C.byref(ls)))
    return [(mesh[l], deg[l]) for l in range(n.value)], bool(ls.value)


def _coarse_plan(coarse_solver: str, n_level0_dofs_global: int, level0_distributed=False, sharded_amg_requested=False) -> int:
    """mgamd_coarse_plan: COARSE_PLAIN | COARSE_NESTED (the geometric stand-in) | COARSE_SHARDED_AMG"""
    plan = C.c_int()
    _chk(_lib.mgamd_coarse_plan(coarse_solver.encode(), C.c_uint64(n_level0_dofs_global), int(level0_distributed),
                                int(sharded_amg_requested), C.byref(plan)))
    return plan.value


def _coarse_resolve(coarse_solver: str, n_level0_dofs: int, level0_sharded=False, has_nested=False, has_amg_global=False) -> str:
    """mgamd_debug_coarse_resolve: the coarse solver a multigrid built from these would report as coarse_solver_used();
    MgamdError where its construction would fail"""
    used = C.create_string_buffer(32)
    _chk(_lib.mgamd_debug_coarse_resolve(coarse_solver.encode(), C.c_uint64(n_level0_dofs), int(level0_sharded), int(has_nested),
                                         int(has_amg_global), used))
    return used.value.decode()


def _partition_defaults(n_ranks: int, p_low: int = 1):
    """mgamd_partition_defaults: (rank group of the two-tier partition, cells from which a level is cut over all ranks, over groups);
    at p_low = 1 the thresholds are DoFs: the defaults of DistributedHierarchy's min_root_dofs and min_subset_dofs"""
    group, root, sub = C.c_uint(), C.c_uint64(), C.c_uint64()
    _chk(_lib.mgamd_partition_defaults(n_ranks, p_low, C.byref(group), C.byref(root), C.byref(sub)))
    return group.value, root.value, sub.value


_, MIN_ROOT_DOFS_DEFAULT, MIN_SUBSET_DOFS_DEFAULT = _partition_defaults(1)


def _build_levels(ctx, meshes, plan, number_type, max_brick, smoother, partition=None, rank=0, level_comm=None, local_smoothing=False,
                  first_dofs=None, shared_last=None, mass_coefficient=0.0):
    """(DoFs, operators, transfers, smoothers) of the levels plan = [(mesh index, degree)], coarse -> fine.
    smoother: (degree, smoothing_range, eig_cg_n_iterations) of every PreconditionChebyshev
    partition, rank, level_comm: one rank's share of a sharded hierarchy; level_comm(mesh index) is the communicator of a distributed
    mesh, None on a replicated one
    local_smoothing: the meshes are Triangulation.level_mesh(l)
    first_dofs: existing DoFs that are level 0's (HPMG-local: the ones the local-smoothing cycle underneath acts on)
    shared_last: (dofs, operator, smoother) of another hierarchy's level that is the finest one here (the coarse stand-in)
    max_brick=-1: bricks on large levels, single-cell slots on the latency-bound small ones (level_tables.hpp)
    mass_coefficient: sigma of K + sigma M, set on every level's DoFs before its operator is built"""
    shared = [] if shared_last is None else [shared_last]
    lo, hi = int(first_dofs is not None), len(plan) - len(shared)
    dofs = [first_dofs][:lo] + [DoFs(meshes[mi], p, max_brick, partition, mi, rank, local_smoothing) for mi, p in plan[lo:hi]]
    for d in dofs:
        d.set_mass_coefficient(mass_coefficient)
    ops = [Operator(ctx, d, number_type, level_comm(mi) if level_comm else None) for d, (mi, _) in zip(dofs, plan)]
    dofs, ops = dofs + [s[0] for s in shared], ops + [s[1] for s in shared]
    transfers = [None] + [MGTwoLevelTransfer(ops[l], ops[l - 1]) for l in range(1, len(ops))]
    smoothers = [PreconditionChebyshev(op, *smoother) for op in ops[:hi]] + [s[2] for s in shared]
    return dofs, ops, transfers, smoothers


class CoarseHierarchy:
    """Geometric stand-in for the reference's AMG coarse solvers (mgamd.h: "gmg_vcycle"): the h-multigrid on the coarse
    level of a PMG hierarchy (the lowest-degree space on the finest mesh); its finest level shares that level's objects."""

    def __init__(self, ctx, tria, dofs0, op0, smoother0, smoother_degree, smoothing_range, eig_cg_n_iterations, number_type, max_brick,
                 mass_coefficient=0.0):
        self.trias = create_geometric_coarsening_sequence(tria)
        plan, _ = _level_plan("HMG-global", len(self.trias), dofs0.degree)
        self.dofs, self.operators, self.transfers, self.smoothers = _build_levels(
            ctx, self.trias, plan, number_type, max_brick, (smoother_degree, smoothing_range, eig_cg_n_iterations),
            shared_last=(dofs0, op0, smoother0), mass_coefficient=mass_coefficient)
        self.mg = PreconditionMG(ctx, self.operators, self.transfers, self.smoothers, "amg")


class Hierarchy:
    """What solve_with_global_coarsening and solve_with_local_smoothing build (ref:multigrid_throughput.cc:1443-1666, 1670-1873)."""

    def __init__(self, ctx: Context, geometry="quadrant", n_ref_global=3, degree=1, mg_type="HMG-global", n_ref_local=0,
                 smoother_degree=3, smoothing_range=20.0, eig_cg_n_iterations=20, coarse_solver="amg", number_type=F64,
                 max_brick=-1, coarse_n_cycles=1, mass_coefficient=0.0, coefficient=None, coarse_coefficient=None, dirichlet_faces=None,
                 robin=None):
        """mass_coefficient: sigma >= 0 of the operator K + sigma M (-Laplace u + sigma u) on every level, the stand-in and nested
        hierarchies included; the local-smoothing types refuse a non-zero value
        coefficient: the diffusion coefficient a of -div(a grad u) + sigma u: f(x, y, z), evaluated at the leaf centres of the
        finest mesh before the coarsening sequence is built, or one value per leaf; None keeps what the mesh carries (a = 1 for
        a named geometry).  If `geometry` is a Triangulation of the caller's, the values are SET ON IT (Triangulation.set_coefficient):
        the mesh is the carrier of the coefficient, and the caller's object shows them afterwards.
        coarse_coefficient: g(tria) -> values, called for every coarse mesh of the coarsening sequence in place of the mean over each
        leaf (create_geometric_coarsening_sequence); refused for the types without coarse meshes (PMG, HPMG-local, AMG, AMGPETSc),
        where it would have no effect.  The local-smoothing types refuse a coefficient.
        dirichlet_faces: 6-bit mask of the Dirichlet faces (Triangulation.set_dirichlet_faces); None keeps what the mesh carries (63
        for a named geometry).  Like the coefficient it is SET ON a caller's Triangulation, and every level inherits it.  The
        local-smoothing types refuse another mask than 63; mask 0 with mass_coefficient 0 (singular) is refused by the library.
        robin: Robin coefficients of the convective faces (Triangulation.set_robin_coefficients), set on the mesh after the mask; None
        keeps what the mesh carries.  The local-smoothing types refuse a positive value.  One positive value makes mask 0 with
        mass_coefficient 0 regular.  Levels with a convective face run their transfers un-fused (DESIGN.md "Convective faces")."""
        self.ctx = ctx
        self.mass_coefficient = mass_coefficient
        # `geometry` may also be a caller-built Triangulation (Triangulation.from_leaves)
        fine = geometry if isinstance(geometry, Triangulation) else Triangulation(geometry, n_ref_global, n_ref_local)
        if mg_type in ("HMG-local", "HPMG-local") and (coefficient is not None or fine.has_coefficient()):
            raise MgamdError(f"Type '{mg_type}' with a diffusion coefficient: not implemented (local smoothing: the refinement-edge "
                             "matrices have no coefficient)")
        if coarse_coefficient is not None and mg_type not in ("HMG-global", "HPMG"):
            raise MgamdError(f"Type '{mg_type}' has no coarse meshes: coarse_coefficient would have no effect")
        _apply_dirichlet_faces(fine, mg_type, dirichlet_faces, robin)
        _apply_coefficient(fine, coefficient)
        if mg_type in ("AMG", "AMGPETSc"):
            # solve_with_amg (ref:multigrid_throughput.cc:1877-1966): no multigrid levels; CG on the assembled matrix of the one
            # level with the AMG built on it: solve_cg(h.system_matrix, h.amg, x, b).  FP64 whatever number_type says, as in the
            # reference; coarse_n_cycles: AMG cycles per application.  AMGPETSc (BoomerAMG's role): the same solver.
            self.trias, self.degrees = [fine], [degree]
            self.dofs = [DoFs(fine, degree, max_brick)]
            self.dofs[0].set_mass_coefficient(mass_coefficient)
            self.fine_operator = Operator(ctx, self.dofs[0], F64)
            self.operators, self.transfers, self.smoothers, self.coarse, self.mg = [self.fine_operator], [None], [None], None, None
            self.system_matrix = self.fine_operator.get_system_matrix()
            self.amg = PreconditionAMG(self.system_matrix, coarse_n_cycles)
            self.n_dofs = self.dofs[0].n_dofs
            return
        smoother = (smoother_degree, smoothing_range, eig_cg_n_iterations)
        if mg_type == "HMG-local":
            self._build_local_smoothing(ctx, fine, degree, smoother, coarse_solver, number_type, max_brick)
            return
        # the meshes the levels live on: the coarsening sequence of the h-levels; the p-levels of PMG and HPMG-local need the one mesh
        meshes = create_geometric_coarsening_sequence(fine, coarse_coefficient) if mg_type in ("HMG-global", "HPMG") else [fine]
        plan, _ = _level_plan(mg_type, len(meshes), degree)
        first_dofs, nested = None, None
        if mg_type == "HPMG-local":
            # ref:multigrid_throughput.cc:1685-1695,1846-1860: p-multigrid on the active mesh whose coarse problem (lowest degree)
            # is handed to ONE local-smoothing V-cycle (MGCoarseGridApplyPreconditioner of the intermediate PreconditionMG)
            self._build_local_smoothing(ctx, fine, plan[0][1], smoother, coarse_solver, number_type, max_brick)
            if len(plan) == 1:
                return
            self.ls = dict(trias=self.trias, dofs=self.dofs, operators=self.operators, transfers=self.transfers, smoothers=self.smoothers,
                           mg=self.mg)
            first_dofs, nested, coarse_solver, coarse_n_cycles = self.active_dofs, self.mg, "gmg_vcycle", 1
        self.trias, self.degrees = [meshes[mi] for mi, _ in plan], [p for _, p in plan]
        self.dofs, self.operators, self.transfers, self.smoothers = _build_levels(ctx, meshes, plan, number_type, max_brick, smoother,
                                                                                  first_dofs=first_dofs, mass_coefficient=mass_coefficient)
        self.coarse = None
        if nested is None and _coarse_plan(coarse_solver, self.dofs[0].n_dofs) == COARSE_NESTED:
            # the geometric stand-in for the AMG coarse solvers on a large coarse level (PMG), on one rank by explicit request only
            # ("gmg_vcycle"): V-cycles of the h-multigrid on level 0 ("amg", "cg_with_amg" run the library's smoothed-aggregation AMG)
            self.coarse = CoarseHierarchy(ctx, self.trias[0], self.dofs[0], self.operators[0], self.smoothers[0], *smoother, number_type,
                                          max_brick, mass_coefficient)
            nested = self.coarse.mg
        self.mg = PreconditionMG(ctx, self.operators, self.transfers, self.smoothers, coarse_solver, nested, coarse_n_cycles)
        self.fine_operator = self.operators[-1] if number_type == F64 else Operator(ctx, self.dofs[-1], F64)
        self.n_dofs = self.dofs[-1].n_dofs

    def _build_local_smoothing(self, ctx, fine, degree, smoother, coarse_solver, number_type, max_brick):
        """solve_with_local_smoothing (ref:multigrid_throughput.cc:1670-1873): operators on the refinement levels 0..L of the
        octree, MGTransferMatrixFree between them, edge matrices, the outer operator on the active mesh"""
        if self.mass_coefficient != 0.0:
            raise MgamdError(f"mass coefficient {self.mass_coefficient} with local smoothing: not implemented (the refinement-edge "
                             "matrices have no mass term)")
        self.active_dofs = DoFs(fine, degree, max_brick)
        meshes = [fine.level_mesh(l) for l in range(fine.n_levels)]
        plan, local_smoothing = _level_plan("HMG-local", len(meshes), degree)
        self.trias, self.degrees = [meshes[mi] for mi, _ in plan], [p for _, p in plan]
        self.dofs, self.operators, self.transfers, self.smoothers = _build_levels(ctx, meshes, plan, number_type, max_brick, smoother,
                                                                                  local_smoothing=local_smoothing)
        self.coarse = None
        self.mg = PreconditionMG(ctx, self.operators, self.transfers, self.smoothers, coarse_solver, local_smoothing=self.active_dofs)
        self.fine_operator = Operator(ctx, self.active_dofs, F64)
        self.n_dofs = self.active_dofs.n_dofs


class DistributedHierarchy:
    """One rank's share of the hierarchy (HMG-global, PMG or HPMG): levels on meshes below the partition's root level are
    replicated, the others hold this rank's cells and exchange the partial sums of shared DoFs through `comm` (RCCL over
    xGMI in production).  The p-levels of PMG/HPMG live on the finest mesh: they inherit its partition, p-transfers are
    rank-local, and the p = 1 coarse problem of PMG is solved by the distributed CG (+ Chebyshev) or, for the AMG choices,
    by V-cycles of the (equally sharded) h-multigrid below it."""

    def __init__(self, ctx: Context, comm: Communicator, geometry="quadrant", n_ref_global=3, degree=1, smoother_degree=3,
                 smoothing_range=20.0, eig_cg_n_iterations=20, coarse_solver="amg", number_type=F64, hanging_weight=2.0, max_brick=-1,
                 min_root_dofs=MIN_ROOT_DOFS_DEFAULT, mg_type="HMG-global", coarse_n_cycles=1, subset_group=None,
                 min_subset_dofs=MIN_SUBSET_DOFS_DEFAULT, sharded_amg=False, amg_min_sharded_rows=AMG_MIN_SHARDED_ROWS_DEFAULT,
                 mass_coefficient=0.0, coefficient=None, coarse_coefficient=None, dirichlet_faces=None, robin=None):
        """dirichlet_faces, robin: as for Hierarchy (every rank passes the same)
        coefficient, coarse_coefficient: the diffusion coefficient, as for Hierarchy (every rank passes the same; set on the
        caller's Triangulation if one is passed; the coarsening sequence exists for every type here, so coarse_coefficient always acts)
        sharded_amg: run the AMG coarse solvers ("amg", "cg_with_amg", "amg_petsc") on a large coarse level as the library's
        smoothed-aggregation AMG cut into rows over the ranks (replicated setup, sharded cycle; levels of at most
        amg_min_sharded_rows rows replicated) instead of the geometric stand-in "gmg_vcycle".  Off by default."""
        self.ctx, self.comm = ctx, comm
        if mg_type not in ("HMG-global", "PMG", "HPMG"):
            raise MgamdError(f"Type '{mg_type}' not implemented")
        fine = geometry if isinstance(geometry, Triangulation) else Triangulation(geometry, n_ref_global)
        _apply_dirichlet_faces(fine, mg_type, dirichlet_faces, robin)
        _apply_coefficient(fine, coefficient)
        self.mesh_sequence = create_geometric_coarsening_sequence(fine, coarse_coefficient)
        # (mesh index, degree) of every multigrid level, coarse -> fine (ref:multigrid_throughput.cc:1506-1571)
        self.plan, _ = _level_plan(mg_type, len(self.mesh_sequence), degree)
        # levels below ~4 M DoFs stay replicated: their single-GPU time (latency-bound: 0.34 ms for 2.3 M DoFs at p=4, 0.33 ms for
        # 2.2 M at p=1) is below what a distributed level pays for its 8 halo exchanges per cycle on top of its own kernels; levels
        # between min_subset_dofs and min_root_dofs are cut into n_ranks / subset_group parts, each held by a group of ranks
        # (Partition tiers); the default group is mgamd_partition_defaults'
        p_low = min(p for _, p in self.plan)
        if subset_group is None:
            subset_group = _partition_defaults(comm.n_ranks)[0]
        self.partition = Partition(self.mesh_sequence, comm.n_ranks, hanging_weight, min_root_dofs // p_low ** 3, subset_group,
                                   min_subset_dofs // p_low ** 3)
        sub_comm = comm.subset(self.partition.group) if self.partition.group > 1 else comm
        self.level_comm = lambda mi: comm if mi >= self.partition.root_level else sub_comm
        smoother = (smoother_degree, smoothing_range, eig_cg_n_iterations)

        def mesh_comm(mi):
            return self.level_comm(mi) if comm.n_ranks > 1 and mi >= self.partition.sub_root_level else None

        def build(plan, shared_last=None):
            return _build_levels(ctx, self.mesh_sequence, plan, number_type, max_brick, smoother, self.partition, comm.rank, mesh_comm,
                                 shared_last=shared_last, mass_coefficient=mass_coefficient)

        self.trias = [self.mesh_sequence[mi] for mi, _ in self.plan]
        self.degrees = [p for _, p in self.plan]
        self.distributed = [mesh_comm(mi) is not None for mi, _ in self.plan]
        self.dofs, self.operators, self.transfers, self.smoothers = build(self.plan)
        self.coarse, self.amg_global_dofs = None, None
        mi0, p0 = self.plan[0]
        extra = _coarse_plan(coarse_solver, self.global_level_dofs(ctx)[0], self.distributed[0], sharded_amg)
        if extra == COARSE_SHARDED_AMG:
            # every rank builds the one-rank AMG from the global tables of level 0's space and keeps its rows (amg_shard.hpp)
            self.amg_global_dofs = DoFs(self.mesh_sequence[mi0], p0, max_brick)
            self.amg_global_dofs.set_mass_coefficient(mass_coefficient)
            self.mg = PreconditionMG(ctx, self.operators, self.transfers, self.smoothers, coarse_solver, None, coarse_n_cycles,
                                     sharded_amg=self.amg_global_dofs, amg_min_sharded_rows=amg_min_sharded_rows)
        else:
            if extra == COARSE_NESTED:
                # geometric stand-in for the AMG coarse solvers: the h-multigrid on level 0's space (mgamd.h, "gmg_vcycle"); the
                # algebraic multigrid is built from ONE rank's assembled matrix, so a sharded coarse level takes the stand-in
                cplan, _ = _level_plan("HMG-global", mi0 + 1, p0)
                cd, cops, ctr, csm = build(cplan, (self.dofs[0], self.operators[0], self.smoothers[0]))
                self.coarse = PreconditionMG(ctx, cops, ctr, csm, "amg")
                self.coarse.parts = (cd, [mesh_comm(mi) is not None for mi, _ in cplan])
            self.mg = PreconditionMG(ctx, self.operators, self.transfers, self.smoothers, coarse_solver, self.coarse, coarse_n_cycles)
        self.fine_operator = self.operators[-1]
        self.n_local = self.dofs[-1].n_dofs
        self.n_dofs = self.global_level_dofs(ctx)[-1]

    def global_level_dofs(self, ctx):
        """DoFs per multigrid level: owned DoFs summed over the pieces of the level (replicated levels are complete on every rank)"""
        return [int(round(self.level_comm(self.plan[l][0]).allreduce_sum(ctx, float(op.n_owned())))) if self.distributed[l]
                else self.dofs[l].n_dofs for l, op in enumerate(self.operators)]

    def layout(self):
        """how many pieces every multigrid level is cut into (n_ranks, n_ranks / group on the subset tier, 1 = replicated)"""
        return [self.partition.n_parts(mi) if self.comm.n_ranks > 1 else 1 for mi, _ in self.plan]
