/* mgamd.h -- C ABI of the MI355X-native matrix-free multigrid V-cycle.
 *
 * Drop-in boundary for the hot path of peterrum/dealii-multigrid's multigrid_throughput.cc.
 * The reference has no FFI: its path sits behind deal.II's duck-typed C++ template concepts
 * (SURVEY.md section 8b).  Every entry point below names the reference interface it replaces; the
 * header-only C++ layer `dealii_multigrid_amd/csrc/mgamd.hpp` re-exposes them as classes with
 * deal.II's method names (Operator::vmult, PreconditionChebyshev::vmult/step,
 * MGTwoLevelTransfer::prolongate_and_add, PreconditionMG::vmult, SolverCG::solve ...).
 *
 * Conventions: every function returns 0 on success and a non-zero status on failure, never
 * throws across the ABI; `mgamd_last_error()` returns the message of the calling thread's last
 * failure.  Every *_create has a *_destroy.  Vectors are device resident and owned by the library;
 * host transfer is explicit.  Calls on one context are ordered on that context's HIP stream and
 * are asynchronous unless they return data to the host.  One host thread per context.
 * Device functions fail with status MGAMD_ERR_NO_DEVICE when no gfx950 device is usable: there is
 * no CPU fallback in this library.
 */
#ifndef MGAMD_H
#define MGAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGAMD_OK 0
#define MGAMD_ERR 1
#define MGAMD_ERR_NO_DEVICE 2
#define MGAMD_ERR_INVALID 3

#define MGAMD_INVALID_DOF 0xFFFFFFFFu

typedef struct mgamd_ctx       mgamd_ctx;       /* device + stream (+ communicator)                    */
typedef struct mgamd_tria      mgamd_tria;      /* octree mesh  <-> parallel::distributed::Triangulation */
typedef struct mgamd_dofs      mgamd_dofs;      /* DoFHandler + AffineConstraints + MatrixFree tables    */
typedef struct mgamd_vec       mgamd_vec;       /* LinearAlgebra::distributed::Vector<Number>            */
typedef struct mgamd_level_op  mgamd_level_op;  /* Operator<3,1,Number>  (ref:include/operator.h:11)    */
typedef struct mgamd_cheb      mgamd_cheb;      /* PreconditionChebyshev<Operator,Vector,DiagonalMatrix> */
typedef struct mgamd_transfer2 mgamd_transfer2; /* MGTwoLevelTransfer<3,Vector>                          */
typedef struct mgamd_mg        mgamd_mg;        /* Multigrid + PreconditionMG + MGTransferGlobalCoarsening */
typedef struct mgamd_matrix    mgamd_matrix;    /* TrilinosWrappers::SparseMatrix: Operator::get_trilinos_system_matrix, on the device */
typedef struct mgamd_amg       mgamd_amg;       /* TrilinosWrappers::PreconditionAMG on that matrix                                    */
typedef struct mgamd_partition mgamd_partition; /* domain decomposition of the level hierarchy (one rank per GPU) */
typedef struct mgamd_comm      mgamd_comm;      /* communicator: RCCL over xGMI, or the in-process simulator      */
typedef struct mgamd_point_set mgamd_point_set; /* Utilities::MPI::RemotePointEvaluation: located points of one operator           */
typedef struct mgamd_sim_group mgamd_sim_group; /* the ranks of one in-process simulation                         */

const char *mgamd_last_error(void);
const char *mgamd_version(void);

/* ---------------------------------------------------------------------------------------------
 * Host-side setup (no GPU needed)
 * ------------------------------------------------------------------------------------------- */

/* GridGenerator::{hyper_cube+refine_global, create_quadrant, create_quadrant_flexible,
 * create_annulus, create_circle}: ref:multigrid_throughput.cc:2048-2062, ref:include/grid_generator.h.
 * geometry in {"hypercube","quadrant","quadrant_flexible","annulus","circle"}. */
int mgamd_tria_create(const char *geometry, unsigned n_ref_global, unsigned n_ref_local, mgamd_tria **out);
/* A caller-built mesh: the active cells of a parallel::distributed::Triangulation<3> over ONE root cell [-1,1]^3 (what the
 * reference hands to the path: ref:multigrid_throughput.cc:2048-2062 builds it, :1540-1604 consumes it), given as octree leaves
 * (level, i, j, k), 0 <= i, j, k < 2^level, in any order.  The leaves must tile the cube exactly and be 2:1 balanced across
 * faces, edges and corners (p4est's full balance, deal.II's default); otherwise MGAMD_ERR_INVALID with the offending leaf in
 * mgamd_last_error().  Zero Dirichlet data on the whole boundary, as for the named geometries (mgamd_tria_set_dirichlet_faces
 * changes that for either). */
int mgamd_tria_create_from_leaves(uint64_t n_leaves, const uint8_t *level, const uint32_t *i, const uint32_t *j, const uint32_t *k,
                                  mgamd_tria **out);
/* one level of MGTransferGlobalCoarseningTools::create_geometric_coarsening_sequence
 * (ref:multigrid_throughput.cc:2219-2224): coarsen every family once, re-balance. */
int mgamd_tria_coarsen(const mgamd_tria *fine, mgamd_tria **out);
/* Flagged refinement, this project's counterpart of Triangulation::execute_coarsening_and_refinement with refine flags only: every
 * leaf t with flags[t] != 0 (n_cells bytes, order of mgamd_tria_get_cells) is replaced by its eight children, then the minimal ripple
 * to the full 2:1 balance runs, and the result passes the checks of mgamd_tria_create_from_leaves.  A child inherits its parent's
 * diffusion coefficient value (if one is set); the dirichlet_faces mask and the Robin coefficients are copied.  parent (may be NULL):
 * for each cell of *out the index of the cell of t that is it or contains it; the caller provides AT LEAST 8 n_cells(t) entries (no
 * cell of t is split more than once, so *out has at most that many cells; mgamd_tria_info(*out) gives the number written).  On a balanced mesh no cell of t is split more than
 * once by one call, so (t, *out) is a pair the two-level transfer describes (coarse = t, fine = *out).
 * MGAMD_ERR_INVALID, by name: flags == NULL; a flagged cell at the deepest level the octree keys allow. */
int mgamd_tria_refine(const mgamd_tria *t, const uint8_t *flags, mgamd_tria **out, uint64_t *parent);
int mgamd_tria_destroy(mgamd_tria *t);
/* n_global_active_cells(), n_global_levels(), cells with a coarser face/edge neighbour
 * (table columns n_cells / n_cells_hn: ref:multigrid_throughput.cc:2177-2190, 2329-2331). */
int mgamd_tria_info(const mgamd_tria *t, uint64_t *n_cells, uint32_t *n_levels, uint64_t *n_cells_hn);
/* leaves in Morton (p4est) order; arrays of n_cells entries, any may be NULL */
int mgamd_tria_get_cells(const mgamd_tria *t, uint8_t *level, uint32_t *i, uint32_t *j, uint32_t *k, uint16_t *mask);

/* Diffusion coefficient: the operator of every level is  -div(a grad u) + sigma u  with a > 0 constant on each leaf, in the
 * matrices  K_a + sigma M,  K_a = sum over cells of a_c h_c (K (x) M (x) M + M (x) K (x) M + M (x) M (x) K).
 * set_coefficient takes n_cells values in the order of mgamd_tria_get_cells; NULL resets to a = 1, which is also the state of a
 * new triangulation.  MGAMD_ERR_INVALID, with the index and the value in mgamd_last_error(), for a value that is <= 0, NaN or
 * infinite.  get_coefficient writes n_cells values (ones if none is set).
 * mgamd_tria_coarsen carries the coefficient down: a coarse leaf gets the volume-weighted arithmetic mean of the fine leaves it
 * covers (its own value, or the mean of its eight children) -- a re-discretisation, not a Galerkin product; the caller may
 * overwrite a coarse mesh's values afterwards (e.g. with a harmonic mean).
 * mgamd_dofs_create and mgamd_dofs_create_local COPY the coefficient of their mesh: a later set_coefficient does not reach
 * tables that exist, and everything built from the tables (operators, matrices, right-hand sides, AMG) follows that copy.
 * Local smoothing with a coefficient is not implemented: mgamd_tria_level_mesh of such a triangulation is MGAMD_ERR_INVALID.
 * mgamd_mg_create_sharded_amg refuses a global_coarse_dofs whose coefficient differs from level 0's. */
int mgamd_tria_set_coefficient(mgamd_tria *t, const double *a);
int mgamd_tria_get_coefficient(const mgamd_tria *t, double *a);
int mgamd_tria_has_coefficient(const mgamd_tria *t, int *has);

/* Boundary conditions per face of the cube [-1,1]^3; this project's extension of the reference's homogeneous Dirichlet condition on
 * boundary id 0, the whole surface (ref:multigrid_throughput.cc:1585-1593).  Faces are numbered f = 2 axis + side: 0 is x = -1, 1 is
 * x = +1, 2 is y = -1, ... 5 is z = +1.  Bit f of the mask set: face f is Dirichlet; clear: natural (Neumann, zero flux unless
 * mgamd_dofs_rhs_boundary_flux adds one).  A boundary DoF is Dirichlet iff it lies on at least one Dirichlet face (shared edges and
 * corners included); a DoF on natural faces only is an ordinary unknown.  The Gaussian data g is imposed on Dirichlet faces only.
 * The default of every new triangulation is 0x3F, all Dirichlet.  MGAMD_ERR_INVALID for a mask > 63.
 * mgamd_tria_coarsen inherits the mask; mgamd_dofs_create and mgamd_dofs_create_local COPY it, as they copy the coefficient, and
 * mgamd_dofs_dirichlet_faces reads that copy.  Local smoothing is not implemented for another mask than 0x3F: mgamd_tria_level_mesh
 * is MGAMD_ERR_INVALID then.
 * Mask 0 with mass coefficient sigma == 0 is the singular pure-Neumann operator (constants in its kernel).  Operators, mass
 * products, inverse diagonals and Chebyshev smoothers are built on it; mgamd_mg_create*, mgamd_matrix_create (and with it
 * mgamd_amg_create), mgamd_dofs_amg_setup_info, mgamd_solve_cg* and mgamd_time_stepper_create are MGAMD_ERR_INVALID with the mask
 * and sigma in mgamd_last_error(): no mean-value projection is built. */
int mgamd_tria_set_dirichlet_faces(mgamd_tria *t, unsigned mask);
int mgamd_tria_get_dirichlet_faces(const mgamd_tria *t, unsigned *mask);
/* Convective (Robin) faces, this project's extension:  a grad u . n + beta_f (u - u_ext,f) = 0  on face f of the cube, beta_f >= 0, one
 * value per face in the numbering above; the default is 0 on every face (natural or Dirichlet, as the mask says).  The operator
 * becomes  A = K_a + sigma M + sum_f beta_f B_f,  B_f the surface mass matrix of face f, in every product, residual, smoother,
 * inverse diagonal and assembled matrix (not in the mass product).  u_ext needs no entry of its own: its load
 * beta_f u_ext,f int_{face f} phi_i  is mgamd_dofs_rhs_boundary_flux with q[f] = beta_f u_ext,f.
 * MGAMD_ERR_INVALID, naming the face and the value: a negative, NaN or infinite beta_f; beta_f > 0 on a face whose Dirichlet bit is
 * set (checked here against the current mask and in mgamd_tria_set_dirichlet_faces against the current beta, so the two setters
 * work in either order).  mgamd_tria_coarsen inherits the values (a re-discretisation, like the coefficient); mgamd_dofs_create and
 * mgamd_dofs_create_local COPY them, and mgamd_dofs_robin_coefficients reads that copy.  Local smoothing is not implemented with
 * any beta_f > 0: mgamd_tria_level_mesh is MGAMD_ERR_INVALID then.  One beta_f > 0 makes the operator regular: mask 0 with sigma 0
 * is then accepted by every solver.  The level transfers fused into the operator passes are not used on a level with a beta_f > 0
 * (mgamd_transfer2_n_fused_bricks reports 0 there). */
int mgamd_tria_set_robin_coefficients(mgamd_tria *t, const double beta[6]);
int mgamd_tria_get_robin_coefficients(const mgamd_tria *t, double beta[6]);

typedef struct
{
  uint32_t degree;
  uint64_t n_cells;
  uint32_t n_dofs;      /* DoFHandler::n_dofs()                                              */
  uint32_t n_interior;  /* [0, n_interior): slot-interior DoFs, contiguous per slot          */
  uint32_t n_tail;      /* then the shared unconstrained DoFs                                */
  uint32_t n_dirichlet; /* then Dirichlet DoFs                                               */
  uint32_t n_hanging;   /* then hanging-node DoFs                                            */
  uint32_t n_groups;    /* slot groups (brick sizes)                                         */
  uint32_t group_B[8];  /* cells per direction of each group's bricks                        */
  uint64_t group_slots[8];
  /* sharded levels (mgamd_dofs_create_local): the tail is [owned | copies]; *_owned count each DoF once globally */
  uint32_t n_tail_owned, n_dirichlet_owned, n_hanging_owned;
  uint32_t n_peers;       /* ranks this rank exchanges partial sums with on this level               */
  uint32_t n_halo_send;   /* tail entries sent (= received) per exchange                              */
  /* local-smoothing levels (mgamd_dofs_create_level): refinement-edge DoFs, numbered between the tail and the Dirichlet
   * DoFs: [ I | T | E | D | H ] */
  uint32_t n_edge;
  /* sharded levels: the first group_halo_slots[g] slots of group g touch DoFs shared with other ranks (the halo exchange of
   * an operator application runs underneath the remaining slots) */
  uint64_t group_halo_slots[8];
} mgamd_dofs_info_t;

/* DoFHandler::distribute_dofs(FE_Q(degree)) + zero Dirichlet on boundary id 0 + hanging-node
 * constraints + MatrixFree::reinit tables (ref:multigrid_throughput.cc:1578-1595,
 * ref:include/operator.h:24-47).  max_brick = 0 selects the largest brick that fits LDS;
 * max_brick = 1 disables bricks (every cell a generic slot); max_brick = -1 ("auto", what the
 * harness and the hierarchies use) is 0 on large levels and 1 on latency-bound small ones. */
int mgamd_dofs_create(const mgamd_tria *t, int degree, int max_brick, mgamd_dofs **out);
int mgamd_dofs_destroy(mgamd_dofs *d);
int mgamd_dofs_info(const mgamd_dofs *d, mgamd_dofs_info_t *info);
/* slot group and slot index of every cell (0xFE: cell of another rank) */
int mgamd_dofs_get_cell_slots(const mgamd_dofs *d, uint8_t *group, uint32_t *slot);
/* geometric identity of each DoF: keys[5*i..] = {px,py,pz,dirmask,level} (tests / oracle matching) */
int mgamd_dofs_get_keys(const mgamd_dofs *d, int32_t *keys);
/* per cell (p+1)^3 gathered DoF indices, x fastest; hanging entities resolved to the parent's
 * DoFs; MGAMD_INVALID_DOF marks Dirichlet DoFs */
int mgamd_dofs_get_cell_dofs(const mgamd_dofs *d, uint32_t *out);
/* Operator::rhs for f == 1, g == 0 (ref:include/operator.h:362-447, ref:multigrid_throughput.cc:2286-2291) */
int mgamd_dofs_rhs_constant(const mgamd_dofs *d, double *out);
/* Operator::rhs for SimulationType `kind` (0 "Constant": f = 1, g = 0; 1 "Gaussian": source and boundary values of
 * ref:multigrid_throughput.cc:60-125,2294-2298): QGauss(p+1) load vector minus the Dirichlet lifting, constrained rows 0
 * (ref:include/operator.h:362-447).  The lifting is that of mgamd_dofs_rhs_dirichlet, mass part included, for the Gaussian at the
 * support points of the Dirichlet DoFs. */
int mgamd_dofs_rhs(const mgamd_dofs *d, int kind, double *out);
/* AffineConstraints::distribute on a host vector of n_dofs values: mgamd_dofs_distribute_values with the boundary values of `kind`
 * at the support points of the Dirichlet DoFs (kind 0: exact zeros) */
int mgamd_dofs_distribute(const mgamd_dofs *d, int kind, double *x);
/* the dirichlet_faces mask these tables were built with (ref:multigrid_throughput.cc:1585-1593 fixes it to the whole boundary) */
int mgamd_dofs_dirichlet_faces(const mgamd_dofs *d, unsigned *mask);
/* boundary load of one constant flux q[f] per face f (a grad u . n = q_f on natural faces):  out_i = sum_f q_f int_{Gamma_f} phi_i,
 * mapped through the hanging-node constraints like the volume load of mgamd_dofs_rhs, constrained rows 0; independent of the
 * diffusion coefficient and of sigma, and additive to mgamd_dofs_rhs (ref:include/operator.h:362-447 has no boundary term).
 * MGAMD_ERR_INVALID, naming the face, for a non-zero q[f] on a Dirichlet face. */
int mgamd_dofs_rhs_boundary_flux(const mgamd_dofs *d, const double q[6], double *out);
/* the Robin coefficients these tables were built with (mgamd_tria_set_robin_coefficients).  The load of a convective face's
 * exterior temperature is mgamd_dofs_rhs_boundary_flux with q[f] = beta_f u_ext,f: that function refuses Dirichlet faces only. */
int mgamd_dofs_robin_coefficients(const mgamd_dofs *d, double beta[6]);
/* the table of boundary cell faces on convective faces that the face kernel walks (this rank's cells, Morton order): *n_faces
 * entries of (degree+1)^2 DoF indices (hanging entities resolved to the parent's DoFs, 0xFFFFFFFF on Dirichlet DoFs), one byte of
 * hanging flags (level_tables.hpp, RobinFaces) and the scale beta_f h^2.  Null arrays are skipped: call once for the count. */
int mgamd_dofs_robin_faces(const mgamd_dofs *d, uint64_t *n_faces, uint32_t *idx, uint8_t *flags, double *scale);
/* Non-zero Dirichlet data, this project's extension.  The data is a vector g of n_dofs values in the level's numbering of which only
 * the entries at Dirichlet DoFs are ever read (so the nodal interpolant of any function may be passed); a hanging node on the
 * boundary gets its value from its parents.  With g^ = g on Dirichlet DoFs and 0 elsewhere and C the hanging-node interpolation,
 *     out_i = -[C^T (K_a + s sigma M) C g^]_i  on free rows, 0 on constrained rows,  s = 1 if include_mass else 0:
 * the lifting of the data, a load vector additive to mgamd_dofs_rhs, mgamd_dofs_rhs_boundary_flux and M f.  It runs over the cells
 * of mgamd_dofs_dirichlet_cells only.  MGAMD_ERR_INVALID, naming both faces, where a face with a Robin coefficient > 0 shares an
 * edge with a Dirichlet face (every Dirichlet face but the opposite one: the face term of the lifting is not built), and for the
 * tables of a local-smoothing level. */
int mgamd_dofs_rhs_dirichlet(const mgamd_dofs *d, const double *g, int include_mass, double *out);
/* x: Dirichlet DoFs take the values of g, then hanging DoFs are interpolated from their parents; free DoFs are untouched */
int mgamd_dofs_distribute_values(const mgamd_dofs *d, const double *g, double *x);
/* g = v[f] on the Dirichlet DoFs of face f (a DoF on several Dirichlet faces takes the lowest-numbered one), 0 elsewhere.
 * MGAMD_ERR_INVALID, naming the face, for a non-finite value and for a non-zero value on a natural face. */
int mgamd_dofs_dirichlet_face_values(const mgamd_dofs *d, const double v[6], double *g);
/* the table the lifting walks: this rank's cells, in Morton order, that gather at least one Dirichlet DoF.  *n_cells entries of
 * (degree+1)^3 DoF indices (x fastest, hanging entities resolved to the parent's DoFs, Dirichlet DoFs with their real index), the
 * cell's hanging mask and scale[2] = {a h, h}.  Null arrays are skipped: call once for the count. */
int mgamd_dofs_dirichlet_cells(const mgamd_dofs *d, uint64_t *n_cells, uint32_t *idx, uint16_t *mask, double *scale);
/* support point of every DoF: xyz[3 i ..] */
int mgamd_dofs_node_positions(const mgamd_dofs *d, double *xyz);
/* The physical points of the tensor Gauss rule QGauss(n_q)^3 on every leaf (in deal.II: FEValues::get_quadrature_points over the
 * active cells), the points at which mgamd_level_op_integrate_difference_values expects its data: xyz[3 ((cell n_q + qz) n_q + qy) n_q
 * + qx) ..], leaves in the order of mgamd_tria_get_cells, qx fastest; 3 n_cells n_q^3 doubles.  Each coordinate is the leaf's corner plus
 * h times the point of the rule on [0, 1], one multiplication and one addition in double.  n_q: p + 1, p + 2 or p + 3; 0 stands for
 * p + 2.  Host only, no GPU needed.  MGAMD_ERR_INVALID, by name: any other n_q; sharded tables ("not implemented: sharded"); the
 * tables of a local-smoothing level. */
int mgamd_dofs_quadrature_points(const mgamd_dofs *d, int n_q, double *xyz);
/* Cell evaluate and integrate on the host, in double (in deal.II: FEEvaluation::evaluate / FEEvaluation::integrate over a cell loop;
 * the load of a function is VectorTools::create_right_hand_side).  The rule is QGauss(n_q)^3 on every leaf K with edge h_K, weights
 * w_q summing to 1, at the points of mgamd_dofs_quadrature_points(d, n_q, .); values are laid out [cell][qz][qy][qx], gradients
 * [cell][component][qz][qy][qx], leaves in the order of mgamd_tria_get_cells.
 * mgamd_dofs_integrate: out_i = sum_K sum_q w_q h_K^3 ( values_q phi_i(x_q) + gradients_q . grad phi_i(x_q) ), mapped through the
 * transposed hanging-node interpolation; out (n_dofs values) is overwritten and every constrained row (Dirichlet and hanging) is 0.
 * Either of values and gradients may be NULL, not both.  No coefficient and no sigma are applied: a caller who wants the load of
 * a_K F or sigma f multiplies the data.  values = f at the points is the load of the source f; gradients = F is the divergence-form
 * load int F . grad phi_i.
 * mgamd_dofs_evaluate: values and/or gradients (either may be NULL, not both) of the level's Q_p function of u, the physical
 * gradient included; entries of u at free and Dirichlet DoFs are read, hanging entries never.
 * No GPU needed.  MGAMD_ERR_INVALID, by name: n_q outside {0, p + 1, p + 2, p + 3}; sharded tables ("integrate: not implemented:
 * sharded"); the tables of a local-smoothing level; neither values nor gradients; out == NULL, u == NULL. */
int mgamd_dofs_integrate(const mgamd_dofs *d, const double *values, const double *gradients, int n_q, double *out);
int mgamd_dofs_evaluate(const mgamd_dofs *d, const double *u, int n_q, double *values, double *gradients);
/* Point evaluation and point sources on the host, in double (in deal.II: GridTools::find_active_cell_around_point;
 * VectorTools::point_value / point_gradient, FEPointEvaluation; VectorTools::create_point_source_vector).  The domain is [-1, 1]^3;
 * points are n triples xyz[3k...], always double.
 * Location.  Per coordinate s = (x + 1) 2^14 (one addition in double, then an exact scale) and c = min(2^15 - 1, floor(s)); a point
 * is FOUND iff all three s lie in [0, 2^15] (NaN is not found).  Its leaf is the one whose Morton interval holds the key of
 * (c_x, c_y, c_z): a point on an interior face, edge or vertex belongs to the leaf on its UPPER side, a point on a face = +1 to the
 * last leaf.  The reference coordinate is (s - corner) / edge per coordinate, exact after the one addition, in [0, 1) and 1 only on
 * the +1 faces.  There is no search radius and no tolerance outside the cube beyond the rounding of x + 1: a point outside by 2^-40 is not found.
 * mgamd_dofs_locate_points: cell[k] in the order of mgamd_tria_get_cells (-1: not found) and ref[3k...] (0 where not found).
 * mgamd_dofs_point_evaluate: values[k] = u_h(x_k) and/or gradients[c n + k] = d_c u_h(x_k), the physical gradient, laid out by
 * component [3][n]; either may be NULL, not both.  u_h is continuous, so values do not depend on the tie rule; gradients are the
 * ONE-SIDED gradients of the point's leaf.  Entries of u at free and Dirichlet DoFs are read, hanging entries never.  A point
 * that is not found gets exactly 0 in every output, silently: check cell[k] >= 0.
 * mgamd_dofs_point_integrate: out_i = sum_k ( values_k phi_i(x_k) + gradients_k . grad phi_i(x_k) ), mapped through the transposed
 * hanging-node interpolation: point functionals, a Dirac load and (through gradients) a dipole, with NO quadrature weight and NO
 * h^3.  out (n_dofs values) is overwritten, every constrained row (Dirichlet and hanging) is 0, points that are not found add
 * nothing; no coefficient and no sigma are applied.  Either of values and gradients may be NULL, not both.
 * No GPU needed.  MGAMD_ERR_INVALID, by name ("locate_points: ...", "point_evaluate: ...", "point_integrate: ..."): sharded tables
 * ("not implemented: sharded"); the tables of a local-smoothing level; a null pointer; neither values nor gradients. */
int mgamd_dofs_locate_points(const mgamd_dofs *d, uint64_t n, const double *xyz, int32_t *cell, double *ref);
int mgamd_dofs_point_evaluate(const mgamd_dofs *d, uint64_t n, const double *xyz, const double *u, double *values, double *gradients);
int mgamd_dofs_point_integrate(const mgamd_dofs *d, uint64_t n, const double *xyz, const double *values, const double *gradients, double *out);
/* The mass term: the operator becomes A = K + sigma M, the weak form of -Laplace u + sigma u (sigma = 1 / dt for a backward-Euler
 * step of the heat equation); this project's extension, the reference solves sigma = 0 only.  sigma is a property of the level
 * tables, next to the cell sizes and the constraints; the default is 0.  Everything DERIVED from the tables reads it when it is
 * built and keeps its own copy: mgamd_level_op_create[_distributed] (and with them smoothers, the "direct" coarse inverse and the
 * collapsed coarse levels), mgamd_dofs_matrix, mgamd_matrix_create, the AMG coarse solvers, mgamd_amg_*, and mgamd_dofs_rhs /
 * mgamd_level_op_rhs_kind for kind 1 (load -Laplace u_g + sigma u_g, Dirichlet lifting with K + sigma M; kind 0, f = 1 and g = 0, does
 * not depend on sigma).  Transfers and partitions do not depend on it.  A time-stepping caller sets the new sigma on the tables of
 * every level and re-creates operators, smoothers and the multigrid object; tables, transfer plans and partitions are reused.
 * MGAMD_ERR_INVALID, with the value in mgamd_last_error(), for sigma < 0 (indefinite Helmholtz), for NaN and infinity, and for a
 * non-zero sigma on local-smoothing level tables (mgamd_dofs_create_level: the refinement-edge matrices have no mass term).
 * mgamd_mg_create_sharded_amg refuses a global_coarse_dofs whose sigma differs from level 0's.
 * What takes mgamd_dofs alone (mgamd_dofs_matrix, mgamd_matrix_create, mgamd_dofs_rhs, mgamd_dofs_amg_setup_info) follows the
 * CURRENT sigma of the tables; what is handed an operator next to them checks that the two agree: the AMG coarse solver of
 * mgamd_mg_create*, and Operator::get_system_matrix of the C++ and Python layers, refuse tables whose sigma was changed after the
 * operator was built.  The "direct" inverse and the collapsed levels are formed through the operator itself. */
int mgamd_dofs_set_mass_coefficient(mgamd_dofs *d, double sigma);
int mgamd_dofs_mass_coefficient(const mgamd_dofs *d, double *sigma);
/* smallest and largest diffusion coefficient the tables were built with, over this rank's cells (1, 1 if the mesh had none) */
int mgamd_dofs_coefficient_range(const mgamd_dofs *d, double *min, double *max);

/* Operator::get_trilinos_system_matrix / get_petsc_system_matrix (ref:include/operator.h:244-358: MatrixFreeTools::compute_matrix of
 * the cell kernel with the constraints): the assembled level matrix C^T K C + identity on the constrained rows, CSR with sorted
 * columns, in this library's DoF numbering.  Call with NULL arrays for *nnz; row_ptr has n_dofs + 1 entries.  It is what the AMG
 * coarse solver is built on. */
int mgamd_dofs_matrix(const mgamd_dofs *d, uint64_t *nnz, uint32_t *row_ptr, uint32_t *col, double *val);
/* sizes of the smoothed-aggregation hierarchy the "amg" coarse solver builds on that matrix (mgamd_mg_create): rows and non-zeros
 * per AMG level, finest first (arrays of max_levels entries, may be NULL) */
int mgamd_dofs_amg_setup_info(const mgamd_dofs *d, uint32_t *n_levels, uint32_t *rows, uint64_t *nnz, uint32_t max_levels);

/* Local smoothing (`HMG-local`, ref:multigrid_throughput.cc:1670-1873): level `level` of the refinement hierarchy = ALL
 * cells of that refinement level, active or not (DoFHandler::distribute_mg_dofs); its DoFs + zero Dirichlet boundary +
 * refinement-edge set (MGConstrainedDoFs / MGTools::extract_inner_interface_dofs, ref:include/operator.h:49-70,539-556);
 * and the copy_to_mg / copy_from_mg index pairs of that level (MGLevelGlobalTransfer, interface DoFs skipped): call with
 * NULL arrays for the count. */
int mgamd_tria_level_mesh(const mgamd_tria *fine, unsigned level, mgamd_tria **out);
int mgamd_dofs_create_level(const mgamd_tria *level_mesh, int degree, int max_brick, mgamd_dofs **out);
int mgamd_ls_copy_indices(const mgamd_dofs *active_mesh_dofs, const mgamd_dofs *level_dofs, unsigned level, uint64_t *count,
                          uint32_t *global_idx, uint32_t *level_idx);

/* Domain decomposition (the reference partitions with p4est + RepartitioningPolicyTools,
 * ref:multigrid_throughput.cc:2066-2175).  trias: the level meshes, coarsest first.  A root level is chosen; its leaves are
 * cut in Morton order into n_ranks chunks of equal weight (hanging-node cells weigh `hanging_weight`, cf. CellWeightPolicy);
 * finer levels inherit the owner of their root ancestor, coarser levels are replicated on every rank. */
int mgamd_partition_create(const mgamd_tria *const *trias, unsigned n_levels, unsigned n_ranks, double hanging_weight,
                           mgamd_partition **out);
/* same, keeping every level with fewer than min_root_cells cells replicated (a distributed level pays one halo exchange
 * per operator application whatever its size) */
int mgamd_partition_create_ex(const mgamd_tria *const *trias, unsigned n_levels, unsigned n_ranks, double hanging_weight,
                              uint64_t min_root_cells, mgamd_partition **out);
/* Two tiers (csrc/partition.hpp): levels below the root level with at least min_sub_root_cells cells are cut into
 * n_ranks / group PARTS, each held (and worked on) by `group` consecutive ranks -- the counterpart of the reference's
 * agglomeration of coarse levels onto fewer processes (ref:multigrid_throughput.cc:379-418,1464-1501), without idle ranks.
 * group: a power of two that divides n_ranks; 1 = mgamd_partition_create_ex.  mgamd_partition_tiers reports the first such level
 * (== root level if there is none) and the group size; mgamd_dofs_create_local / mgamd_partition_get_owner accept those levels
 * (owners are part numbers there); their operators take mgamd_comm_subset(comm, group). */
int mgamd_partition_create_tiered(const mgamd_tria *const *trias, unsigned n_levels, unsigned n_ranks, double hanging_weight,
                                  uint64_t min_root_cells, unsigned group, uint64_t min_sub_root_cells, mgamd_partition **out);
int mgamd_partition_tiers(const mgamd_partition *p, unsigned *sub_root_level, unsigned *group);
int mgamd_partition_destroy(mgamd_partition *p);
/* MGTools::print_multigrid_statistics for this partition (ref:include/mg_tools.h:267-512; verbose-mode table columns
 * workload_eff, workload_path_max, vertical_eff, horizontal_eff, mem_total: ref:multigrid_throughput.cc:1657-1665), in that
 * order in stats[5]; definitions in csrc/partition.hpp */
int mgamd_partition_statistics(const mgamd_partition *p, double stats[5]);
int mgamd_partition_info(const mgamd_partition *p, unsigned *root_level, unsigned *n_ranks);
/* owner rank of every cell of a distributed level (level >= root_level) */
int mgamd_partition_get_owner(const mgamd_partition *p, unsigned level, uint16_t *owner);
/* level tables of one rank: distributed levels hold the rank's cells only (plus its halo plan), replicated levels are
 * identical to mgamd_dofs_create */
int mgamd_dofs_create_local(const mgamd_partition *p, unsigned level, unsigned rank, int degree, int max_brick, mgamd_dofs **out);

/* halo plan of a distributed level (tests / host-side emulation): sizes = {n_peers, n_send, n_shared, n_contrib};
 * peers[n_peers], peer_offset[n_peers+1], pack_idx[n_send] (tail index = global index - n_interior), and for every shared
 * tail DoF its tail index sh_tail[n_shared], CSR sh_ptr[n_shared+1] into sh_src[n_contrib] (-1 = own partial, else position
 * in the concatenated receive buffer, ascending rank order) and sh_owner_src[n_shared] (-1 if this rank owns the DoF) */
int mgamd_dofs_halo_sizes(const mgamd_dofs *d, uint32_t sizes[4]);
int mgamd_dofs_halo_get(const mgamd_dofs *d, int32_t *peers, uint32_t *peer_offset, uint32_t *pack_idx, uint32_t *sh_tail,
                        uint32_t *sh_ptr, int32_t *sh_src, int32_t *sh_owner_src);

/* raw two-level transfer tables (for the CPU oracle): kind 0 identity, 1 h-embedding, 2 p-embedding */
int mgamd_transfer_tables_info(const mgamd_dofs *fine, const mgamd_dofs *coarse, uint64_t n_patches[3], uint32_t nf[3]);
int mgamd_transfer_tables_get(const mgamd_dofs *fine, const mgamd_dofs *coarse, int kind, uint32_t *coarse_idx,
                              uint16_t *coarse_mask, uint32_t *fine_idx);

/* ---------------------------------------------------------------------------------------------
 * Hierarchy policy (plain integer functions, no GPU): what the harness, the C++ layer and the Python module build is decided
 * here and nowhere else.
 * ------------------------------------------------------------------------------------------- */

/* most DoFs of a coarse level that is solved exactly ("direct": a dense inverse) */
#define MGAMD_DIRECT_COARSE_MAX_DOFS 4096u

/* The multigrid levels of `type`, coarse -> fine, as (mesh_index[l], degrees[l]) over the caller's n_meshes meshes (coarsest first;
 * ref:multigrid_throughput.cc:1506-1571, 1685-1695).  The degrees of the p-levels are create_polynomial_coarsening_sequence(degree)
 * (bisection: 7 -> 1, 3, 7):
 *   "HMG-global"  (l, degree) on every mesh
 *   "PMG"         the p-levels on the LAST mesh (one rank passes its one mesh, a sharded run the partition's mesh sequence)
 *   "HPMG"        every mesh at the lowest degree, then the remaining p-levels on the last mesh
 *   "HMG-local"   (l, degree) on every mesh, the meshes being the refinement levels (mgamd_tria_level_mesh): *local_smoothing = 1
 *   "HPMG-local"  as "PMG"; its coarse solver is the "HMG-local" hierarchy at the lowest degree, which the caller plans separately
 * Any other type: MGAMD_ERR, "Type '...': not implemented".  MGAMD_ERR_INVALID if the levels exceed max_levels. */
int mgamd_level_plan(const char *type, unsigned n_meshes, unsigned degree, unsigned max_levels, unsigned *n_levels, unsigned *mesh_index,
                     unsigned *degrees, int *local_smoothing);

/* What the coarse solver `coarse_name` needs next to the levels, given the GLOBAL number of DoFs of level 0, whether level 0 is
 * distributed and whether the caller asked for the sharded AMG:
 *   at most MGAMD_DIRECT_COARSE_MAX_DOFS DoFs                                          -> MGAMD_COARSE_PLAIN
 *   else, "amg" | "cg_with_amg" | "amg_petsc" with the sharded AMG requested            -> MGAMD_COARSE_SHARDED_AMG
 *   else, "gmg_vcycle", or one of those three names on a distributed level 0            -> MGAMD_COARSE_NESTED
 *   else                                                                                -> MGAMD_COARSE_PLAIN
 * NESTED: build the h-multigrid on level 0's space and pass it to mgamd_mg_create_nested; SHARDED_AMG: build the global DoFs of
 * that space and call mgamd_mg_create_sharded_amg. */
#define MGAMD_COARSE_PLAIN 0
#define MGAMD_COARSE_NESTED 1
#define MGAMD_COARSE_SHARDED_AMG 2
int mgamd_coarse_plan(const char *coarse_name, uint64_t n_level0_dofs_global, int level0_distributed, int sharded_amg_requested, int *plan);

/* Defaults of mgamd_partition_create_tiered for n_ranks ranks and a hierarchy whose lowest degree is p_low: *group = 4 from 8 ranks
 * on if 4 divides n_ranks, 2 from 4 ranks on if 2 does, else 1; levels of >= 4 000 000 / p_low^3 cells (~4 M DoFs) are cut over all
 * ranks (*min_root_cells), those of >= 1 000 000 / p_low^3 cells over the groups (*min_sub_root_cells).  Any pointer may be NULL. */
int mgamd_partition_defaults(unsigned n_ranks, unsigned p_low, unsigned *group, uint64_t *min_root_cells, uint64_t *min_sub_root_cells);

/* ---------------------------------------------------------------------------------------------
 * Device runtime
 * ------------------------------------------------------------------------------------------- */
int mgamd_ctx_create(int device, mgamd_ctx **out);
int mgamd_ctx_destroy(mgamd_ctx *ctx);
int mgamd_ctx_synchronize(mgamd_ctx *ctx);
/* the HIP stream all work of this context is submitted to (hipStream_t as void*) */
int mgamd_ctx_stream(mgamd_ctx *ctx, void **stream);

/* Communicators.  RCCL: every rank calls mgamd_comm_rccl_create with the same 128-byte id obtained once from
 * mgamd_comm_rccl_unique_id (distribute it with any host-side channel, e.g. torch.distributed / MPI).  Simulator: all
 * ranks live in one process as host threads sharing one GPU; used to test the sharded path on a single device. */
int mgamd_comm_rccl_unique_id(char id[128]);
int mgamd_comm_rccl_create(mgamd_ctx *ctx, unsigned n_ranks, unsigned rank, const char id[128], mgamd_comm **out);
int mgamd_sim_group_create(unsigned n_ranks, mgamd_sim_group **out);
int mgamd_sim_group_destroy(mgamd_sim_group *g);
int mgamd_comm_sim_create(mgamd_sim_group *g, unsigned rank, mgamd_comm **out);
/* the communicator of a level that is cut into n_ranks / group parts (mgamd_partition_create_tiered): rank = part, halo peers are
 * parts, sums over the parts; keeps `base` alive */
int mgamd_comm_subset(mgamd_comm *base, unsigned group, mgamd_comm **out);
int mgamd_comm_destroy(mgamd_comm *c);
/* sum of a host scalar over all ranks (blocking) */
int mgamd_comm_allreduce_sum(mgamd_comm *c, mgamd_ctx *ctx, double value, double *result);

/* number_type: 8 = double, 4 = float (MGNumberType, ref:multigrid_throughput.cc:2430-2433) */
#define MGAMD_F64 8
#define MGAMD_F32 4

/* Vectors (LinearAlgebra::distributed::Vector: ref:include/operator.h:17) */
int mgamd_vec_create(mgamd_ctx *ctx, uint64_t n, int number_type, mgamd_vec **out);
int mgamd_vec_destroy(mgamd_vec *v);
int mgamd_vec_size(const mgamd_vec *v, uint64_t *n);
int mgamd_vec_from_host(mgamd_vec *v, const double *src); /* casts when the vector is float */
int mgamd_vec_to_host(const mgamd_vec *v, double *dst);
int mgamd_vec_set(mgamd_vec *v, double value);                       /* v = value               */
int mgamd_vec_copy(mgamd_vec *dst, const mgamd_vec *src);            /* dst = src (casts)       */
int mgamd_vec_axpy(mgamd_vec *y, double a, const mgamd_vec *x);      /* y += a x                */
int mgamd_vec_sadd(mgamd_vec *y, double s, double a, const mgamd_vec *x); /* y = s y + a x      */
int mgamd_vec_dot(const mgamd_vec *x, const mgamd_vec *y, double *result);
int mgamd_vec_norm2(const mgamd_vec *x, double *result);

/* Operator::reinit (ref:include/operator.h:24-47).  Every degree mgamd_dofs_create accepts (1 ... 7) has device kernels in both
 * number types; degrees above 7 are refused by mgamd_dofs_create with MGAMD_ERR_INVALID. */
int mgamd_level_op_create(mgamd_ctx *ctx, const mgamd_dofs *dofs, int number_type, mgamd_level_op **out);
/* same, for a level built with mgamd_dofs_create_local: vmult / inverse diagonal / rhs / smoother / transfers complete
 * the sums of shared DoFs across ranks through `comm` (may be NULL for replicated levels) */
int mgamd_level_op_create_distributed(mgamd_ctx *ctx, const mgamd_dofs *dofs, int number_type, mgamd_comm *comm, mgamd_level_op **out);
int mgamd_level_op_destroy(mgamd_level_op *op);
/* inner product over the GLOBAL vector (every DoF counted once across ranks) */
int mgamd_level_op_dot(mgamd_level_op *op, const mgamd_vec *x, const mgamd_vec *y, double *result);
/* the export half of MatrixFree::cell_loop's ghost exchange on a distributed level (LinearAlgebra::distributed::Vector::
 * compress(VectorOperation::add), ref:include/operator.h:166-167): the entries of shared DoFs of v become the sum over the
 * sharing ranks, identical on all of them; stream-ordered; no-op on a level that is not distributed.  bench.py times it. */
int mgamd_level_op_exchange_add_tail(mgamd_level_op *op, mgamd_vec *v);
/* number of DoFs this rank owns (sums to DoFHandler::n_dofs() over the ranks) */
int mgamd_level_op_n_owned(const mgamd_level_op *op, uint64_t *n);
int mgamd_level_op_m(const mgamd_level_op *op, uint64_t *n); /* Operator::m (ref:include/operator.h:123) */
/* the mass coefficient the operator was BUILT with (mgamd_dofs_set_mass_coefficient; later changes of the tables do not reach it) */
int mgamd_level_op_mass_coefficient(const mgamd_level_op *op, double *sigma);
/* Operator::initialize_dof_vector (ref:include/operator.h:140) */
int mgamd_level_op_init_vector(const mgamd_level_op *op, mgamd_vec **out);
/* Operator::vmult: dst = A src, identity on constrained rows (ref:include/operator.h:152-183) */
int mgamd_level_op_vmult(mgamd_level_op *op, mgamd_vec *dst, const mgamd_vec *src);
/* dst = C^T M C src: the mass matrix of the level's space; rows and columns of constrained DoFs are zero.  The same launches as
 * mgamd_level_op_vmult (one-rank and sharded) with three 1D mass products per lattice in place of the operator's six.  Entries of
 * src on constrained DoFs (Dirichlet, hanging) are never read; the result does not depend on the operator's mass coefficient.
 * M src is what a source f(t) contributes to a time step, the right-hand side of an L2 projection, and x^T M x the squared L2 norm.
 * MGAMD_ERR_INVALID for dst == src, vectors of the wrong size or number type, and the operator of a local-smoothing level
 * (mgamd_dofs_create_level); the active-mesh operator of a local-smoothing hierarchy is an ordinary operator and works. */
int mgamd_level_op_vmult_mass(mgamd_level_op *op, mgamd_vec *dst, const mgamd_vec *src);
/* Operator::compute_inverse_diagonal (ref:include/operator.h:228-242) */
int mgamd_level_op_inverse_diagonal(mgamd_level_op *op, mgamd_vec *diagonal);
/* Operator::rhs with f == 1, g == 0 (ref:include/operator.h:362-447) */
int mgamd_level_op_rhs(mgamd_level_op *op, mgamd_vec *rhs);
/* the same for SimulationType `kind` (see mgamd_dofs_rhs) */
int mgamd_level_op_rhs_kind(mgamd_level_op *op, int kind, mgamd_vec *rhs);
/* mgamd_dofs_rhs_boundary_flux into a device vector of the operator; on a distributed operator each rank integrates over its own
 * cells and the shared entries are completed over the ranks, as for mgamd_level_op_rhs_kind */
int mgamd_level_op_rhs_boundary_flux(mgamd_level_op *op, const double q[6], mgamd_vec *rhs);
/* constraints.distribute(solution) after the solve, for SimulationType `kind`: the boundary values of `kind` are computed on the host
 * (mgamd_dofs_distribute) and copied to the device once, in the operator's number type; the kernels of
 * mgamd_level_op_distribute_values then fill x, stream-ordered behind whatever the stream holds for x.  Nothing is copied from the
 * device to the host; the call returns when x is filled.  Works on the operator of a local-smoothing level too (its
 * refinement-edge entries are left alone). */
int mgamd_level_op_distribute(mgamd_level_op *op, int kind, mgamd_vec *x);
/* mgamd_dofs_rhs_dirichlet on the device: rhs is OVERWRITTEN with the lifting of the Dirichlet data g (a device vector of n_dofs
 * values of which only the entries at Dirichlet DoFs are read), with the operator's own mass coefficient where include_mass is set.
 * One kernel over the cells of mgamd_dofs_dirichlet_cells, stream-ordered, no host copy of a vector; on a distributed operator each
 * rank lifts over its own cells and the shared entries are completed over the ranks.  Constrained rows are 0; without a Dirichlet
 * face nothing is launched and rhs is 0.  MGAMD_ERR_INVALID for vectors of the wrong size or number type, rhs == g, the operator of
 * a local-smoothing level (the active-mesh operator of such a hierarchy is an ordinary one and works) and a convective face that
 * shares an edge with a Dirichlet face (see mgamd_dofs_rhs_dirichlet). */
int mgamd_level_op_rhs_dirichlet(mgamd_level_op *op, const mgamd_vec *g, int include_mass, mgamd_vec *rhs);
/* mgamd_dofs_distribute_values on the device, stream-ordered: the Dirichlet range of x is copied from g, then every hanging DoF is
 * interpolated from its parents (one thread per hanging DoF; a Dirichlet parent contributes the value just written).  Free entries
 * of x are untouched.  mgamd_level_op_distribute runs the same two kernels on the built-in values.  MGAMD_ERR_INVALID for vectors of
 * the wrong size or number type and for the operator of a local-smoothing level. */
int mgamd_level_op_distribute_values(mgamd_level_op *op, mgamd_vec *x, const mgamd_vec *g);
/* The jump error indicator, this project's own (in deal.II's place: KellyErrorEstimator).  For the level's Q_p function u_h (the
 * entries of u at free and Dirichlet DoFs; hanging entries are never read) and every leaf K with edge length h_K
 *     eta_K^2 = (h_K / 24) sum over the six faces F of K of  int_F r_F^2 dS
 * with r_F the jump of the normal flux a d_n u_h across F: against a neighbour of the same level; against a neighbour one level
 * coarser, whose flux is evaluated on K's face; against four finer neighbours as the sum over the four quarter faces (the weight
 * stays h_K / 24 of the cell that receives it, so a quarter face counts once for the coarse and once for the fine cell, each with
 * its own h).  On a boundary face f = 2 axis + side: nothing if q == NULL or the face is Dirichlet, else
 * r = q[f] - beta_f u_h - a d_n u_h with the outward normal, beta_f the Robin coefficient of the tables and q the six constants
 * of mgamd_level_op_rhs_boundary_flux (a convective face passes q[f] = beta_f u_ext).  a is the per-leaf diffusion coefficient.
 * h_K is the edge length, not deal.II's diameter: a constant factor that does not change which cells are marked.  The integrals
 * are exact (mass-matrix quadratic forms); all arithmetic after the load is FP64 for both number types.
 * eta: host array of n_cells values in the order of mgamd_tria_get_cells.  Two kernels, stream-ordered behind whatever the stream
 * holds for u; returns after the copy to the host.  No atomics: two calls return bit-identical arrays.  The cell table, the
 * neighbour table and the flux scratch (4 (p+1)^3 + 48 (p+1)^2 + 128 bytes per cell) are built by the first call and freed
 * with the operator; an operator that is never asked allocates and launches nothing.
 * MGAMD_ERR_INVALID, by name: a distributed operator ("not implemented: sharded"); the operator of a local-smoothing level; a
 * vector of the wrong size or number type; a non-finite q[f]; a non-zero q[f] on a Dirichlet face; eta == NULL. */
int mgamd_level_op_estimate_error(mgamd_level_op *op, const mgamd_vec *u, const double q[6], double *eta);

/* The error norms per leaf, the partner of the indicator (in deal.II: VectorTools::integrate_difference into a per-cell vector; the
 * global value is the l2 norm of that vector for the first three norms and its maximum for the last, VectorTools::compute_global_error,
 * which mgamd.hpp and the Python module provide as compute_global_error). */
#define MGAMD_NORM_L2 0
#define MGAMD_NORM_H1_SEMINORM 1
#define MGAMD_NORM_ENERGY 2
#define MGAMD_NORM_LINFTY 3
/* For the level's Q_p function u_h (the entries of u at free and Dirichlet DoFs; hanging entries are never read), an "exact" function
 * w and the tensor rule QGauss(n_q)^3 with weights w_q (summing to 1) on every leaf K with edge length h_K:
 *     MGAMD_NORM_L2           sqrt( sum_q w_q h_K^3 (u_h - w)^2 )
 *     MGAMD_NORM_H1_SEMINORM  sqrt( sum_q w_q h_K^3 |grad u_h - grad w|^2 )
 *     MGAMD_NORM_ENERGY       sqrt( sum_q w_q h_K^3 ( a_K |grad u_h - grad w|^2 + sigma (u_h - w)^2 ) )
 *     MGAMD_NORM_LINFTY       max_q |u_h - w|
 * a_K is the leaf's diffusion coefficient and sigma the mass coefficient the operator was BUILT with.  The energy norm has volume
 * terms only: no Robin surface term beta int u^2 is added.  The values are norms, not squares, like eta.
 * kind: the built-in w, evaluated on the device in double: 0 is w = 0 (the norms of u_h itself), 1 the Gaussian of SimulationType
 * "Gaussian" (the function mgamd_dofs_rhs(kind = 1) takes its data from), value and gradient in closed form.
 * n_q: p + 1, p + 2 or p + 3 points per direction; 0 stands for p + 2.
 * out: host array of n_cells values in the order of mgamd_tria_get_cells.  One kernel, stream-ordered behind whatever the stream holds
 * for u; returns after the copy to the host.  All arithmetic after the loads is FP64 for both number types; no atomics and a fixed
 * order of every leaf's sum: two calls return bit-identical arrays.  The gather table (4 (p+1)^3 + 18 bytes per cell) is the
 * indicator's, one copy, built by whichever of the two calls comes first; the norms add 32 bytes per cell.  An operator that is never
 * asked allocates and launches nothing.
 * MGAMD_ERR_INVALID, by name: a distributed operator or sharded tables ("integrate_difference: not implemented: sharded"); the
 * operator of a local-smoothing level (the active-mesh operator of such a hierarchy works); u of the wrong size or number type; n_q
 * outside {0, p + 1, p + 2, p + 3}; an unknown norm or kind; out == NULL. */
int mgamd_level_op_integrate_difference(mgamd_level_op *op, const mgamd_vec *u, int kind, int n_q, int norm, double *out);
/* The same with caller data for w at the points of mgamd_dofs_quadrature_points(d, n_q, .), device vectors in the operator's number
 * type (converted to double at the load): values, n_cells n_q^3 entries laid out [cell][qz][qy][qx], read by every norm but
 * MGAMD_NORM_H1_SEMINORM (may be NULL there); gradients, 3 n_cells n_q^3 entries laid out [cell][component][qz][qy][qx], read by
 * MGAMD_NORM_H1_SEMINORM and MGAMD_NORM_ENERGY only (may be NULL for the other two).  Note the layouts: the points come interleaved
 * (x, y, z per point), the gradients come by component.
 * MGAMD_ERR_INVALID, by name: the refusals above; values or gradients of the wrong size or number type; values == NULL where they are
 * read; a gradient norm without gradients. */
int mgamd_level_op_integrate_difference_values(mgamd_level_op *op, const mgamd_vec *u, const mgamd_vec *values, const mgamd_vec *gradients,
                                               int n_q, int norm, double *out);
/* mgamd_dofs_evaluate on the device (in deal.II: FEEvaluation::evaluate with EvaluationFlags::values | gradients over a cell loop):
 * values (n_cells n_q^3 entries, [cell][qz][qy][qx]) and/or gradients (3 n_cells n_q^3 entries, [cell][component][qz][qy][qx]) of
 * the level's Q_p function of u at the points of mgamd_dofs_quadrature_points(d, n_q, .), device vectors in the operator's number
 * type; either output may be NULL, not both.  Entries of u at free and Dirichlet DoFs are read, hanging entries never.  All arithmetic
 * after the gather is FP64 for both number types and the store converts; no atomics and a fixed order of every sum: two calls give
 * the same bits.  One kernel, stream-ordered; nothing is copied to the host.  The gather table (4 (p+1)^3 + 18 bytes per cell) is the
 * one of the indicator and the error norms, built by whichever call comes first; neither the neighbour table nor the norms' arrays
 * are built.  An operator that is never asked allocates and launches nothing.
 * MGAMD_ERR_INVALID, by name: a distributed operator or sharded tables ("evaluate: not implemented: sharded"); the operator of a
 * local-smoothing level; n_q outside {0, p + 1, p + 2, p + 3}; a vector of the wrong size or number type; neither values nor
 * gradients; u == NULL; an output that is u or the other output. */
int mgamd_level_op_evaluate(mgamd_level_op *op, const mgamd_vec *u, int n_q, mgamd_vec *values, mgamd_vec *gradients);
/* mgamd_dofs_integrate on the device (in deal.II: FEEvaluation::integrate + distribute_local_to_global over a cell loop; with
 * values = f at the points it is VectorTools::create_right_hand_side):
 *     b_i = sum_K sum_q w_q h_K^3 ( values_q phi_i(x_q) + gradients_q . grad phi_i(x_q) )   through C^T,
 * device vectors in the operator's number type in the layouts above; either input may be NULL, not both.  b is OVERWRITTEN: a
 * stream-ordered memset comes before the kernel, and every constrained row (Dirichlet and hanging) is exactly 0 whatever b held.
 * No coefficient and no sigma are applied.  The arithmetic is FP64 up to the scatter; the scatter is an atomic add in the vector's
 * number type, so a row that several leaves share takes its addends in no fixed order: the result is NOT bit-reproducible across
 * calls (it is where every row has one addend, as on a one-leaf mesh).  Stream-ordered, nothing is copied to the host; the data
 * never leaves the device.  Tables as for mgamd_level_op_evaluate.
 * MGAMD_ERR_INVALID, by name: the refusals above with "integrate:"; neither values nor gradients; b == NULL; b aliasing an input. */
int mgamd_level_op_integrate(mgamd_level_op *op, const mgamd_vec *values, const mgamd_vec *gradients, int n_q, mgamd_vec *b);
/* Point sets: the host functions above on the device (in deal.II: Utilities::MPI::RemotePointEvaluation::reinit, then
 * VectorTools::point_values / point_gradients for many vectors, and VectorTools::create_point_source_vector for the transpose).
 * mgamd_level_op_point_set_create locates n points (xyz[3k...], host memory, always double) on the leaves of the operator with one
 * kernel, by the rule of mgamd_dofs_locate_points bit for bit, and bins them by leaf into a list of occupied leaves; the set is
 * then used for many vectors (a probe inside a time loop).  The binning runs on the host when the set is built and the call
 * returns after it.  n = 0 is allowed: it uploads nothing and launches no kernel (integrate on an empty set, or on a set
 * without a found point, still overwrites b with its stream-ordered memset and records its two timing events).  The sorted Morton keys of the leaves with their corners (24 bytes per
 * leaf) are uploaded by the operator's first point set, the gather table (shared with the indicator, the norms and
 * mgamd_level_op_evaluate) by the first evaluate or integrate; an operator that is never asked holds nothing.  A set holds 28 bytes
 * per point plus 8 per found point and 8 per occupied leaf.  It belongs to its operator: its device arrays are freed by
 * mgamd_point_set_destroy or with the operator, whichever comes first, and a handle that outlives its operator refuses every call
 * but destroy.
 * mgamd_point_set_get: n, the number of found points, and per point the leaf (-1: not found) and the reference coordinate; any
 * pointer may be NULL.
 * mgamd_point_set_evaluate (VectorTools::point_values, point_gradients): values (n entries) and/or gradients (3 n entries,
 * [component][point]) of u at the points, device vectors in the operator's number type, in the CALLER'S point order; either
 * output may be NULL, not both.  Values do not depend on the tie rule of the location, gradients are the one-sided gradients of the
 * point's leaf.  Points that are not found get exactly 0, silently (mgamd_point_set_get tells).  Entries of u at free and
 * Dirichlet DoFs are read, hanging entries never.  All arithmetic after the gather is FP64 for both number types and the store
 * converts; no atomics and a fixed order of every sum: two calls give the same bits.  Stream-ordered, nothing is copied to the host.
 * mgamd_point_set_integrate (VectorTools::create_point_source_vector): b_i = sum_k ( values_k phi_i(x_k) + gradients_k . grad
 * phi_i(x_k) ) through C^T, no quadrature weight and no h^3; b is OVERWRITTEN (a stream-ordered memset comes before the kernel),
 * every constrained row is exactly 0, points that are not found add nothing, no coefficient and no sigma are applied.  The points
 * of a leaf are summed in a fixed order in FP64; the scatter is an atomic add in the vector's number type, so a row shared by
 * several occupied leaves takes its addends in no fixed order: NOT bit-reproducible across calls (it is where every row has one
 * addend, as on a one-leaf mesh).
 * op is the operator that created the set.  MGAMD_ERR_INVALID, by name ("point_set: ...", "point_evaluate: ...",
 * "point_integrate: ..."): a distributed operator or sharded tables ("not implemented: sharded"); the operator of a local-smoothing
 * level; a null pointer; a vector of the wrong size or number type; neither values nor gradients; b aliasing an input; an output
 * that is u or the other output; a point set used with an operator other than its own. */
/* the number type of the operator's vectors, MGAMD_F64 or MGAMD_F32: what the outputs of a point set must have */
int mgamd_level_op_number_type(const mgamd_level_op *op, int *number_type);
int mgamd_level_op_point_set_create(mgamd_level_op *op, uint64_t n, const double *xyz, mgamd_point_set **out);
int mgamd_point_set_destroy(mgamd_point_set *ps);
int mgamd_point_set_get(const mgamd_point_set *ps, uint64_t *n, uint64_t *n_found, int32_t *cell, double *ref);
int mgamd_point_set_evaluate(mgamd_point_set *ps, mgamd_level_op *op, const mgamd_vec *u, mgamd_vec *values, mgamd_vec *gradients);
int mgamd_point_set_integrate(mgamd_point_set *ps, mgamd_level_op *op, const mgamd_vec *values, const mgamd_vec *gradients, mgamd_vec *b);

/* PreconditionChebyshev (ref:multigrid_throughput.cc:849-852, 867-883): the inverse diagonal is
 * computed internally (DiagonalMatrix preconditioner); eigenvalues are estimated at creation with
 * eig_cg_n_iterations CG steps, max *= 1.2, min = max / smoothing_range. */
int mgamd_cheb_create(mgamd_level_op *op, unsigned degree, double smoothing_range, unsigned eig_cg_n_iterations,
                      mgamd_cheb **out);
int mgamd_cheb_destroy(mgamd_cheb *c);
int mgamd_cheb_vmult(mgamd_cheb *c, mgamd_vec *dst, const mgamd_vec *src); /* zero start: MGSmoother::apply  */
int mgamd_cheb_step(mgamd_cheb *c, mgamd_vec *dst, const mgamd_vec *src);  /* general start: MGSmoother::smooth */
int mgamd_cheb_get_eigen_estimates(const mgamd_cheb *c, double *min_eigenvalue, double *max_eigenvalue);

/* MGTwoLevelTransfer::reinit(dof_fine, dof_coarse, constraint_fine, constraint_coarse)
 * (ref:multigrid_throughput.cc:1600-1604) */
int mgamd_transfer2_create(mgamd_level_op *fine, mgamd_level_op *coarse, mgamd_transfer2 **out);
int mgamd_transfer2_destroy(mgamd_transfer2 *t);
int mgamd_transfer2_prolongate_and_add(mgamd_transfer2 *t, mgamd_vec *dst_fine, const mgamd_vec *src_coarse);
int mgamd_transfer2_restrict_and_add(mgamd_transfer2 *t, mgamd_vec *dst_coarse, const mgamd_vec *src_fine);
/* Inside mgamd_mg_vcycle the part of a transfer that belongs to the fine level's 17-point lattice bricks runs INSIDE the level
 * operator's passes (restriction in the residual pass, prolongation in the first post-smoothing pass: the steps
 * Multigrid::level_v_step runs back to back, ref:multigrid_throughput.cc:1093-1099); *n = number of such bricks (0: none;
 * MGAMD_NO_FUSED_TRANSFER=1 in the environment disables it).  The two entry points above always do the whole transfer. */
int mgamd_transfer2_n_fused_bricks(const mgamd_transfer2 *t, uint64_t *n);

/* Multigrid + PreconditionMG over MGTransferGlobalCoarsening (ref:multigrid_throughput.cc:1093-1133,
 * 1618-1621).  levels[0] is the coarsest; transfers[l] connects levels l-1 and l (transfers[0] unused,
 * may be NULL); smoothers[0] is only used by coarse solver "cg_with_chebyshev".
 * coarse_solver (CoarseGridSolverType, ref:multigrid_throughput.cc:909-1077):
 *   "direct"             dense inverse (coarse levels up to MGAMD_DIRECT_COARSE_MAX_DOFS DoFs)
 *   "cg", "cg_with_chebyshev"   SolverCG to reltol 1e-4, unpreconditioned / with the level-0 Chebyshev smoother (:911-944)
 *   "amg", "cg_with_amg", "amg_petsc"   the reference applies Trilinos ML / BoomerAMG to Operator::get_trilinos_system_matrix
 *                        (:945-1077).  Here: on a coarse level of at most MGAMD_DIRECT_COARSE_MAX_DOFS DoFs (global coarsening ends
 *                        on one cell) an exact solve ("direct"); on a larger one (PMG: the p = 1 space on the finest mesh) the
 *                        library's OWN smoothed-aggregation AMG on the assembled level matrix (mgamd_dofs_matrix; Chebyshev(2)
 *                        smoothing, dense coarsest solve), applied CoarseSolverNCycles times as the coarse solver ("amg") or as the
 *                        preconditioner of the coarse CG ("cg_with_amg").  Same role and inputs as ML, not the same aggregates: its
 *                        iteration counts cannot be parity-checked against ML.
 * mgamd_mg_create_nested additionally takes n_cycles (CoarseSolverNCycles) and, optionally, `coarse_mg`: a geometric multigrid
 * whose finest level IS levels[0]; if given, it takes the AMG's place ("gmg_vcycle": x = V(b), x += V(b - A x) ...).  Whether a
 * caller has to build one, or the global DoFs for mgamd_mg_create_sharded_amg, is mgamd_coarse_plan's decision; "gmg_vcycle"
 * without `coarse_mg` is "direct" on a level of at most MGAMD_DIRECT_COARSE_MAX_DOFS DoFs and MGAMD_ERR_INVALID on a larger one.
 * mgamd_mg_coarse_solver_used returns what runs: "direct" | "cg" | "cg_with_chebyshev" | "amg" | "cg_with_amg" | "gmg_vcycle". */
int mgamd_mg_create(mgamd_ctx *ctx, unsigned n_levels, mgamd_level_op *const *levels, mgamd_transfer2 *const *transfers,
                    mgamd_cheb *const *smoothers, const char *coarse_solver, mgamd_mg **out);
int mgamd_mg_create_nested(mgamd_ctx *ctx, unsigned n_levels, mgamd_level_op *const *levels, mgamd_transfer2 *const *transfers,
                           mgamd_cheb *const *smoothers, const char *coarse_solver, mgamd_mg *coarse_mg, unsigned n_cycles,
                           mgamd_mg **out);
int mgamd_mg_coarse_solver_used(const mgamd_mg *mg, char name[32]);
/* The AMG coarse solvers on a SHARDED level 0 ("replicated setup, sharded cycle"; not the default: without this entry a sharded
 * coarse level keeps the geometric stand-in "gmg_vcycle" or refuses).  `global_coarse_dofs` = mgamd_dofs_create on the mesh and
 * degree of levels[0] with the max_brick a one-rank hierarchy would pass: every rank builds the one-rank smoothed-aggregation
 * hierarchy from it (identical aggregates, P, R A P, lambda_max, coarsest inverse) and keeps its rows of A, P and R.  Level 0: the
 * owner of the DoF in the partition owns the row; an aggregate belongs to the rank that owns most of its members.  Levels of at most
 * `min_sharded_rows` global rows (and always the dense coarsest one) are replicated; MGAMD_AMG_MIN_SHARDED_ROWS_DEFAULT is a guess,
 * the cost of the ghost imports has not been measured on multi-GPU hardware.  coarse_solver: "amg" | "cg_with_amg" | "amg_petsc";
 * mgamd_mg_coarse_solver_used then reports "amg" or "cg_with_amg" (the distributed coarse CG preconditioned by the sharded cycle).
 * MGAMD_ERR_INVALID for local-smoothing levels and for a level 0 held by groups of ranks (mgamd_comm_subset with group > 1). */
#define MGAMD_AMG_MIN_SHARDED_ROWS_DEFAULT 20000u
int mgamd_mg_create_sharded_amg(mgamd_ctx *ctx, unsigned n_levels, mgamd_level_op *const *levels, mgamd_transfer2 *const *transfers,
                                mgamd_cheb *const *smoothers, const char *coarse_solver, const mgamd_dofs *global_coarse_dofs,
                                unsigned n_cycles, uint32_t min_sharded_rows, mgamd_mg **out);
/* read-only: the levels of the algebraic coarse solver that runs (finest first), 5 numbers each: global rows, rows this rank owns,
 * ghost columns it imports, peers it exchanges with, 1 if the level is replicated.  *n_levels = 0: no AMG runs.  `info` may be
 * null; at most max_levels levels are written. */
/* inner CG iterations of the coarse solvers "cg", "cg_with_chebyshev", "cg_with_amg", accumulated since the multigrid was built */
int mgamd_mg_coarse_iterations(const mgamd_mg *mg, uint64_t *n_iterations);
int mgamd_mg_amg_layout(const mgamd_mg *mg, uint32_t *n_levels, uint32_t *info, uint32_t max_levels);
/* Local smoothing (`HMG-local`: solve_with_local_smoothing, ref:multigrid_throughput.cc:1670-1873).  levels[l] = Operator on
 * refinement level l (mgamd_dofs_create_level: edge-constrained level operator, ref:include/operator.h:49-120,152-183),
 * transfers = MGTransferMatrixFree between the refinement levels, Multigrid with the interface (edge) matrices
 * (ref:multigrid_throughput.cc:1081-1130), PreconditionMG::vmult on vectors of the ACTIVE mesh `active_mesh_dofs`
 * (copy_to_mg / copy_from_mg).  Stage 5 of the stage callback / timing is the edge prolongation. */
int mgamd_mg_create_local_smoothing(mgamd_ctx *ctx, unsigned n_levels, mgamd_level_op *const *levels, mgamd_transfer2 *const *transfers,
                                    mgamd_cheb *const *smoothers, const mgamd_dofs *active_mesh_dofs, const char *coarse_solver,
                                    mgamd_mg **out);
/* Operator::vmult_interface_up (ref:include/operator.h:203-226): dst = A with the refinement-edge DoFs unconstrained, applied
 * to src restricted to those DoFs (MatrixFreeOperators::MGInterfaceOperator::Tvmult) */
int mgamd_level_op_vmult_interface_up(mgamd_level_op *op, mgamd_vec *dst, const mgamd_vec *src);
/* Operator::vmult_interface_down (ref:include/operator.h:191-201): the plain cell loop, identity on the constrained (Dirichlet,
 * hanging) rows only; on a local-smoothing level the refinement-edge DoFs take part as ordinary DoFs.  This is what
 * MatrixFreeOperators::MGInterfaceOperator::vmult forwards to, i.e. the matrix of Multigrid's residual step in the reference
 * (ref:multigrid_throughput.cc:857-862).  On a level without refinement edges it equals mgamd_level_op_vmult. */
int mgamd_level_op_vmult_interface_down(mgamd_level_op *op, mgamd_vec *dst, const mgamd_vec *src);
/* Levels up to 2048 DoFs (MGAMD_COLLAPSE_MAX_DOFS) with a direct coarse solver are applied as ONE tabulated dense matrix
 * (the zero-start V-cycle below a level is a linear map of its defect; result-equivalent).  This switches the
 * tabulated path off/on at run time (bench.py reports the cycle time both ways); *collapse_level = the level it replaces
 * (0: none). */
int mgamd_mg_set_collapse(mgamd_mg *mg, int enable, unsigned *collapse_level);
int mgamd_mg_destroy(mgamd_mg *mg);
/* PreconditionMG::vmult: z = V-cycle(r)  (ref:multigrid_throughput.cc:1132-1133) -- the metric's unit of work.
 * z and r are vectors of the finest level's outer number type (double). */
int mgamd_mg_vcycle(mgamd_mg *mg, mgamd_vec *z, const mgamd_vec *r);
/* Multigrid::connect_{pre_smoother_step,residual_step,restriction,coarse_solve,prolongation,
 * edge_prolongation,post_smoother_step} + PreconditionMG::connect_transfer_to_{mg,global}
 * (ref:multigrid_throughput.cc:1183-1192, 1233-1234).  stage 0..6 as in the reference's timer index,
 * 7 = transfer_to_mg, 8 = transfer_to_global.  With a callback installed the V-cycle runs eagerly
 * and synchronises the stream around every stage so host clocks are meaningful. */
typedef void (*mgamd_stage_callback)(int stage, int start, unsigned level, void *user);
int mgamd_mg_set_stage_callback(mgamd_mg *mg, mgamd_stage_callback cb, void *user);
/* Stage times WITHOUT host synchronisation: while enabled, a HIP event pair is recorded on the stream around every stage
 * of the unchanged cycle (collapsed coarse levels included: they appear as the coarse solve, stage 3, of the collapse
 * level).  mgamd_mg_stage_times synchronises once, ADDS the elapsed milliseconds of all stages recorded since the last
 * read to ms[stage * n_levels + level] (9 x n_levels entries) and returns the number of stage records consumed.  This is
 * how the harness fills the reference's time_pre ... time_to_global columns (ref:multigrid_throughput.cc:1381-1401). */
int mgamd_mg_stage_timing(mgamd_mg *mg, int enable);
int mgamd_mg_stage_times(mgamd_mg *mg, double *ms, unsigned n_levels, uint64_t *n_records);
/* run `n` V-cycles back to back and return the average time per cycle in milliseconds, measured
 * with HIP events on the context's stream (bench.py / harness). use_graph != 0 replays a captured
 * hipGraph of one cycle. */
int mgamd_mg_time_vcycles(mgamd_mg *mg, mgamd_vec *z, const mgamd_vec *r, unsigned n, int use_graph, double *ms_per_cycle);

/* SolverCG + ReductionControl with PreconditionMG (ref:multigrid_throughput.cc:1140-1147, 1238-1254,
 * 1625-1635): solves A x = b from x = 0; returns last_step() and the final residual norm. */
int mgamd_solve_cg(mgamd_level_op *A, mgamd_mg *preconditioner, mgamd_vec *x, const mgamd_vec *b, double reltol, double abstol,
                   unsigned maxiter, unsigned *n_iterations, double *residual_norm);

/* -------------------------------------------------------------------------------------------
 * theta-scheme for the heat equation  M u' + K u = M f  (homogeneous Dirichlet data, f a vector of nodal values) with constant
 * step dt on the operator A = K + sigma M, sigma = 1 / (theta dt), and its multigrid; 0 < theta <= 1 (1: implicit Euler, 0.5:
 * Crank-Nicolson).  The caller sets sigma on every level (mgamd_dofs_set_mass_coefficient) before building operators and
 * multigrid.  One step solves for the increment delta = u_new - u:
 *     w = theta f_new + (1 - theta) f_old + sigma u;   r = M w - A u, zero on constrained rows;   A delta = r / theta;   u += delta
 * with mgamd_solve_cg's CG from delta = 0, so u is the initial guess and reltol acts on the residual of the INCREMENT.
 * The stepper owns its work vectors (allocated at creation, none per step); all work is enqueued on the context's stream and the
 * host read-backs are those of the CG.  Constrained entries of u are never read and are 0 on return: a vector that
 * mgamd_level_op_distribute filled for output may be passed back in.  One rank or sharded (A and the multigrid distributed alike).
 * MGAMD_ERR_INVALID, with the values in mgamd_last_error(): theta outside (0, 1], dt <= 0, NaN or infinity;
 * |sigma theta dt - 1| > 1e-12 for A's mass coefficient sigma; an operator that is not MGAMD_F64 (the outer solve is FP64 as in
 * mgamd_solve_cg; the levels of the multigrid may be FP32); a local-smoothing level operator; in a step: vectors of the wrong size
 * or number type, exactly one of f_old / f_new.  A refused step changes neither u nor the time.
 * The operator and the multigrid must outlive the stepper.  Changing dt or theta: new sigma, new operators, multigrid and stepper.
 * ------------------------------------------------------------------------------------------- */
typedef struct mgamd_time_stepper mgamd_time_stepper;
int mgamd_time_stepper_create(mgamd_level_op *A, mgamd_mg *preconditioner, double theta, double dt, mgamd_time_stepper **out);
/* one step in place; f_old / f_new: nodal source values at t and t + dt, both NULL for f = 0; n_iterations, residual_norm: of the
 * CG for the increment (may be NULL) */
int mgamd_time_stepper_step(mgamd_time_stepper *ts, mgamd_vec *u, const mgamd_vec *f_old, const mgamd_vec *f_new, double reltol,
                            double abstol, unsigned maxiter, unsigned *n_iterations, double *residual_norm);
/* The same step with non-zero, time-dependent Dirichlet data and a boundary load.  g_old / g_new: Dirichlet values at t and t + dt
 * (vectors of n_dofs values, only the entries at Dirichlet DoFs are read), both NULL for homogeneous data; load: a boundary load
 * l = theta l_new + (1 - theta) l_old (mgamd_level_op_rhs_boundary_flux: a flux, beta u_ext), may be NULL.  On the free rows
 *     A delta = (M w + l - A u - K_ID g_old) / theta - A_ID (g_new - g_old);   u += delta
 * (two launches of the lifting kernel of mgamd_level_op_rhs_dirichlet: stiffness only for g_old, K + sigma M for the increment).
 * Constrained entries of u are still never read and are 0 on return: for output run mgamd_level_op_distribute_values(u, g_new).
 * The mass product ignores the values of f on Dirichlet DoFs, so a source that is non-zero on a Dirichlet face loses M_ID f_D.
 * With g_old, g_new and load all NULL this is mgamd_time_stepper_step, launch for launch.  MGAMD_ERR_INVALID in addition: exactly
 * one of g_old / g_new; a convective face that shares an edge with a Dirichlet face (mgamd_dofs_rhs_dirichlet). */
int mgamd_time_stepper_step_data(mgamd_time_stepper *ts, mgamd_vec *u, const mgamd_vec *f_old, const mgamd_vec *f_new,
                                 const mgamd_vec *g_old, const mgamd_vec *g_new, const mgamd_vec *load, double reltol, double abstol,
                                 unsigned maxiter, unsigned *n_iterations, double *residual_norm);
/* the time reached (n_steps dt, starting at 0) and the number of steps taken; either may be NULL */
int  mgamd_time_stepper_time(const mgamd_time_stepper *ts, double *t, uint64_t *n_steps);
void mgamd_time_stepper_destroy(mgamd_time_stepper *ts);

/* ---------------------------------------------------------------------------------------------
 * Type "AMG" / "AMGPETSc": CG on the assembled system matrix with an AMG preconditioner built on it (solve_with_amg,
 * ref:multigrid_throughput.cc:1877-1966, called at :2337-2338) -- the baseline the reference measures its matrix-free multigrid
 * against.  FP64 only (the reference runs this path in double whatever MGNumberType says), one rank.  Every entry below returns
 * MGAMD_ERR_INVALID, with the reason in mgamd_last_error(), for a distributed level (mgamd_dofs_create_local), a local-smoothing
 * level (mgamd_dofs_create_level) and MGAMD_F32 vectors.
 * ------------------------------------------------------------------------------------------- */
/* Operator::get_trilinos_system_matrix() (ref:include/operator.h:244-287): the matrix of mgamd_dofs_matrix, assembled on the host
 * and held on the device as CSR.  The host setup bounds the usable size (32-bit row pointers: < 2^32 entries). */
int mgamd_matrix_create(mgamd_ctx *ctx, const mgamd_dofs *dofs, mgamd_matrix **out);
int mgamd_matrix_destroy(mgamd_matrix *A);
/* rows, stored entries and the lanes per row of its products (64: one wavefront per row, the long rows of degree >= 2; 4-32: the
 * coarse solver's kernel).  Any pointer may be NULL. */
int mgamd_matrix_info(const mgamd_matrix *A, uint64_t *n_rows, uint64_t *nnz, int *lanes);
/* SparseMatrix::vmult as SolverCG calls it (ref:multigrid_throughput.cc:1913-1914): dst = A src, dst != src */
int mgamd_matrix_vmult(mgamd_matrix *A, mgamd_vec *dst, const mgamd_vec *src);
/* TrilinosWrappers::PreconditionAMG::initialize(matrix, AdditionalData()) (ref:multigrid_throughput.cc:1907-1909; defaults: 1 cycle,
 * aggregation threshold 1e-4, 2 smoother sweeps): the library's own smoothed-aggregation AMG (see mgamd_mg_create) on A, n_cycles
 * cycles per application (>= 1).  Level 0 works on A's device arrays: the matrix is on the device once; P keeps it alive. */
int mgamd_amg_create(mgamd_matrix *A, unsigned n_cycles, mgamd_amg **out);
int mgamd_amg_destroy(mgamd_amg *P);
/* PreconditionAMG::vmult: z = n_cycles V-cycles applied to r, z != r */
int mgamd_amg_vmult(mgamd_amg *P, mgamd_vec *z, const mgamd_vec *r);
/* rows of every AMG level, finest first (`rows` may be NULL; at most max_levels entries are written) */
int mgamd_amg_layout(const mgamd_amg *P, uint32_t *n_levels, uint32_t *rows, uint32_t max_levels);
/* SolverCG<VectorType>(ReductionControl).solve(op.get_trilinos_system_matrix(), dst, src, preconditioner)
 * (ref:multigrid_throughput.cc:1911-1915) from x = 0; preconditioner NULL: PreconditionIdentity.  A p and p . A p come from one pass
 * over the matrix. */
int mgamd_solve_cg_matrix(mgamd_matrix *A, mgamd_amg *preconditioner, mgamd_vec *x, const mgamd_vec *b, double reltol, double abstol,
                          unsigned maxiter, unsigned *n_iterations, double *residual_norm);

#ifdef __cplusplus
}
#endif
#endif /* MGAMD_H */
