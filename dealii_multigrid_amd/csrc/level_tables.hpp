// Host-side level description: what deal.II's DoFHandler + AffineConstraints + MatrixFree::reinit
// produce for one multigrid level in the reference (ref:include/operator.h:24-47,
// ref:multigrid_throughput.cc:1578-1595), re-designed for a GPU with 160 KB of LDS per CU.
//
// Data layout:
//  * The leaves are grouped into SLOTS: a slot is either a BRICK = complete uniform subtree of
//    B^3 equal-size cells without hanging nodes (B a power of two, node lattice N = p*B+1 <= 17 per
//    direction), or a single cell (B = 1, may carry hanging faces/edges).
//  * DoFs are numbered  [ I | T | D | H ]:
//      I  slot-interior DoFs (strictly inside a slot's node lattice; touched by that slot only),
//         contiguous per slot in lattice-lexicographic order  -> implicit, coalesced addressing
//      T  'tail': unconstrained DoFs on slot shells (shared between slots), in first-touch order
//      D  Dirichlet DoFs: those on a Dirichlet face of the mesh (Tria::dirichlet_faces; the default, every face, is the reference's
//         boundary id 0 = whole boundary, ref:multigrid_throughput.cc:1585-1591).  DoFs on natural faces only are T (or H)
//      H  hanging-node DoFs (own DoFs of fine faces/edges next to a coarser cell); like deal.II
//         they are part of the vector (n_dofs parity) but only ever see the identity row
//         (ref:include/operator.h:170-172).
//  * A cell with hanging faces/edges gathers, like deal.II's matrix-free hanging-node path, the
//    DoFs of the *parent* face/edge in the same local slot and then interpolates in-cell with
//    the 1D matrices FE1D::I[c]; its configuration is Tria::masks.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "fe1d.hpp"
#include "octree.hpp"

#include <map>

namespace mgamd
{
  // sharded runs: who else references a DoF on an inter-rank interface (see partition.hpp)
  struct SharedInfo
  {
    uint64_t others  = 0; // other ranks referencing the DoF
    uint64_t regular = 0; // ranks (including this one) referencing it as a node of one of their own cells
  };
  // the owner is the lowest rank among the regular referencers: it is guaranteed to have a transfer patch for the DoF
  inline int
  shared_owner(const SharedInfo &si)
  {
    return __builtin_ctzll(si.regular);
  }
} // namespace mgamd

namespace mgamd
{
  constexpr uint32_t INVALID_DOF = 0xFFFFFFFFu;

  // max_brick = -1 ("auto"): levels below this many DoFs are latency-bound (a few microseconds per kernel whatever it
  // does).  If such a level needs more than one slot group, it uses single-cell slots only: one lattice launch per
  // operator application instead of one per brick size.  Measured on MI355X: -8 % V-cycle time for the octant at p=1
  // (17 M DoFs) and p=4 (17.5 M DoFs); uniform meshes (one brick group per level anyway) keep their bricks.
  constexpr size_t SMALL_LEVEL_DOFS = 500000;
  inline bool
  is_small_level(size_t n_cells, int p)
  {
    return n_cells * (size_t)(p * p * p) < SMALL_LEVEL_DOFS;
  }

  inline int
  max_brick_for_degree(int p)
  {
    int B = 1;
    while (2 * B * p + 1 <= 17)
      B *= 2;
    return B;
  }

  // position of lattice node (x,y,z) in the shell enumeration.  The shell is listed FACE BY FACE -- z=0, z=N-1,
  // then y=0, y=N-1 (without the z-face rows), then x=0, x=N-1 (without the y- and z-face rows) -- each face as a
  // contiguous 2D block in (outer, inner) lexicographic order.  Tail DoFs are numbered in first-touch order of
  // this enumeration, so a face shared by two bricks is ONE contiguous run of the tail segment for both of
  // them: shell gathers and shell atomics of a wave hit consecutive addresses (measured: 2.7x over-fetch with
  // the plain lattice-order enumeration).
  inline int
  shell_slot_of(int N, int x, int y, int z)
  {
    const int M = N - 2;
    if (z == 0)
      return y * N + x;
    if (z == N - 1)
      return N * N + y * N + x;
    int s = 2 * N * N;
    if (y == 0)
      return s + (z - 1) * N + x;
    s += M * N;
    if (y == N - 1)
      return s + (z - 1) * N + x;
    s += M * N;
    if (x == 0)
      return s + (z - 1) * M + (y - 1);
    s += M * M;
    return s + (z - 1) * M + (y - 1);
  }

  struct SlotGroup
  {
    int                   B = 1, N = 2, n_interior = 0, n_shell = 8;
    std::vector<uint32_t> interior_base; // per slot: global index of its first interior DoF
    std::vector<uint32_t> shell_idx;     // per slot x n_shell: global DoF or INVALID_DOF (Dirichlet)
    std::vector<uint16_t> mask;          // per slot: constraint configuration (0 for bricks)
    std::vector<uint32_t> fmask;         // bricks (B >= 2), per slot: hanging faces/edges of the whole brick (family_* helpers), 0 = none
    std::vector<double>   h;             // per slot: cell edge length
    std::vector<double>   a;             // per slot: diffusion coefficient, the one value all its cells carry (1 if the mesh has none)
    std::vector<uint32_t> first_cell;    // per slot: index of its first cell in Tria::cells
    std::vector<uint16_t> shell_pos;     // n_shell: lattice index (z*N+y)*N+x of each shell entry
    // sharded levels: the first n_halo_slots slots of the group touch DoFs shared with other ranks; the halo exchange of an
    // operator application only needs them, so the others run underneath it (runtime.hip, apply_P)
    uint32_t n_halo_slots = 0;
    // p = 1, B > 2: the constrained bricks form a group of their own (their kernel carries the embedding passes; the
    // unconstrained bricks keep the lean kernel).  Families (B = 2) share the group of the 2^3 bricks.
    bool constrained_group = false;
    size_t
    n_slots() const
    {
      return interior_base.size();
    }
  };

  struct DofKey
  {
    int32_t px, py, pz, dirmask, level;
  };

  inline uint64_t
  pack_key(uint32_t px, uint32_t py, uint32_t pz, int dm, int level)
  {
    return ((uint64_t)px << 43) | ((uint64_t)py << 25) | ((uint64_t)pz << 7) | ((uint64_t)dm << 4) | (uint64_t)(dm ? level : 0);
  }
  inline DofKey
  unpack_key(uint64_t k)
  {
    return DofKey{(int32_t)(k >> 43), (int32_t)((k >> 25) & 0x3ffff), (int32_t)((k >> 7) & 0x3ffff), (int32_t)((k >> 4) & 7),
                  (int32_t)(k & 15)};
  }

  // in-cell hanging-node interpolation (and its transpose) on (p+1)^3 gathered values
  inline void
  interpolate_hanging(const FE1D &fe, uint16_t mask, double *v, bool transpose)
  {
    if (!(mask >> MASK_FACE_SHIFT))
      return;
    const int p = fe.p, n = p + 1;
    const int cp[3]     = {mask & 1, (mask >> 1) & 1, (mask >> 2) & 1};
    const int stride[3] = {1, n, n * n};
    double    tmp[MAX_DEGREE + 1];
    for (int dd = 0; dd < 3; ++dd)
      {
        const int     d = transpose ? 2 - dd : dd;
        const int     e = (d + 1) % 3, f = (d + 2) % 3;
        const bool    fe_c = (mask >> (MASK_FACE_SHIFT + e)) & 1, ff_c = (mask >> (MASK_FACE_SHIFT + f)) & 1,
                   ed_c    = (mask >> (MASK_EDGE_SHIFT + d)) & 1;
        const double *Ic   = fe.I[cp[d]].data();
        for (int ae = 0; ae < n; ++ae)
          for (int af = 0; af < n; ++af)
            {
              const bool on_e = ae == cp[e] * p, on_f = af == cp[f] * p;
              if (!((fe_c && on_e) || (ff_c && on_f) || (ed_c && on_e && on_f)))
                continue;
              double *line = v + ae * stride[e] + af * stride[f];
              for (int a = 0; a < n; ++a)
                {
                  double s = 0;
                  for (int b = 0; b < n; ++b)
                    s += (transpose ? Ic[b * n + a] : Ic[a * n + b]) * line[b * stride[d]];
                  tmp[a] = s;
                }
              for (int a = 0; a < n; ++a)
                line[a * stride[d]] = tmp[a];
            }
      }
  }

  // ---- families with hanging nodes as constrained 2^3 bricks -------------------------------------------------
  // The 8 children of one parent next to a coarser neighbour: the neighbour has the parent's size, so a hanging face of
  // the family IS one face of the parent cell and its (2p+1)^2 lattice nodes are E (x) E times the parent face's
  // (p+1)^2 DoFs, E = [I0; I1] the 1D two-cell embedding; a hanging edge likewise with one E.  The brick lattice stores
  // the parent DoFs ON the entity: parent coordinate c < p along a free direction at lattice coordinate c, c = p at the
  // far end 2p (so vertices and the nodes of edges shared by two hanging faces have ONE position, their own); the other
  // positions of the entity carry no DoF.  The embedding runs in place, direction by direction, before the sweeps and
  // its transpose after them.
  // Family mask: bit 2*d + side = face with normal d hangs; bit 6 + 4*d + s1 + 2*s2 = edge along d hangs, s1/s2 the
  // sides in directions (d+1)%3, (d+2)%3.
  inline bool
  family_face(uint32_t fm, int d, int side)
  {
    return (fm >> (2 * d + side)) & 1;
  }
  inline bool
  family_edge(uint32_t fm, int d, int s1, int s2)
  {
    return (fm >> (6 + 4 * d + s1 + 2 * s2)) & 1;
  }
  // lattice node n (coordinates 0..B p) of a constrained brick: does it lie on a hanging face/edge?  pinned[d]: the
  // coordinate is fixed by the hanging entity (its parent coordinate is 0 or p of the outermost parent cell), otherwise it
  // runs along the entity
  inline bool
  family_node_constrained(uint32_t fm, int p, int B, const int n[3], bool pinned[3])
  {
    const int N1 = B * p;
    bool      any = false;
    for (int d = 0; d < 3; ++d)
      {
        pinned[d] = (n[d] == 0 && family_face(fm, d, 0)) || (n[d] == N1 && family_face(fm, d, 1));
        any |= pinned[d];
      }
    if (any)
      return true;
    for (int d = 0; d < 3; ++d)
      {
        const int e = (d + 1) % 3, f = (d + 2) % 3;
        if ((n[e] == 0 || n[e] == N1) && (n[f] == 0 || n[f] == N1) && family_edge(fm, d, n[e] == N1, n[f] == N1))
          {
            pinned[e] = pinned[f] = true;
            return true;
          }
      }
    return false;
  }
  // Constrained BRICKS of any size (B = 2: a family).  A brick of B^3 equal cells next to coarser cells qualifies if the
  // hanging entities are WHOLE faces / WHOLE edges of the brick: a hanging brick face then is (B/2)^2 faces of parent-size
  // cells and carries the parents' (p B/2 + 1)^2 DoFs.  Along a lattice line the parent DoF k p + c (parent cell k, local
  // coordinate c) is stored at lattice coordinate 2 k p + c for c < p (c = p: the next parent cell's c = 0, or B p at the end);
  // the other positions of the entity carry no DoF and are filled by the in-place embedding E = [I0; I1] per parent cell.
  // mask of the brick from its cells: bpos[c] = position of cell c inside the brick, cm[c] = its cell mask; false if the
  // cells do not describe whole-face / whole-edge constraints
  inline bool
  brick_mask_from_cells(int B, int p, const std::vector<std::array<int, 3>> &bpos, const std::vector<uint16_t> &cm, uint32_t &fm)
  {
    fm = 0;
    const size_t nc = bpos.size();
    for (size_t c = 0; c < nc; ++c)
      {
        const int cp[3] = {bpos[c][0] & 1, bpos[c][1] & 1, bpos[c][2] & 1};
        if ((cm[c] & 7) != (cp[0] | (cp[1] << 1) | (cp[2] << 2)))
          return false;
        bool out[3]; // is the parent-side face of this cell in direction d on the brick boundary?
        for (int d = 0; d < 3; ++d)
          out[d] = bpos[c][d] == (cp[d] ? B - 1 : 0);
        for (int d = 0; d < 3; ++d)
          {
            if ((cm[c] >> (MASK_FACE_SHIFT + d)) & 1)
              {
                if (!out[d])
                  return false;
                fm |= 1u << (2 * d + cp[d]);
              }
            if ((cm[c] >> (MASK_EDGE_SHIFT + d)) & 1)
              {
                const int e = (d + 1) % 3, f = (d + 2) % 3;
                // an edge bit that only mirrors a hanging face of this cell needs no edge of its own
                const bool fe = (cm[c] >> (MASK_FACE_SHIFT + e)) & 1, ff = (cm[c] >> (MASK_FACE_SHIFT + f)) & 1;
                if (fe || ff)
                  continue;
                if (!out[e] || !out[f])
                  return false;
                fm |= 1u << (6 + 4 * d + cp[e] + 2 * cp[f]);
              }
          }
      }
    // every cell must see exactly the constraints the brick mask implies
    for (size_t c = 0; c < nc; ++c)
      {
        const int cp[3] = {bpos[c][0] & 1, bpos[c][1] & 1, bpos[c][2] & 1};
        for (int z = 0; z <= p; ++z)
          for (int y = 0; y <= p; ++y)
            for (int x = 0; x <= p; ++x)
              {
                const int  a[3] = {x, y, z};
                const int  n[3] = {bpos[c][0] * p + x, bpos[c][1] * p + y, bpos[c][2] * p + z};
                bool       pinned[3];
                const bool fam  = family_node_constrained(fm, p, B, n, pinned);
                bool       cell = false;
                if (cm[c] >> MASK_FACE_SHIFT)
                  {
                    bool on[3];
                    for (int d = 0; d < 3; ++d)
                      on[d] = a[d] == cp[d] * p;
                    for (int d = 0; d < 3; ++d)
                      cell |= (((cm[c] >> (MASK_FACE_SHIFT + d)) & 1) && on[d]) ||
                              (((cm[c] >> (MASK_EDGE_SHIFT + d)) & 1) && on[(d + 1) % 3] && on[(d + 2) % 3]);
                  }
                if (fam != cell)
                  return false;
              }
      }
    return true;
  }
  // lattice coordinate -> does a parent DoF live there along a free direction, and which (parent cell k, local c)?
  inline bool
  family_parent_position(int p, int B, int n, int &k, int &c)
  {
    if (n == B * p)
      {
        k = B / 2 - 1;
        c = p;
        return true;
      }
    k = n / (2 * p);
    c = n % (2 * p);
    return c < p;
  }
  // the embedding (transpose = false) or its transpose on the (B p + 1)^3 lattice of a constrained brick, host version
  inline void
  interpolate_family(const FE1D &fe, int B, uint32_t fm, double *v, bool transpose)
  {
    if (!fm)
      return;
    const int p = fe.p, n = p + 1, N = B * p + 1, BC = B / 2;
    const int stride[3] = {1, N, N * N};
    std::vector<double> in(N), out(N);
    auto      E = [&](int a, int b) { return a <= p ? fe.I[0][a * n + b] : fe.I[1][(a - p) * n + b]; };
    for (int dd = 0; dd < 3; ++dd)
      {
        const int d = transpose ? 2 - dd : dd, e = (d + 1) % 3, f = (d + 2) % 3;
        for (int ae = 0; ae < N; ++ae)
          for (int af = 0; af < N; ++af)
            {
              const bool xe = ae == 0 || ae == N - 1, xf = af == 0 || af == N - 1;
              const bool on = (ae == 0 && family_face(fm, e, 0)) || (ae == N - 1 && family_face(fm, e, 1)) ||
                              (af == 0 && family_face(fm, f, 0)) || (af == N - 1 && family_face(fm, f, 1)) ||
                              (xe && xf && family_edge(fm, d, ae == N - 1, af == N - 1));
              if (!on)
                continue;
              double *line = v + ae * stride[e] + af * stride[f];
              for (int i = 0; i < N; ++i)
                in[i] = line[i * stride[d]];
              for (int i = 0; i < N; ++i)
                out[i] = 0;
              for (int k = 0; k < BC; ++k)
                {
                  auto pos = [&](int b) { return 2 * k * p + (b < p ? b : 2 * p); }; // parent DoF b of parent cell k
                  if (!transpose)
                    for (int a = 0; a <= 2 * p; ++a)
                      {
                        double s = 0;
                        for (int b = 0; b < n; ++b)
                          s += E(a, b) * in[pos(b)];
                        out[2 * k * p + a] = s; // the node shared with the next parent cell gets the same value twice
                      }
                  else
                    for (int a = (k == 0 ? 0 : 1); a <= 2 * p; ++a) // a fine node shared by two parent cells counts once
                      for (int b = 0; b < n; ++b)
                        out[pos(b)] += E(a, b) * in[2 * k * p + a];
                }
              for (int i = 0; i < N; ++i)
                line[i * stride[d]] = out[i];
            }
      }
  }

  class LevelTables
  {
  public:
    int                    p = 1;
    const Tria            *tria = nullptr;
    FE1D                   fe;
    std::vector<SlotGroup> groups; // one per brick size, largest first; last = single cells
    uint32_t               n_dofs = 0, n_interior = 0, n_tail = 0, n_dirichlet = 0, n_hanging = 0;
    // Local smoothing (`HMG-local`): a LEVEL of the refinement hierarchy = all cells of one refinement level, which cover
    // only part of the domain.  The DoFs on the boundary of that region which are not on the domain boundary are the
    // REFINEMENT-EDGE DoFs (MGTools::extract_inner_interface_dofs, ref:include/operator.h:49-70,539-556): numbered
    // [ I | T | E | D | H ].  The level operator treats E like D (zero input, identity row); the edge matrices treat them
    // like T.  Their shell entries keep the real index: the kernels compare it with a gather / scatter LIMIT (D entries
    // are INVALID = 0xFFFFFFFF, above every limit).
    bool     ls_level = false;
    uint32_t n_edge   = 0;
    // Mass coefficient sigma >= 0 of the shifted operator  K + sigma M  (weak form of -Laplace u + sigma u; DESIGN.md "Mass
    // term").  Everything built FROM the tables (level operators, assembled matrices, the Gaussian right-hand side) reads it at
    // its construction and keeps its own copy; 0 = the Laplace operator.  Local-smoothing levels refuse a non-zero value (their
    // refinement-edge matrices carry no mass term).
    double sigma = 0.0;
    // Diffusion coefficient a of  -div(a grad u) + sigma u,  one value per cell: the triangulation's at the time these tables
    // were built (a later Tria::set_coefficient does not reach them); empty: a = 1.  The slots carry it too (SlotGroup::a): a
    // brick is only formed of cells with the bit-identical value (DESIGN.md "Diffusion coefficient").
    std::vector<double> coefficient;
    // Which faces of the cube are Dirichlet (bit f = 2 axis + side; Tria::dirichlet_faces at the time these tables were built).  A
    // DoF on natural faces only is an ordinary unknown: tail class, or hanging if it hangs (DESIGN.md "Boundary conditions").
    unsigned dirichlet_faces = Tria::ALL_DIRICHLET;
    // Robin coefficient beta_f >= 0 per face of the cube (Tria::robin at the time these tables were built): the operator is
    // K_a + sigma M + sum_f beta_f B_f, B_f the surface mass matrix of face f (DESIGN.md "Convective faces").  All 0: no face term.
    double robin[6] = {0, 0, 0, 0, 0, 0};
    bool
    has_robin() const
    {
      for (int f = 0; f < 6; ++f)
        if (robin[f] > 0.0)
          return true;
      return false;
    }
    // The boundary cell faces of this rank's cells that lie on a face with beta_f > 0, in the order of the cells (Morton) and of the
    // faces within a cell.  A face has n2 = (p+1)^2 nodes, the lower of its two in-face axes (u < v) fastest.
    //   idx    [n][n2]  the DoF the cell gathers at the face node (cell_node_index: hanging entities resolved to the parent's DoFs,
    //                   INVALID_DOF on Dirichlet DoFs)
    //   flags  [n]      the restriction of the cell's constraint mask to the face: bit 0 the line along u at v = cv p hangs, bit 1
    //                   the line along v at u = cu p hangs; bits 2 and 3 are cu and cv, the cell's child position along u and v
    //                   (which half I_0 / I_1 of the parent's line it sees).  The two other in-face edges never hang: they lie
    //                   inside the parent.  The boundary face itself never hangs, and along its normal the interpolation is the
    //                   identity on face nodes (the cell's child position there is the boundary side).
    //   scale  [n]      beta_f h^2
    // The face term of one entry is  scale C2^T (M (x) M) C2  on idx, C2 the interpolation along u, then along v, on the flagged lines.
    struct RobinFaces
    {
      std::vector<uint32_t> idx;
      std::vector<uint8_t>  flags;
      std::vector<double>   scale;
      size_t
      size() const
      {
        return scale.size();
      }
    } robin_faces;
    // the face-local interpolation C2 (or its transpose) of one entry of robin_faces on n2 values
    void
    robin_face_interpolate(uint8_t flags, double *v, bool transpose) const
    {
      const int n = p + 1, cu = (flags >> 2) & 1, cv = (flags >> 3) & 1;
      double    tmp[MAX_DEGREE + 1];
      for (int pass = 0; pass < 2; ++pass)
        {
          const bool along_u = (pass == 0) != transpose;
          if (!((flags >> (along_u ? 0 : 1)) & 1))
            continue;
          const double *Ic     = fe.I[along_u ? cu : cv].data();
          double       *line   = along_u ? v + cv * p * n : v + cu * p;
          const int     stride = along_u ? 1 : n;
          for (int a = 0; a < n; ++a)
            {
              double s = 0;
              for (int b = 0; b < n; ++b)
                s += (transpose ? Ic[b * n + a] : Ic[a * n + b]) * line[b * stride];
              tmp[a] = s;
            }
          for (int a = 0; a < n; ++a)
            line[a * stride] = tmp[a];
        }
    }
    // the n2 x n2 matrix  scale C2^T (M (x) M) C2  of entry e (row-major), for the assembled matrix
    void
    robin_face_matrix(size_t e, std::vector<double> &B) const
    {
      const int           n = p + 1, n2 = n * n;
      std::vector<double> v(n2), w(n2);
      B.assign((size_t)n2 * n2, 0.0);
      for (int j = 0; j < n2; ++j)
        {
          std::fill(v.begin(), v.end(), 0.0);
          v[j] = 1.0;
          robin_face_interpolate(robin_faces.flags[e], v.data(), false);
          for (int bv = 0; bv < n; ++bv)
            for (int bu = 0; bu < n; ++bu)
              {
                double s = 0;
                for (int av = 0; av < n; ++av)
                  for (int au = 0; au < n; ++au)
                    s += fe.M[bu * n + au] * fe.M[bv * n + av] * v[av * n + au];
                w[bv * n + bu] = robin_faces.scale[e] * s;
              }
          robin_face_interpolate(robin_faces.flags[e], w.data(), true);
          for (int i = 0; i < n2; ++i)
            B[(size_t)i * n2 + j] = w[i];
        }
    }
    // Non-zero Dirichlet data (DESIGN.md "Dirichlet data"): this rank's cells, in Morton order, that gather at least one Dirichlet
    // DoF.  The lifting  b_I -= A_ID g  only runs over them.  Built where the tables have a Dirichlet face; on the levels of local
    // smoothing too, for the Gaussian right-hand side (their refinement-edge DoFs keep their index, as in cell_node_index, and
    // their rows are constrained), though the entry points for caller data refuse those levels.
    //   idx    [n][n3]  the DoF the cell gathers at node (x fastest), hanging entities resolved to the parent's DoFs as in
    //                   cell_node_index, but a Dirichlet DoF keeps its real index (in [first_dirichlet(), + n_dirichlet))
    //   mask   [n]      the cell's constraint mask (Tria::masks)
    //   scale  [n][2]   a h and h
    struct DirichletCells
    {
      std::vector<uint32_t> idx;
      std::vector<uint16_t> mask;
      std::vector<double>   scale;
      size_t
      size() const
      {
        return mask.size();
      }
    } dirichlet_cells;
    // Error indicator (DESIGN.md "Error indicator and refinement"): the tables of the two jump kernels, over ALL leaves in Morton
    // order.  Not a member: the first estimate of an operator builds them (LevelOperator), nothing else pays for them.  The gather
    // part (idx, mask, scale) is also the table of the error norms (DESIGN.md "Error norms"), which leave code and nbr empty.
    //   idx    [n][n3]    as DirichletCells::idx: hanging entities resolved to the parent's DoFs, Dirichlet DoFs with their real
    //                     index, so that only free and Dirichlet entries of the vector are read
    //   mask   [n]        the cell's constraint mask
    //   scale  [n][2]     a / h (the factor of the nodal normal flux) and h
    //   code   [n][6], nbr [n][6][4]   Tria::face_neighbours
    struct EstimatorCells
    {
      std::vector<uint32_t> idx, nbr;
      std::vector<uint16_t> mask;
      std::vector<double>   scale;
      std::vector<uint8_t>  code;
      size_t
      size() const
      {
        return mask.size();
      }
      size_t
      bytes() const
      {
        return idx.size() * 4 + nbr.size() * 4 + mask.size() * 2 + scale.size() * 8 + code.size();
      }
    };
    bool
    is_sharded() const
    {
      return owned != nullptr;
    }
    void
    refuse_estimate(const char *who = "estimate_error") const
    {
      if (is_sharded())
        throw std::invalid_argument(std::string(who) + ": not implemented: sharded (the tables hold one rank's cells of a distributed level" +
                                    (std::strcmp(who, "estimate_error") == 0 ? "; the jumps across the cut need the neighbour rank's fluxes)" :
                                                                               "; the per-leaf order is that of one rank's whole mesh)"));
      if (ls_level)
        throw std::invalid_argument(std::string(who) + ": refused on the level of a local-smoothing hierarchy (its cells cover part of the domain "
                                                       "and its refinement-edge DoFs are constrained); use the active-mesh operator");
    }
    // the gather part (idx, mask, scale) is what the error norms need too (kernels_error_norm.hpp); the neighbour part (code, nbr)
    // is the indicator's alone and is added by whichever estimate comes first (LevelOperator keeps ONE idx for both)
    void
    build_estimator_cells(EstimatorCells &ec, bool with_neighbours = true, const char *who = "estimate_error") const
    {
      refuse_estimate(who);
      const int    n = p + 1, n3 = n * n * n;
      const size_t nc = tria->cells.size();
      ec.idx.resize(nc * n3);
      ec.mask.assign(tria->masks.begin(), tria->masks.end());
      ec.scale.resize(nc * 2);
      for (size_t ci = 0; ci < nc; ++ci)
        {
          gather_cell(ci, &ec.idx[ci * n3], true);
          const double h       = 2.0 / (double)(1u << tria->cells[ci].level);
          ec.scale[2 * ci]     = coefficient_of(ci) / h;
          ec.scale[2 * ci + 1] = h;
        }
      if (with_neighbours)
        tria->face_neighbours(ec.code, ec.nbr);
    }
    // Error norms (DESIGN.md "Error norms"): n_q of integrate_difference, 0 standing for p + 2; refused outside p + 1 ... p + 3
    int
    resolve_n_q(int n_q, const char *who) const
    {
      if (n_q == 0)
        return p + 2;
      if (n_q < p + 1 || n_q > p + 3)
        throw std::invalid_argument(std::string(who) + ": n_q = " + std::to_string(n_q) + " refused: 0 (for p + 2) or one of p + 1, p + 2, p + 3 = " +
                                    std::to_string(p + 1) + ", " + std::to_string(p + 2) + ", " + std::to_string(p + 3));
      return n_q;
    }
    // the lower corner of every leaf, [n_cells][3]
    void
    cell_origins(std::vector<double> &o) const
    {
      const size_t nc = tria->cells.size();
      o.resize(nc * 3);
      for (size_t ci = 0; ci < nc; ++ci)
        {
          const Cell  &c = tria->cells[ci];
          const double h = 2.0 / (double)(1u << c.level);
          o[3 * ci]      = -1.0 + h * c.i;
          o[3 * ci + 1]  = -1.0 + h * c.j;
          o[3 * ci + 2]  = -1.0 + h * c.k;
        }
    }
    // the physical points of the tensor rule QGauss(n_q)^3 on every leaf, [cell][qz][qy][qx][3]: corner + h x_q per coordinate (one
    // multiplication and one addition in double, the expression of compute_rhs_function), leaves in the order of the mesh's cells
    void
    quadrature_points(int n_q, std::vector<double> &xyz) const
    {
      refuse_estimate("quadrature_points");
      const int           nq = resolve_n_q(n_q, "quadrature_points");
      std::vector<double> x01, w01, o;
      FE1D::gauss_rule(nq, x01, w01);
      cell_origins(o);
      const size_t nc = tria->cells.size(), nq3 = (size_t)nq * nq * nq;
      xyz.resize(nc * nq3 * 3);
      for (size_t ci = 0; ci < nc; ++ci)
        {
          const double h = 2.0 / (double)(1u << tria->cells[ci].level);
          double      *x = &xyz[ci * nq3 * 3];
          for (int qz = 0; qz < nq; ++qz)
            for (int qy = 0; qy < nq; ++qy)
              for (int qx = 0; qx < nq; ++qx, x += 3)
                {
                  x[0] = o[3 * ci] + h * x01[qx];
                  x[1] = o[3 * ci + 1] + h * x01[qy];
                  x[2] = o[3 * ci + 2] + h * x01[qz];
                }
        }
    }
    bool
    is_dirichlet_index(uint32_t gi) const
    {
      return gi >= first_dirichlet() && gi < first_dirichlet() + n_dirichlet;
    }
    static const char *
    face_name(int f)
    {
      static const char *const name[6] = {"x=-1", "x=+1", "y=-1", "y=+1", "z=-1", "z=+1"};
      return name[f];
    }
    // The lifting goes through the cell matrices only.  The surface mass matrix of a convective face couples to the Dirichlet DoFs
    // on an edge it shares with a Dirichlet face: every Dirichlet face but the opposite one.  That term is not built: refused.
    void
    refuse_dirichlet_lift(const char *who) const
    {
      if (ls_level)
        throw std::invalid_argument(std::string(who) + ": refused on the level of a local-smoothing hierarchy (its refinement-edge DoFs "
                                                       "are constrained like Dirichlet DoFs); use the active-mesh operator");
      for (int f = 0; f < 6; ++f)
        if (robin[f] > 0.0)
          for (int f2 = 0; f2 < 6; ++f2)
            if (((dirichlet_faces >> f2) & 1) && (f2 >> 1) != (f >> 1))
              throw std::invalid_argument(std::string(who) + ": refused, the convective face " + std::to_string(f) + " (" + face_name(f) +
                                          ", Robin coefficient " + std::to_string(robin[f]) + ") shares an edge with the Dirichlet face " +
                                          std::to_string(f2) + " (" + face_name(f2) +
                                          "): the lifting of Dirichlet data carries no face term; only the face opposite a convective "
                                          "face may be Dirichlet");
    }
    // lift(g, include_mass) = -[C^T (K_a + s sigma M) C g^]  on free rows, 0 on constrained rows; g^ = g on Dirichlet DoFs, 0
    // elsewhere (the entries of g at free and hanging DoFs are not read)
    void
    compute_rhs_dirichlet(const double *g, bool include_mass, std::vector<double> &b) const
    {
      refuse_dirichlet_lift("rhs_dirichlet");
      b.assign(n_dofs, 0.0);
      dirichlet_lift_add(g, include_mass, -1.0, b);
    }
    // g = v[f] on the Dirichlet DoFs of face f (the lowest-numbered Dirichlet face of a DoF on several), 0 elsewhere
    void
    dirichlet_face_values(const double v[6], std::vector<double> &g) const
    {
      for (int f = 0; f < 6; ++f)
        {
          if (!std::isfinite(v[f]))
            throw std::invalid_argument("Dirichlet value on face " + std::to_string(f) + " (" + face_name(f) + ") is not finite");
          if (v[f] != 0.0 && !((dirichlet_faces >> f) & 1))
            throw std::invalid_argument("Dirichlet value " + std::to_string(v[f]) + " on face " + std::to_string(f) + " (" + face_name(f) +
                                        ") refused: the face is natural (dirichlet_faces mask " + std::to_string(dirichlet_faces) +
                                        "), a Dirichlet value needs a Dirichlet face");
        }
      g.assign(n_dofs, 0.0);
      const int32_t top = p << LMAX;
      keymap_for_each([&](uint64_t key, int32_t idx) {
        if (!is_dirichlet_index((uint32_t)idx))
          return;
        const DofKey  k    = unpack_key(key);
        const int32_t x[3] = {k.px, k.py, k.pz};
        for (int f = 0; f < 6; ++f)
          if (((dirichlet_faces >> f) & 1) && x[f >> 1] == ((f & 1) ? top : 0))
            {
              g[idx] = v[f];
              return;
            }
      });
    }
    // g = data_g(kind, support point) on the Dirichlet DoFs, 0 elsewhere: the built-in data of SimulationType `kind` as caller data
    void
    dirichlet_kind_values(int kind, std::vector<double> &g) const
    {
      g.assign(n_dofs, 0.0);
      if (kind == 0)
        return;
      keymap_for_each([&](uint64_t key, int32_t idx) {
        if (!is_dirichlet_index((uint32_t)idx))
          return;
        double x[3];
        key_position(unpack_key(key), x);
        g[idx] = data_g(kind, x);
      });
    }
    // support point of the DoF behind a key
    void
    key_position(const DofKey &k, double xyz[3]) const
    {
      const int32_t x[3] = {k.px, k.py, k.pz};
      for (int d = 0; d < 3; ++d)
        {
          // a coordinate strictly inside a cell (direction mask bit set) is a node of the key's level; the others are vertices
          const int     lev = ((k.dirmask >> d) & 1) ? k.level : LMAX;
          const int32_t q   = x[d] >> (LMAX - lev); // cell index * p + local node
          xyz[d]            = -1.0 + 2.0 / (double)(1u << lev) * ((double)(q / p) + fe.nodes[q % p]);
        }
    }
    // support point of every DoF, [n_dofs][3]
    void
    export_node_positions(std::vector<double> &xyz) const
    {
      std::vector<DofKey> keys;
      export_dof_keys(keys);
      xyz.assign((size_t)n_dofs * 3, 0.0);
      for (uint32_t i = 0; i < n_dofs; ++i)
        key_position(keys[i], &xyz[(size_t)i * 3]);
    }
    // distribute for caller data: Dirichlet DoFs take the values of g, then the hanging DoFs are interpolated from their parents;
    // free DoFs are untouched
    void
    distribute_values(const double *g, std::vector<double> &x) const
    {
      for (uint32_t i = first_dirichlet(); i < first_dirichlet() + n_dirichlet; ++i)
        x[i] = g[i];
      distribute_hanging(x);
    }
    // The hanging DoFs as rows of parents and weights (CSR over the hanging range, row r = DoF first_dirichlet() + n_dirichlet + r),
    // from the same per-cell interpolation as distribute_hanging: row of node t = C^T e_t.  A DoF no local cell reaches has no entries.
    void
    hanging_rows(std::vector<uint32_t> &ptr, std::vector<uint32_t> &col, std::vector<double> &val) const
    {
      const int      n = p + 1, n3 = n * n * n;
      const uint32_t first_hanging = first_dirichlet() + n_dirichlet, nh = n_dofs - first_hanging;
      std::vector<std::vector<std::pair<uint32_t, double>>> rows(nh);
      std::vector<uint8_t>                                  done(nh, 0);
      std::vector<double>                                   w(n3);
      std::vector<uint32_t>                                 idx(n3);
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        {
          const uint16_t mask = tria->masks[ci];
          if (!cell_is_local(ci) || !(mask >> MASK_FACE_SHIFT))
            continue;
          bool gathered = false;
          for (int t = 0; t < n3; ++t)
            {
              const int a[3] = {t % n, (t / n) % n, t / (n * n)};
              bool      corner;
              if (!node_on_constrained_entity(mask, p, a, &corner) || corner)
                continue;
              const int32_t *own = keymap.find(own_key(tria->cells[ci], a));
              if (!own || (uint32_t)*own < first_hanging || done[*own - first_hanging])
                continue;
              if (!gathered)
                gather_cell(ci, idx.data(), true);
              gathered = true;
              std::fill(w.begin(), w.end(), 0.0);
              w[t] = 1.0;
              interpolate_hanging(fe, mask, w.data(), true);
              auto &row = rows[*own - first_hanging];
              for (int s = 0; s < n3; ++s)
                if (w[s] != 0.0 && idx[s] != INVALID_DOF)
                  row.push_back({idx[s], w[s]});
              done[*own - first_hanging] = 1;
            }
        }
      ptr.assign(nh + 1, 0);
      col.clear();
      val.clear();
      for (uint32_t r = 0; r < nh; ++r)
        {
          for (const auto &e : rows[r])
            {
              col.push_back(e.first);
              val.push_back(e.second);
            }
          ptr[r + 1] = (uint32_t)col.size();
        }
    }
    // cell_node_index with the real index on Dirichlet DoFs (INVALID_DOF only where the DoF is not numbered on this rank)
    uint32_t
    gathered_index(size_t ci, const int a[3]) const
    {
      uint32_t id = cell_node_index(ci, a);
      if (id == INVALID_DOF)
        if (const int32_t *gi = keymap.find(resolved_key(ci, a)))
          id = (uint32_t)*gi;
      return id;
    }
    // the (p+1)^3 indices cell ci gathers, x fastest: cell_node_index, or gathered_index where real_dirichlet_index is set
    void
    gather_cell(size_t ci, uint32_t *idx, bool real_dirichlet_index) const
    {
      const int n = p + 1;
      for (int t = 0; t < n * n * n; ++t)
        {
          const int a[3] = {t % n, (t / n) % n, t / (n * n)};
          idx[t]         = real_dirichlet_index ? gathered_index(ci, a) : cell_node_index(ci, a);
        }
    }

    // no Dirichlet face, sigma == 0 and no convective face: the constants are in the operator's kernel.  Operators stay available;
    // solvers refuse.
    bool
    singular() const
    {
      return dirichlet_faces == 0 && sigma == 0.0 && !has_robin();
    }
    void
    refuse_singular(const char *who) const
    {
      if (singular())
        throw std::invalid_argument(std::string(who) + ": refused, the operator is singular: dirichlet_faces mask 0 (no Dirichlet face) with "
                                    "mass coefficient sigma = 0 and no convective face has the constants in its kernel, and no mean-value projection is built");
    }
    double
    coefficient_of(size_t cell) const
    {
      return coefficient.empty() ? 1.0 : coefficient[cell];
    }
    // smallest and largest value over this rank's cells
    void
    coefficient_range(double &lo, double &hi) const
    {
      lo = hi = 1.0;
      bool first = true;
      for (size_t ci = 0; ci < coefficient.size(); ++ci)
        if (cell_is_local(ci))
          {
            lo    = first ? coefficient[ci] : std::min(lo, coefficient[ci]);
            hi    = first ? coefficient[ci] : std::max(hi, coefficient[ci]);
            first = false;
          }
    }
    void
    set_mass_coefficient(double s)
    {
      if (!(s >= 0.0) || !std::isfinite(s))
        throw std::invalid_argument("mass coefficient " + std::to_string(s) + " refused: it must be finite and >= 0");
      if (ls_level && s != 0.0)
        throw std::invalid_argument("mass coefficient " + std::to_string(s) +
                                    " refused: local-smoothing level tables only take 0 (refinement-edge matrices have no mass term)");
      sigma = s;
    }
    static constexpr int      CLS_SHIFT = 29;
    static constexpr uint32_t CLS_MASK  = (1u << CLS_SHIFT) - 1;
    // distributed runs: the tail is [owned | copies of DoFs owned by a lower rank]; *_owned count each DoF once globally
    uint32_t n_tail_owned = 0, n_dirichlet_owned = 0, n_hanging_owned = 0;
    // per cell: group, slot-in-group
    std::vector<uint8_t>  cell_group;
    std::vector<uint32_t> cell_slot;
    FlatMap               keymap; // packed key -> global index (T, D, H DoFs only)

    // owned: optional per-cell flags (distributed runs: this rank's cells); shared: key -> mask of other sharing ranks
    LevelTables(const Tria &t, int degree, int max_brick = 0, const std::vector<uint8_t> *owned = nullptr, bool helpers_only = false,
                const std::map<uint64_t, SharedInfo> *shared = nullptr, int my_rank = 0, bool local_smoothing_level = false)
      : p(degree)
      , tria(&t)
      , fe(degree)
      , ls_level(local_smoothing_level)
      , owned(owned)
      , shared(shared)
      , my_rank(my_rank)
    {
      coefficient     = t.coefficient;
      dirichlet_faces = t.dirichlet_faces;
      std::copy(t.robin, t.robin + 6, robin);
      if (ls_level && has_robin())
        throw std::invalid_argument("local-smoothing level tables of a triangulation with Robin coefficients (convective faces): not "
                                    "implemented, only all coefficients 0");
      if (ls_level && dirichlet_faces != Tria::ALL_DIRICHLET)
        throw std::invalid_argument("local-smoothing level tables of a triangulation with the dirichlet_faces mask " +
                                    std::to_string(dirichlet_faces) + ": not implemented, only the mask 63");
      if (ls_level && !coefficient.empty())
        throw std::invalid_argument("local-smoothing level tables of a triangulation with a diffusion coefficient: not implemented "
                                    "(the refinement-edge matrices have no coefficient)");
      if (ls_level && (owned || shared))
        throw std::runtime_error("local-smoothing levels are not sharded in this build");
      if (!helpers_only)
        build(max_brick > 0 ? std::min(max_brick, max_brick_for_degree(p)) : max_brick_for_degree(p));
    }
    bool
    cell_is_local(size_t ci) const
    {
      return cell_group[ci] < 0xFE;
    }

    uint32_t
    first_constrained() const
    {
      return n_interior + n_tail; // refinement-edge DoFs count as constrained for the level operator
    }
    uint32_t
    first_dirichlet() const
    {
      return n_interior + n_tail + n_edge;
    }

    // is local node (a,b,c) of a masked cell on one of its hanging faces/edges?
    static bool
    node_on_constrained_entity(uint16_t mask, int p, const int a[3], bool *parent_corner = nullptr)
    {
      const int cp[3] = {mask & 1, (mask >> 1) & 1, (mask >> 2) & 1};
      bool      on[3];
      for (int d = 0; d < 3; ++d)
        on[d] = a[d] == cp[d] * p;
      if (parent_corner)
        *parent_corner = on[0] && on[1] && on[2];
      for (int d = 0; d < 3; ++d)
        {
          if (((mask >> (MASK_FACE_SHIFT + d)) & 1) && on[d])
            return true;
          if (((mask >> (MASK_EDGE_SHIFT + d)) & 1) && on[(d + 1) % 3] && on[(d + 2) % 3])
            return true;
        }
      return false;
    }

    // key of the DoF that cell `ci` gathers at local node a (parent-resolved for hanging entities)
    uint64_t
    resolved_key(size_t ci, const int a[3]) const
    {
      const Cell    &c    = tria->cells[ci];
      const uint16_t mask = tria->masks[ci];
      if ((mask >> MASK_FACE_SHIFT) && node_on_constrained_entity(mask, p, a))
        return own_key(Cell{c.i >> 1, c.j >> 1, c.k >> 1, (uint8_t)(c.level - 1)}, a);
      return own_key(c, a);
    }
    uint64_t
    own_key(const Cell &c, const int a[3]) const
    {
      const uint32_t S  = 1u << (LMAX - c.level);
      const int      dm = (a[0] % p ? 1 : 0) | (a[1] % p ? 2 : 0) | (a[2] % p ? 4 : 0);
      return pack_key((c.i * p + a[0]) * S, (c.j * p + a[1]) * S, (c.k * p + a[2]) * S, dm, c.level);
    }
    // does the DoF lie on at least one Dirichlet face of the mesh (dirichlet_faces; edges and corners shared with one count)?
    bool
    key_on_dirichlet_face(uint64_t key) const
    {
      const DofKey  k    = unpack_key(key);
      const int32_t top  = p << LMAX;
      const int32_t x[3] = {k.px, k.py, k.pz};
      for (int d = 0; d < 3; ++d)
        if ((x[d] == 0 && ((dirichlet_faces >> (2 * d)) & 1)) || (x[d] == top && ((dirichlet_faces >> (2 * d + 1)) & 1)))
          return true;
      return false;
    }

    // global DoF index gathered by cell ci at local node (a0,a1,a2); INVALID_DOF for Dirichlet.
    // *constrained: node lies on a hanging face/edge (index then refers to the parent entity's DoF)
    uint32_t
    cell_node_index(size_t ci, const int a[3], bool *constrained = nullptr, bool *parent_corner = nullptr) const
    {
      if (!cell_is_local(ci))
        {
          if (constrained)
            *constrained = false;
          if (parent_corner)
            *parent_corner = false;
          return INVALID_DOF;
        }
      const SlotGroup &g    = groups[cell_group[ci]];
      const uint32_t   s    = cell_slot[ci];
      const Cell      &c    = tria->cells[ci];
      const uint16_t   mask = tria->masks[ci];
      if (constrained)
        *constrained = (mask >> MASK_FACE_SHIFT) ? node_on_constrained_entity(mask, p, a, parent_corner) : false;
      if (g.B >= 2 && g.fmask[s] && (mask >> MASK_FACE_SHIFT) && node_on_constrained_entity(mask, p, a))
        {
          // cell of a constrained brick: the parent entity's DoF, as for a single cell
          const int32_t *idx = keymap.find(resolved_key(ci, a));
          if (!idx)
            throw std::runtime_error("constrained family: parent DoF not numbered");
          const uint32_t gi = (uint32_t)*idx;
          return (gi >= first_dirichlet() && gi < first_dirichlet() + n_dirichlet) ? INVALID_DOF : gi;
        }
      const int x = (c.i & (g.B - 1)) * p + a[0], y = (c.j & (g.B - 1)) * p + a[1], z = (c.k & (g.B - 1)) * p + a[2];
      const int N = g.N;
      if (x > 0 && y > 0 && z > 0 && x < N - 1 && y < N - 1 && z < N - 1)
        return g.interior_base[s] + ((z - 1) * (N - 2) + (y - 1)) * (N - 2) + (x - 1);
      return g.shell_idx[(size_t)s * g.n_shell + shell_slot_of(N, x, y, z)];
    }

    // full per-cell table (resolved indices, x fastest), for the CPU oracle and tests
    void
    export_cell_dofs(std::vector<uint32_t> &out) const
    {
      const size_t n3 = (size_t)(p + 1) * (p + 1) * (p + 1);
      out.resize(tria->cells.size() * n3);
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        gather_cell(ci, &out[ci * n3], false);
    }

    // geometric identity of every DoF (for matching against an independently numbered oracle)
    void
    export_dof_keys(std::vector<DofKey> &out) const
    {
      out.assign(n_dofs, DofKey{-1, -1, -1, -1, -1});
      for (const SlotGroup &g : groups)
        for (size_t s = 0; s < g.n_slots(); ++s)
          {
            const Cell &c = tria->cells[g.first_cell[s]];
            const Cell  anchor{c.i & ~(uint32_t)(g.B - 1), c.j & ~(uint32_t)(g.B - 1), c.k & ~(uint32_t)(g.B - 1), c.level};
            const int   N = g.N;
            for (int z = 1; z < N - 1; ++z)
              for (int y = 1; y < N - 1; ++y)
                for (int x = 1; x < N - 1; ++x)
                  {
                    const int a[3] = {x, y, z};
                    out[g.interior_base[s] + ((z - 1) * (N - 2) + (y - 1)) * (N - 2) + (x - 1)] = unpack_key(own_key(anchor, a));
                  }
          }
      keymap_for_each([&](uint64_t key, int32_t idx) {
        DofKey k = unpack_key(key);
        out[idx] = k;
      });
    }

    // right-hand side for f == 1, homogeneous Dirichlet data (ref:include/operator.h:362-413;
    // the lifting of ref:include/operator.h:415-446 vanishes for g == 0)
    void
    compute_rhs_constant(std::vector<double> &b) const
    {
      b.assign(n_dofs, 0.0);
      const int n = p + 1;
      for (const SlotGroup &g : groups)
        {
          const int           N = g.N;
          std::vector<double> m1(N, 0.0); // assembled 1D load vector over the brick line
          for (int cb = 0; cb < g.B; ++cb)
            for (int a = 0; a < n; ++a)
              m1[cb * p + a] += fe.m[a];
          std::vector<double> loc((size_t)N * N * N);
          for (size_t s = 0; s < g.n_slots(); ++s)
            {
              const double h3 = g.h[s] * g.h[s] * g.h[s];
              for (int z = 0; z < N; ++z)
                for (int y = 0; y < N; ++y)
                  for (int x = 0; x < N; ++x)
                    loc[(z * N + y) * N + x] = h3 * m1[x] * m1[y] * m1[z];
              if (g.B == 1)
                interpolate_hanging(fe, g.mask[s], loc.data(), true);
              else if (g.B >= 2 && g.fmask[s])
                interpolate_family(fe, g.B, g.fmask[s], loc.data(), true);
              for (int z = 0; z < N; ++z)
                for (int y = 0; y < N; ++y)
                  for (int x = 0; x < N; ++x)
                    {
                      uint32_t idx;
                      if (x > 0 && y > 0 && z > 0 && x < N - 1 && y < N - 1 && z < N - 1)
                        idx = g.interior_base[s] + ((z - 1) * (N - 2) + (y - 1)) * (N - 2) + (x - 1);
                      else
                        idx = g.shell_idx[s * g.n_shell + shell_slot_of(N, x, y, z)];
                      if (idx != INVALID_DOF)
                        b[idx] += loc[(z * N + y) * N + x];
                    }
            }
        }
    }

    // ---- general data: SimulationType "Gaussian" (ref:multigrid_throughput.cc:60-125,2294-2298) -------------------
    // u_exact = sum over centres of exp(-|x - c|^2 / w^2) / (sqrt(2 pi) w)^3, f = -Laplace u_exact; the reference uses
    // one centre (-0.5,-0.5,-0.5) and w = 0.1.  kind 0: f = 1, g = 0 (the default "Constant").
    static double
    gaussian_solution(const double x[3])
    {
      const double w = 0.1, c[3] = {-0.5, -0.5, -0.5};
      double       r2 = 0;
      for (int d = 0; d < 3; ++d)
        r2 += (x[d] - c[d]) * (x[d] - c[d]);
      const double s = std::sqrt(2.0 * 3.14159265358979323846) * w;
      return std::exp(-r2 / (w * w)) / (s * s * s);
    }
    static double
    gaussian_rhs(const double x[3])
    {
      const double w = 0.1, c[3] = {-0.5, -0.5, -0.5};
      double       r2 = 0;
      for (int d = 0; d < 3; ++d)
        r2 += (x[d] - c[d]) * (x[d] - c[d]);
      const double s = std::sqrt(2.0 * 3.14159265358979323846) * w;
      return (2.0 * 3 - 4.0 * r2 / (w * w)) / (w * w) * std::exp(-r2 / (w * w)) / (s * s * s);
    }
    static double
    data_f(int kind, const double x[3])
    {
      return kind == 0 ? 1.0 : gaussian_rhs(x);
    }
    static double
    data_g(int kind, const double x[3])
    {
      return kind == 0 ? 0.0 : gaussian_solution(x);
    }
    // out = A (or A^T) along direction d of one cell's (p+1)^3 values (x fastest); A is (p+1)^2, row-major
    void
    sweep_1d(const double *A, bool transposed, int d, const double *in, double *out) const
    {
      const int n = p + 1, n3 = n * n * n, st = d == 0 ? 1 : (d == 1 ? n : n * n);
      const int row = transposed ? 1 : n, col = transposed ? n : 1;
      for (int line = 0; line < n3; line += st * n) // the lines along d start at line + i, i < st
        for (int a = 0; a < n; ++a)
          for (int i = 0; i < st; ++i)
            {
              double s = 0;
              for (int b = 0; b < n; ++b)
                s += A[a * row + b * col] * in[line + i + b * st];
              out[line + i + a * st] = s;
            }
    }
    // y = K_cell x on one cell's (p+1)^3 values (x fastest), h = cell size
    void
    cell_stiffness_apply(double h, const double *x, double *y) const
    {
      const int           n = p + 1, n3 = n * n * n;
      std::vector<double> t1(n3), t2(n3), t3(n3);
      for (int i = 0; i < n3; ++i)
        y[i] = 0;
      for (int dk = 0; dk < 3; ++dk)
        { // K in direction dk, M in the others
          sweep_1d((dk == 0 ? fe.K : fe.M).data(), false, 0, x, t1.data());
          sweep_1d((dk == 1 ? fe.K : fe.M).data(), false, 1, t1.data(), t2.data());
          sweep_1d((dk == 2 ? fe.K : fe.M).data(), false, 2, t2.data(), t3.data());
          for (int i = 0; i < n3; ++i)
            y[i] += h * t3[i];
        }
    }
    // y += sigma M_cell x,  M_cell = h^3 M (x) M (x) M
    void
    cell_mass_add(double h, double sigma, const double *x, double *y) const
    {
      const int           n = p + 1, n3 = n * n * n;
      std::vector<double> t1(n3), t2(n3);
      sweep_1d(fe.M.data(), false, 0, x, t1.data());
      sweep_1d(fe.M.data(), false, 1, t1.data(), t2.data());
      sweep_1d(fe.M.data(), false, 2, t2.data(), t1.data());
      for (int i = 0; i < n3; ++i)
        y[i] += sigma * h * h * h * t1[i];
    }

    // right-hand side for data `kind` (ref:include/operator.h:362-447): load vector by QGauss(p+1) quadrature of f, constrained
    // rows 0, minus the lifting of the boundary interpolant of g (dirichlet_kind_values through dirichlet_lift_add).
    // With a mass coefficient the manufactured load is -Laplace u_g + sigma u_g and the lifting uses K + sigma M.
    void
    compute_rhs_function(int kind, std::vector<double> &b) const
    {
      if (kind == 0)
        {
          compute_rhs_constant(b);
          return;
        }
      // the lifting of non-zero Dirichlet data below goes through the cell matrices only: a convective face next to a Dirichlet face
      // couples the two through its surface mass matrix, which it would miss
      if (has_robin())
        throw std::invalid_argument("right-hand side of SimulationType " + std::to_string(kind) +
                                    " with Robin coefficients (convective faces): not implemented, the lifting of non-zero Dirichlet "
                                    "data carries no face term; only kind 0 (f = 1, g = 0)");
      b.assign(n_dofs, 0.0);
      const int             n = p + 1, n3 = n * n * n;
      std::vector<double>   fq(n3), t1(n3), t2(n3), load(n3);
      std::vector<uint32_t> idx(n3);
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        {
          if (!cell_is_local(ci))
            continue;
          const Cell  &c    = tria->cells[ci];
          const double h    = 2.0 / (double)(1u << c.level);
          const double o[3] = {-1.0 + h * c.i, -1.0 + h * c.j, -1.0 + h * c.k};
          // f at the quadrature points, times JxW
          for (int qz = 0; qz < n; ++qz)
            for (int qy = 0; qy < n; ++qy)
              for (int qx = 0; qx < n; ++qx)
                {
                  const double x[3] = {o[0] + h * fe.xq[qx], o[1] + h * fe.xq[qy], o[2] + h * fe.xq[qz]};
                  const double f    = sigma != 0.0 ? data_f(kind, x) + sigma * data_g(kind, x) : data_f(kind, x);
                  fq[(qz * n + qy) * n + qx] = f * h * h * h * fe.wq[qx] * fe.wq[qy] * fe.wq[qz];
                }
          // integrate against the shape functions: load[a] = sum_q S[q][a] ... per direction
          sweep_1d(fe.S.data(), true, 0, fq.data(), t1.data());
          sweep_1d(fe.S.data(), true, 1, t1.data(), t2.data());
          sweep_1d(fe.S.data(), true, 2, t2.data(), load.data());
          interpolate_hanging(fe, tria->masks[ci], load.data(), true);
          gather_cell(ci, idx.data(), false);
          for (int t = 0; t < n3; ++t)
            if (idx[t] != INVALID_DOF)
              b[idx[t]] += load[t];
        }
      for (uint32_t i = first_constrained(); i < n_dofs; ++i)
        b[i] = 0.0;
      std::vector<double> g;
      dirichlet_kind_values(kind, g);
      dirichlet_lift_add(g.data(), true, -1.0, b);
    }

    // ---- cell evaluate and integrate (DESIGN.md "Cell evaluate and integrate"; on the device: kernels_cell_values.hpp) -------------
    // sweep_1d for the rectangular matrices of a rule with n_q != p + 1: out = A (or A^T) along direction d of a tensor with the
    // extents dims[3] (x fastest); A is rows x cols, row-major.  Not transposed: dims[d] == cols, the extent becomes rows;
    // transposed: dims[d] == rows, the extent becomes cols.  dims is updated.
    static void
    sweep_1d_rect(const double *A, int rows, int cols, bool transposed, int d, int dims[3], const double *in, std::vector<double> &out)
    {
      const int n_in = dims[d], n_out = transposed ? cols : rows;
      const int st = d == 0 ? 1 : (d == 1 ? dims[0] : dims[0] * dims[1]), outer = dims[0] * dims[1] * dims[2] / (st * n_in);
      out.assign((size_t)st * n_out * outer, 0.0);
      for (int o = 0; o < outer; ++o)
        for (int a = 0; a < n_out; ++a)
          for (int i = 0; i < st; ++i)
            {
              double s = 0;
              for (int b = 0; b < n_in; ++b)
                s += (transposed ? A[b * cols + a] : A[a * cols + b]) * in[(o * n_in + b) * st + i];
              out[(o * n_out + a) * st + i] = s;
            }
      dims[d] = n_out;
    }
    // values [cell][qz][qy][qx] and/or gradients [cell][component][qz][qy][qx] (either may be null, not both) of the level's Q_p
    // function of u at the points of quadrature_points(n_q): free and Dirichlet entries of u are read, hanging entries never
    void
    evaluate_values(const double *u, int n_q, double *values, double *gradients) const
    {
      refuse_estimate("evaluate");
      const int nq = resolve_n_q(n_q, "evaluate");
      if (!u)
        throw std::invalid_argument("evaluate: u is null (n_dofs values)");
      if (!values && !gradients)
        throw std::invalid_argument("evaluate: neither values nor gradients (at least one output)");
      const int             n = p + 1, n3 = n * n * n, nq3 = nq * nq * nq;
      std::vector<double>   xq, wq, S, G, loc(n3), t1, t2, t3;
      std::vector<uint32_t> idx(n3);
      fe.shape_at_gauss(nq, xq, wq, S, G);
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        {
          const double h = 2.0 / (double)(1u << tria->cells[ci].level);
          gather_cell(ci, idx.data(), true);
          for (int t = 0; t < n3; ++t)
            loc[t] = idx[t] != INVALID_DOF ? u[idx[t]] : 0.0;
          interpolate_hanging(fe, tria->masks[ci], loc.data(), false);
          // component -1: the value (S, S, S); component c: G along c
          for (int c = values ? -1 : 0; c < (gradients ? 3 : 0); ++c)
            {
              int dims[3] = {n, n, n};
              sweep_1d_rect((c == 0 ? G : S).data(), nq, n, false, 0, dims, loc.data(), t1);
              sweep_1d_rect((c == 1 ? G : S).data(), nq, n, false, 1, dims, t1.data(), t2);
              sweep_1d_rect((c == 2 ? G : S).data(), nq, n, false, 2, dims, t2.data(), t3);
              double *out = c < 0 ? values + ci * nq3 : gradients + (ci * 3 + c) * nq3;
              for (int q = 0; q < nq3; ++q)
                out[q] = c < 0 ? t3[q] : t3[q] / h;
            }
        }
    }
    // b_i = sum_K sum_q w_q h_K^3 (v_q phi_i(x_q) + V_q . grad phi_i(x_q)) through C^T; b is overwritten, constrained rows 0; no
    // coefficient and no sigma (values, gradients in the layouts of evaluate_values; either may be null, not both)
    void
    integrate_values(const double *values, const double *gradients, int n_q, std::vector<double> &b) const
    {
      refuse_estimate("integrate");
      const int nq = resolve_n_q(n_q, "integrate");
      if (!values && !gradients)
        throw std::invalid_argument("integrate: neither values nor gradients (at least one input)");
      b.assign(n_dofs, 0.0);
      const int             n = p + 1, n3 = n * n * n, nq3 = nq * nq * nq;
      std::vector<double>   xq, wq, S, G, fq(nq3), load(n3), t1, t2, t3;
      std::vector<uint32_t> idx(n3);
      fe.shape_at_gauss(nq, xq, wq, S, G);
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        {
          const double h = 2.0 / (double)(1u << tria->cells[ci].level);
          std::fill(load.begin(), load.end(), 0.0);
          for (int c = values ? -1 : 0; c < (gradients ? 3 : 0); ++c)
            {
              const double *in = c < 0 ? values + ci * nq3 : gradients + (ci * 3 + c) * nq3;
              const double  jw = c < 0 ? h * h * h : h * h; // JxW, with the 1 / h of the gradient
              for (int qz = 0; qz < nq; ++qz)
                for (int qy = 0; qy < nq; ++qy)
                  for (int qx = 0; qx < nq; ++qx)
                    fq[(qz * nq + qy) * nq + qx] = in[(qz * nq + qy) * nq + qx] * jw * wq[qx] * wq[qy] * wq[qz];
              int dims[3] = {nq, nq, nq};
              sweep_1d_rect((c == 0 ? G : S).data(), nq, n, true, 0, dims, fq.data(), t1);
              sweep_1d_rect((c == 1 ? G : S).data(), nq, n, true, 1, dims, t1.data(), t2);
              sweep_1d_rect((c == 2 ? G : S).data(), nq, n, true, 2, dims, t2.data(), t3);
              for (int t = 0; t < n3; ++t)
                load[t] += t3[t];
            }
          interpolate_hanging(fe, tria->masks[ci], load.data(), true);
          gather_cell(ci, idx.data(), false);
          for (int t = 0; t < n3; ++t)
            if (idx[t] != INVALID_DOF)
              b[idx[t]] += load[t];
        }
      for (uint32_t i = first_constrained(); i < n_dofs; ++i)
        b[i] = 0.0;
    }

    // ---- point evaluation and point sources (DESIGN.md "Point evaluation and point sources"; on the device: kernels_point_values.hpp)
    // The sorted Morton keys of the leaves (the mesh's cells ARE in this order: Tria::finalize); leaf t covers [key_t, key_{t+1}).
    void
    leaf_keys(std::vector<uint64_t> &keys) const
    {
      keys.resize(tria->cells.size());
      for (size_t ci = 0; ci < keys.size(); ++ci)
        keys[ci] = morton(tria->cells[ci]);
    }
    // the leaf and the reference coordinate of one point by the rule of octree.hpp point_key: false when the point is not found
    bool
    locate_point(const std::vector<uint64_t> &keys, const double x[3], int32_t &cell, double ref[3]) const
    {
      double   s[3];
      uint64_t key;
      cell   = -1;
      ref[0] = ref[1] = ref[2] = 0.0;
      if (!point_key(x, s, key))
        return false;
      cell          = (int32_t)(std::upper_bound(keys.begin(), keys.end(), key) - keys.begin()) - 1;
      const Cell  &c = tria->cells[cell];
      const double e = (double)(1u << (LMAX - c.level)); // the leaf's edge in integer coordinates
      ref[0]         = (s[0] - (double)c.i * e) / e;     // exact: s - corner is a multiple of ulp(s) below s, e a power of two
      ref[1]         = (s[1] - (double)c.j * e) / e;
      ref[2]         = (s[2] - (double)c.k * e) / e;
      return true;
    }
    // cell[k] (-1: not found) and ref[3k...] in [0, 1] (0 where not found) of the n points xyz[3k...]
    void
    locate_points(size_t n, const double *xyz, int32_t *cell, double *ref) const
    {
      refuse_estimate("locate_points");
      if (n && (!xyz || !cell || !ref))
        throw std::invalid_argument("locate_points: a null pointer (xyz and ref: 3 n doubles, cell: n integers)");
      std::vector<uint64_t> keys;
      leaf_keys(keys);
      for (size_t k = 0; k < n; ++k)
        locate_point(keys, xyz + 3 * k, cell[k], ref + 3 * k);
    }
    // values[k] = u_h(x_k) and/or gradients[c n + k] = d_c u_h(x_k) (either may be null, not both), the one-sided gradient of the
    // point's leaf; exactly 0 where the point is not found.  Free and Dirichlet entries of u are read, hanging entries never.
    void
    point_evaluate(size_t n, const double *xyz, const double *u, double *values, double *gradients) const
    {
      refuse_estimate("point_evaluate");
      if (!u)
        throw std::invalid_argument("point_evaluate: u is null (n_dofs values)");
      if (n && !xyz)
        throw std::invalid_argument("point_evaluate: xyz is null (3 n doubles)");
      if (!values && !gradients)
        throw std::invalid_argument("point_evaluate: neither values nor gradients (at least one output)");
      const int             n1 = p + 1, n3 = n1 * n1 * n1;
      std::vector<uint64_t> keys;
      std::vector<double>   loc(n3), L(3 * n1), D(3 * n1);
      std::vector<uint32_t> idx(n3);
      leaf_keys(keys);
      int32_t held = -1; // the leaf whose conforming nodal values loc holds
      for (size_t k = 0; k < n; ++k)
        {
          int32_t ci;
          double  ref[3], v = 0.0, g[3] = {0.0, 0.0, 0.0};
          if (locate_point(keys, xyz + 3 * k, ci, ref))
            {
              if (ci != held)
                {
                  gather_cell(ci, idx.data(), true);
                  for (int t = 0; t < n3; ++t)
                    loc[t] = idx[t] != INVALID_DOF ? u[idx[t]] : 0.0;
                  interpolate_hanging(fe, tria->masks[ci], loc.data(), false);
                  held = ci;
                }
              const double h = 2.0 / (double)(1u << tria->cells[ci].level);
              for (int d = 0; d < 3; ++d)
                FE1D::lagrange(fe.nodes, ref[d], &L[d * n1], &D[d * n1]);
              for (int c = 0; c < n1; ++c)
                for (int b = 0; b < n1; ++b)
                  for (int a = 0; a < n1; ++a)
                    {
                      const double w = loc[(c * n1 + b) * n1 + a];
                      v += L[2 * n1 + c] * L[n1 + b] * L[a] * w;
                      g[0] += L[2 * n1 + c] * L[n1 + b] * D[a] * w;
                      g[1] += L[2 * n1 + c] * D[n1 + b] * L[a] * w;
                      g[2] += D[2 * n1 + c] * L[n1 + b] * L[a] * w;
                    }
              for (int d = 0; d < 3; ++d)
                g[d] /= h;
            }
          if (values)
            values[k] = v;
          if (gradients)
            for (int d = 0; d < 3; ++d)
              gradients[d * n + k] = g[d];
        }
    }
    // b_i = sum_k ( w_k phi_i(x_k) + W_k . grad phi_i(x_k) ) through C^T: point functionals, no quadrature weight and no h^3.  b is
    // overwritten, constrained rows 0, points that are not found add nothing; no coefficient and no sigma.  values [n], gradients
    // [3][n]; either may be null, not both.
    void
    point_integrate(size_t n, const double *xyz, const double *values, const double *gradients, std::vector<double> &b) const
    {
      refuse_estimate("point_integrate");
      if (n && !xyz)
        throw std::invalid_argument("point_integrate: xyz is null (3 n doubles)");
      if (!values && !gradients)
        throw std::invalid_argument("point_integrate: neither values nor gradients (at least one input)");
      b.assign(n_dofs, 0.0);
      const int             n1 = p + 1, n3 = n1 * n1 * n1;
      std::vector<uint64_t> keys;
      std::vector<double>   load(n3), L(3 * n1), D(3 * n1);
      std::vector<uint32_t> idx(n3);
      leaf_keys(keys);
      for (size_t k = 0; k < n; ++k)
        {
          int32_t ci;
          double  ref[3];
          if (!locate_point(keys, xyz + 3 * k, ci, ref))
            continue;
          const double h = 2.0 / (double)(1u << tria->cells[ci].level);
          const double w = values ? values[k] : 0.0;
          const double W[3] = {gradients ? gradients[k] / h : 0.0, gradients ? gradients[n + k] / h : 0.0, gradients ? gradients[2 * n + k] / h : 0.0};
          for (int d = 0; d < 3; ++d)
            FE1D::lagrange(fe.nodes, ref[d], &L[d * n1], &D[d * n1]);
          for (int c = 0; c < n1; ++c)
            for (int bb = 0; bb < n1; ++bb)
              for (int a = 0; a < n1; ++a)
                load[(c * n1 + bb) * n1 + a] = w * L[2 * n1 + c] * L[n1 + bb] * L[a] + W[0] * L[2 * n1 + c] * L[n1 + bb] * D[a] +
                                               W[1] * L[2 * n1 + c] * D[n1 + bb] * L[a] + W[2] * D[2 * n1 + c] * L[n1 + bb] * L[a];
          interpolate_hanging(fe, tria->masks[ci], load.data(), true);
          gather_cell(ci, idx.data(), false);
          for (int t = 0; t < n3; ++t)
            if (idx[t] != INVALID_DOF)
              b[idx[t]] += load[t];
        }
      for (uint32_t i = first_constrained(); i < n_dofs; ++i)
        b[i] = 0.0;
    }

    // the refusals of a boundary flux; the error indicator takes the same six constants and refuses them in the same words
    void
    check_boundary_flux(const double q[6]) const
    {
      for (int f = 0; f < 6; ++f)
        {
          if (!std::isfinite(q[f]))
            throw std::invalid_argument("boundary flux on face " + std::to_string(f) + " (" + face_name(f) + ") is not finite");
          if (q[f] != 0.0 && ((dirichlet_faces >> f) & 1))
            throw std::invalid_argument("boundary flux " + std::to_string(q[f]) + " on face " + std::to_string(f) + " (" + face_name(f) +
                                        ") refused: the face is Dirichlet (dirichlet_faces mask " + std::to_string(dirichlet_faces) +
                                        "), a flux load needs a natural face");
        }
    }
    // boundary load of a constant flux q[f] through every natural face f of the cube:  b_i = sum_f q_f int_{Gamma_f} phi_i.  Per
    // boundary cell face the face nodes get q h^2 m (x) m; then C^T through the hanging-node constraints, as the volume load;
    // constrained rows 0.  Independent of a and sigma.  A non-zero flux on a Dirichlet face is refused by name.
    void
    compute_rhs_boundary_flux(const double q[6], std::vector<double> &b) const
    {
      check_boundary_flux(q);
      b.assign(n_dofs, 0.0);
      const int             n = p + 1, n3 = n * n * n;
      std::vector<double>   load(n3);
      std::vector<uint32_t> idx(n3);
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        {
          if (!cell_is_local(ci))
            continue;
          const Cell    &c      = tria->cells[ci];
          const uint32_t last   = (1u << c.level) - 1;
          const uint32_t ijk[3] = {c.i, c.j, c.k};
          const double   h      = 2.0 / (double)(1u << c.level);
          bool           any    = false;
          std::fill(load.begin(), load.end(), 0.0);
          for (int f = 0; f < 6; ++f)
            {
              const int d = f >> 1, side = f & 1;
              if (q[f] == 0.0 || ijk[d] != (side ? last : 0u))
                continue;
              any          = true;
              const int st[3] = {1, n, n * n};
              const int e = (d + 1) % 3, g = (d + 2) % 3;
              for (int ae = 0; ae < n; ++ae)
                for (int ag = 0; ag < n; ++ag)
                  load[side * p * st[d] + ae * st[e] + ag * st[g]] += q[f] * h * h * fe.m[ae] * fe.m[ag];
            }
          if (!any)
            continue;
          interpolate_hanging(fe, tria->masks[ci], load.data(), true);
          gather_cell(ci, idx.data(), false);
          for (int t = 0; t < n3; ++t)
            if (idx[t] != INVALID_DOF)
              b[idx[t]] += load[t];
        }
      for (uint32_t i = first_constrained(); i < n_dofs; ++i)
        b[i] = 0.0;
    }

    // constraints.distribute(x) for data `kind`: Dirichlet DoFs = g at their support point, hanging-node DoFs = the
    // interpolant of their parent face/edge (x holds the solved free DoFs)
    void
    distribute(int kind, std::vector<double> &x) const
    {
      std::vector<double> g;
      dirichlet_kind_values(kind, g);
      distribute_values(g.data(), x);
    }
    // hanging-node DoFs = the interpolant of their parent face/edge, Dirichlet parents included (their values are in x)
    void
    distribute_hanging(std::vector<double> &x) const
    {
      const int             n = p + 1, n3 = n * n * n;
      std::vector<double>   v(n3);
      std::vector<uint32_t> idx(n3);
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        {
          const uint16_t mask = tria->masks[ci];
          if (!cell_is_local(ci) || !(mask >> MASK_FACE_SHIFT))
            continue;
          gather_cell(ci, idx.data(), true); // (a Dirichlet parent keeps its index: its value is in x)
          for (int t = 0; t < n3; ++t)
            v[t] = idx[t] != INVALID_DOF ? x[idx[t]] : 0.0;
          interpolate_hanging(fe, mask, v.data(), false);
          for (int t = 0; t < n3; ++t)
            {
              const int a[3] = {t % n, (t / n) % n, t / (n * n)};
              bool      corner;
              if (node_on_constrained_entity(mask, p, a, &corner) && !corner)
                if (const int32_t *own = keymap.find(own_key(tria->cells[ci], a)))
                  x[*own] = v[t];
            }
        }
    }

    template <class F>
    void
    keymap_for_each(F f) const
    {
      for (size_t t = 0; t < key_list.size(); ++t)
        f(key_list[t], key_index[t]);
    }
    // sharded runs: does this rank own the T/D/H DoF behind `key` (it is not shared, or this rank is its shared_owner)?
    bool
    key_owned(uint64_t key) const
    {
      if (!shared)
        return true;
      const auto it = shared->find(key);
      return it == shared->end() || shared_owner(it->second) == my_rank;
    }

  private:
    std::vector<uint64_t>               key_list;  // keys of T/D/H DoFs in creation order
    std::vector<int32_t>                key_index; // their final global indices
    const std::vector<uint8_t>         *owned   = nullptr;
    const std::map<uint64_t, SharedInfo> *shared  = nullptr;
    int                                 my_rank = 0;

    // the two cells carry the bit-identical coefficient (a brick's cells must: one scale per slot)
    bool
    same_coefficient(size_t c0, size_t c1) const
    {
      return coefficient.empty() || std::memcmp(&coefficient[c0], &coefficient[c1], sizeof(double)) == 0;
    }

    void
    build(int Bmax)
    {
      const auto  &cells = tria->cells;
      const auto  &masks = tria->masks;
      const size_t nc    = cells.size();
      // ---- 1. slot decomposition
      std::vector<int> sizes;
      // at p = 1 the 2^3 and 4^3 bricks are left to the single-cell cluster kernel, which is faster per cell than the
      // lattice kernel on small lattices and saves a launch per size and application (octant, 17 M DoFs, measured:
      // sizes {16,8,4,2,1} 2.93 ms per V-cycle, {16,8,4,1} 2.66, later {16,8,4,1} 2.31, {16,8,1} 2.23, {16,1} 2.29)
      const bool hanging_bricks = getenv("MGAMD_NO_HANGING_BRICKS") == nullptr;
      // p >= 2: only families (the 8 children of one cell) may be constrained bricks
      // (larger constrained bricks only at p = 1: kernels.hpp brick_may_be_constrained, with the measurements)
      const int  max_constrained_brick = p != 1 ? 2 : 1 << 30;
      const int  skip                  = p == 1 ? 6 : 0; // bit mask of the brick sizes left out
      std::vector<bool> constrained_only;
      for (int B = Bmax; B >= 1; B /= 2)
        if (B == 1 || B == Bmax || !(skip & B))
          {
            sizes.push_back(B);
            constrained_only.push_back(false);
            if (B > 2 && hanging_bricks && B <= max_constrained_brick)
              { // second group of this size for the constrained bricks
                sizes.push_back(B);
                constrained_only.push_back(true);
              }
          }
      groups.resize(sizes.size());
      cell_group.assign(nc, 0xFF);
      cell_slot.assign(nc, 0);
      if (owned)
        for (size_t t = 0; t < nc; ++t)
          if (!(*owned)[t])
            cell_group[t] = 0xFE; // not ours
      for (size_t gi = 0; gi < sizes.size(); ++gi)
        {
          SlotGroup &g = groups[gi];
          g.B                 = sizes[gi];
          g.constrained_group = constrained_only[gi];
          g.N          = p * g.B + 1;
          g.n_interior = (g.N - 2) * (g.N - 2) * (g.N - 2);
          g.n_shell    = g.N * g.N * g.N - g.n_interior;
          g.shell_pos.resize(g.n_shell);
          for (int z = 0; z < g.N; ++z)
            for (int y = 0; y < g.N; ++y)
              for (int x = 0; x < g.N; ++x)
                if (!(x > 0 && y > 0 && z > 0 && x < g.N - 1 && y < g.N - 1 && z < g.N - 1))
                  g.shell_pos[shell_slot_of(g.N, x, y, z)] = (uint16_t)((z * g.N + y) * g.N + x);
          const int    B  = g.B;
          const size_t B3 = (size_t)B * B * B;
          int          b  = 0;
          while ((1 << b) < B)
            ++b;
          size_t t = 0;
          while (t < nc)
            {
              if (cell_group[t] != 0xFF)
                {
                  ++t;
                  continue;
                }
              const Cell &c = cells[t];
              bool        ok;
              uint32_t    fm = 0;
              if (B == 1)
                ok = true;
              else
                {
                  ok = c.level >= b && !(c.i & (B - 1)) && !(c.j & (B - 1)) && !(c.k & (B - 1)) && t + B3 <= nc;
                  bool hanging = false;
                  for (size_t s = 0; ok && s < B3; ++s)
                    {
                      const Cell &d = cells[t + s];
                      ok = d.level == c.level && (d.i >> b) == (c.i >> b) && (d.j >> b) == (c.j >> b) && (d.k >> b) == (c.k >> b) &&
                           cell_group[t + s] == 0xFF && same_coefficient(t, t + s);
                      hanging |= (masks[t + s] >> MASK_FACE_SHIFT) != 0;
                    }
                  if (ok && hanging)
                    {
                      // a brick whose hanging entities are whole faces / whole edges stays a (constrained) brick
                      ok = false;
                      if (hanging_bricks && B <= max_constrained_brick && c.level >= 1)
                        {
                          std::vector<std::array<int, 3>> bpos(B3);
                          std::vector<uint16_t>           cm(B3);
                          for (size_t s2 = 0; s2 < B3; ++s2)
                            {
                              const Cell &d = cells[t + s2];
                              bpos[s2]      = {(int)(d.i - c.i), (int)(d.j - c.j), (int)(d.k - c.k)};
                              cm[s2]        = masks[t + s2];
                            }
                          ok = brick_mask_from_cells(B, p, bpos, cm, fm);
                        }
                    }
                  // B > 2: constrained bricks only into the constrained group of this size, the others into the plain one
                  // (the plain group is scanned first; an unclaimed constrained brick is picked up by the next group)
                  if (ok && B > 2 && (fm != 0) != g.constrained_group)
                    ok = false;
                }
              if (!ok)
                {
                  ++t;
                  continue;
                }
              const uint32_t slot = (uint32_t)g.first_cell.size();
              g.first_cell.push_back((uint32_t)t);
              g.mask.push_back(B == 1 ? masks[t] : 0);
              if (B >= 2)
                g.fmask.push_back(fm);
              g.h.push_back(2.0 / (double)(1u << c.level));
              g.a.push_back(coefficient_of(t));
              for (size_t s = 0; s < B3; ++s)
                {
                  cell_group[t + s] = (uint8_t)gi;
                  cell_slot[t + s]  = slot;
                }
              t += B3;
            }
          g.interior_base.assign(g.first_cell.size(), 0);
          g.shell_idx.assign(g.first_cell.size() * (size_t)g.n_shell, INVALID_DOF);
        }
      // ---- 2. interior numbering, slots in Morton order of their first cell
      struct Ref
      {
        uint32_t first_cell, group, slot;
      };
      std::vector<Ref> order;
      for (size_t gi = 0; gi < groups.size(); ++gi)
        for (size_t s = 0; s < groups[gi].n_slots(); ++s)
          order.push_back(Ref{groups[gi].first_cell[s], (uint32_t)gi, (uint32_t)s});
      std::sort(order.begin(), order.end(), [](const Ref &a, const Ref &b) { return a.first_cell < b.first_cell; });
      uint64_t next = 0;
      for (const Ref &r : order)
        {
          groups[r.group].interior_base[r.slot] = (uint32_t)next;
          next += groups[r.group].n_interior;
        }
      if (next > 0xFFFFFFF0ull)
        throw std::runtime_error("level exceeds 32-bit DoF indices");
      n_interior = (uint32_t)next;
      // ---- 3. shell DoFs: class 0 tail, 1 Dirichlet, 2 hanging; provisional id = (class<<30 | counter)
      keymap.erase_all_and_reserve(1024);
      // local smoothing: keys of the DoFs on faces of level cells whose neighbour position is inside the domain but not
      // covered by a cell of this level
      FlatMap edge_keys;
      edge_keys.erase_all_and_reserve(1024);
      if (ls_level)
        for (size_t ci = 0; ci < nc; ++ci)
          {
            const Cell   &c     = cells[ci];
            const int64_t n1    = (int64_t)1 << c.level;
            const int64_t id[3] = {c.i, c.j, c.k};
            for (int d = 0; d < 3; ++d)
              for (int side = 0; side < 2; ++side)
                {
                  int64_t nb[3] = {id[0], id[1], id[2]};
                  nb[d] += side ? 1 : -1;
                  if (nb[d] < 0 || nb[d] >= n1 || tria->find_leaf(c.level, nb[0], nb[1], nb[2]) >= 0)
                    continue;
                  const int e = (d + 1) % 3, f = (d + 2) % 3;
                  for (int ae = 0; ae <= p; ++ae)
                    for (int af = 0; af <= p; ++af)
                      {
                        int a[3];
                        a[d] = side * p;
                        a[e] = ae;
                        a[f] = af;
                        edge_keys.insert(own_key(c, a), 1);
                      }
                }
          }
      uint32_t counter[5] = {0, 0, 0, 0, 0}; // 0 tail (owned), 1 Dirichlet, 2 hanging, 3 tail copy of a lower rank's DoF, 4 refinement edge
      uint32_t n_copy_d = 0, n_copy_h = 0;
      auto     classify = [&](uint64_t key, int cls) -> int32_t {
        bool     ins;
        int32_t *v = keymap.insert(key, 0, &ins);
        if (ins)
          {
            if (shared)
              {
                auto it = shared->find(key);
                if (it != shared->end() && shared_owner(it->second) != my_rank)
                  { // another rank owns this DoF (the lowest rank that references it as a node of one of its cells)
                    if (cls == 0)
                      cls = 3;
                    else if (cls == 1)
                      ++n_copy_d;
                    else
                      ++n_copy_h;
                  }
              }
            *v = (int32_t)(((uint32_t)cls << CLS_SHIFT) | counter[cls]++);
            key_list.push_back(key);
          }
        return *v;
      };
      for (const Ref &r : order)
        {
          SlotGroup   &g = groups[r.group];
          const size_t ci = g.first_cell[r.slot];
          const Cell  &c  = cells[ci];
          const Cell   anchor{c.i & ~(uint32_t)(g.B - 1), c.j & ~(uint32_t)(g.B - 1), c.k & ~(uint32_t)(g.B - 1), c.level};
          for (int s = 0; s < g.n_shell; ++s)
            {
              const int lin  = g.shell_pos[s];
              const int a[3] = {lin % g.N, (lin / g.N) % g.N, lin / (g.N * g.N)};
              uint64_t key;
              if (g.B == 1)
                key = resolved_key(ci, a);
              else if (g.B >= 2 && g.fmask[r.slot])
                {
                  // hanging face/edge of a constrained brick: the parent DoF k p + c of parent cell k sits at lattice
                  // coordinate 2 k p + c (c < p; c = p: B p at the far end); the other lattice positions carry no DoF (filled
                  // by the embedding)
                  bool pinned[3];
                  if (family_node_constrained(g.fmask[r.slot], p, g.B, a, pinned))
                    {
                      int  ap[3], kc[3];
                      bool dof = true;
                      for (int d = 0; d < 3; ++d)
                        {
                          if (pinned[d])
                            {
                              kc[d] = a[d] ? g.B / 2 - 1 : 0;
                              ap[d] = a[d] ? p : 0;
                            }
                          else
                            dof &= family_parent_position(p, g.B, a[d], kc[d], ap[d]);
                        }
                      if (!dof)
                        {
                          g.shell_idx[(size_t)r.slot * g.n_shell + s] = INVALID_DOF;
                          continue;
                        }
                      key = own_key(Cell{(anchor.i >> 1) + (uint32_t)kc[0], (anchor.j >> 1) + (uint32_t)kc[1], (anchor.k >> 1) + (uint32_t)kc[2],
                                         (uint8_t)(c.level - 1)},
                                    ap);
                    }
                  else
                    key = own_key(anchor, a);
                }
              else
                key = own_key(anchor, a);
              const int32_t id = classify(key, key_on_dirichlet_face(key) ? 1 : ((ls_level && edge_keys.find(key)) ? 4 : 0));
              g.shell_idx[(size_t)r.slot * g.n_shell + s] = (uint32_t)id; // provisional
            }
        }
      // own DoFs of hanging faces/edges (single cells and cells of constrained families alike)
      for (size_t ci = 0; ci < nc; ++ci)
        if (cell_is_local(ci) && (masks[ci] >> MASK_FACE_SHIFT))
          for (int z = 0; z <= p; ++z)
            for (int y = 0; y <= p; ++y)
              for (int x = 0; x <= p; ++x)
                {
                  const int a[3] = {x, y, z};
                  bool      corner;
                  if (node_on_constrained_entity(masks[ci], p, a, &corner) && !corner)
                    {
                      const uint64_t key = own_key(cells[ci], a);
                      if (!keymap.find(key))
                        classify(key, 2);
                    }
                }
      n_tail_owned      = counter[0];
      n_tail            = counter[0] + counter[3];
      n_dirichlet       = counter[1];
      n_hanging         = counter[2];
      n_edge            = counter[4];
      n_dirichlet_owned = n_dirichlet - n_copy_d;
      n_hanging_owned   = n_hanging - n_copy_h;
      const uint64_t total = (uint64_t)n_interior + n_tail + n_edge + n_dirichlet + n_hanging;
      if (total > 0xFFFFFFF0ull)
        throw std::runtime_error("level exceeds 32-bit DoF indices");
      n_dofs                 = (uint32_t)total;
      const uint32_t base[5] = {n_interior, n_interior + n_tail + n_edge, n_interior + n_tail + n_edge + n_dirichlet, n_interior + n_tail_owned,
                                n_interior + n_tail};
      auto           final_index = [&](uint32_t prov) {
        const uint32_t c = prov & CLS_MASK;
        return base[prov >> CLS_SHIFT] + c;
      };
      key_index.resize(key_list.size());
      for (size_t t = 0; t < key_list.size(); ++t)
        {
          int32_t *v   = keymap.find(key_list[t]);
          *v           = (int32_t)final_index((uint32_t)*v);
          key_index[t] = *v;
        }
      for (SlotGroup &g : groups)
        for (uint32_t &v : g.shell_idx)
          v = (v == INVALID_DOF || (v >> CLS_SHIFT) == 1) ? INVALID_DOF : final_index(v);
      // ---- 4. sharded level: slots that touch shared DoFs first (stable), per group
      if (shared && !shared->empty())
        {
          std::vector<uint8_t> is_shared(n_dofs, 0);
          for (size_t t = 0; t < key_list.size(); ++t)
            if (shared->find(key_list[t]) != shared->end())
              is_shared[key_index[t]] = 1;
          for (size_t gi = 0; gi < groups.size(); ++gi)
            {
              SlotGroup   &g  = groups[gi];
              const size_t ns = g.n_slots();
              if (!ns)
                continue;
              std::vector<uint32_t> perm; // new position -> old slot
              std::vector<uint8_t>  halo(ns, 0);
              for (size_t sl = 0; sl < ns; ++sl)
                for (int t = 0; t < g.n_shell && !halo[sl]; ++t)
                  {
                    const uint32_t v = g.shell_idx[sl * g.n_shell + t];
                    if (v != INVALID_DOF && is_shared[v])
                      halo[sl] = 1;
                  }
              for (size_t sl = 0; sl < ns; ++sl)
                if (halo[sl])
                  perm.push_back((uint32_t)sl);
              g.n_halo_slots = (uint32_t)perm.size();
              for (size_t sl = 0; sl < ns; ++sl)
                if (!halo[sl])
                  perm.push_back((uint32_t)sl);
              auto permute = [&](auto &v, size_t width) {
                if (v.empty())
                  return;
                auto old = v;
                for (size_t n2 = 0; n2 < ns; ++n2)
                  std::copy(old.begin() + perm[n2] * width, old.begin() + (perm[n2] + 1) * width, v.begin() + n2 * width);
              };
              permute(g.interior_base, 1);
              permute(g.shell_idx, (size_t)g.n_shell);
              permute(g.mask, 1);
              permute(g.fmask, 1);
              permute(g.h, 1);
              permute(g.a, 1);
              permute(g.first_cell, 1);
              std::vector<uint32_t> new_of_old(ns);
              for (size_t n2 = 0; n2 < ns; ++n2)
                new_of_old[perm[n2]] = (uint32_t)n2;
              for (size_t ci = 0; ci < nc; ++ci)
                if (cell_group[ci] == gi)
                  cell_slot[ci] = new_of_old[cell_slot[ci]];
            }
        }
      build_robin_faces();
      build_dirichlet_cells();
    }

    // b += alpha C^T (K_a + s sigma M) C g^  on the free rows, over dirichlet_cells: the core of compute_rhs_dirichlet and of the
    // Gaussian right-hand side.  Host restatement of dirichlet_lift_kernel.  It refuses nothing: its callers do
    void
    dirichlet_lift_add(const double *g, bool include_mass, double alpha, std::vector<double> &b) const
    {
      const int           n = p + 1, n3 = n * n * n;
      std::vector<double> xg(n3), lift(n3);
      for (size_t e = 0; e < dirichlet_cells.size(); ++e)
        {
          const uint32_t *idx = &dirichlet_cells.idx[e * n3];
          for (int t = 0; t < n3; ++t)
            xg[t] = is_dirichlet_index(idx[t]) ? g[idx[t]] : 0.0;
          const uint16_t mask = dirichlet_cells.mask[e];
          const double   ah = dirichlet_cells.scale[2 * e], h = dirichlet_cells.scale[2 * e + 1];
          interpolate_hanging(fe, mask, xg.data(), false);
          cell_stiffness_apply(ah, xg.data(), lift.data());
          if (include_mass && sigma != 0.0)
            cell_mass_add(h, sigma, xg.data(), lift.data());
          interpolate_hanging(fe, mask, lift.data(), true);
          for (int t = 0; t < n3; ++t)
            if (idx[t] < first_constrained())
              b[idx[t]] += alpha * lift[t];
        }
    }

    // dirichlet_cells from the final numbering; nothing without a Dirichlet face
    void
    build_dirichlet_cells()
    {
      if (dirichlet_faces == 0 || n_dirichlet == 0)
        return;
      const int             n = p + 1, n3 = n * n * n;
      std::vector<uint32_t> idx(n3);
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        {
          if (!cell_is_local(ci))
            continue;
          const Cell    &c      = tria->cells[ci];
          const uint16_t mask   = tria->masks[ci];
          const uint32_t ijk[3] = {c.i, c.j, c.k};
          // a cell gathers DoFs of its own nodes and, on hanging entities, of its parent's: only cells that touch a Dirichlet face
          // themselves or through their parent can hold one
          bool near = false;
          for (int lev = c.level; lev >= (int)c.level - ((mask >> MASK_FACE_SHIFT) ? 1 : 0) && lev >= 0; --lev)
            for (int d = 0; d < 3; ++d)
              {
                const uint32_t q = ijk[d] >> (c.level - lev), last = (1u << lev) - 1;
                near |= (q == 0 && ((dirichlet_faces >> (2 * d)) & 1)) || (q == last && ((dirichlet_faces >> (2 * d + 1)) & 1));
              }
          if (!near)
            continue;
          gather_cell(ci, idx.data(), true);
          if (std::none_of(idx.begin(), idx.end(), [&](uint32_t i) { return is_dirichlet_index(i); }))
            continue;
          const double h = 2.0 / (double)(1u << c.level);
          dirichlet_cells.idx.insert(dirichlet_cells.idx.end(), idx.begin(), idx.end());
          dirichlet_cells.mask.push_back(mask);
          dirichlet_cells.scale.push_back(coefficient_of(ci) * h);
          dirichlet_cells.scale.push_back(h);
        }
    }

    // robin_faces from the final numbering; nothing where every beta is 0
    void
    build_robin_faces()
    {
      if (!has_robin())
        return;
      const int n = p + 1;
      for (size_t ci = 0; ci < tria->cells.size(); ++ci)
        {
          if (!cell_is_local(ci))
            continue;
          const Cell    &c      = tria->cells[ci];
          const uint16_t mask   = tria->masks[ci];
          const uint32_t last   = (1u << c.level) - 1;
          const uint32_t ijk[3] = {c.i, c.j, c.k};
          const double   h      = 2.0 / (double)(1u << c.level);
          for (int f = 0; f < 6; ++f)
            {
              const int d = f >> 1, side = f & 1;
              if (!(robin[f] > 0.0) || ijk[d] != (side ? last : 0u))
                continue;
              const int u = d == 0 ? 1 : 0, v = d == 2 ? 1 : 2; // the in-face axes, u < v
              for (int av = 0; av < n; ++av)
                for (int au = 0; au < n; ++au)
                  {
                    int a[3];
                    a[d] = side * p;
                    a[u] = au;
                    a[v] = av;
                    robin_faces.idx.push_back(cell_node_index(ci, a));
                  }
              const bool    hanging = (mask >> MASK_FACE_SHIFT) != 0;
              const int     cu = (mask >> u) & 1, cv = (mask >> v) & 1;
              // interpolate_hanging, pass along u: the line at v = cv p, normal coordinate = the boundary side, is flagged by the
              // hanging face with normal v or the hanging edge along u; likewise along v
              const bool hang_u = hanging && (((mask >> (MASK_FACE_SHIFT + v)) & 1) || ((mask >> (MASK_EDGE_SHIFT + u)) & 1));
              const bool hang_v = hanging && (((mask >> (MASK_FACE_SHIFT + u)) & 1) || ((mask >> (MASK_EDGE_SHIFT + v)) & 1));
              if (hanging && (((mask >> d) & 1) != side || ((mask >> (MASK_FACE_SHIFT + d)) & 1)))
                throw std::runtime_error("convective faces: a boundary cell face with a hanging face of its own");
              robin_faces.flags.push_back((uint8_t)((hang_u ? 1 : 0) | (hang_v ? 2 : 0) | (cu << 2) | (cv << 3)));
              robin_faces.scale.push_back(robin[f] * h * h);
            }
        }
    }
  };
} // namespace mgamd
