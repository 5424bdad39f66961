// C ABI, host-side setup entry points (include/mgamd.h, section "Host-side setup").
#include "api_common.hpp"

using namespace mgamd;

namespace mgamd
{
  thread_local std::string g_last_error;
}

struct mgamd_amg_host
{
  AmgHierarchyHost H;
};

struct mgamd_amg_shard
{
  AmgHierarchyHost          H;
  unsigned                  n_sharded = 0;
  std::vector<AmgShardPlan> plans; // one per rank
};

extern "C" {

const char *
mgamd_last_error(void)
{
  return g_last_error.c_str();
}

const char *
mgamd_version(void)
{
  return "mgamd 0.1 (gfx950)";
}

// ---- hierarchy policy (mgamd.h, "Hierarchy policy") ----------------------------------------------------------
int
mgamd_level_plan(const char *type, unsigned n_meshes, unsigned degree, unsigned max_levels, unsigned *n_levels, unsigned *mesh_index,
                 unsigned *degrees, int *local_smoothing)
{
  MGAMD_TRY
  if (!type || !n_levels || !mesh_index || !degrees || !local_smoothing)
    throw std::invalid_argument("null argument");
  if (n_meshes == 0 || degree == 0)
    throw std::invalid_argument("level plan: needs a mesh and a degree >= 1");
  const std::string t = type;
  // create_polynomial_coarsening_sequence(degree, bisect) (ref:multigrid_throughput.cc:1506-1510), lowest degree first
  std::vector<unsigned> pseq{degree};
  while (pseq.back() > 1)
    pseq.push_back(pseq.back() / 2);
  std::reverse(pseq.begin(), pseq.end());
  std::vector<std::pair<unsigned, unsigned>> plan;
  if (t == "HMG-global" || t == "HMG-local")
    for (unsigned l = 0; l < n_meshes; ++l)
      plan.emplace_back(l, degree);
  else if (t == "PMG" || t == "HPMG" || t == "HPMG-local")
    {
      // HPMG: h-levels at the lowest degree first (ref:multigrid_throughput.cc:1518-1519,1551-1553,1569-1571)
      for (unsigned l = 0; t == "HPMG" && l + 1 < n_meshes; ++l)
        plan.emplace_back(l, pseq.front());
      for (const unsigned p : pseq)
        plan.emplace_back(n_meshes - 1, p);
    }
  else
    throw std::runtime_error("Type '" + t + "': not implemented");
  if (plan.size() > max_levels)
    throw std::invalid_argument("level plan: " + std::to_string(plan.size()) + " levels, room for " + std::to_string(max_levels));
  for (size_t l = 0; l < plan.size(); ++l)
    mesh_index[l] = plan[l].first, degrees[l] = plan[l].second;
  *n_levels        = (unsigned)plan.size();
  *local_smoothing = t == "HMG-local";
  MGAMD_CATCH
}

// (the GLOBAL DoF count of level 0: every rank of a sharded run, and a one-rank run of the same problem, decide alike)
int
mgamd_coarse_plan(const char *coarse_name, uint64_t n_level0_dofs_global, int level0_distributed, int sharded_amg_requested, int *plan)
{
  MGAMD_TRY
  if (!coarse_name || !plan)
    throw std::invalid_argument("null argument");
  const std::string c   = coarse_name;
  const bool        amg = is_amg_name(c);
  if (n_level0_dofs_global <= MGAMD_DIRECT_COARSE_MAX_DOFS)
    *plan = MGAMD_COARSE_PLAIN;
  else if (amg && sharded_amg_requested)
    *plan = MGAMD_COARSE_SHARDED_AMG;
  else if (c == "gmg_vcycle" || (amg && level0_distributed)) // the AMG is built from ONE rank's assembled matrix
    *plan = MGAMD_COARSE_NESTED;
  else
    *plan = MGAMD_COARSE_PLAIN;
  MGAMD_CATCH
}

int
mgamd_debug_coarse_resolve(const char *name, uint64_t n_level0_dofs, int level0_sharded, int has_nested, int has_amg_global, char used[32])
{
  MGAMD_TRY
  if (!name || !used)
    throw std::invalid_argument("null argument");
  const char *k = coarse_kind_name(resolve_coarse_kind(name, n_level0_dofs, level0_sharded != 0, has_nested != 0, has_amg_global != 0));
  snprintf(used, 32, "%s", k);
  MGAMD_CATCH
}

int
mgamd_partition_defaults(unsigned n_ranks, unsigned p_low, unsigned *group, uint64_t *min_root_cells, uint64_t *min_sub_root_cells)
{
  MGAMD_TRY
  if (p_low == 0)
    throw std::invalid_argument("partition defaults: degree 0");
  const uint64_t p3 = (uint64_t)p_low * p_low * p_low;
  if (group)
    *group = (n_ranks >= 8 && n_ranks % 4 == 0) ? 4 : ((n_ranks >= 4 && n_ranks % 2 == 0) ? 2 : 1);
  if (min_root_cells)
    *min_root_cells = (uint64_t)4000000 / p3;
  if (min_sub_root_cells)
    *min_sub_root_cells = (uint64_t)1000000 / p3;
  MGAMD_CATCH
}

int
mgamd_tria_create(const char *geometry, unsigned n_ref_global, unsigned n_ref_local, mgamd_tria **out)
{
  MGAMD_TRY
  if (!geometry || !out)
    throw std::invalid_argument("null argument");
  auto *t = new mgamd_tria;
  t->tria = std::make_shared<Tria>(Tria::create(geometry, n_ref_global, n_ref_local));
  *out    = t;
  MGAMD_CATCH
}

int
mgamd_tria_create_from_leaves(uint64_t n_leaves, const uint8_t *level, const uint32_t *i, const uint32_t *j, const uint32_t *k, mgamd_tria **out)
{
  MGAMD_TRY
  if (!level || !i || !j || !k || !out)
    throw std::invalid_argument("null argument");
  std::vector<Cell> leaves(n_leaves);
  for (uint64_t t = 0; t < n_leaves; ++t)
    leaves[t] = Cell{i[t], j[t], k[t], level[t]};
  auto *t = new mgamd_tria;
  try
    {
      t->tria = std::make_shared<Tria>(Tria::from_leaves_checked(std::move(leaves)));
    }
  catch (...)
    {
      delete t;
      throw;
    }
  *out = t;
  MGAMD_CATCH
}

int
mgamd_dofs_matrix(const mgamd_dofs *d, uint64_t *nnz, uint32_t *row_ptr, uint32_t *col, double *val)
{
  MGAMD_TRY
  if (!d || !nnz)
    throw std::invalid_argument("null argument");
  if (d->halo)
    throw std::invalid_argument("mgamd_dofs_matrix: the level is distributed");
  const CSR A = assemble_level_matrix(*d->tables);
  *nnz        = A.nnz();
  if (row_ptr)
    std::copy(A.ptr.begin(), A.ptr.end(), row_ptr);
  if (col)
    std::copy(A.col.begin(), A.col.end(), col);
  if (val)
    std::copy(A.val.begin(), A.val.end(), val);
  MGAMD_CATCH
}

int
mgamd_dofs_set_mass_coefficient(mgamd_dofs *d, double sigma)
{
  MGAMD_TRY
  if (!d)
    throw std::invalid_argument("null argument");
  d->tables->set_mass_coefficient(sigma); // (refuses negative and non-finite values, and non-zero ones on local-smoothing levels)
  MGAMD_CATCH
}

int
mgamd_dofs_mass_coefficient(const mgamd_dofs *d, double *sigma)
{
  MGAMD_TRY
  if (!d || !sigma)
    throw std::invalid_argument("null argument");
  *sigma = d->tables->sigma;
  MGAMD_CATCH
}

int
mgamd_debug_amg_shard_match_rows(const mgamd_dofs *global, const mgamd_dofs *local, uint32_t *rows)
{
  MGAMD_TRY
  if (!global || !local)
    throw std::invalid_argument("null argument");
  const std::vector<uint32_t> r = match_rows_by_key(*global->tables, *local->tables, local->tables->sigma);
  if (rows)
    std::copy(r.begin(), r.end(), rows);
  MGAMD_CATCH
}

int
mgamd_debug_csr_row_pointers(uint32_t n_rows, const uint64_t *row_counts, uint32_t *ptr)
{
  MGAMD_TRY
  if ((n_rows && !row_counts) || !ptr)
    throw std::invalid_argument("null argument");
  const std::vector<uint32_t> p = csr_row_pointers(std::vector<uint64_t>(row_counts, row_counts + n_rows));
  std::copy(p.begin(), p.end(), ptr);
  MGAMD_CATCH
}

int
mgamd_dofs_amg_setup_info(const mgamd_dofs *d, uint32_t *n_levels, uint32_t *rows, uint64_t *nnz, uint32_t max_levels)
{
  MGAMD_TRY
  if (!d || !n_levels)
    throw std::invalid_argument("null argument");
  d->tables->refuse_singular("AMG setup");
  const AmgHierarchyHost H = build_smoothed_aggregation(assemble_level_matrix(*d->tables));
  *n_levels                = (uint32_t)H.levels.size();
  for (uint32_t l = 0; l < H.levels.size() && l < max_levels; ++l)
    {
      if (rows)
        rows[l] = H.levels[l].A.n_rows;
      if (nnz)
        nnz[l] = H.levels[l].A.nnz();
    }
  MGAMD_CATCH
}

int
mgamd_debug_amg_host_create(const mgamd_dofs *d, mgamd_amg_host **out)
{
  MGAMD_TRY
  if (!d || !out)
    throw std::invalid_argument("null argument");
  if (d->halo)
    throw std::invalid_argument("mgamd_debug_amg_host_create: the level is distributed");
  *out = new mgamd_amg_host{build_smoothed_aggregation(assemble_level_matrix(*d->tables))};
  MGAMD_CATCH
}

int
mgamd_debug_amg_host_destroy(mgamd_amg_host *h)
{
  delete h;
  return MGAMD_OK;
}

int
mgamd_debug_amg_host_n_levels(const mgamd_amg_host *h, uint32_t *n_levels)
{
  MGAMD_TRY
  if (!h || !n_levels)
    throw std::invalid_argument("null argument");
  *n_levels = (uint32_t)h->H.levels.size();
  MGAMD_CATCH
}

int
mgamd_debug_amg_host_level_info(const mgamd_amg_host *h, uint32_t level, uint32_t *n_rows, uint64_t *nnz_A, uint32_t *n_cols_P,
                                uint64_t *nnz_P, uint32_t *n_aggregates, double *lambda_max)
{
  MGAMD_TRY
  if (!h)
    throw std::invalid_argument("null argument");
  if (level >= h->H.levels.size())
    throw std::invalid_argument("mgamd_debug_amg_host_level_info: level out of range");
  const AmgLevelHost &L = h->H.levels[level];
  if (n_rows)
    *n_rows = L.A.n_rows;
  if (nnz_A)
    *nnz_A = L.A.nnz();
  if (n_cols_P)
    *n_cols_P = L.P.n_cols;
  if (nnz_P)
    *nnz_P = L.P.nnz();
  if (n_aggregates)
    *n_aggregates = L.n_aggregates;
  if (lambda_max)
    *lambda_max = L.lambda_max;
  MGAMD_CATCH
}

int
mgamd_debug_amg_host_level_get(const mgamd_amg_host *h, uint32_t level, uint32_t *A_ptr, uint32_t *A_col, double *A_val, uint32_t *P_ptr,
                               uint32_t *P_col, double *P_val, int32_t *agg)
{
  MGAMD_TRY
  if (!h)
    throw std::invalid_argument("null argument");
  if (level >= h->H.levels.size())
    throw std::invalid_argument("mgamd_debug_amg_host_level_get: level out of range");
  const AmgLevelHost &L = h->H.levels[level];
  if (A_ptr)
    std::copy(L.A.ptr.begin(), L.A.ptr.end(), A_ptr);
  if (A_col)
    std::copy(L.A.col.begin(), L.A.col.end(), A_col);
  if (A_val)
    std::copy(L.A.val.begin(), L.A.val.end(), A_val);
  if (P_ptr)
    std::copy(L.P.ptr.begin(), L.P.ptr.end(), P_ptr);
  if (P_col)
    std::copy(L.P.col.begin(), L.P.col.end(), P_col);
  if (P_val)
    std::copy(L.P.val.begin(), L.P.val.end(), P_val);
  if (agg)
    std::copy(L.agg.begin(), L.agg.end(), agg);
  MGAMD_CATCH
}

int
mgamd_debug_amg_shard_create(const mgamd_partition *p, unsigned level, int degree, int max_brick, uint32_t min_sharded_rows,
                             mgamd_amg_shard **out)
{
  MGAMD_TRY
  if (!p || !out || level >= p->trias.size())
    throw std::invalid_argument("bad argument");
  if (p->part.subset((int)level) && p->part.group > 1)
    throw std::invalid_argument("sharded AMG: the level is held by groups of ranks (a subset tier of the partition)");
  const int  n_ranks = p->part.n_ranks;
  const bool cut     = n_ranks > 1 && !p->part.replicated((int)level);
  mgamd_tria t{p->trias[level]};
  mgamd_dofs *gd = nullptr;
  if (mgamd_dofs_create(&t, degree, max_brick, &gd) != MGAMD_OK)
    throw std::invalid_argument(g_last_error);
  std::unique_ptr<mgamd_dofs> global(gd);
  auto                        h = std::make_unique<mgamd_amg_shard>();
  h->H                          = build_smoothed_aggregation(assemble_level_matrix(*global->tables));
  const uint32_t n0             = h->H.levels[0].A.n_rows;
  h->n_sharded                  = cut ? amg_n_sharded_levels(h->H, n_ranks, min_sharded_rows) : 0;
  std::vector<uint32_t>              count(n0, cut ? 0 : 1);
  std::vector<int32_t>               owner0(n0, 0);
  std::vector<std::vector<uint32_t>> mirror(n_ranks);
  if (cut)
    for (int r = 0; r < n_ranks; ++r)
      {
        mgamd_dofs *ld = nullptr;
        if (mgamd_dofs_create_local(p, level, (unsigned)r, degree, max_brick, &ld) != MGAMD_OK)
          throw std::runtime_error(g_last_error);
        std::unique_ptr<mgamd_dofs> local(ld);
        const auto                  grow = match_rows_by_key(*global->tables, *local->tables, local->tables->sigma);
        const auto                  own  = local_dof_owned(*local->tables);
        for (uint32_t d = 0; d < local->tables->n_dofs; ++d)
          if (own[d])
            {
              ++count[grow[d]];
              owner0[grow[d]] = r;
            }
          else if (d >= local->tables->first_constrained())
            mirror[r].push_back(grow[d]);
        std::sort(mirror[r].begin(), mirror[r].end());
      }
  check_owned_once(count, "level 0");
  const auto owners = amg_level_owners(h->H, owner0, n_ranks, h->n_sharded);
  for (int r = 0; r < n_ranks; ++r)
    h->plans.push_back(build_amg_shard_plan(h->H, owners, mirror[r], n_ranks, r));
  *out = h.release();
  MGAMD_CATCH
}

int
mgamd_debug_amg_shard_destroy(mgamd_amg_shard *h)
{
  delete h;
  return MGAMD_OK;
}

int
mgamd_debug_amg_shard_n_levels(const mgamd_amg_shard *h, uint32_t *n_levels, uint32_t *n_sharded_levels)
{
  MGAMD_TRY
  if (!h)
    throw std::invalid_argument("null argument");
  if (n_levels)
    *n_levels = (uint32_t)h->H.levels.size();
  if (n_sharded_levels)
    *n_sharded_levels = h->n_sharded;
  MGAMD_CATCH
}

int
mgamd_debug_amg_shard_level_info(const mgamd_amg_shard *h, unsigned rank, uint32_t level, uint32_t info[12])
{
  MGAMD_TRY
  if (!h || !info || rank >= h->plans.size() || level >= h->H.levels.size())
    throw std::invalid_argument("bad argument");
  const AmgShardLevel &L = h->plans[rank].levels[level];
  const uint32_t       v[12] = {L.replicated ? 1u : 0u, L.n_global,          L.n_rows,           L.n_mirror,
                                L.n_interior,           L.n_ghost,           L.n_recv,           (uint32_t)L.peers.size(),
                                (uint32_t)L.A.nnz(),    (uint32_t)L.P.nnz(), (uint32_t)L.R.nnz(), L.R.n_rows};
  std::copy(v, v + 12, info);
  MGAMD_CATCH
}

int
mgamd_debug_amg_shard_level_get(const mgamd_amg_shard *h, unsigned rank, uint32_t level, uint32_t *rows, uint32_t *ghost, int32_t *peers,
                                uint32_t *peer_offset, uint32_t *send_count, uint32_t *recv_count, uint32_t *send_idx, uint32_t *A_ptr,
                                uint32_t *A_col, double *A_val, uint32_t *P_ptr, uint32_t *P_col, double *P_val, uint32_t *R_ptr,
                                uint32_t *R_col, double *R_val)
{
  MGAMD_TRY
  if (!h || rank >= h->plans.size() || level >= h->H.levels.size())
    throw std::invalid_argument("bad argument");
  const AmgShardLevel &L   = h->plans[rank].levels[level];
  auto                 cpy = [](auto *dst, const auto &v) {
    if (dst && !v.empty())
      std::copy(v.begin(), v.end(), dst);
  };
  cpy(rows, L.rows);
  cpy(ghost, L.ghost);
  cpy(peers, L.peers);
  cpy(peer_offset, L.peer_offset);
  cpy(send_count, L.send_count);
  cpy(recv_count, L.recv_count);
  cpy(send_idx, L.send_idx);
  cpy(A_ptr, L.A.ptr);
  cpy(A_col, L.A.col);
  cpy(A_val, L.A.val);
  cpy(P_ptr, L.P.ptr);
  cpy(P_col, L.P.col);
  cpy(P_val, L.P.val);
  cpy(R_ptr, L.R.ptr);
  cpy(R_col, L.R.col);
  cpy(R_val, L.R.val);
  MGAMD_CATCH
}

int
mgamd_tria_coarsen(const mgamd_tria *fine, mgamd_tria **out)
{
  MGAMD_TRY
  if (!fine || !out)
    throw std::invalid_argument("null argument");
  auto *t = new mgamd_tria;
  t->tria = std::make_shared<Tria>(fine->tria->coarsen_global());
  *out    = t;
  MGAMD_CATCH
}

int
mgamd_tria_refine(const mgamd_tria *t, const uint8_t *flags, mgamd_tria **out, uint64_t *parent)
{
  MGAMD_TRY
  if (!t || !out)
    throw std::invalid_argument("null argument");
  std::vector<uint64_t> par;
  auto                  fine = std::make_shared<Tria>(t->tria->refine(flags, parent ? &par : nullptr)); // (refuses null flags, by name)
  if (parent)
    std::copy(par.begin(), par.end(), parent);
  auto *r = new mgamd_tria;
  r->tria = std::move(fine);
  *out    = r;
  MGAMD_CATCH
}

int
mgamd_debug_tria_face_neighbours(const mgamd_tria *t, uint8_t *code, uint32_t *nbr)
{
  MGAMD_TRY
  if (!t)
    throw std::invalid_argument("null argument");
  std::vector<uint8_t>  c;
  std::vector<uint32_t> n;
  t->tria->face_neighbours(c, n);
  if (code)
    std::copy(c.begin(), c.end(), code);
  if (nbr)
    std::copy(n.begin(), n.end(), nbr);
  MGAMD_CATCH
}

int
mgamd_tria_destroy(mgamd_tria *t)
{
  delete t;
  return MGAMD_OK;
}

int
mgamd_tria_info(const mgamd_tria *t, uint64_t *n_cells, uint32_t *n_levels, uint64_t *n_cells_hn)
{
  MGAMD_TRY
  if (!t)
    throw std::invalid_argument("null argument");
  if (n_cells)
    *n_cells = t->tria->n_cells();
  if (n_levels)
    *n_levels = (uint32_t)t->tria->n_levels();
  if (n_cells_hn)
    *n_cells_hn = t->tria->n_cells_with_hanging_nodes();
  MGAMD_CATCH
}

int
mgamd_tria_get_cells(const mgamd_tria *t, uint8_t *level, uint32_t *i, uint32_t *j, uint32_t *k, uint16_t *mask)
{
  MGAMD_TRY
  if (!t)
    throw std::invalid_argument("null argument");
  const auto &c = t->tria->cells;
  for (size_t n = 0; n < c.size(); ++n)
    {
      if (level)
        level[n] = c[n].level;
      if (i)
        i[n] = c[n].i;
      if (j)
        j[n] = c[n].j;
      if (k)
        k[n] = c[n].k;
      if (mask)
        mask[n] = t->tria->masks[n];
    }
  MGAMD_CATCH
}

int
mgamd_tria_set_coefficient(mgamd_tria *t, const double *a)
{
  MGAMD_TRY
  if (!t)
    throw std::invalid_argument("null argument");
  t->tria->set_coefficient(a); // (refuses values that are not finite and > 0, by index)
  MGAMD_CATCH
}

int
mgamd_tria_get_coefficient(const mgamd_tria *t, double *a)
{
  MGAMD_TRY
  if (!t || !a)
    throw std::invalid_argument("null argument");
  for (size_t n = 0; n < t->tria->cells.size(); ++n)
    a[n] = t->tria->coefficient_of(n);
  MGAMD_CATCH
}

int
mgamd_tria_has_coefficient(const mgamd_tria *t, int *has)
{
  MGAMD_TRY
  if (!t || !has)
    throw std::invalid_argument("null argument");
  *has = t->tria->coefficient.empty() ? 0 : 1;
  MGAMD_CATCH
}

int
mgamd_tria_set_dirichlet_faces(mgamd_tria *t, unsigned mask)
{
  MGAMD_TRY
  if (!t)
    throw std::invalid_argument("null argument");
  t->tria->set_dirichlet_faces(mask); // (refuses a mask > 63)
  MGAMD_CATCH
}

int
mgamd_tria_get_dirichlet_faces(const mgamd_tria *t, unsigned *mask)
{
  MGAMD_TRY
  if (!t || !mask)
    throw std::invalid_argument("null argument");
  *mask = t->tria->dirichlet_faces;
  MGAMD_CATCH
}

int
mgamd_dofs_dirichlet_faces(const mgamd_dofs *d, unsigned *mask)
{
  MGAMD_TRY
  if (!d || !mask)
    throw std::invalid_argument("null argument");
  *mask = d->tables->dirichlet_faces;
  MGAMD_CATCH
}

int
mgamd_tria_set_robin_coefficients(mgamd_tria *t, const double beta[6])
{
  MGAMD_TRY
  if (!t || !beta)
    throw std::invalid_argument("null argument");
  t->tria->set_robin_coefficients(beta); // (refuses a negative or non-finite value, and a positive one on a Dirichlet face)
  MGAMD_CATCH
}

int
mgamd_tria_get_robin_coefficients(const mgamd_tria *t, double beta[6])
{
  MGAMD_TRY
  if (!t || !beta)
    throw std::invalid_argument("null argument");
  std::copy(t->tria->robin, t->tria->robin + 6, beta);
  MGAMD_CATCH
}

int
mgamd_dofs_robin_coefficients(const mgamd_dofs *d, double beta[6])
{
  MGAMD_TRY
  if (!d || !beta)
    throw std::invalid_argument("null argument");
  std::copy(d->tables->robin, d->tables->robin + 6, beta);
  MGAMD_CATCH
}

int
mgamd_dofs_robin_faces(const mgamd_dofs *d, uint64_t *n_faces, uint32_t *idx, uint8_t *flags, double *scale)
{
  MGAMD_TRY
  if (!d || !n_faces)
    throw std::invalid_argument("null argument");
  const auto &rf = d->tables->robin_faces;
  *n_faces       = rf.size();
  if (idx)
    std::copy(rf.idx.begin(), rf.idx.end(), idx);
  if (flags)
    std::copy(rf.flags.begin(), rf.flags.end(), flags);
  if (scale)
    std::copy(rf.scale.begin(), rf.scale.end(), scale);
  MGAMD_CATCH
}

int
mgamd_dofs_rhs_boundary_flux(const mgamd_dofs *d, const double q[6], double *out)
{
  MGAMD_TRY
  if (!d || !q || !out)
    throw std::invalid_argument("null argument");
  std::vector<double> b;
  d->tables->compute_rhs_boundary_flux(q, b); // (refuses a flux on a Dirichlet face, by name)
  std::copy(b.begin(), b.end(), out);
  MGAMD_CATCH
}

int
mgamd_dofs_dirichlet_cells(const mgamd_dofs *d, uint64_t *n_cells, uint32_t *idx, uint16_t *mask, double *scale)
{
  MGAMD_TRY
  if (!d || !n_cells)
    throw std::invalid_argument("null argument");
  const auto &dc = d->tables->dirichlet_cells;
  *n_cells       = dc.size();
  if (idx)
    std::copy(dc.idx.begin(), dc.idx.end(), idx);
  if (mask)
    std::copy(dc.mask.begin(), dc.mask.end(), mask);
  if (scale)
    std::copy(dc.scale.begin(), dc.scale.end(), scale);
  MGAMD_CATCH
}

int
mgamd_dofs_rhs_dirichlet(const mgamd_dofs *d, const double *g, int include_mass, double *out)
{
  MGAMD_TRY
  if (!d || !g || !out)
    throw std::invalid_argument("null argument");
  std::vector<double> b;
  d->tables->compute_rhs_dirichlet(g, include_mass != 0, b); // (refuses a convective face next to a Dirichlet face, by name)
  std::copy(b.begin(), b.end(), out);
  MGAMD_CATCH
}

int
mgamd_dofs_distribute_values(const mgamd_dofs *d, const double *g, double *x)
{
  MGAMD_TRY
  if (!d || !g || !x)
    throw std::invalid_argument("null argument");
  std::vector<double> v(x, x + d->tables->n_dofs);
  d->tables->distribute_values(g, v);
  std::copy(v.begin(), v.end(), x);
  MGAMD_CATCH
}

int
mgamd_dofs_dirichlet_face_values(const mgamd_dofs *d, const double v[6], double *g)
{
  MGAMD_TRY
  if (!d || !v || !g)
    throw std::invalid_argument("null argument");
  std::vector<double> h;
  d->tables->dirichlet_face_values(v, h); // (refuses a value on a natural face, by name)
  std::copy(h.begin(), h.end(), g);
  MGAMD_CATCH
}

int
mgamd_dofs_node_positions(const mgamd_dofs *d, double *xyz)
{
  MGAMD_TRY
  if (!d || !xyz)
    throw std::invalid_argument("null argument");
  std::vector<double> h;
  d->tables->export_node_positions(h);
  std::copy(h.begin(), h.end(), xyz);
  MGAMD_CATCH
}

int
mgamd_dofs_quadrature_points(const mgamd_dofs *d, int n_q, double *xyz)
{
  MGAMD_TRY
  if (!d || !xyz)
    throw std::invalid_argument("null argument");
  std::vector<double> h;
  d->tables->quadrature_points(n_q, h); // (refuses n_q, sharded tables and local-smoothing levels by name)
  std::copy(h.begin(), h.end(), xyz);
  MGAMD_CATCH
}

int
mgamd_dofs_integrate(const mgamd_dofs *d, const double *values, const double *gradients, int n_q, double *out)
{
  MGAMD_TRY
  if (!d)
    throw std::invalid_argument("null argument");
  if (!out)
    throw std::invalid_argument("integrate: out is null (n_dofs values)");
  std::vector<double> b;
  d->tables->integrate_values(values, gradients, n_q, b); // (refuses n_q, missing data, sharded tables and local-smoothing levels by name)
  std::copy(b.begin(), b.end(), out);
  MGAMD_CATCH
}

int
mgamd_dofs_evaluate(const mgamd_dofs *d, const double *u, int n_q, double *values, double *gradients)
{
  MGAMD_TRY
  if (!d)
    throw std::invalid_argument("null argument");
  d->tables->evaluate_values(u, n_q, values, gradients); // (refuses a null u, n_q, missing outputs, sharded tables and local-smoothing levels)
  MGAMD_CATCH
}

int
mgamd_dofs_locate_points(const mgamd_dofs *d, uint64_t n, const double *xyz, int32_t *cell, double *ref)
{
  MGAMD_TRY
  if (!d)
    throw std::invalid_argument("null argument");
  d->tables->locate_points(n, xyz, cell, ref); // (refuses null pointers, sharded tables and local-smoothing levels by name)
  MGAMD_CATCH
}

int
mgamd_dofs_point_evaluate(const mgamd_dofs *d, uint64_t n, const double *xyz, const double *u, double *values, double *gradients)
{
  MGAMD_TRY
  if (!d)
    throw std::invalid_argument("null argument");
  d->tables->point_evaluate(n, xyz, u, values, gradients); // (refuses a null u or xyz, missing outputs, sharded tables, local-smoothing levels)
  MGAMD_CATCH
}

int
mgamd_dofs_point_integrate(const mgamd_dofs *d, uint64_t n, const double *xyz, const double *values, const double *gradients, double *out)
{
  MGAMD_TRY
  if (!d)
    throw std::invalid_argument("null argument");
  if (!out)
    throw std::invalid_argument("point_integrate: out is null (n_dofs values)");
  std::vector<double> b;
  d->tables->point_integrate(n, xyz, values, gradients, b); // (refuses a null xyz, missing data, sharded tables and local-smoothing levels by name)
  std::copy(b.begin(), b.end(), out);
  MGAMD_CATCH
}

int
mgamd_dofs_coefficient_range(const mgamd_dofs *d, double *min, double *max)
{
  MGAMD_TRY
  if (!d || !min || !max)
    throw std::invalid_argument("null argument");
  d->tables->coefficient_range(*min, *max);
  MGAMD_CATCH
}

static size_t
n_nonempty_groups(const LevelTables &L)
{
  size_t n = 0;
  for (const auto &g : L.groups)
    n += g.n_slots() > 0;
  return n;
}

int
mgamd_dofs_create(const mgamd_tria *t, int degree, int max_brick, mgamd_dofs **out)
{
  MGAMD_TRY
  if (!t || !out)
    throw std::invalid_argument("null argument");
  if (degree < 1 || degree > MAX_DEGREE)
    throw std::invalid_argument("degree must be in [1," + std::to_string(MAX_DEGREE) + "]");
  auto *d   = new mgamd_dofs;
  d->tria   = t->tria;
  d->tables = std::make_shared<LevelTables>(*d->tria, degree, std::max(max_brick, 0));
  if (max_brick < 0 && is_small_level(d->tria->n_cells(), degree) && n_nonempty_groups(*d->tables) > 1)
    d->tables = std::make_shared<LevelTables>(*d->tria, degree, 1);
  *out      = d;
  MGAMD_CATCH
}

int
mgamd_dofs_destroy(mgamd_dofs *d)
{
  delete d;
  return MGAMD_OK;
}

int
mgamd_dofs_info(const mgamd_dofs *d, mgamd_dofs_info_t *info)
{
  MGAMD_TRY
  if (!d || !info)
    throw std::invalid_argument("null argument");
  const LevelTables &L = *d->tables;
  std::memset(info, 0, sizeof(*info));
  info->degree      = L.p;
  info->n_cells     = L.tria->n_cells();
  info->n_dofs      = L.n_dofs;
  info->n_interior  = L.n_interior;
  info->n_tail      = L.n_tail;
  info->n_dirichlet = L.n_dirichlet;
  info->n_hanging   = L.n_hanging;
  info->n_groups    = (uint32_t)L.groups.size();
  info->n_tail_owned      = L.n_tail_owned;
  info->n_dirichlet_owned = L.n_dirichlet_owned;
  info->n_hanging_owned   = L.n_hanging_owned;
  info->n_peers           = d->halo ? (uint32_t)d->halo->peers.size() : 0;
  info->n_halo_send       = d->halo ? (uint32_t)d->halo->pack_idx.size() : 0;
  info->n_edge            = L.n_edge;
  for (size_t g = 0; g < L.groups.size() && g < 8; ++g)
    {
      info->group_B[g]     = L.groups[g].B;
      info->group_slots[g] = L.groups[g].n_slots();
      info->group_halo_slots[g] = L.groups[g].n_halo_slots;
    }
  MGAMD_CATCH
}

int
mgamd_tria_level_mesh(const mgamd_tria *fine, unsigned level, mgamd_tria **out)
{
  MGAMD_TRY
  if (!fine || !out)
    throw std::invalid_argument("null argument");
  if ((int)level >= fine->tria->n_levels())
    throw std::invalid_argument("level_mesh: the mesh has no cells on that refinement level");
  auto *t = new mgamd_tria;
  t->tria = std::make_shared<Tria>(fine->tria->level_mesh((int)level));
  *out    = t;
  MGAMD_CATCH
}

int
mgamd_dofs_create_level(const mgamd_tria *level_mesh, int degree, int max_brick, mgamd_dofs **out)
{
  MGAMD_TRY
  if (!level_mesh || !out)
    throw std::invalid_argument("null argument");
  if (degree < 1 || degree > MAX_DEGREE)
    throw std::invalid_argument("degree must be in [1," + std::to_string(MAX_DEGREE) + "]");
  auto *d = new mgamd_dofs;
  d->tria = level_mesh->tria;
  try
    {
      d->tables = std::make_shared<LevelTables>(*d->tria, degree, std::max(max_brick, 0), nullptr, false, nullptr, 0, true);
      if (max_brick < 0 && is_small_level(d->tria->n_cells(), degree) && n_nonempty_groups(*d->tables) > 1)
        d->tables = std::make_shared<LevelTables>(*d->tria, degree, 1, nullptr, false, nullptr, 0, true);
    }
  catch (...)
    {
      delete d;
      throw;
    }
  *out = d;
  MGAMD_CATCH
}

int
mgamd_ls_copy_indices(const mgamd_dofs *active_mesh_dofs, const mgamd_dofs *level_dofs, unsigned level, uint64_t *count, uint32_t *global_idx,
                      uint32_t *level_idx)
{
  MGAMD_TRY
  if (!active_mesh_dofs || !level_dofs || !count)
    throw std::invalid_argument("null argument");
  std::vector<uint32_t> g, l;
  ls_copy_indices(*active_mesh_dofs->tables, *level_dofs->tables, (int)level, g, l);
  *count = g.size();
  if (global_idx)
    std::copy(g.begin(), g.end(), global_idx);
  if (level_idx)
    std::copy(l.begin(), l.end(), level_idx);
  MGAMD_CATCH
}

int
mgamd_dofs_get_cell_slots(const mgamd_dofs *d, uint8_t *group, uint32_t *slot)
{
  MGAMD_TRY
  if (!d || !group || !slot)
    throw std::invalid_argument("null argument");
  const LevelTables &L = *d->tables;
  std::copy(L.cell_group.begin(), L.cell_group.end(), group);
  std::copy(L.cell_slot.begin(), L.cell_slot.end(), slot);
  MGAMD_CATCH
}

int
mgamd_dofs_get_keys(const mgamd_dofs *d, int32_t *keys)
{
  MGAMD_TRY
  if (!d || !keys)
    throw std::invalid_argument("null argument");
  std::vector<DofKey> k;
  d->tables->export_dof_keys(k);
  static_assert(sizeof(DofKey) == 5 * sizeof(int32_t), "DofKey layout");
  std::memcpy(keys, k.data(), k.size() * sizeof(DofKey));
  MGAMD_CATCH
}

int
mgamd_dofs_get_cell_dofs(const mgamd_dofs *d, uint32_t *out)
{
  MGAMD_TRY
  if (!d || !out)
    throw std::invalid_argument("null argument");
  std::vector<uint32_t> v;
  d->tables->export_cell_dofs(v);
  std::memcpy(out, v.data(), v.size() * sizeof(uint32_t));
  MGAMD_CATCH
}

int
mgamd_dofs_rhs(const mgamd_dofs *d, int kind, double *out)
{
  MGAMD_TRY
  if (!d || !out)
    throw std::invalid_argument("null argument");
  if (kind != 0 && kind != 1)
    throw std::invalid_argument("SimulationType kind must be 0 (Constant) or 1 (Gaussian)");
  std::vector<double> b;
  d->tables->compute_rhs_function(kind, b);
  std::memcpy(out, b.data(), b.size() * sizeof(double));
  MGAMD_CATCH
}

int
mgamd_dofs_distribute(const mgamd_dofs *d, int kind, double *x)
{
  MGAMD_TRY
  if (!d || !x)
    throw std::invalid_argument("null argument");
  if (kind != 0 && kind != 1)
    throw std::invalid_argument("SimulationType kind must be 0 (Constant) or 1 (Gaussian)");
  std::vector<double> v(x, x + d->tables->n_dofs);
  d->tables->distribute(kind, v);
  std::memcpy(x, v.data(), v.size() * sizeof(double));
  MGAMD_CATCH
}

int
mgamd_dofs_rhs_constant(const mgamd_dofs *d, double *out)
{
  MGAMD_TRY
  if (!d || !out)
    throw std::invalid_argument("null argument");
  std::vector<double> b;
  d->tables->compute_rhs_constant(b);
  std::memcpy(out, b.data(), b.size() * sizeof(double));
  MGAMD_CATCH
}

int
mgamd_partition_create(const mgamd_tria *const *trias, unsigned n_levels, unsigned n_ranks, double hanging_weight, mgamd_partition **out)
{
  return mgamd_partition_create_ex(trias, n_levels, n_ranks, hanging_weight, 0, out);
}

int
mgamd_partition_create_ex(const mgamd_tria *const *trias, unsigned n_levels, unsigned n_ranks, double hanging_weight,
                          uint64_t min_root_cells, mgamd_partition **out)
{
  return mgamd_partition_create_tiered(trias, n_levels, n_ranks, hanging_weight, min_root_cells, 1, 0, out);
}

int
mgamd_partition_create_tiered(const mgamd_tria *const *trias, unsigned n_levels, unsigned n_ranks, double hanging_weight,
                              uint64_t min_root_cells, unsigned group, uint64_t min_sub_root_cells, mgamd_partition **out)
{
  MGAMD_TRY
  if (!trias || !out || n_levels == 0 || n_ranks == 0 || group == 0)
    throw std::invalid_argument("bad argument");
  auto                     *p = new mgamd_partition;
  std::vector<const Tria *> raw;
  for (unsigned l = 0; l < n_levels; ++l)
    {
      if (!trias[l])
        throw std::invalid_argument("null triangulation");
      p->trias.push_back(trias[l]->tria);
      raw.push_back(trias[l]->tria.get());
    }
  try
    {
      p->part = make_partition(raw, (int)n_ranks, hanging_weight, 32, (size_t)min_root_cells, (int)group, (size_t)min_sub_root_cells);
    }
  catch (...)
    {
      delete p;
      throw;
    }
  *out = p;
  MGAMD_CATCH
}

int
mgamd_partition_destroy(mgamd_partition *p)
{
  delete p;
  return MGAMD_OK;
}

int
mgamd_partition_info(const mgamd_partition *p, unsigned *root_level, unsigned *n_ranks)
{
  MGAMD_TRY
  if (!p)
    throw std::invalid_argument("null argument");
  if (root_level)
    *root_level = (unsigned)p->part.root_level;
  if (n_ranks)
    *n_ranks = (unsigned)p->part.n_ranks;
  MGAMD_CATCH
}

int
mgamd_partition_tiers(const mgamd_partition *p, unsigned *sub_root_level, unsigned *group)
{
  MGAMD_TRY
  if (!p)
    throw std::invalid_argument("null argument");
  if (sub_root_level)
    *sub_root_level = (unsigned)p->part.sub_root_level;
  if (group)
    *group = (unsigned)p->part.group;
  MGAMD_CATCH
}

int
mgamd_partition_statistics(const mgamd_partition *p, double stats[5])
{
  MGAMD_TRY
  if (!p || !stats)
    throw std::invalid_argument("null argument");
  std::vector<const Tria *> trias;
  for (const auto &t : p->trias)
    trias.push_back(t.get());
  const PartitionStatistics st = partition_statistics(trias, p->part);
  stats[0] = st.workload_eff;
  stats[1] = st.workload_path_max;
  stats[2] = st.vertical_eff;
  stats[3] = st.horizontal_eff;
  stats[4] = st.mem_total;
  MGAMD_CATCH
}

int
mgamd_partition_get_owner(const mgamd_partition *p, unsigned level, uint16_t *owner)
{
  MGAMD_TRY
  if (!p || !owner || level >= p->trias.size() || (int)level < p->part.sub_root_level)
    throw std::invalid_argument("bad argument");
  const auto &o = p->part.level_owner((int)level);
  std::memcpy(owner, o.data(), o.size() * sizeof(uint16_t));
  MGAMD_CATCH
}

int
mgamd_dofs_create_local(const mgamd_partition *p, unsigned level, unsigned rank, int degree, int max_brick, mgamd_dofs **out)
{
  MGAMD_TRY
  if (!p || !out || level >= p->trias.size() || (int)rank >= p->part.n_ranks)
    throw std::invalid_argument("bad argument");
  if (degree < 1 || degree > MAX_DEGREE)
    throw std::invalid_argument("degree must be in [1," + std::to_string(MAX_DEGREE) + "]");
  auto *d    = new mgamd_dofs;
  d->tria    = p->trias[level];
  // the level's pieces and the one this rank works on (subset levels: parts, shared by the ranks of a group)
  const int np = p->part.n_parts((int)level), my = p->part.part_of((int)level, (int)rank);
  d->n_ranks   = np;
  d->rank      = my;
  try
    {
      if (p->part.replicated((int)level) || p->part.n_ranks == 1)
        {
          d->tables = std::make_shared<LevelTables>(*d->tria, degree, std::max(max_brick, 0));
          if (max_brick < 0 && is_small_level(d->tria->n_cells(), degree) && n_nonempty_groups(*d->tables) > 1)
            d->tables = std::make_shared<LevelTables>(*d->tria, degree, 1);
        }
      else
        {
          const auto &owner = p->part.level_owner((int)level);
          d->owned          = std::make_shared<std::vector<uint8_t>>(owner.size());
          for (size_t c = 0; c < owner.size(); ++c)
            (*d->owned)[c] = owner[c] == my;
          d->shared = std::make_shared<std::map<uint64_t, SharedInfo>>(shared_keys(*d->tria, owner, np, my, degree));
          d->tables = std::make_shared<LevelTables>(*d->tria, degree, std::max(max_brick, 0), d->owned.get(), false, d->shared.get(), my);
          if (max_brick < 0 && is_small_level(d->tria->n_cells() / np, degree) && n_nonempty_groups(*d->tables) > 1)
            d->tables = std::make_shared<LevelTables>(*d->tria, degree, 1, d->owned.get(), false, d->shared.get(), my);
          d->halo   = std::make_shared<HaloPlan>(make_halo_plan(*d->tables, *d->shared, np, my));
        }
    }
  catch (...)
    {
      delete d;
      throw;
    }
  *out = d;
  MGAMD_CATCH
}

int
mgamd_dofs_halo_sizes(const mgamd_dofs *d, uint32_t sizes[4])
{
  MGAMD_TRY
  if (!d || !sizes)
    throw std::invalid_argument("null argument");
  sizes[0] = sizes[1] = sizes[2] = sizes[3] = 0;
  if (d->halo)
    {
      sizes[0] = (uint32_t)d->halo->peers.size();
      sizes[1] = (uint32_t)d->halo->pack_idx.size();
      sizes[2] = (uint32_t)d->halo->sh_tail.size();
      sizes[3] = (uint32_t)d->halo->sh_src.size();
    }
  MGAMD_CATCH
}

int
mgamd_dofs_halo_get(const mgamd_dofs *d, int32_t *peers, uint32_t *peer_offset, uint32_t *pack_idx, uint32_t *sh_tail, uint32_t *sh_ptr,
                    int32_t *sh_src, int32_t *sh_owner_src)
{
  MGAMD_TRY
  if (!d || !d->halo)
    throw std::invalid_argument("not a distributed level");
  const HaloPlan &H   = *d->halo;
  auto            cpy = [](auto *dst, const auto &v) {
    if (dst && !v.empty())
      std::memcpy(dst, v.data(), v.size() * sizeof(v[0]));
  };
  cpy(peers, H.peers);
  cpy(peer_offset, H.peer_offset);
  cpy(pack_idx, H.pack_idx);
  cpy(sh_tail, H.sh_tail);
  cpy(sh_ptr, H.sh_ptr);
  cpy(sh_src, H.sh_src);
  cpy(sh_owner_src, H.sh_owner_src);
  MGAMD_CATCH
}

int
mgamd_transfer_tables_info(const mgamd_dofs *fine, const mgamd_dofs *coarse, uint64_t n_patches[3], uint32_t nf[3])
{
  MGAMD_TRY
  if (!fine || !coarse)
    throw std::invalid_argument("null argument");
  TransferTables T(*fine->tables, *coarse->tables);
  for (int k = 0; k < 3; ++k)
    {
      if (n_patches)
        n_patches[k] = T.groups[k].n_patches();
      if (nf)
        nf[k] = T.groups[k].nf;
    }
  MGAMD_CATCH
}

int
mgamd_transfer_tables_get(const mgamd_dofs *fine, const mgamd_dofs *coarse, int kind, uint32_t *coarse_idx, uint16_t *coarse_mask,
                          uint32_t *fine_idx)
{
  MGAMD_TRY
  if (!fine || !coarse || kind < 0 || kind > 2)
    throw std::invalid_argument("bad argument");
  TransferTables       T(*fine->tables, *coarse->tables);
  const TransferGroup &g = T.groups[kind];
  if (coarse_idx)
    std::memcpy(coarse_idx, g.coarse_idx.data(), g.coarse_idx.size() * sizeof(uint32_t));
  if (coarse_mask)
    std::memcpy(coarse_mask, g.coarse_mask.data(), g.coarse_mask.size() * sizeof(uint16_t));
  if (fine_idx)
    std::memcpy(fine_idx, g.fine_idx.data(), g.fine_idx.size() * sizeof(uint32_t));
  MGAMD_CATCH
}

} // extern "C"
