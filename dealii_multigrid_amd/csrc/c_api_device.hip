// C ABI, device entry points (include/mgamd.h, section "Device runtime").
#include "runtime.hpp"
#include "kernels_amg.hpp"
#include <cstdio>

using namespace mgamd;

#define REQUIRE(cond)                                    \
  if (!(cond))                                           \
  throw std::invalid_argument("null or invalid argument: " #cond)

extern "C" {

int
mgamd_ctx_create(int device, mgamd_ctx **out)
{
  MGAMD_TRY
  REQUIRE(out);
  auto *c = new mgamd_ctx;
  try
    {
      c->ctx = std::make_unique<Ctx>(device);
    }
  catch (...)
    {
      delete c;
      throw;
    }
  *out = c;
  MGAMD_CATCH
}

int
mgamd_ctx_destroy(mgamd_ctx *ctx)
{
  delete ctx;
  return MGAMD_OK;
}

int
mgamd_ctx_synchronize(mgamd_ctx *ctx)
{
  MGAMD_TRY
  REQUIRE(ctx);
  ctx->ctx->sync();
  MGAMD_CATCH
}

int
mgamd_ctx_stream(mgamd_ctx *ctx, void **stream)
{
  MGAMD_TRY
  REQUIRE(ctx && stream);
  *stream = (void *)ctx->ctx->stream;
  MGAMD_CATCH
}

int
mgamd_vec_create(mgamd_ctx *ctx, uint64_t n, int number_type, mgamd_vec **out)
{
  MGAMD_TRY
  REQUIRE(ctx && out);
  *out = vec_create(ctx->ctx.get(), n, number_type);
  MGAMD_CATCH
}

int
mgamd_vec_destroy(mgamd_vec *v)
{
  delete v;
  return MGAMD_OK;
}

int
mgamd_vec_size(const mgamd_vec *v, uint64_t *n)
{
  MGAMD_TRY
  REQUIRE(v && n);
  *n = v->n;
  MGAMD_CATCH
}

int
mgamd_vec_from_host(mgamd_vec *v, const double *src)
{
  MGAMD_TRY
  REQUIRE(v && src);
  if (v->type == MGAMD_F64)
    HIP_CHECK(hipMemcpyAsync(v->data, src, v->n * 8, hipMemcpyHostToDevice, v->ctx->stream));
  else
    {
      std::vector<float> f(src, src + v->n);
      HIP_CHECK(hipMemcpyAsync(v->data, f.data(), v->n * 4, hipMemcpyHostToDevice, v->ctx->stream));
      v->ctx->sync();
    }
  v->ctx->sync();
  MGAMD_CATCH
}

int
mgamd_vec_to_host(const mgamd_vec *v, double *dst)
{
  MGAMD_TRY
  REQUIRE(v && dst);
  if (v->type == MGAMD_F64)
    {
      HIP_CHECK(hipMemcpyAsync(dst, v->data, v->n * 8, hipMemcpyDeviceToHost, v->ctx->stream));
      v->ctx->sync();
    }
  else
    {
      std::vector<float> f(v->n);
      HIP_CHECK(hipMemcpyAsync(f.data(), v->data, v->n * 4, hipMemcpyDeviceToHost, v->ctx->stream));
      v->ctx->sync();
      for (size_t i = 0; i < v->n; ++i)
        dst[i] = f[i];
    }
  MGAMD_CATCH
}

int
mgamd_vec_set(mgamd_vec *v, double value)
{
  MGAMD_TRY
  REQUIRE(v);
  vec_set(*v, value);
  MGAMD_CATCH
}

int
mgamd_vec_copy(mgamd_vec *dst, const mgamd_vec *src)
{
  MGAMD_TRY
  REQUIRE(dst && src);
  vec_copy(*dst, *src);
  MGAMD_CATCH
}

int
mgamd_vec_axpy(mgamd_vec *y, double a, const mgamd_vec *x)
{
  MGAMD_TRY
  REQUIRE(y && x);
  vec_sadd(*y, 1.0, a, *x);
  MGAMD_CATCH
}

int
mgamd_vec_sadd(mgamd_vec *y, double s, double a, const mgamd_vec *x)
{
  MGAMD_TRY
  REQUIRE(y && x);
  vec_sadd(*y, s, a, *x);
  MGAMD_CATCH
}

int
mgamd_vec_dot(const mgamd_vec *x, const mgamd_vec *y, double *result)
{
  MGAMD_TRY
  REQUIRE(x && y && result);
  *result = vec_dot(*x, *y);
  MGAMD_CATCH
}

int
mgamd_vec_norm2(const mgamd_vec *x, double *result)
{
  MGAMD_TRY
  REQUIRE(x && result);
  *result = std::sqrt(vec_dot(*x, *x));
  MGAMD_CATCH
}

int
mgamd_level_op_create(mgamd_ctx *ctx, const mgamd_dofs *dofs, int number_type, mgamd_level_op **out)
{
  MGAMD_TRY
  REQUIRE(ctx && dofs && out);
  auto *h = new mgamd_level_op;
  try
    {
      h->op.reset(make_level_operator(ctx->ctx.get(), dofs, number_type));
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_level_op_create_distributed(mgamd_ctx *ctx, const mgamd_dofs *dofs, int number_type, mgamd_comm *comm, mgamd_level_op **out)
{
  MGAMD_TRY
  REQUIRE(ctx && dofs && out);
  if (dofs->halo && !comm)
    throw std::invalid_argument("a distributed level needs a communicator");
  auto *h = new mgamd_level_op;
  try
    {
      h->op.reset(make_level_operator(ctx->ctx.get(), dofs, number_type, comm ? comm->comm : nullptr));
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_level_op_dot(mgamd_level_op *op, const mgamd_vec *x, const mgamd_vec *y, double *result)
{
  MGAMD_TRY
  REQUIRE(op && x && y && result);
  *result = op->op->dot(*x, *y);
  MGAMD_CATCH
}

int
mgamd_level_op_n_owned(const mgamd_level_op *op, uint64_t *n)
{
  MGAMD_TRY
  REQUIRE(op && n);
  *n = op->op->comm ? op->op->n_dofs_owned() : op->op->n_dofs();
  MGAMD_CATCH
}

int
mgamd_comm_rccl_unique_id(char id[128])
{
  MGAMD_TRY
  REQUIRE(id);
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId u;
  RcclComm::check(ncclGetUniqueId(&u), "ncclGetUniqueId");
  std::memcpy(id, &u, 128);
  MGAMD_CATCH
}

int
mgamd_comm_rccl_create(mgamd_ctx *ctx, unsigned n_ranks, unsigned rank, const char id[128], mgamd_comm **out)
{
  MGAMD_TRY
  REQUIRE(ctx && id && out && rank < n_ranks);
  HIP_CHECK(hipSetDevice(ctx->ctx->device));
  ncclUniqueId u;
  std::memcpy(&u, id, 128);
  auto *c = new mgamd_comm;
  try
    {
      c->comm = std::make_shared<RcclComm>((int)n_ranks, (int)rank, u);
    }
  catch (...)
    {
      delete c;
      throw;
    }
  *out = c;
  MGAMD_CATCH
}

int
mgamd_sim_group_create(unsigned n_ranks, mgamd_sim_group **out)
{
  MGAMD_TRY
  REQUIRE(out && n_ranks > 0);
  auto *g  = new mgamd_sim_group;
  g->group = std::make_shared<SimGroup>((int)n_ranks);
  *out     = g;
  MGAMD_CATCH
}

int
mgamd_sim_group_destroy(mgamd_sim_group *g)
{
  delete g;
  return MGAMD_OK;
}

int
mgamd_comm_sim_create(mgamd_sim_group *g, unsigned rank, mgamd_comm **out)
{
  MGAMD_TRY
  REQUIRE(g && out && (int)rank < g->group->n);
  auto *c = new mgamd_comm;
  c->comm = std::make_shared<SimComm>(g->group, (int)rank);
  *out    = c;
  MGAMD_CATCH
}

int
mgamd_comm_subset(mgamd_comm *base, unsigned group, mgamd_comm **out)
{
  MGAMD_TRY
  if (!base || !base->comm || !out || group == 0)
    throw std::invalid_argument("bad argument");
  auto *c = new mgamd_comm;
  try
    {
      c->comm = std::make_shared<SubsetComm>(base->comm, (int)group);
    }
  catch (...)
    {
      delete c;
      throw;
    }
  *out = c;
  MGAMD_CATCH
}

int
mgamd_comm_destroy(mgamd_comm *c)
{
  delete c;
  return MGAMD_OK;
}

int
mgamd_comm_allreduce_sum(mgamd_comm *c, mgamd_ctx *ctx, double value, double *result)
{
  MGAMD_TRY
  REQUIRE(c && ctx && result);
  *result = c->comm->allreduce_sum_host(value, ctx->ctx->stream);
  MGAMD_CATCH
}

int
mgamd_level_op_destroy(mgamd_level_op *op)
{
  delete op;
  return MGAMD_OK;
}

int
mgamd_level_op_m(const mgamd_level_op *op, uint64_t *n)
{
  MGAMD_TRY
  REQUIRE(op && n);
  *n = op->op->n_dofs();
  MGAMD_CATCH
}

int
mgamd_level_op_mass_coefficient(const mgamd_level_op *op, double *sigma)
{
  MGAMD_TRY
  REQUIRE(op && sigma);
  *sigma = op->op->sigma;
  MGAMD_CATCH
}

int
mgamd_level_op_init_vector(const mgamd_level_op *op, mgamd_vec **out)
{
  MGAMD_TRY
  REQUIRE(op && out);
  *out = vec_create(op->op->ctx, op->op->n_dofs(), op->op->type);
  MGAMD_CATCH
}

int
mgamd_level_op_vmult(mgamd_level_op *op, mgamd_vec *dst, const mgamd_vec *src)
{
  MGAMD_TRY
  REQUIRE(op && dst && src);
  op->op->vmult(*dst, *src);
  MGAMD_CATCH
}

int
mgamd_level_op_vmult_mass(mgamd_level_op *op, mgamd_vec *dst, const mgamd_vec *src)
{
  MGAMD_TRY
  REQUIRE(op && dst && src);
  op->op->vmult_mass(*dst, *src);
  MGAMD_CATCH
}

int
mgamd_level_op_inverse_diagonal(mgamd_level_op *op, mgamd_vec *diagonal)
{
  MGAMD_TRY
  REQUIRE(op && diagonal);
  if (diagonal->type != op->op->type)
    throw std::invalid_argument("vector number type does not match the operator's");
  op->op->compute_inverse_diagonal(*diagonal);
  MGAMD_CATCH
}

int
mgamd_level_op_rhs(mgamd_level_op *op, mgamd_vec *rhs)
{
  MGAMD_TRY
  REQUIRE(op && rhs);
  op->op->rhs(*rhs);
  MGAMD_CATCH
}

int
mgamd_level_op_rhs_kind(mgamd_level_op *op, int kind, mgamd_vec *rhs)
{
  MGAMD_TRY
  REQUIRE(op && rhs);
  if (kind != 0 && kind != 1)
    throw std::invalid_argument("SimulationType kind must be 0 (Constant) or 1 (Gaussian)");
  op->op->rhs(*rhs, kind);
  MGAMD_CATCH
}

int
mgamd_level_op_rhs_boundary_flux(mgamd_level_op *op, const double q[6], mgamd_vec *rhs)
{
  MGAMD_TRY
  REQUIRE(op && q && rhs);
  op->op->rhs_boundary_flux(*rhs, q);
  MGAMD_CATCH
}

int
mgamd_level_op_distribute(mgamd_level_op *op, int kind, mgamd_vec *x)
{
  MGAMD_TRY
  REQUIRE(op && x);
  if (kind != 0 && kind != 1)
    throw std::invalid_argument("SimulationType kind must be 0 (Constant) or 1 (Gaussian)");
  op->op->distribute(*x, kind);
  MGAMD_CATCH
}

int
mgamd_level_op_rhs_dirichlet(mgamd_level_op *op, const mgamd_vec *g, int include_mass, mgamd_vec *rhs)
{
  MGAMD_TRY
  REQUIRE(op && g && rhs);
  op->op->rhs_dirichlet(*rhs, *g, include_mass != 0);
  MGAMD_CATCH
}

int
mgamd_level_op_distribute_values(mgamd_level_op *op, mgamd_vec *x, const mgamd_vec *g)
{
  MGAMD_TRY
  REQUIRE(op && x && g);
  op->op->distribute_values(*x, *g);
  MGAMD_CATCH
}

int
mgamd_level_op_estimate_error(mgamd_level_op *op, const mgamd_vec *u, const double q[6], double *eta)
{
  MGAMD_TRY
  REQUIRE(op && u);
  op->op->estimate_error(*u, q, eta); // (refuses a null eta by name)
  MGAMD_CATCH
}

int
mgamd_debug_level_op_estimator_info(const mgamd_level_op *op, uint64_t *bytes, double *build_ms, double *kernel_ms)
{
  MGAMD_TRY
  REQUIRE(op);
  uint64_t b  = 0;
  double   t0 = 0.0, t1 = 0.0;
  op->op->estimator_info(b, t0, t1);
  if (bytes)
    *bytes = b;
  if (build_ms)
    *build_ms = t0;
  if (kernel_ms)
    *kernel_ms = t1;
  MGAMD_CATCH
}

int
mgamd_level_op_integrate_difference(mgamd_level_op *op, const mgamd_vec *u, int kind, int n_q, int norm, double *out)
{
  MGAMD_TRY
  REQUIRE(op && u);
  if (kind != 0 && kind != 1)
    throw std::invalid_argument("integrate_difference: unknown kind " + std::to_string(kind) + " (0: w = 0, 1: the Gaussian)");
  op->op->integrate_difference(*u, kind, nullptr, nullptr, n_q, norm, out); // (refuses a null out by name)
  MGAMD_CATCH
}

int
mgamd_level_op_integrate_difference_values(mgamd_level_op *op, const mgamd_vec *u, const mgamd_vec *values, const mgamd_vec *gradients, int n_q,
                                           int norm, double *out)
{
  MGAMD_TRY
  REQUIRE(op && u);
  op->op->integrate_difference(*u, -1, values, gradients, n_q, norm, out); // (refuses missing data by name)
  MGAMD_CATCH
}

int
mgamd_debug_level_op_error_norm_info(const mgamd_level_op *op, uint64_t *bytes, double *kernel_ms, int *neighbours_built)
{
  MGAMD_TRY
  REQUIRE(op);
  uint64_t b  = 0;
  double   t  = 0.0;
  int      nb = 0;
  op->op->error_norm_info(b, t, nb);
  if (bytes)
    *bytes = b;
  if (kernel_ms)
    *kernel_ms = t;
  if (neighbours_built)
    *neighbours_built = nb;
  MGAMD_CATCH
}

int
mgamd_level_op_evaluate(mgamd_level_op *op, const mgamd_vec *u, int n_q, mgamd_vec *values, mgamd_vec *gradients)
{
  MGAMD_TRY
  REQUIRE(op);
  op->op->evaluate(u, n_q, values, gradients); // (refuses a null u and missing outputs by name)
  MGAMD_CATCH
}

int
mgamd_level_op_integrate(mgamd_level_op *op, const mgamd_vec *values, const mgamd_vec *gradients, int n_q, mgamd_vec *b)
{
  MGAMD_TRY
  REQUIRE(op);
  op->op->integrate(values, gradients, n_q, b); // (refuses a null b and missing data by name)
  MGAMD_CATCH
}

int
mgamd_debug_level_op_cell_values_info(const mgamd_level_op *op, uint64_t *bytes, double *evaluate_ms, double *integrate_ms)
{
  MGAMD_TRY
  REQUIRE(op);
  uint64_t b  = 0;
  double   t0 = 0.0, t1 = 0.0;
  op->op->cell_values_info(b, t0, t1);
  if (bytes)
    *bytes = b;
  if (evaluate_ms)
    *evaluate_ms = t0;
  if (integrate_ms)
    *integrate_ms = t1;
  MGAMD_CATCH
}

int
mgamd_level_op_number_type(const mgamd_level_op *op, int *number_type)
{
  MGAMD_TRY
  REQUIRE(op && number_type);
  *number_type = op->op->type;
  MGAMD_CATCH
}

int
mgamd_level_op_point_set_create(mgamd_level_op *op, uint64_t n, const double *xyz, mgamd_point_set **out)
{
  MGAMD_TRY
  if (!op || !out)
    throw std::invalid_argument("point_set: a null pointer (the operator and the result)");
  auto ps = op->op->point_set_create(n, xyz); // (refuses a null xyz, a distributed operator and a local-smoothing level by name)
  *out    = new mgamd_point_set{std::move(ps)};
  MGAMD_CATCH
}

int
mgamd_point_set_destroy(mgamd_point_set *ps)
{
  MGAMD_TRY
  if (ps)
    {
      if (ps->ps->op)
        ps->ps->op->point_set_destroy(ps->ps.get());
      delete ps;
    }
  MGAMD_CATCH
}

int
mgamd_point_set_get(const mgamd_point_set *ps, uint64_t *n, uint64_t *n_found, int32_t *cell, double *ref)
{
  MGAMD_TRY
  if (!ps)
    throw std::invalid_argument("point_set: a null pointer (the point set)");
  if (n)
    *n = ps->ps->n;
  if (n_found)
    *n_found = ps->ps->n_found;
  if (cell || ref)
    ps->ps->get(cell, ref);
  MGAMD_CATCH
}

// the set against the operator the caller names
static void
require_own_operator(const mgamd_point_set *ps, const mgamd_level_op *op, const char *who)
{
  if (!ps || !op)
    throw std::invalid_argument(std::string(who) + ": a null pointer (the point set and its operator)");
  if (ps->ps->op != op->op.get())
    throw std::invalid_argument(std::string(who) + ": the point set belongs to another operator (a set is located on the leaves of the operator "
                                                   "that created it)");
}

int
mgamd_point_set_evaluate(mgamd_point_set *ps, mgamd_level_op *op, const mgamd_vec *u, mgamd_vec *values, mgamd_vec *gradients)
{
  MGAMD_TRY
  require_own_operator(ps, op, "point_evaluate");
  ps->ps->evaluate(u, values, gradients); // (refuses a null u and missing outputs by name)
  MGAMD_CATCH
}

int
mgamd_point_set_integrate(mgamd_point_set *ps, mgamd_level_op *op, const mgamd_vec *values, const mgamd_vec *gradients, mgamd_vec *b)
{
  MGAMD_TRY
  require_own_operator(ps, op, "point_integrate");
  ps->ps->integrate(values, gradients, b); // (refuses a null b and missing data by name)
  MGAMD_CATCH
}

int
mgamd_debug_point_set_info(const mgamd_level_op *op, const mgamd_point_set *ps, uint64_t *operator_bytes, uint64_t *gather_bytes, uint64_t *set_bytes,
                           double *build_ms, double *locate_ms, double *evaluate_ms, double *integrate_ms)
{
  MGAMD_TRY
  REQUIRE(op || ps);
  uint64_t b  = 0;
  double   t[4] = {0.0, 0.0, 0.0, 0.0};
  if (ps)
    ps->ps->info(b, t[0], t[1], t[2], t[3]);
  uint64_t locator = 0, gather = 0;
  if (op)
    op->op->point_tables_bytes(locator, gather);
  if (operator_bytes)
    *operator_bytes = locator;
  if (gather_bytes)
    *gather_bytes = gather;
  if (set_bytes)
    *set_bytes = b;
  double *out[4] = {build_ms, locate_ms, evaluate_ms, integrate_ms};
  for (int k = 0; k < 4; ++k)
    if (out[k])
      *out[k] = t[k];
  MGAMD_CATCH
}

int
mgamd_level_op_debug_stamps(mgamd_level_op *op, unsigned long long *out, uint64_t max_count, uint64_t *count)
{
  MGAMD_TRY
  REQUIRE(op && out && count);
  *count = op->op->read_debug_stamps(out, max_count);
  MGAMD_CATCH
}

int
mgamd_cheb_create(mgamd_level_op *op, unsigned degree, double smoothing_range, unsigned eig_cg_n_iterations, mgamd_cheb **out)
{
  MGAMD_TRY
  REQUIRE(op && out);
  auto *h = new mgamd_cheb;
  try
    {
      h->c.reset(make_chebyshev(op->op.get(), degree, smoothing_range, eig_cg_n_iterations));
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_cheb_destroy(mgamd_cheb *c)
{
  delete c;
  return MGAMD_OK;
}

int
mgamd_cheb_vmult(mgamd_cheb *c, mgamd_vec *dst, const mgamd_vec *src)
{
  MGAMD_TRY
  REQUIRE(c && dst && src);
  c->c->vmult(*dst, *src);
  MGAMD_CATCH
}

int
mgamd_cheb_step(mgamd_cheb *c, mgamd_vec *dst, const mgamd_vec *src)
{
  MGAMD_TRY
  REQUIRE(c && dst && src);
  c->c->step(*dst, *src);
  MGAMD_CATCH
}

int
mgamd_cheb_get_eigen_estimates(const mgamd_cheb *c, double *min_eigenvalue, double *max_eigenvalue)
{
  MGAMD_TRY
  REQUIRE(c);
  if (min_eigenvalue)
    *min_eigenvalue = c->c->min_eig;
  if (max_eigenvalue)
    *max_eigenvalue = c->c->max_eig;
  MGAMD_CATCH
}

int
mgamd_transfer2_create(mgamd_level_op *fine, mgamd_level_op *coarse, mgamd_transfer2 **out)
{
  MGAMD_TRY
  REQUIRE(fine && coarse && out);
  auto *h = new mgamd_transfer2;
  try
    {
      h->t.reset(make_transfer2(fine->op.get(), coarse->op.get()));
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_transfer2_destroy(mgamd_transfer2 *t)
{
  delete t;
  return MGAMD_OK;
}

int
mgamd_transfer2_prolongate_and_add(mgamd_transfer2 *t, mgamd_vec *dst_fine, const mgamd_vec *src_coarse)
{
  MGAMD_TRY
  REQUIRE(t && dst_fine && src_coarse);
  t->t->prolongate_and_add(*dst_fine, *src_coarse);
  MGAMD_CATCH
}

int
mgamd_transfer2_restrict_and_add(mgamd_transfer2 *t, mgamd_vec *dst_coarse, const mgamd_vec *src_fine)
{
  MGAMD_TRY
  REQUIRE(t && dst_coarse && src_fine);
  t->t->restrict_and_add(*dst_coarse, *src_fine);
  MGAMD_CATCH
}

int
mgamd_transfer2_n_fused_bricks(const mgamd_transfer2 *t, uint64_t *n)
{
  MGAMD_TRY
  REQUIRE(t && n);
  *n = t->t->n_fused_bricks_total();
  MGAMD_CATCH
}

int
mgamd_mg_create(mgamd_ctx *ctx, unsigned n_levels, mgamd_level_op *const *levels, mgamd_transfer2 *const *transfers,
                mgamd_cheb *const *smoothers, const char *coarse_solver, mgamd_mg **out)
{
  MGAMD_TRY
  REQUIRE(ctx && levels && out && n_levels > 0 && (n_levels == 1 || (transfers && smoothers)));
  std::vector<LevelOperatorBase *> L(n_levels, nullptr);
  std::vector<Transfer2Base *>     Tr(n_levels, nullptr);
  std::vector<ChebyshevBase *>     Sm(n_levels, nullptr);
  for (unsigned l = 0; l < n_levels; ++l)
    {
      REQUIRE(levels[l]);
      L[l] = levels[l]->op.get();
      if (transfers && transfers[l])
        Tr[l] = transfers[l]->t.get();
      if (smoothers && smoothers[l])
        Sm[l] = smoothers[l]->c.get();
    }
  auto *h = new mgamd_mg;
  try
    {
      h->mg.reset(make_multigrid(ctx->ctx.get(), n_levels, L.data(), Tr.data(), Sm.data(), coarse_solver ? coarse_solver : "direct"));
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_mg_create_nested(mgamd_ctx *ctx, unsigned n_levels, mgamd_level_op *const *levels, mgamd_transfer2 *const *transfers,
                       mgamd_cheb *const *smoothers, const char *coarse_solver, mgamd_mg *coarse_mg, unsigned n_cycles, mgamd_mg **out)
{
  MGAMD_TRY
  REQUIRE(ctx && levels && out && n_levels > 0 && (n_levels == 1 || (transfers && smoothers)));
  std::vector<LevelOperatorBase *> L(n_levels, nullptr);
  std::vector<Transfer2Base *>     Tr(n_levels, nullptr);
  std::vector<ChebyshevBase *>     Sm(n_levels, nullptr);
  for (unsigned l = 0; l < n_levels; ++l)
    {
      REQUIRE(levels[l]);
      L[l] = levels[l]->op.get();
      if (transfers && transfers[l])
        Tr[l] = transfers[l]->t.get();
      if (smoothers && smoothers[l])
        Sm[l] = smoothers[l]->c.get();
    }
  auto *h = new mgamd_mg;
  try
    {
      h->mg.reset(make_multigrid(ctx->ctx.get(), n_levels, L.data(), Tr.data(), Sm.data(), coarse_solver ? coarse_solver : "amg",
                                 coarse_mg ? coarse_mg->mg.get() : nullptr, n_cycles));
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_mg_create_sharded_amg(mgamd_ctx *ctx, unsigned n_levels, mgamd_level_op *const *levels, mgamd_transfer2 *const *transfers,
                            mgamd_cheb *const *smoothers, const char *coarse_solver, const mgamd_dofs *global_coarse_dofs, unsigned n_cycles,
                            uint32_t min_sharded_rows, mgamd_mg **out)
{
  MGAMD_TRY
  REQUIRE(ctx && levels && out && global_coarse_dofs && n_levels > 0 && (n_levels == 1 || (transfers && smoothers)));
  if (global_coarse_dofs->halo)
    throw std::invalid_argument("mgamd_mg_create_sharded_amg: global_coarse_dofs must be the GLOBAL level (mgamd_dofs_create)");
  std::vector<LevelOperatorBase *> L(n_levels, nullptr);
  std::vector<Transfer2Base *>     Tr(n_levels, nullptr);
  std::vector<ChebyshevBase *>     Sm(n_levels, nullptr);
  for (unsigned l = 0; l < n_levels; ++l)
    {
      REQUIRE(levels[l]);
      L[l] = levels[l]->op.get();
      if (transfers && transfers[l])
        Tr[l] = transfers[l]->t.get();
      if (smoothers && smoothers[l])
        Sm[l] = smoothers[l]->c.get();
    }
  auto *h = new mgamd_mg;
  try
    {
      h->mg.reset(make_multigrid(ctx->ctx.get(), n_levels, L.data(), Tr.data(), Sm.data(), coarse_solver ? coarse_solver : "amg", nullptr,
                                 n_cycles, global_coarse_dofs->tables.get(), min_sharded_rows));
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_mg_coarse_iterations(const mgamd_mg *mg, uint64_t *n_iterations)
{
  MGAMD_TRY
  REQUIRE(mg && n_iterations);
  *n_iterations = mg->mg->coarse_cg_iterations();
  MGAMD_CATCH
}

int
mgamd_mg_amg_layout(const mgamd_mg *mg, uint32_t *n_levels, uint32_t *info, uint32_t max_levels)
{
  MGAMD_TRY
  REQUIRE(mg && n_levels);
  std::vector<uint32_t> v;
  mg->mg->amg_layout(v);
  *n_levels = (uint32_t)(v.size() / 5);
  if (info)
    std::copy(v.begin(), v.begin() + 5 * std::min<size_t>(v.size() / 5, max_levels), info);
  MGAMD_CATCH
}

int
mgamd_mg_create_local_smoothing(mgamd_ctx *ctx, unsigned n_levels, mgamd_level_op *const *levels, mgamd_transfer2 *const *transfers,
                                mgamd_cheb *const *smoothers, const mgamd_dofs *active_mesh_dofs, const char *coarse_solver, mgamd_mg **out)
{
  MGAMD_TRY
  REQUIRE(ctx && levels && out && active_mesh_dofs && n_levels > 0 && (n_levels == 1 || (transfers && smoothers)));
  std::vector<LevelOperatorBase *> L(n_levels, nullptr);
  std::vector<Transfer2Base *>     Tr(n_levels, nullptr);
  std::vector<ChebyshevBase *>     Sm(n_levels, nullptr);
  for (unsigned l = 0; l < n_levels; ++l)
    {
      REQUIRE(levels[l]);
      L[l] = levels[l]->op.get();
      if (transfers && transfers[l])
        Tr[l] = transfers[l]->t.get();
      if (smoothers && smoothers[l])
        Sm[l] = smoothers[l]->c.get();
    }
  auto *h = new mgamd_mg;
  try
    {
      h->mg.reset(make_multigrid(ctx->ctx.get(), n_levels, L.data(), Tr.data(), Sm.data(), coarse_solver ? coarse_solver : "amg"));
      h->mg->setup_local_smoothing(*active_mesh_dofs->tables);
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_level_op_exchange_add_tail(mgamd_level_op *op, mgamd_vec *v)
{
  MGAMD_TRY
  REQUIRE(op && v);
  op->op->exchange_add_tail(*v);
  MGAMD_CATCH
}

int
mgamd_level_op_vmult_interface_up(mgamd_level_op *op, mgamd_vec *dst, const mgamd_vec *src)
{
  MGAMD_TRY
  REQUIRE(op && dst && src);
  op->op->vmult_interface_up(*dst, *src);
  MGAMD_CATCH
}

int
mgamd_level_op_vmult_interface_down(mgamd_level_op *op, mgamd_vec *dst, const mgamd_vec *src)
{
  MGAMD_TRY
  REQUIRE(op && dst && src);
  op->op->vmult_interface_down(*dst, *src);
  MGAMD_CATCH
}

int
mgamd_mg_set_collapse(mgamd_mg *mg, int enable, unsigned *collapse_level)
{
  MGAMD_TRY
  REQUIRE(mg);
  const unsigned l = mg->mg->set_collapse(enable != 0);
  if (collapse_level)
    *collapse_level = l;
  MGAMD_CATCH
}

int
mgamd_mg_coarse_solver_used(const mgamd_mg *mg, char name[32])
{
  MGAMD_TRY
  REQUIRE(mg && name);
  std::snprintf(name, 32, "%s", mg->mg->coarse_used.c_str());
  MGAMD_CATCH
}

int
mgamd_mg_destroy(mgamd_mg *mg)
{
  delete mg;
  return MGAMD_OK;
}

int
mgamd_mg_vcycle(mgamd_mg *mg, mgamd_vec *z, const mgamd_vec *r)
{
  MGAMD_TRY
  REQUIRE(mg && z && r);
  mg->mg->vcycle(*z, *r);
  MGAMD_CATCH
}

int
mgamd_mg_set_stage_callback(mgamd_mg *mg, mgamd_stage_callback cb, void *user)
{
  MGAMD_TRY
  REQUIRE(mg);
  mg->mg->cb      = cb;
  mg->mg->cb_user = user;
  MGAMD_CATCH
}

int
mgamd_mg_stage_timing(mgamd_mg *mg, int enable)
{
  MGAMD_TRY
  if (!mg)
    throw std::invalid_argument("null argument");
  mg->mg->set_stage_timing(enable != 0);
  MGAMD_CATCH
}

int
mgamd_mg_stage_times(mgamd_mg *mg, double *ms, unsigned n_levels, uint64_t *n_records)
{
  MGAMD_TRY
  if (!mg || !ms)
    throw std::invalid_argument("null argument");
  if (n_levels != mg->mg->n_levels())
    throw std::invalid_argument("stage_times: ms must hold 9 x n_levels entries");
  const size_t n = mg->mg->read_stage_times(ms);
  if (n_records)
    *n_records = n;
  MGAMD_CATCH
}

int
mgamd_mg_time_vcycles(mgamd_mg *mg, mgamd_vec *z, const mgamd_vec *r, unsigned n, int use_graph, double *ms_per_cycle)
{
  MGAMD_TRY
  REQUIRE(mg && z && r && ms_per_cycle);
  *ms_per_cycle = mg->mg->time_vcycles(*z, *r, n, use_graph != 0);
  MGAMD_CATCH
}

int
mgamd_solve_cg(mgamd_level_op *A, mgamd_mg *preconditioner, mgamd_vec *x, const mgamd_vec *b, double reltol, double abstol,
               unsigned maxiter, unsigned *n_iterations, double *residual_norm)
{
  MGAMD_TRY
  REQUIRE(A && x && b);
  unsigned it  = 0;
  double   res = 0;
  solve_cg(*A->op, preconditioner ? preconditioner->mg.get() : nullptr, *x, *b, reltol, abstol, maxiter, it, res);
  if (n_iterations)
    *n_iterations = it;
  if (residual_norm)
    *residual_norm = res;
  MGAMD_CATCH
}

int
mgamd_time_stepper_create(mgamd_level_op *A, mgamd_mg *preconditioner, double theta, double dt, mgamd_time_stepper **out)
{
  MGAMD_TRY
  REQUIRE(A && out);
  auto ts = std::make_unique<mgamd_time_stepper>();
  ts->ts.reset(make_theta_stepper(*A->op, preconditioner ? preconditioner->mg.get() : nullptr, theta, dt));
  *out = ts.release();
  MGAMD_CATCH
}

int
mgamd_time_stepper_step(mgamd_time_stepper *ts, mgamd_vec *u, const mgamd_vec *f_old, const mgamd_vec *f_new, double reltol, double abstol,
                        unsigned maxiter, unsigned *n_iterations, double *residual_norm)
{
  MGAMD_TRY
  REQUIRE(ts && u);
  unsigned it  = 0;
  double   res = 0;
  ts->ts->step(*u, f_old, f_new, reltol, abstol, maxiter, it, res);
  if (n_iterations)
    *n_iterations = it;
  if (residual_norm)
    *residual_norm = res;
  MGAMD_CATCH
}

int
mgamd_time_stepper_step_data(mgamd_time_stepper *ts, mgamd_vec *u, const mgamd_vec *f_old, const mgamd_vec *f_new, const mgamd_vec *g_old,
                             const mgamd_vec *g_new, const mgamd_vec *load, double reltol, double abstol, unsigned maxiter,
                             unsigned *n_iterations, double *residual_norm)
{
  MGAMD_TRY
  REQUIRE(ts && u);
  unsigned it  = 0;
  double   res = 0;
  ts->ts->step_data(*u, f_old, f_new, g_old, g_new, load, reltol, abstol, maxiter, it, res);
  if (n_iterations)
    *n_iterations = it;
  if (residual_norm)
    *residual_norm = res;
  MGAMD_CATCH
}

int
mgamd_time_stepper_time(const mgamd_time_stepper *ts, double *t, uint64_t *n_steps)
{
  MGAMD_TRY
  REQUIRE(ts);
  if (t)
    *t = ts->ts->t;
  if (n_steps)
    *n_steps = ts->ts->n_steps;
  MGAMD_CATCH
}

void
mgamd_time_stepper_destroy(mgamd_time_stepper *ts)
{
  delete ts;
}

int
mgamd_ctx_kernel_profile(mgamd_ctx *ctx, int enable)
{
  MGAMD_TRY
  REQUIRE(ctx);
  Ctx &c = *ctx->ctx;
  c.harvest_profile();
  c.profile       = enable != 0;
  c.prof_ms_accum = 0;
  c.prof_n_accum  = 0;
  c.prof_bytes    = 0;
  c.prof_bytes_moved = 0;
  MGAMD_CATCH
}

int
mgamd_ctx_kernel_profile_brick(mgamd_ctx *ctx, int brick_size)
{
  MGAMD_TRY
  REQUIRE(ctx);
  ctx->ctx->prof_brick = brick_size;
  MGAMD_CATCH
}

int
mgamd_ctx_kernel_profile_read(mgamd_ctx *ctx, double *total_ms, uint64_t *n_launches, double *algorithmic_bytes)
{
  MGAMD_TRY
  REQUIRE(ctx);
  Ctx &c = *ctx->ctx;
  c.harvest_profile();
  if (total_ms)
    *total_ms = c.prof_ms_accum;
  if (n_launches)
    *n_launches = c.prof_n_accum;
  if (algorithmic_bytes)
    *algorithmic_bytes = c.prof_bytes;
  MGAMD_CATCH
}

int
mgamd_ctx_kernel_profile_bytes_moved(mgamd_ctx *ctx, double *bytes_moved)
{
  MGAMD_TRY
  REQUIRE(ctx);
  REQUIRE(bytes_moved);
  *bytes_moved = ctx->ctx->prof_bytes_moved;
  MGAMD_CATCH
}

} // extern "C"

namespace
{
  template <typename T>
  void
  debug_csr_spmv(Ctx &c, int mode, int lanes, uint32_t n_rows, uint32_t n_cols, const uint32_t *ptr, const uint32_t *col, const double *val,
                 const double *x, double *y, const double *b, const double *xold, bool xold_is_y, const double *dinv, double f1, double f2,
                 int max_blocks, double *dot, int *blocks)
  {
    const size_t nnz = ptr[n_rows];
    auto         dev = [&](DBuf<T> &buf, const double *h, size_t n) -> T * {
      if (!h)
        return nullptr;
      std::vector<T> v(std::max<size_t>(n, 1), T(0));
      std::copy(h, h + n, v.begin());
      buf.upload(v);
      return buf.p;
    };
    DBuf<uint32_t> dptr, dcol;
    dptr.upload(std::vector<uint32_t>(ptr, ptr + n_rows + 1));
    dcol.upload(std::vector<uint32_t>(std::max<size_t>(nnz, 1), 0));
    if (nnz)
      HIP_CHECK(hipMemcpy(dcol.p, col, nnz * sizeof(uint32_t), hipMemcpyHostToDevice));
    DBuf<T> dval, dx, dy, db, dxold, ddinv;
    dev(dval, val, nnz);
    dev(dx, x, n_cols);
    T *yp = dev(dy, y, n_rows);
    const int g = launch_csr_spmv<T>(c.stream, mode, lanes, n_rows, dptr.p, dcol.p, dval.p, dx.p, yp, dev(db, b, n_rows),
                                     xold_is_y ? yp : dev(dxold, xold, n_rows), dev(ddinv, dinv, n_rows), f1, f2,
                                     mode == SPMV_DOT ? c.d_partial : nullptr, max_blocks);
    if (blocks)
      *blocks = g;
    if (mode == SPMV_DOT)
      {
        // as the solver finishes the sum
        hipLaunchKernelGGL(vec_dot_final_kernel<>, 1, 256, 0, c.stream, c.d_partial, g, c.d_result);
        HIP_CHECK(hipMemcpyAsync(c.h_result, c.d_result, sizeof(double), hipMemcpyDeviceToHost, c.stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        if (dot)
          *dot = c.h_result[0];
      }
    std::vector<T> out(std::max<size_t>(n_rows, 1));
    HIP_CHECK(hipMemcpyAsync(out.data(), yp, (size_t)n_rows * sizeof(T), hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    std::copy(out.begin(), out.begin() + n_rows, y);
  }
} // namespace

extern "C" {

int
mgamd_debug_csr_spmv_ex(mgamd_ctx *ctx, int number_type, int mode, int lanes, uint32_t n_rows, uint32_t n_cols, const uint32_t *ptr,
                        const uint32_t *col, const double *val, const double *x, double *y, const double *b, const double *xold,
                        int xold_is_y, const double *dinv, double f1, double f2, int max_blocks, int *lanes_used, int *blocks, double *dot)
{
  MGAMD_TRY
  REQUIRE(ctx && ptr && x && y);
  REQUIRE(number_type == MGAMD_F64 || number_type == MGAMD_F32);
  REQUIRE(mode >= 0 && mode <= 4);
  REQUIRE(lanes == 0 || lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64);
  REQUIRE(number_type == MGAMD_F64 || (mode != 4 && lanes != 64));
  REQUIRE(max_blocks >= 0);
  // every index the kernel follows is checked here, on the host
  REQUIRE(ptr[0] == 0);
  for (uint32_t i = 0; i < n_rows; ++i)
    REQUIRE(ptr[i + 1] >= ptr[i]);
  REQUIRE(ptr[n_rows] == 0 || (col && val));
  for (uint32_t k = 0; k < ptr[n_rows]; ++k)
    REQUIRE(col[k] < n_cols);
  REQUIRE(mode != 2 || b);
  REQUIRE(mode != 3 || (b && dinv && n_cols == n_rows));
  REQUIRE(mode != 4 || n_cols == n_rows);
  REQUIRE(!(xold_is_y && xold));
  if (!lanes)
    lanes = csr_spmv_lanes(n_rows, ptr[n_rows]);
  if (lanes_used)
    *lanes_used = lanes;
  if (blocks)
    *blocks = 0;
  if (dot)
    *dot = 0.0;
  if (number_type == MGAMD_F64)
    debug_csr_spmv<double>(*ctx->ctx, mode, lanes, n_rows, n_cols, ptr, col, val, x, y, b, xold, xold_is_y != 0, dinv, f1, f2, max_blocks, dot,
                           blocks);
  else
    debug_csr_spmv<float>(*ctx->ctx, mode, lanes, n_rows, n_cols, ptr, col, val, x, y, b, xold, xold_is_y != 0, dinv, f1, f2, max_blocks, dot,
                          blocks);
  MGAMD_CATCH
}

int
mgamd_debug_csr_spmv(mgamd_ctx *ctx, int number_type, int mode, int lanes, uint32_t n_rows, uint32_t n_cols, const uint32_t *ptr,
                     const uint32_t *col, const double *val, const double *x, double *y, const double *b, const double *xold, int xold_is_y,
                     const double *dinv, double f1, double f2, int *lanes_used)
{
  return mgamd_debug_csr_spmv_ex(ctx, number_type, mode, lanes, n_rows, n_cols, ptr, col, val, x, y, b, xold, xold_is_y, dinv, f1, f2, 0,
                                 lanes_used, nullptr, nullptr);
}

int
mgamd_debug_csr_spmv_lanes_long(uint32_t n_rows, uint64_t nnz, int *lanes)
{
  MGAMD_TRY
  REQUIRE(lanes);
  *lanes = csr_spmv_lanes_long(n_rows, nnz);
  MGAMD_CATCH
}

// ---- Type "AMG": the assembled matrix, its AMG, CG on the pair (mgamd.h)
int
mgamd_matrix_create(mgamd_ctx *ctx, const mgamd_dofs *dofs, mgamd_matrix **out)
{
  MGAMD_TRY
  REQUIRE(ctx && dofs && out);
  auto *h = new mgamd_matrix;
  try
    {
      h->A = make_assembled_matrix(ctx->ctx.get(), dofs);
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_matrix_destroy(mgamd_matrix *A)
{
  delete A;
  return MGAMD_OK;
}

int
mgamd_matrix_info(const mgamd_matrix *A, uint64_t *n_rows, uint64_t *nnz, int *lanes)
{
  MGAMD_TRY
  REQUIRE(A);
  if (n_rows)
    *n_rows = A->A->n_rows;
  if (nnz)
    *nnz = A->A->nnz;
  if (lanes)
    *lanes = A->A->lanes;
  MGAMD_CATCH
}

int
mgamd_matrix_vmult(mgamd_matrix *A, mgamd_vec *dst, const mgamd_vec *src)
{
  MGAMD_TRY
  REQUIRE(A && dst && src);
  A->A->vmult(*dst, *src);
  MGAMD_CATCH
}

int
mgamd_debug_matrix_time_spmv(mgamd_matrix *A, int mode, int lanes, unsigned reps, double *ms_per_launch)
{
  MGAMD_TRY
  REQUIRE(A && ms_per_launch);
  REQUIRE(mode == 0 || mode == 3 || mode == 4);
  *ms_per_launch = A->A->time_spmv(mode, lanes, reps);
  MGAMD_CATCH
}

int
mgamd_amg_create(mgamd_matrix *A, unsigned n_cycles, mgamd_amg **out)
{
  MGAMD_TRY
  REQUIRE(A && out);
  auto *h = new mgamd_amg;
  try
    {
      h->P.reset(make_amg_preconditioner(A->A, n_cycles));
    }
  catch (...)
    {
      delete h;
      throw;
    }
  *out = h;
  MGAMD_CATCH
}

int
mgamd_amg_destroy(mgamd_amg *P)
{
  delete P;
  return MGAMD_OK;
}

int
mgamd_amg_vmult(mgamd_amg *P, mgamd_vec *z, const mgamd_vec *r)
{
  MGAMD_TRY
  REQUIRE(P && z && r);
  P->P->vmult(*z, *r);
  MGAMD_CATCH
}

int
mgamd_amg_layout(const mgamd_amg *P, uint32_t *n_levels, uint32_t *rows, uint32_t max_levels)
{
  MGAMD_TRY
  REQUIRE(P && n_levels);
  std::vector<uint32_t> v;
  P->P->layout(v);
  *n_levels = (uint32_t)v.size();
  if (rows)
    std::copy(v.begin(), v.begin() + std::min<size_t>(v.size(), max_levels), rows);
  MGAMD_CATCH
}

int
mgamd_solve_cg_matrix(mgamd_matrix *A, mgamd_amg *preconditioner, mgamd_vec *x, const mgamd_vec *b, double reltol, double abstol,
                      unsigned maxiter, unsigned *n_iterations, double *residual_norm)
{
  MGAMD_TRY
  REQUIRE(A && x && b);
  unsigned it  = 0;
  double   res = 0;
  solve_cg_matrix(*A->A, preconditioner ? preconditioner->P.get() : nullptr, *x, *b, reltol, abstol, maxiter, it, res);
  if (n_iterations)
    *n_iterations = it;
  if (residual_norm)
    *residual_norm = res;
  MGAMD_CATCH
}

} // extern "C"
