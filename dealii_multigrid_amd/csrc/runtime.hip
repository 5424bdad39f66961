// Device runtime implementation (see runtime.hpp).  Compiled with hipcc --offload-arch=gfx950.
#include "runtime.hpp"
#include "level_operator.hpp"
#include "amg.hpp"
#include "amg_shard.hpp"

#include <chrono>
#include <cmath>
#include <mutex>
#include <set>
#include <unordered_map>
#include <cstring>
#include <type_traits>

namespace mgamd
{
  // ------------------------------------------------------------------------------------------
  // Context
  // ------------------------------------------------------------------------------------------
  Ctx::Ctx(int dev)
    : device(dev)
  {
    int        count = 0;
    hipError_t e     = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
      throw NoDeviceError("no HIP device available: this library has no CPU fallback");
    if (dev < 0 || dev >= count)
      throw std::invalid_argument("device index out of range");
    HIP_CHECK(hipSetDevice(dev));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
      throw NoDeviceError(std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    sync_events.resize(64);
    for (hipEvent_t &e : sync_events)
      HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_CHECK(hipMalloc((void **)&d_partial, 1024 * sizeof(double)));
    HIP_CHECK(hipMalloc((void **)&d_result, 8 * sizeof(double)));
    HIP_CHECK(hipMalloc((void **)&d_cg, 8 * sizeof(double)));
    HIP_CHECK(hipHostMalloc((void **)&h_result, 8 * sizeof(double)));
  }

  Ctx::~Ctx()
  {
    (void)hipStreamSynchronize(stream);
    (void)hipStreamSynchronize(side);
    for (hipEvent_t e : sync_events)
      (void)hipEventDestroy(e);
    (void)hipStreamDestroy(side);
    for (auto &p : prof_events)
      {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
      }
    (void)hipFree(d_partial);
    (void)hipFree(d_result);
    (void)hipFree(d_cg);
    (void)hipHostFree(h_result);
    (void)hipStreamDestroy(stream);
  }

  void
  Ctx::harvest_profile()
  {
    sync();
    for (size_t i = 0; i < prof_used; ++i)
      {
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, prof_events[i].first, prof_events[i].second));
        prof_ms_accum += ms;
      }
    prof_n_accum += prof_used;
    prof_used = 0;
  }

} // namespace mgamd

mgamd_vec::~mgamd_vec()
{
  if (data)
    (void)hipFree(data);
}

namespace mgamd
{
  mgamd_vec *
  vec_create(Ctx *ctx, size_t n, int type)
  {
    if (type != MGAMD_F64 && type != MGAMD_F32)
      throw std::invalid_argument("number_type must be MGAMD_F64 or MGAMD_F32");
    auto v  = std::make_unique<mgamd_vec>();
    v->ctx  = ctx;
    v->n    = n;
    v->type = type;
    if (n)
      {
        HIP_CHECK(hipMalloc(&v->data, n * (size_t)type));
        HIP_CHECK(hipMemsetAsync(v->data, 0, n * (size_t)type, ctx->stream));
      }
    return v.release();
  }

  void
  vec_set(mgamd_vec &v, double value)
  {
    if (!v.n)
      return;
    if (v.type == MGAMD_F64)
      hipLaunchKernelGGL(vec_set_kernel<double>, grid_for(v.n), 256, 0, v.ctx->stream, v.as<double>(), value, v.n);
    else
      hipLaunchKernelGGL(vec_set_kernel<float>, grid_for(v.n), 256, 0, v.ctx->stream, v.as<float>(), (float)value, v.n);
  }

  void
  vec_copy(mgamd_vec &d, const mgamd_vec &s)
  {
    if (d.n != s.n)
      throw std::invalid_argument("vector size mismatch");
    if (!d.n)
      return;
    const int    g  = grid_for(d.n);
    hipStream_t  st = d.ctx->stream;
    if (d.type == MGAMD_F64 && s.type == MGAMD_F64)
      HIP_CHECK(hipMemcpyAsync(d.data, s.data, d.n * 8, hipMemcpyDeviceToDevice, st));
    else if (d.type == MGAMD_F32 && s.type == MGAMD_F32)
      HIP_CHECK(hipMemcpyAsync(d.data, s.data, d.n * 4, hipMemcpyDeviceToDevice, st));
    else if (d.type == MGAMD_F32)
      hipLaunchKernelGGL((vec_copy_kernel<float, double>), g, 256, 0, st, d.as<float>(), s.as<double>(), d.n);
    else
      hipLaunchKernelGGL((vec_copy_kernel<double, float>), g, 256, 0, st, d.as<double>(), s.as<float>(), d.n);
  }

  void
  vec_sadd(mgamd_vec &y, double s, double a, const mgamd_vec &x)
  {
    if (y.n != x.n || y.type != x.type)
      throw std::invalid_argument("vector mismatch");
    if (!y.n)
      return;
    if (y.type == MGAMD_F64)
      hipLaunchKernelGGL(vec_sadd_kernel<double>, grid_for(y.n), 256, 0, y.ctx->stream, y.as<double>(), s, a, x.as<double>(), y.n);
    else
      hipLaunchKernelGGL(vec_sadd_kernel<float>, grid_for(y.n), 256, 0, y.ctx->stream, y.as<float>(), (float)s, (float)a, x.as<float>(),
                         y.n);
  }


  // S[slot] = x . y over the first n entries, summed over the ranks of `comm` (stream-ordered, no host synchronisation)
  template <typename T>
  static void
  dot_to_device(Ctx *ctx, Comm *comm, double *S, const T *x, const T *y, size_t n, int slot)
  {
    int g = std::min(grid_for(std::max<size_t>(n, 1)), 1024);
    hipLaunchKernelGGL(cg_dot_kernel<T>, g, 256, 0, ctx->stream, x, y, n, ctx->d_partial);
    hipLaunchKernelGGL(vec_dot_final_kernel<>, 1, 256, 0, ctx->stream, ctx->d_partial, g, S + slot);
    if (comm)
      comm->allreduce_sum(S + slot, 1, MGAMD_F64, ctx->stream);
  }
  static double
  read_scalar(Ctx *ctx, const double *S, int slot)
  {
    HIP_CHECK(hipMemcpyAsync(ctx->h_result, S + slot, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    return ctx->h_result[0];
  }

  // Device-resident preconditioned CG from x = 0 (SolverCG + ReductionControl: ref:multigrid_throughput.cc:1143-1144,
  // 888-895).  vmult(Ap, p) and precond(z, r) enqueue work on the stream; r holds b on entry.  n_dot: entries counted by
  // the inner products (the owned prefix on a sharded level, all otherwise).  One host read-back per iteration (the
  // residual norm); alpha, beta and the three inner products never leave the device: they live in S (8 doubles, one array per
  // solver instance -- the coarse CG of a V-cycle runs INSIDE the outer CG's preconditioner).
  // vmult_dot (optional): Ap = A p and S[2] = p . Ap in one pass over the matrix (the assembled operator's SPMV_DOT launch), in
  // place of vmult and the inner product after it
  template <typename T, typename VMULT, typename PRECOND>
  static void
  device_pcg(Ctx *ctx, Comm *comm, double *S, size_t n, size_t n_dot, T *x, T *r, T *z, T *p, T *Ap, VMULT vmult, PRECOND precond, double reltol,
             double abstol, unsigned maxiter, unsigned &n_iterations, double &residual,
             const std::function<void(T *, const T *, double *)> &vmult_dot = nullptr)
  {
    const int g  = grid_for(n);
    const int gd = std::min(g, 1024);
    HIP_CHECK(hipMemsetAsync(x, 0, n * sizeof(T), ctx->stream));
    dot_to_device(ctx, comm, S, r, r, n_dot, 3);
    double       res  = std::sqrt(read_scalar(ctx, S, 3));
    const double res0 = res;
    n_iterations      = 0;
    residual          = res;
    if (res <= abstol)
      return;
    precond(z, r);
    HIP_CHECK(hipMemcpyAsync(p, z, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    int cur = 0; // S[cur] = r.z
    dot_to_device(ctx, comm, S, r, z, n_dot, cur);
    for (unsigned it = 1; it <= maxiter; ++it)
      {
        if (vmult_dot)
          vmult_dot(Ap, p, S + 2);
        else
          {
            vmult(Ap, p);
            dot_to_device(ctx, comm, S, p, Ap, n_dot, 2);
          }
        hipLaunchKernelGGL(cg_update_xr_kernel<T>, gd, 256, 0, ctx->stream, x, r, p, Ap, n, n_dot, S, cur, ctx->d_partial);
        hipLaunchKernelGGL(vec_dot_final_kernel<>, 1, 256, 0, ctx->stream, ctx->d_partial, gd, S + 3);
        if (comm)
          comm->allreduce_sum(S + 3, 1, MGAMD_F64, ctx->stream);
        res          = std::sqrt(read_scalar(ctx, S, 3));
        n_iterations = it;
        residual     = res;
        if (res < reltol * res0 || res <= abstol)
          break;
        precond(z, r);
        dot_to_device(ctx, comm, S, r, z, n_dot, 1 - cur);
        hipLaunchKernelGGL(cg_update_p_kernel<T>, g, 256, 0, ctx->stream, p, z, n, S, 1 - cur, cur);
        cur = 1 - cur;
      }
    HIP_CHECK(hipGetLastError());
  }

  double
  vec_dot(const mgamd_vec &x, const mgamd_vec &y)
  {
    if (x.n != y.n || x.type != y.type)
      throw std::invalid_argument("vector mismatch");
    return x.type == MGAMD_F64 ? dot_raw(x.ctx, x.as<double>(), y.as<double>(), x.n) : dot_raw(x.ctx, x.as<float>(), y.as<float>(), x.n);
  }

  // host values -> a device vector of either number type, on the stream; returns when they have arrived
  static void
  upload(Ctx *ctx, mgamd_vec &v, const std::vector<double> &h)
  {
    std::vector<float> f;
    if (v.type == MGAMD_F32)
      f.assign(h.begin(), h.end());
    const void *src = v.type == MGAMD_F32 ? (const void *)f.data() : (const void *)h.data();
    HIP_CHECK(hipMemcpyAsync(v.data, src, h.size() * (size_t)v.type, hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();
  }

  // the built-in Dirichlet values of `kind` as caller data: computed on the host, uploaded once, distributed by the kernels of
  // distribute_values behind whatever the stream holds for x
  void
  LevelOperatorBase::distribute(mgamd_vec &x, int kind)
  {
    if (x.n != n_dofs())
      throw std::invalid_argument("distribute: vector size mismatch");
    std::vector<double> g;
    tables->dirichlet_kind_values(kind, g);
    std::unique_ptr<mgamd_vec> gd(vec_create(ctx, x.n, x.type));
    upload(ctx, *gd, g);
    distribute_values_core(x, *gd);
    ctx->sync(); // gd is freed on return
  }

  void
  LevelOperatorBase::rhs(mgamd_vec &b, int kind)
  {
    if (b.n != n_dofs())
      throw std::invalid_argument("rhs: vector size mismatch");
    std::vector<double> h;
    tables->compute_rhs_function(kind, h);
    upload_load(b, h);
  }

  void
  LevelOperatorBase::rhs_boundary_flux(mgamd_vec &b, const double q[6])
  {
    if (b.n != n_dofs())
      throw std::invalid_argument("rhs_boundary_flux: vector size mismatch");
    std::vector<double> h;
    tables->compute_rhs_boundary_flux(q, h);
    upload_load(b, h);
  }

  // a load vector assembled over this rank's cells -> b, then the other ranks' contributions to shared DoFs
  void
  LevelOperatorBase::upload_load(mgamd_vec &b, const std::vector<double> &h)
  {
    upload(ctx, b, h);
    exchange_add_tail(b); // contributions of the other ranks' cells to shared DoFs
    ctx->sync();
  }

  LevelOperatorBase *
  make_level_operator(Ctx *ctx, const mgamd_dofs *dofs, int type, std::shared_ptr<Comm> comm)
  {
    if (type == MGAMD_F64)
      return new LevelOperator<double>(ctx, dofs, comm);
    if (type == MGAMD_F32)
      return new LevelOperator<float>(ctx, dofs, comm);
    throw std::invalid_argument("number_type must be MGAMD_F64 or MGAMD_F32");
  }

  // ------------------------------------------------------------------------------------------
  // Chebyshev smoother (deal.II PreconditionChebyshev; parameters ref:multigrid_throughput.cc:312-315,867-883)
  // ------------------------------------------------------------------------------------------
  static double
  lanczos_max_eigenvalue(const std::vector<double> &alpha, const std::vector<double> &beta, double *min_ev)
  {
    // symmetric tridiagonal T from the CG coefficients; eigenvalues by implicit QL (tqli, no vectors)
    const int           n = (int)alpha.size();
    std::vector<double> d(n), e(n, 0.0);
    for (int j = 0; j < n; ++j)
      {
        d[j] = 1.0 / alpha[j] + (j > 0 ? beta[j - 1] / alpha[j - 1] : 0.0);
        if (j + 1 < n)
          e[j] = std::sqrt(beta[j]) / alpha[j];
      }
    for (int l = 0; l < n; ++l)
      {
        int iter = 0, m;
        do
          {
            for (m = l; m < n - 1; ++m)
              {
                const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
                if (std::fabs(e[m]) <= 1e-300 + 2.3e-16 * dd)
                  break;
              }
            if (m != l)
              {
                if (iter++ == 200)
                  throw std::runtime_error("tridiagonal eigenvalue iteration did not converge");
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = std::hypot(g, 1.0);
                g        = d[m] - d[l] + e[l] / (g + (g >= 0 ? std::fabs(r) : -std::fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int    i;
                for (i = m - 1; i >= l; --i)
                  {
                    double f = s * e[i], b = c * e[i];
                    e[i + 1] = (r = std::hypot(f, g));
                    if (r == 0.0)
                      {
                        d[i + 1] -= p;
                        e[m] = 0.0;
                        break;
                      }
                    s        = f / r;
                    c        = g / r;
                    g        = d[i + 1] - p;
                    r        = (d[i] - g) * s + 2.0 * c * b;
                    d[i + 1] = g + (p = s * r);
                    g        = c * r - b;
                  }
                if (r == 0.0 && i >= l)
                  continue;
                d[l] -= p;
                e[l] = g;
                e[m] = 0.0;
              }
          }
        while (m != l);
      }
    double mx = d[0], mn = d[0];
    for (double v : d)
      {
        mx = std::max(mx, v);
        mn = std::min(mn, v);
      }
    if (min_ev)
      *min_ev = mn;
    return mx;
  }

  template <typename T>
  struct Chebyshev : ChebyshevBase
  {
    LevelOperator<T> *lop;
    DBuf<T>           dinv, tmp;

    Chebyshev(LevelOperator<T> *o, unsigned deg, double smoothing_range, unsigned eig_cg_n_iterations)
      : lop(o)
    {
      op     = o;
      degree = deg;
      Ctx         *ctx = o->ctx;
      const size_t n   = o->n_dofs();
      dinv.alloc(n);
      tmp.alloc(n);
      {
        // DiagonalMatrix preconditioner (ref:multigrid_throughput.cc:872-875)
        mgamd_vec dv;
        dv.ctx  = ctx;
        dv.n    = n;
        dv.type = (int)sizeof(T);
        dv.data = dinv.p;
        try
          {
            o->compute_inverse_diagonal(dv);
          }
        catch (...)
          {
            dv.data = nullptr;
            throw;
          }
        dv.data = nullptr;
      }
      o->build_dinv_codes(dinv.p);
      estimate_eigenvalues(smoothing_range, eig_cg_n_iterations);
    }

    void
    estimate_eigenvalues(double smoothing_range, unsigned n_it)
    {
      Ctx         *ctx = lop->ctx;
      const size_t n   = lop->n_dofs();
      // initial guess (deal.II set_initial_guess): v_i = (i mod 11) - mean
      std::vector<T> v(n);
      const char    *key_init = getenv("MGAMD_CHEB_KEY_INIT"); // tests: numbering-independent start vector on one rank too
      if (!lop->comm && !(key_init && atoi(key_init)))
        {
          double sum = 0;
          for (size_t i = 0; i < n; ++i)
            sum += (double)(i % 11);
          const T mean = (T)(sum / (double)n);
          for (size_t i = 0; i < n; ++i)
            v[i] = (T)(i % 11) - mean;
        }
      else
        {
          // sharded: there is no global index; use a numbering-independent value per DoF (a hash of its geometric
          // key, identical on every sharing rank), zero on constrained DoFs so that every entry is counted once
          std::vector<DofKey> keys;
          lop->tables->export_dof_keys(keys);
          // (one rank, by MGAMD_CHEB_KEY_INIT: every unconstrained DoF is owned; n_dot() there counts the constrained rows too)
          const size_t nf = (size_t)lop->tables->n_interior + lop->tables->n_tail, nown = lop->comm ? lop->n_dot() : nf;
          double       sum = 0;
          for (size_t i = 0; i < n; ++i)
            {
              const uint64_t hk = FlatMap::mix(pack_key((uint32_t)keys[i].px, (uint32_t)keys[i].py, (uint32_t)keys[i].pz, keys[i].dirmask, keys[i].level));
              v[i]              = i < nf ? (T)(hk % 11) : T(0);
              if (i < nown)
                sum += (double)v[i];
            }
          const double gsum = lop->comm ? lop->comm->allreduce_sum_host(sum, ctx->stream) : sum;
          const double gcnt = lop->comm ? lop->comm->allreduce_sum_host((double)nown, ctx->stream) : (double)nown;
          const T      mean = (T)(gsum / gcnt);
          for (size_t i = 0; i < nf; ++i)
            v[i] -= mean;
        }
      DBuf<T> r, z, d, Ad;
      r.upload(v);
      z.alloc(n);
      d.alloc(n);
      Ad.alloc(n);
      std::vector<double> alphas, betas;
      const int           g    = grid_for(n);
      auto                dot_raw = [&](Ctx *, const T *a, const T *b, size_t) { return lop->dot_raw_global(a, b); };
      double              res0 = std::sqrt(dot_raw(ctx, r.p, r.p, n));
      if (res0 > 0 && n_it > 0)
        {
          // z = D^-1 r ; d = z
          hipLaunchKernelGGL(vec_scaled_product_kernel<T>, g, 256, 0, ctx->stream, z.p, T(1), dinv.p, r.p, n);
          HIP_CHECK(hipMemcpyAsync(d.p, z.p, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
          double rz = dot_raw(ctx, r.p, z.p, n);
          for (unsigned it = 0; it < n_it; ++it)
            {
              lop->vmult_raw(Ad.p, d.p);
              const double dAd = dot_raw(ctx, d.p, Ad.p, n);
              if (!(dAd > 0))
                break;
              const double alpha = rz / dAd;
              hipLaunchKernelGGL(vec_sadd_kernel<T>, g, 256, 0, ctx->stream, r.p, T(1), T(-alpha), Ad.p, n);
              alphas.push_back(alpha);
              const double res = std::sqrt(dot_raw(ctx, r.p, r.p, n));
              if (res <= 1e-10)
                break;
              hipLaunchKernelGGL(vec_scaled_product_kernel<T>, g, 256, 0, ctx->stream, z.p, T(1), dinv.p, r.p, n);
              const double rz_new = dot_raw(ctx, r.p, z.p, n);
              const double beta   = rz_new / rz;
              betas.push_back(beta);
              rz = rz_new;
              hipLaunchKernelGGL(vec_sadd_kernel<T>, g, 256, 0, ctx->stream, d.p, T(beta), T(1), z.p, n);
            }
        }
      if (!alphas.empty())
        {
          betas.resize(alphas.size(), 0.0);
          max_eig = lanczos_max_eigenvalue(alphas, betas, &min_eig);
        }
      else
        min_eig = max_eig = 1.0;
      max_eig *= 1.2; // safety factor, the CG is not converged
      const double a = smoothing_range > 1.0 ? max_eig / smoothing_range : std::min(0.9 * max_eig, min_eig);
      delta          = 0.5 * (max_eig - a);
      theta          = 0.5 * (max_eig + a);
      ctx->sync();
    }

    // zero initial guess; result guaranteed in S; Tb is scratch of the same size
    void
    vmult_raw(T *S, T *Tb, const T *b)
    {
      Ctx         *ctx = lop->ctx;
      const size_t n   = lop->n_dofs();
      T           *cur = (degree % 2 == 1) ? S : Tb;
      T           *oth = (cur == S) ? Tb : S;
      // x_1 = D^-1 b / theta is only materialised when it is the result; the first operator pass computes it on the
      // fly from b and D^-1 (which it reads anyway) and the second one uses it as x_old the same way
      const bool passes = degree >= 2 && std::fabs(delta) >= 1e-40;
      if (!passes)
        hipLaunchKernelGGL(vec_scaled_product_kernel<T>, grid_for(n), 256, 0, ctx->stream, cur, T(1.0 / theta), dinv.p, b, n);
      if (passes)
        {
          double rhok = delta / theta, sigma = theta / delta;
          for (unsigned j = 0; j + 1 < degree; ++j)
            {
              const double rhokp = 1.0 / (2.0 * sigma - rhok);
              const double f1 = rhokp * rhok, f2 = 2.0 * rhokp / delta;
              rhok = rhokp;
              if (j < 2)
                lop->cheb_raw(oth, j == 0 ? nullptr : cur, nullptr, b, dinv.p, f1, f2, (int)j + 1, 1.0 / theta);
              else
                lop->cheb_raw(oth, cur, oth, b, dinv.p, f1, f2);
              std::swap(cur, oth);
            }
        }
      if (cur != S)
        hipLaunchKernelGGL((vec_copy_kernel<T, T>), grid_for(n), 256, 0, ctx->stream, S, cur, n);
    }

    // general initial guess x0 in X; O is scratch; returns the buffer holding the result.  prolongate != nullptr: the initial
    // guess is X + P x_c with the prolongation fused into the first operator pass (X becomes X + P x_c on the way)
    T *
    step_raw(T *X, T *O, const T *b, const FusedTransferHost<T> *prolongate = nullptr, double *out_wide = nullptr)
    {
      // out_wide (float levels): the result is wanted there as doubles; nullptr is returned.  With a plain Chebyshev pass at the end
      // (degree >= 2) that pass stores the doubles itself, otherwise a cast follows
      const bool wide_in_pass = out_wide && degree >= 2 && std::fabs(delta) >= 1e-40 && sizeof(T) == 4;
      T *cur = X, *oth = O;
      if (prolongate)
        lop->cheb_prolongate_raw(oth, cur, b, dinv.p, 1.0 / theta, *prolongate);
      else
        lop->cheb_raw(oth, cur, nullptr, b, dinv.p, 0.0, 1.0 / theta);
      std::swap(cur, oth);
      if (degree >= 2 && std::fabs(delta) >= 1e-40)
        {
          double rhok = delta / theta, sigma = theta / delta;
          for (unsigned j = 0; j + 1 < degree; ++j)
            {
              const double rhokp = 1.0 / (2.0 * sigma - rhok);
              const double f1 = rhokp * rhok, f2 = 2.0 * rhokp / delta;
              rhok = rhokp;
              const bool last = j + 2 == degree;
              lop->cheb_raw(oth, cur, oth, b, dinv.p, f1, f2, 0, 0.0, (last && wide_in_pass) ? out_wide : nullptr);
              std::swap(cur, oth);
            }
        }
      if (out_wide && !wide_in_pass)
        hipLaunchKernelGGL((vec_copy_kernel<double, T>), grid_for(lop->n_dofs()), 256, 0, lop->ctx->stream, out_wide, cur, lop->n_dofs());
      return out_wide ? nullptr : cur;
    }

    void
    vmult(mgamd_vec &dst, const mgamd_vec &src) override
    {
      if (dst.n != lop->n_dofs() || src.n != lop->n_dofs() || dst.data == src.data)
        throw std::invalid_argument("PreconditionChebyshev::vmult: bad vectors");
      vmult_raw(dst.as<T>(), tmp.p, src.as<T>());
    }
    void
    step(mgamd_vec &dst, const mgamd_vec &src) override
    {
      if (dst.n != lop->n_dofs() || src.n != lop->n_dofs() || dst.data == src.data)
        throw std::invalid_argument("PreconditionChebyshev::step: bad vectors");
      T *res = step_raw(dst.as<T>(), tmp.p, src.as<T>());
      if (res != dst.as<T>())
        hipLaunchKernelGGL((vec_copy_kernel<T, T>), grid_for(dst.n), 256, 0, lop->ctx->stream, dst.as<T>(), res, dst.n);
    }
  };

  ChebyshevBase *
  make_chebyshev(LevelOperatorBase *op, unsigned degree, double smoothing_range, unsigned eig_cg_n_iterations)
  {
    if (degree < 1)
      throw std::invalid_argument("SmootherDegree must be >= 1");
    if (op->type == MGAMD_F64)
      return new Chebyshev<double>(static_cast<LevelOperator<double> *>(op), degree, smoothing_range, eig_cg_n_iterations);
    return new Chebyshev<float>(static_cast<LevelOperator<float> *>(op), degree, smoothing_range, eig_cg_n_iterations);
  }

  // ------------------------------------------------------------------------------------------
  // Two-level transfer
  // ------------------------------------------------------------------------------------------
  template <typename T>
  struct Transfer2 : Transfer2Base
  {
    struct GroupD
    {
      int                 kind = 0, nf = 2;
      size_t              n_patches = 0;
      DBuf<uint32_t>      coarse_idx, fine_idx, fine_idx_restrict; // restrict list: copies of other ranks' DoFs removed
      DBuf<uint16_t>      coarse_mask;
      std::vector<double> E;
      // p = 1 h-patches: tables of the register kernels (patch_p1_*_kernel)
      DBuf<uint32_t> p1_uniq_ptr, p1_uniq_idx, p1_fine_t, p1_fine_t_restrict;
      DBuf<uint16_t> p1_loc;
      uint32_t       p1_max_uniq = 0;
      void
      build_p1(const std::vector<uint32_t> &cidx, const std::vector<uint32_t> &fidx, const std::vector<uint32_t> *fidx_restrict)
      {
        const size_t          np = n_patches, nwg = (np + PATCH_P1_BLOCK - 1) / PATCH_P1_BLOCK;
        std::vector<uint32_t> ptr(nwg + 1, 0), idx, tmp;
        std::vector<uint16_t> l(np * 8, 0xFFFFu);
        for (size_t w = 0; w < nwg; ++w)
          {
            const size_t a = w * PATCH_P1_BLOCK, b = std::min(np, a + PATCH_P1_BLOCK);
            tmp.clear();
            for (size_t i = a * 8; i < b * 8; ++i)
              if (cidx[i] != INVALID_DOF)
                tmp.push_back(cidx[i]);
            std::sort(tmp.begin(), tmp.end());
            tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
            for (size_t i = a * 8; i < b * 8; ++i)
              if (cidx[i] != INVALID_DOF)
                l[i] = (uint16_t)(std::lower_bound(tmp.begin(), tmp.end(), cidx[i]) - tmp.begin());
            idx.insert(idx.end(), tmp.begin(), tmp.end());
            ptr[w + 1]  = (uint32_t)idx.size();
            p1_max_uniq = std::max<uint32_t>(p1_max_uniq, (uint32_t)tmp.size());
          }
        if (idx.empty())
          idx.push_back(0);
        auto transpose = [&](const std::vector<uint32_t> &f) {
          std::vector<uint32_t> t(f.size());
          for (size_t q = 0; q < np; ++q)
            for (int k = 0; k < 27; ++k)
              t[(size_t)k * np + q] = f[q * 27 + k];
          return t;
        };
        p1_uniq_ptr.upload(ptr);
        p1_uniq_idx.upload(idx);
        p1_loc.upload(l);
        p1_fine_t.upload(transpose(fidx));
        if (fidx_restrict)
          p1_fine_t_restrict.upload(transpose(*fidx_restrict));
      }
    };
    struct BrickD
    {
      int            B = 2, fine_group = 0;
      size_t         n_bricks = 0;
      size_t         n_unfused = 0; // fused group: the bricks [n_unfused, n_bricks) are transferred inside the operator passes
      bool           fused = false;
      DBuf<uint32_t> slot, coarse_idx, own_shell, own_shell_restrict;
    };
    // Transfers fused into the fine level's operator passes (kernels.hpp MODE_RESIDUAL_RESTRICT / MODE_CHEB_PROLONGATE): tables by
    // SLOT of the fused group.  MGAMD_NO_FUSED_TRANSFER=1 disables them (development A/B; same results up to rounding).
    FusedTransferHost<T> fused;
    DBuf<uint32_t>       fused_flags;
    DBuf<uint32_t>       fused_coarse_idx;
    DBuf<uint8_t>        fused_tail_flags;
    DBuf<uint32_t>       fused_tail_chunks;
    size_t               n_fused_bricks = 0;
    bool
    fused_ready() const
    {
      return fused.group >= 0 && n_fused_bricks > 0;
    }
    uint64_t
    n_fused_bricks_total() const override
    {
      return fused_ready() ? n_fused_bricks : 0;
    }
    GroupD                               grp[3];
    std::vector<std::unique_ptr<BrickD>> bricks;
    LevelOperator<T>                    *fop = nullptr, *cop = nullptr;
    int                                  pc = 1, pf = 1;
    Ctx                                 *ctx = nullptr;
    FE1D                                 fec;

    Transfer2(LevelOperator<T> *f, LevelOperator<T> *c)
      : fec(c->tables->p)
    {
      fine   = f;
      coarse = c;
      fop    = f;
      cop    = c;
      ctx    = f->ctx;
      // the fine group whose bricks carry the fused transfers: the plain 17-point lattices of an h-transfer (persistent
      // workgroups); not on local-smoothing levels (edge rows, partial coverage)
      // nor on a fine level with a convective face: the fused bricks restrict and prolongate tail rows that never pass through the
      // accumulator, where the face kernel adds its term (DESIGN.md "Convective faces": the known cost of such levels)
      int fuse_group = -1;
      if (!getenv("MGAMD_NO_FUSED_TRANSFER") && !f->tables->has_robin() && f->tables->tria != c->tables->tria && f->tables->p == c->tables->p &&
          !f->tables->ls_level && !c->tables->ls_level && fused_transfer_supported(f->tables->p))
        for (size_t gi = 0; gi < f->tables->groups.size(); ++gi)
          {
            const SlotGroup &g = f->tables->groups[gi];
            if (persistent_lattice(g.N) && !g.constrained_group && g.n_slots() > 0)
              fuse_group = (int)gi;
          }
      TransferTables tt(*f->tables, *c->tables, true, fuse_group);
      // sharded fine level: a residual entry that is a copy of another rank's DoF is restricted by its owner only
      const uint32_t copy_lo = f->tables->n_interior + f->tables->n_tail_owned, copy_hi = f->tables->n_interior + f->tables->n_tail;
      auto           owned_only = [&](std::vector<uint32_t> v) {
        for (uint32_t &i : v)
          if (i != INVALID_DOF && i >= copy_lo && i < copy_hi)
            i = INVALID_DOF;
        return v;
      };
      for (const BrickTransferGroup &bg : tt.bricks)
        {
          auto d        = std::make_unique<BrickD>();
          d->B          = bg.B;
          d->fine_group = bg.fine_group;
          d->n_bricks   = bg.n_bricks();
          d->n_unfused  = bg.fused ? bg.n_unfused : bg.n_bricks();
          d->fused      = bg.fused;
          if (bg.fused && bg.n_bricks() > bg.n_unfused)
            {
              const SlotGroup &fg  = f->tables->groups[bg.fine_group];
              const size_t     ns  = fg.n_slots(), nsh = (size_t)fg.n_shell, nc3 = (size_t)bg.Nc * bg.Nc * bg.Nc;
              if (2 * ((nsh + 255) / 256) > 15)
                throw std::runtime_error("fused transfer: shell too large for the flag word");
              std::vector<uint32_t> fl(ns * 256, 0);
              std::vector<uint32_t> ci(ns * nc3, INVALID_DOF);
              for (size_t q = bg.n_unfused; q < bg.n_bricks(); ++q)
                {
                  const size_t sl = bg.slot[q];
                  for (size_t t = 0; t < 256; ++t)
                    fl[sl * 256 + t] = 0x8000u;
                  for (size_t t = 0; t < nsh; ++t)
                    fl[sl * 256 + t % 256] |= (uint32_t)(bg.shell_flags[q * nsh + t] & 3u) << (2 * (t / 256));
                  std::copy(bg.coarse_idx.begin() + q * nc3, bg.coarse_idx.begin() + (q + 1) * nc3, ci.begin() + sl * nc3);
                  for (size_t t = 0; t < nc3; ++t)
                    if (bg.coarse_idx[q * nc3 + t] == INVALID_DOF)
                      fl[sl * 256 + t % 256] |= 1u << (16 + t / 256);
                }
              fused_flags.upload(fl);
              fused_coarse_idx.upload(ci);
              fused_tail_flags.upload(tt.tail_owned_by_fused);
              fused.group      = bg.fine_group;
              fused.flags      = fused_flags.p;
              fused.coarse_idx = fused_coarse_idx.p;
              fused.nc3        = (uint32_t)nc3;
              fused.E          = fec.embedding(1, f->tables->p);
              fused.tail_flags = fused_tail_flags.p;
              n_fused_bricks   = bg.n_bricks() - bg.n_unfused;
              // the rows of the fused residual pass's tail epilogue (apply_P); a sharded level keeps the whole tail
              if (!f->halo && !f->tables->n_edge)
                {
                  std::vector<uint32_t> runs = tt.residual_tail_runs, chunks;
                  if (f->tables->n_dofs > f->tables->n_interior + f->tables->n_tail) // the constrained rows
                    {
                      runs.push_back(f->tables->n_tail);
                      runs.push_back(f->tables->n_dofs - f->tables->n_interior);
                    }
                  for (size_t k = 0; k + 1 < runs.size(); k += 2)
                    for (uint32_t b0 = runs[k]; b0 < runs[k + 1]; b0 += TAIL_CHUNK)
                      {
                        chunks.push_back(b0);
                        chunks.push_back(std::min(runs[k + 1], b0 + TAIL_CHUNK));
                      }
                  fused.n_tail_chunks = (uint32_t)(chunks.size() / 2);
                  if (chunks.empty())
                    chunks.push_back(0);
                  fused_tail_chunks.upload(chunks);
                  fused.tail_chunks = fused_tail_chunks.p;
                }
            }
          d->slot.upload(bg.slot);
          d->coarse_idx.upload(bg.coarse_idx);
          d->own_shell.upload(bg.own_shell);
          if (copy_hi > copy_lo)
            d->own_shell_restrict.upload(owned_only(bg.own_shell));
          bricks.push_back(std::move(d));
        }
      pc = tt.pc;
      pf = tt.pf;
      for (int k = 0; k < 3; ++k)
        {
          grp[k].kind      = k;
          grp[k].nf        = tt.groups[k].nf;
          grp[k].n_patches = tt.groups[k].n_patches();
          if (grp[k].n_patches)
            {
              grp[k].coarse_idx.upload(tt.groups[k].coarse_idx);
              grp[k].coarse_mask.upload(tt.groups[k].coarse_mask);
              grp[k].fine_idx.upload(tt.groups[k].fine_idx);
              if (copy_hi > copy_lo)
                grp[k].fine_idx_restrict.upload(owned_only(tt.groups[k].fine_idx));
              if (k == 1 && tt.pc == 1 && grp[k].nf == 3)
                {
                  if (copy_hi > copy_lo)
                    {
                      const std::vector<uint32_t> fr = owned_only(tt.groups[k].fine_idx);
                      grp[k].build_p1(tt.groups[k].coarse_idx, tt.groups[k].fine_idx, &fr);
                    }
                  else
                    grp[k].build_p1(tt.groups[k].coarse_idx, tt.groups[k].fine_idx, nullptr);
                }
            }
          grp[k].E = fec.embedding(k, pf);
        }
    }

    template <int PC, int NF, bool IDENTITY>
    void
    launch(const GroupD &g, const T *src, T *dst, bool prolongate)
    {
      using G = TransferGeo<PC, NF>;
      TransferArgs<T, PC, NF> a;
      a.coarse_idx  = g.coarse_idx.p;
      a.coarse_mask = g.coarse_mask.p;
      a.fine_idx    = (!prolongate && g.fine_idx_restrict.p) ? g.fine_idx_restrict.p : g.fine_idx.p;
      a.n_patches   = (uint32_t)g.n_patches;
      const int n   = PC + 1;
      for (int i = 0; i < n * n; ++i)
        {
          a.m.M[i] = a.m.K[i] = 0.0;
          a.m.I0[i]           = fec.I[0][i];
          a.m.I1[i]           = fec.I[1][i];
        }
      if ((int)g.E.size() != NF * n)
        throw std::runtime_error("transfer: embedding size mismatch");
      for (int i = 0; i < NF * n; ++i)
        a.E[i] = g.E[i];
      a.src            = src;
      a.dst            = dst;
      const size_t lds = 2 * (size_t)G::SPW * G::NF3 * sizeof(T);
      const int    grid = (int)((g.n_patches + G::SPW - 1) / G::SPW);
      // (two 15-point patch lattices of p = 7 are 54 KB in double: through launch_lds like every launch with large dynamic LDS)
      if (prolongate)
        launch_lds(ctx, ctx->stream, prolongate_kernel<T, PC, NF, IDENTITY>, grid, G::BLOCK, lds, a);
      else
        launch_lds(ctx, ctx->stream, restrict_kernel<T, PC, NF, IDENTITY>, grid, G::BLOCK, lds, a);
      HIP_CHECK(hipGetLastError());
    }

    void
    launch_p1(const GroupD &g, const T *src, T *dst, bool prolongate)
    {
      PatchP1Args<T> a;
      a.uniq_ptr    = g.p1_uniq_ptr.p;
      a.uniq_idx    = g.p1_uniq_idx.p;
      a.loc         = g.p1_loc.p;
      a.coarse_mask = g.coarse_mask.p;
      a.fine_idx_t  = (!prolongate && g.p1_fine_t_restrict.p) ? g.p1_fine_t_restrict.p : g.p1_fine_t.p;
      a.n_patches   = (uint32_t)g.n_patches;
      a.max_uniq    = g.p1_max_uniq;
      for (int i = 0; i < 4; ++i)
        {
          a.m.M[i] = a.m.K[i] = 0.0;
          a.m.I0[i]           = fec.I[0][i];
          a.m.I1[i]           = fec.I[1][i];
        }
      a.src = src;
      a.dst = dst;
      const int    grid = (int)((g.n_patches + PATCH_P1_BLOCK - 1) / PATCH_P1_BLOCK);
      const size_t lds  = (size_t)std::max<uint32_t>(g.p1_max_uniq, 1) * sizeof(T);
      if (prolongate)
        hipLaunchKernelGGL(patch_p1_prolongate_kernel<T>, grid, PATCH_P1_BLOCK, lds, ctx->stream, a);
      else
        hipLaunchKernelGGL(patch_p1_restrict_kernel<T>, grid, PATCH_P1_BLOCK, lds, ctx->stream, a);
      HIP_CHECK(hipGetLastError());
    }

    // the first n_launch bricks of the group (all of them, or the un-fused ones of a fused group)
    template <int P, int B>
    void
    launch_brick(const BrickD &b, const T *src, T *dst, bool prolongate, size_t n_launch)
    {
      if (n_launch == 0)
        return;
      using G = BrickTransferGeo<P, B>;
      BrickTransferArgs<T, P> a;
      const GroupDev<T>      &fg = *fop->groups[b.fine_group];
      a.slot          = b.slot.p;
      a.interior_base = fg.interior_base.p;
      a.shell_pos     = fg.shell_pos.p;
      a.coarse_idx    = b.coarse_idx.p;
      a.own_shell     = (!prolongate && b.own_shell_restrict.p) ? b.own_shell_restrict.p : b.own_shell.p;
      a.n_bricks      = (uint32_t)n_launch;
      const std::vector<double> E = fec.embedding(1, P);
      for (int i = 0; i < (2 * P + 1) * (P + 1); ++i)
        a.E[i] = E[i];
      a.src            = src;
      a.dst            = dst;
      const size_t lds = (size_t)G::LDS * sizeof(T);
      if (prolongate)
        launch_lds(ctx, ctx->stream, brick_prolongate_kernel<T, P, B>, (int)n_launch, G::BLOCK, lds, a);
      else if constexpr (persistent_lattice(G::NF))
        // persistent workgroups, three per CU (<= 168 VGPRs) (kernels.hpp)
        launch_persistent(ctx, ctx->stream, brick_restrict_persistent_kernel<T, P, B>, (int)n_launch, 3, G::BLOCK, lds, a);
      else
        launch_lds(ctx, ctx->stream, brick_restrict_kernel<T, P, B>, (int)n_launch, G::BLOCK, lds, a);
      HIP_CHECK(hipGetLastError());
    }

    // skip_fused: leave out the bricks whose transfer happens inside the operator passes
    void
    run(const T *src, T *dst, bool prolongate, bool skip_fused = false)
    {
      for (auto &b : bricks)
        {
          const size_t nb = skip_fused ? b->n_unfused : b->n_bricks;
          if (!dispatch_degree(pc, [&](auto P) {
                if (!dispatch_brick_size<P(), 2, 4, 8, 16>(b->B, [&](auto B) { launch_brick<P(), B()>(*b, src, dst, prolongate, nb); }))
                  throw std::runtime_error("brick transfer: unsupported brick size");
              }))
            throw std::runtime_error("brick transfer: degree not instantiated");
        }
      for (int k = 0; k < 3; ++k)
        {
          const GroupD &g = grp[k];
          if (!g.n_patches)
            continue;
          const int key = pc * 100 + g.nf;
          if (k == 0)
            {
              if (!dispatch_degree(pc, [&](auto P) { launch<P(), P() + 1, true>(g, src, dst, prolongate); }))
                throw std::runtime_error("transfer: degree not instantiated");
            }
          else
            switch (key)
              {
                case 103:
                  if (g.p1_uniq_ptr.p)
                    launch_p1(g, src, dst, prolongate);
                  else
                    launch<1, 3, false>(g, src, dst, prolongate);
                  break;
                case 104:
                  launch<1, 4, false>(g, src, dst, prolongate);
                  break;
                case 205:
                  launch<2, 5, false>(g, src, dst, prolongate);
                  break;
                case 206: // p-transfer 5 -> 2
                  launch<2, 6, false>(g, src, dst, prolongate);
                  break;
                case 307:
                  launch<3, 7, false>(g, src, dst, prolongate);
                  break;
                case 308: // p-transfer 7 -> 3
                  launch<3, 8, false>(g, src, dst, prolongate);
                  break;
                case 409:
                  launch<4, 9, false>(g, src, dst, prolongate);
                  break;
                case 511:
                  launch<5, 11, false>(g, src, dst, prolongate);
                  break;
                case 613:
                  launch<6, 13, false>(g, src, dst, prolongate);
                  break;
                case 715:
                  launch<7, 15, false>(g, src, dst, prolongate);
                  break;
                default:
                  throw std::runtime_error("transfer: (coarse degree, fine patch) combination not instantiated");
              }
        }
    }

    // Fused passes (fused_ready()): the residual step and the restriction of Multigrid::level_v_step in ONE operator pass
    // (ref:multigrid_throughput.cc:1093-1099 wiring; deal.II level_v_step: residual, restrict_and_add).  t receives the residual
    // rows that the un-fused patches still restrict (everything outside the fused bricks); the coarse defect receives the fused
    // bricks' part directly.  Call restrict_unfused_raw afterwards.
    void
    residual_restrict_raw(T *dst_coarse, T *t, const T *b, const T *x)
    {
      FusedTransferHost<T> f = fused;
      f.coarse               = dst_coarse;
      Epilogue<T> e{t, x, nullptr, b, nullptr, T(0), T(0), T(0)};
      fop->template apply<MODE_RESIDUAL_RESTRICT>(x, e, false, 0, 0, &f);
    }
    void
    restrict_unfused_raw(T *dst_coarse, const T *src_fine)
    {
      run(src_fine, dst_coarse, false, true);
      finish_restriction(dst_coarse);
    }
    // the un-fused part of the prolongation (in place); the fused bricks add theirs while the first post-smoothing pass
    // gathers x (Chebyshev::step_raw with this transfer)
    void
    prolongate_unfused_raw(T *dst_fine, const T *src_coarse)
    {
      run(src_coarse, dst_fine, true, true);
      if (fop->halo)
        fop->import_from_owner_raw(dst_fine + fop->tables->n_interior);
    }
    void
    prolongate_raw(T *dst_fine, const T *src_coarse)
    {
      run(src_coarse, dst_fine, true);
      // sharded runs: a rank that references a shared DoF only through hanging-node resolution has no patch writing its
      // copy, and different ranks evaluate the embedding through different patches: all copies take the owner's value
      if (fop->halo)
        fop->import_from_owner_raw(dst_fine + fop->tables->n_interior);
    }
    void
    restrict_raw(T *dst_coarse, const T *src_fine)
    {
      run(src_fine, dst_coarse, false);
      finish_restriction(dst_coarse);
    }
    void
    finish_restriction(T *dst_coarse)
    {
      // sharded runs: complete the coarse defect across ranks.  Onto a level that is cut into fewer pieces than the fine one (a
      // part held by a group of ranks, Partition tiers): every member of the group has restricted the cells of its own, so the
      // members' vectors are summed first; then the shared DoFs between the parts
      if (auto *sc = dynamic_cast<SubsetComm *>(cop->comm.get()))
        {
          auto     *sf = dynamic_cast<SubsetComm *>(fop->comm.get());
          const int gf = sf ? sf->group : (fop->comm ? 1 : sc->group);
          if (gf != sc->group)
            {
              if (gf != 1)
                throw std::runtime_error("restriction between two rank-subset tiers of different group sizes is not supported");
              sc->replica_sum(dst_coarse, cop->n_dofs(), (int)sizeof(T), ctx->stream);
            }
        }
      if (cop->halo)
        cop->exchange_add_raw(dst_coarse + cop->tables->n_interior);
      else if (fop->comm)
        fop->comm->allreduce_sum(dst_coarse, cop->n_dofs(), (int)sizeof(T), ctx->stream); // onto the replicated level
    }
    void
    prolongate_and_add(mgamd_vec &dst, const mgamd_vec &src) override
    {
      if (dst.n != fine->n_dofs() || src.n != coarse->n_dofs())
        throw std::invalid_argument("prolongate_and_add: vector size mismatch");
      prolongate_raw(dst.as<T>(), src.as<T>());
    }
    void
    restrict_and_add(mgamd_vec &dst, const mgamd_vec &src) override
    {
      if (dst.n != coarse->n_dofs() || src.n != fine->n_dofs())
        throw std::invalid_argument("restrict_and_add: vector size mismatch");
      restrict_raw(dst.as<T>(), src.as<T>());
    }
  };

  Transfer2Base *
  make_transfer2(LevelOperatorBase *fine, LevelOperatorBase *coarse)
  {
    if (fine->type != coarse->type)
      throw std::invalid_argument("transfer: level number types differ");
    if (fine->type == MGAMD_F64)
      return new Transfer2<double>(static_cast<LevelOperator<double> *>(fine), static_cast<LevelOperator<double> *>(coarse));
    return new Transfer2<float>(static_cast<LevelOperator<float> *>(fine), static_cast<LevelOperator<float> *>(coarse));
  }

  // ------------------------------------------------------------------------------------------
  // K7 / K8 launchers (kernels_amg.hpp): the one path of the AMG cycle, of the assembled operator and of mgamd_debug_csr_spmv
  // ------------------------------------------------------------------------------------------
  int
  csr_spmv_lanes(uint32_t n_rows, size_t nnz)
  {
    const double avg = n_rows ? (double)nnz / n_rows : 0.0;
    return avg <= 6 ? 4 : (avg <= 24 ? 8 : (avg <= 64 ? 16 : 32));
  }
  // the assembled operator and its AMG (AssembledMatrix, below) only: K8, a wave per row, above a mean row length of
  // CSR_SPMV_WAVE_MIN_MEAN_ROW (measured: profiles/amg_solver_spmv.txt), K7's choice below it
  int
  csr_spmv_lanes_long(uint32_t n_rows, size_t nnz)
  {
    const double avg       = n_rows ? (double)nnz / n_rows : 0.0;
    const char  *e         = getenv("MGAMD_SPMV_WAVE_MIN_MEAN_ROW");
    const double threshold = e ? atof(e) : CSR_SPMV_WAVE_MIN_MEAN_ROW;
    return avg > threshold ? 64 : csr_spmv_lanes(n_rows, nnz);
  }

  // f(mode tag, lanes tag) with the run-time mode and lane count as compile-time constants
  template <typename F>
  void
  dispatch_spmv(int mode, int lanes, F &&f)
  {
    auto with_lanes = [&](auto mode_tag) {
      switch (lanes)
        {
          case 4:
            f(mode_tag, std::integral_constant<int, 4>());
            break;
          case 8:
            f(mode_tag, std::integral_constant<int, 8>());
            break;
          case 16:
            f(mode_tag, std::integral_constant<int, 16>());
            break;
          case 32:
            f(mode_tag, std::integral_constant<int, 32>());
            break;
          case 64:
            f(mode_tag, std::integral_constant<int, 64>());
            break;
          default:
            throw std::invalid_argument("csr_spmv: lanes must be 4, 8, 16, 32 or 64");
        }
    };
    switch (mode)
      {
        case SPMV_PLAIN:
          with_lanes(std::integral_constant<int, SPMV_PLAIN>());
          break;
        case SPMV_ADD:
          with_lanes(std::integral_constant<int, SPMV_ADD>());
          break;
        case SPMV_RESID:
          with_lanes(std::integral_constant<int, SPMV_RESID>());
          break;
        case SPMV_CHEB:
          with_lanes(std::integral_constant<int, SPMV_CHEB>());
          break;
        case SPMV_DOT:
          with_lanes(std::integral_constant<int, SPMV_DOT>());
          break;
        default:
          throw std::invalid_argument("csr_spmv: unknown mode");
      }
  }

  // all rows of the matrix (csr_spmv_kernel; lanes 64: csr_spmv_wave_kernel); returns the blocks launched.  SPMV_DOT leaves one
  // partial sum per block in `partial` (Ctx::d_partial: 1024 doubles, hence its cap of 1024 blocks).  max_blocks > 0 lowers the
  // cap (tests: a row's result does not depend on the grid).  SPMV_DOT and 64 lanes exist in FP64 only.
  template <typename T>
  int
  launch_csr_spmv(hipStream_t stream, int mode, int lanes, uint32_t n_rows, const uint32_t *ptr, const uint32_t *col, const T *val, const T *x,
                  T *y, const T *b, const T *xold, const T *dinv, double f1, double f2, double *partial, int max_blocks)
  {
    if (!n_rows)
      return 0;
    if (mode == SPMV_DOT && !partial)
      throw std::invalid_argument("csr_spmv: SPMV_DOT needs the buffer of the block partials");
    int grid = 0;
    dispatch_spmv(mode, lanes, [&](auto mode_tag, auto lanes_tag) {
      constexpr int MODE  = decltype(mode_tag)::value;
      constexpr int LANES = decltype(lanes_tag)::value;
      if constexpr ((MODE == SPMV_DOT || LANES == 64) && !std::is_same<T, double>::value)
        throw std::invalid_argument("csr_spmv: SPMV_DOT and 64 lanes per row are FP64 only");
      else
        {
          size_t g = std::min<size_t>(((size_t)n_rows * LANES + 255) / 256, MODE == SPMV_DOT ? 1024 : 4096);
          if (max_blocks > 0)
            g = std::min<size_t>(g, (size_t)max_blocks);
          grid = (int)g;
          if constexpr (LANES == 64)
            hipLaunchKernelGGL((csr_spmv_wave_kernel<T, MODE>), grid, 256, 0, stream, n_rows, ptr, col, val, x, y, b, xold, dinv, T(f1), T(f2),
                               partial);
          else
            hipLaunchKernelGGL((csr_spmv_kernel<T, MODE, LANES>), grid, 256, 0, stream, n_rows, ptr, col, val, x, y, b, xold, dinv, T(f1),
                               T(f2), partial);
        }
    });
    HIP_CHECK(hipGetLastError());
    return grid;
  }
  template int
  launch_csr_spmv<double>(hipStream_t, int, int, uint32_t, const uint32_t *, const uint32_t *, const double *, const double *, double *,
                          const double *, const double *, const double *, double, double, double *, int);
  template int
  launch_csr_spmv<float>(hipStream_t, int, int, uint32_t, const uint32_t *, const uint32_t *, const float *, const float *, float *,
                         const float *, const float *, const float *, double, double, double *, int);

  // the rows [row_begin, row_end) only (csr_spmv_range_kernel): the interior and boundary launches of a sharded level
  template <typename T>
  void
  launch_csr_spmv_range(hipStream_t stream, int mode, int lanes, uint32_t row_begin, uint32_t row_end, const uint32_t *ptr, const uint32_t *col,
                        const T *val, const T *x, T *y, const T *b, const T *xold, const T *dinv, double f1, double f2)
  {
    if (row_end <= row_begin)
      return;
    if (mode == SPMV_DOT || lanes == 64)
      throw std::invalid_argument("csr_spmv: a range of rows has neither SPMV_DOT nor 64 lanes per row");
    const uint32_t n_rows = row_end - row_begin;
    dispatch_spmv(mode, lanes, [&](auto mode_tag, auto lanes_tag) {
      constexpr int MODE  = decltype(mode_tag)::value;
      constexpr int LANES = decltype(lanes_tag)::value;
      if constexpr (MODE != SPMV_DOT && LANES != 64)
        {
          const int grid = (int)std::min<size_t>(((size_t)n_rows * LANES + 255) / 256, 4096);
          hipLaunchKernelGGL((csr_spmv_range_kernel<T, MODE, LANES>), grid, 256, 0, stream, row_begin, row_end, ptr, col, val, x, y, b, xold,
                             dinv, T(f1), T(f2));
        }
    });
    HIP_CHECK(hipGetLastError());
  }

  // ------------------------------------------------------------------------------------------
  // Algebraic multigrid coarse solver on the device (host setup: amg.hpp).  The reference's "amg" / "cg_with_amg" coarse solvers
  // (ref:multigrid_throughput.cc:945-1016) apply Trilinos ML to Operator::get_trilinos_system_matrix; this is an own
  // smoothed-aggregation V-cycle on the same matrix: CSR products fused with the Chebyshev update (kernels.hpp K7).
  //
  // ONE cycle, two set-ups.  On one rank every level is whole and the cycle runs on the caller's vectors.  On a SHARDED coarse level
  // (amg_shard.hpp: replicated setup, sharded cycle) every rank builds the one-rank hierarchy from the global tables of the coarse
  // space and keeps its rows of A, P and R; a product is: interior rows, ghost import on ctx->side underneath them, boundary rows
  // (the level operator's scheme, MGAMD_NO_HALO_OVERLAP=1: one launch after the import).  A whole level is a cut without a cut:
  // its products are one launch over all rows.  The level-0 vectors of a sharded multigrid are consistent copies in the local
  // [I|T|D|H] numbering: the owned rows are gathered on entry; on exit the owned results are scattered, the copies of other ranks'
  // DoFs are zero and the level operator's exchange_add completes them (exact: it adds zeros).
  // ------------------------------------------------------------------------------------------
  template <typename T>
  struct AmgCycle
  {
    struct Mat
    {
      DBuf<uint32_t> ptr, col;
      DBuf<T>        val;
      uint32_t       n_rows = 0, n_cols = 0;
      int            lanes  = 8;
      void
      upload(const CSR &A)
      {
        n_rows = A.n_rows;
        n_cols = A.n_cols;
        ptr.upload(A.ptr);
        col.upload(A.col.empty() ? std::vector<uint32_t>(1, 0) : A.col);
        std::vector<T> v(std::max<size_t>(A.val.size(), 1), T(0));
        std::copy(A.val.begin(), A.val.end(), v.begin());
        val.upload(v);
      }
    };
    struct Lvl
    {
      std::shared_ptr<Mat>  A; // (level 0 of the assembled operator's AMG: the operator's own device matrix)
      Mat                   P, R;
      DBuf<T>               dinv, x, b, r, t, send;
      DBuf<uint32_t>        send_idx;
      double                theta = 1, delta = 0;
      uint32_t              n = 0, n_int = 0, n_recv = 0, n_global = 0, n_owned = 0, n_ghost = 0;
      bool                  replicated = true;
      std::vector<int>      peers;
      std::vector<uint32_t> peer_offset;
    };
    Ctx                              *ctx = nullptr;
    LevelOperator<T>                 *op0 = nullptr; // sharded: level 0 of the multigrid; one rank: null, the cycle runs on its vectors
    std::shared_ptr<Comm>             comm;
    std::vector<std::unique_ptr<Lvl>> lv;
    DBuf<double>                      coarse_inv;
    unsigned                          degree  = 2; // Chebyshev smoother degree (MGAMD_AMG_SMOOTHER_DEGREE: development)
    bool                              overlap = true;
    bool                              long_rows = false; // lanes per row by csr_spmv_lanes_long (the assembled operator's AMG)
    std::shared_ptr<Mat>              shared0;           // that operator's device matrix: level 0's A, not uploaded again
    // level 0 <-> geometric vector
    DBuf<uint32_t> in_amg, in_geo, out_amg, out_geo;
    uint32_t       n_in = 0, n_out = 0;

    int
    lanes_for(const CSR &M) const
    {
      return long_rows ? csr_spmv_lanes_long(M.n_rows, M.nnz()) : csr_spmv_lanes(M.n_rows, M.nnz());
    }
    AmgHierarchyHost
    build_hierarchy(CSR A0)
    {
      if (const char *e = getenv("MGAMD_AMG_SMOOTHER_DEGREE"))
        degree = std::max(1, atoi(e));
      AmgHierarchyHost H = build_smoothed_aggregation(std::move(A0));
      if (H.levels.back().A.n_rows > 4096)
        throw std::runtime_error("AMG: coarsening stalled at " + std::to_string(H.levels.back().A.n_rows) + " rows");
      coarse_inv.upload(H.coarse_inv);
      return H;
    }
    // level G of the hierarchy, cut as P says (null: whole)
    void
    add_level(const AmgLevelHost &G, const AmgShardLevel *P, bool last)
    {
      const bool whole = !P || P->replicated;
      auto       L     = std::make_unique<Lvl>();
      L->n_global = L->n = L->n_int = L->n_owned = G.A.n_rows;
      if (P)
        {
          L->replicated  = P->replicated;
          L->n_global    = P->n_global;
          L->n           = P->n_rows;
          L->n_int       = P->replicated ? P->n_rows : P->launch_interior();
          L->n_recv      = P->n_recv;
          L->n_owned     = P->n_owned();
          L->n_ghost     = P->n_ghost;
          L->peers       = P->peers;
          L->peer_offset = P->peer_offset;
        }
      if (lv.empty() && shared0)
        L->A = shared0;
      else
        {
          L->A = std::make_shared<Mat>();
          L->A->upload(whole ? G.A : P->A);
          L->A->lanes = lanes_for(G.A); // the whole matrix's lanes: the same additions per row however it is cut
        }
      if (!last)
        {
          L->P.upload(whole ? G.P : P->P);
          L->R.upload(whole ? G.R : P->R);
          L->P.lanes = lanes_for(G.P);
          L->R.lanes = lanes_for(G.R);
        }
      std::vector<T> d(std::max<uint32_t>(L->n, 1), T(1));
      for (uint32_t i = 0; i < L->n; ++i)
        d[i] = (T)G.dinv[whole ? i : P->rows[i]];
      L->dinv.upload(d);
      // x, r, t are read through the columns of a product: room for the ghosts behind the local rows
      const size_t nv = std::max<size_t>((size_t)L->n + L->n_recv, 1);
      for (DBuf<T> *v : {&L->r, &L->t})
        {
          v->alloc(nv);
          v->zero(ctx->stream);
        }
      if (op0 || !lv.empty()) // (one rank: level 0 works on the caller's vectors)
        {
          L->x.alloc(nv);
          L->x.zero(ctx->stream);
          L->b.alloc(std::max<uint32_t>(L->n, 1));
          L->b.zero(ctx->stream);
        }
      if (L->n_recv)
        {
          L->send.alloc(L->n_recv);
          L->send_idx.upload(P->send_idx);
        }
      // Chebyshev on [lambda_max / 20, lambda_max] (ML's "smoother: Chebyshev alpha" = 20)
      const double mx = G.lambda_max, mn = mx / 20.0;
      L->theta = 0.5 * (mx + mn);
      L->delta = 0.5 * (mx - mn);
      lv.push_back(std::move(L));
    }

    // one rank: the hierarchy of the level's own tables, every level whole
    AmgCycle(Ctx *c, const LevelTables &tables)
      : ctx(c)
    {
      const AmgHierarchyHost H = build_hierarchy(assemble_level_matrix(tables)); // (refuses local-smoothing levels)
      for (size_t l = 0; l < H.levels.size(); ++l)
        add_level(H.levels[l], nullptr, l + 1 == H.levels.size());
    }

    // one rank, the assembled operator's preconditioner (AssembledMatrix): the hierarchy of its matrix A0, whose device copy
    // dev0 is level 0's; K8 on the matrices with long rows
    AmgCycle(Ctx *c, const CSR &A0, std::shared_ptr<Mat> dev0)
      : ctx(c)
      , long_rows(true)
      , shared0(std::move(dev0))
    {
      const AmgHierarchyHost H = build_hierarchy(A0);
      for (size_t l = 0; l < H.levels.size(); ++l)
        add_level(H.levels[l], nullptr, l + 1 == H.levels.size());
      ctx->sync();
    }

    // sharded level 0: the hierarchy of the global tables, this rank's rows of it
    AmgCycle(Ctx *c, LevelOperator<T> *op, const LevelTables &global, uint32_t min_sharded_rows)
      : ctx(c)
      , op0(op)
      , comm(op->comm)
    {
      overlap = getenv("MGAMD_NO_HALO_OVERLAP") == nullptr;
      if (auto *sub = dynamic_cast<SubsetComm *>(comm.get()))
        if (sub->group > 1)
          throw std::invalid_argument("sharded AMG: level 0 is held by groups of ranks (a subset tier of the partition); the sharded "
                                      "algebraic multigrid needs a level 0 that is cut over all ranks");
      const int          n_ranks = comm ? comm->n_ranks : 1, rank = comm ? comm->rank : 0;
      const LevelTables &local   = *op->tables;
      const std::vector<uint32_t> grow = match_rows_by_key(global, local, op->sigma); // (refuses another space, another operator)
      const std::vector<uint8_t>  own  = local_dof_owned(local);
      const AmgHierarchyHost      H    = build_hierarchy(assemble_level_matrix(global));
      const uint32_t              n0   = H.levels[0].A.n_rows;
      // owner stamps: one all-reduce builds the owner map of level 0 and checks that every row is owned exactly once
      std::vector<double> stamp(2 * (size_t)n0, 0.0);
      for (uint32_t d = 0; d < local.n_dofs; ++d)
        if (own[d])
          {
            stamp[grow[d]] += 1.0;
            stamp[n0 + grow[d]] += (double)(rank + 1);
          }
      if (comm)
        {
          DBuf<double> ds;
          ds.upload(stamp);
          comm->allreduce_sum(ds.p, stamp.size(), 8, ctx->stream);
          HIP_CHECK(hipMemcpyAsync(stamp.data(), ds.p, stamp.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
          ctx->sync();
        }
      std::vector<uint32_t> count(n0);
      std::vector<int32_t>  owner0(n0);
      for (uint32_t i = 0; i < n0; ++i)
        {
          count[i]  = (uint32_t)std::lround(stamp[i]);
          owner0[i] = (int32_t)std::lround(stamp[n0 + i]) - 1;
        }
      check_owned_once(count, "level 0");
      std::vector<uint32_t> mirror0;
      for (uint32_t d = local.first_constrained(); d < local.n_dofs; ++d)
        if (!own[d])
          mirror0.push_back(grow[d]);
      std::sort(mirror0.begin(), mirror0.end());
      const unsigned     n_sharded = amg_n_sharded_levels(H, n_ranks, min_sharded_rows);
      const AmgShardPlan S = build_amg_shard_plan(H, amg_level_owners(H, owner0, n_ranks, n_sharded), mirror0, n_ranks, rank);

      for (size_t l = 0; l < H.levels.size(); ++l)
        add_level(H.levels[l], &S.levels[l], l + 1 == H.levels.size());

      std::vector<uint32_t> ia, ig, oa, og;
      if (S.levels[0].replicated)
        {
          // the whole vector on every rank: owned entries in, all-reduce; every local entry (copies included) out
          for (uint32_t d = 0; d < local.n_dofs; ++d)
            {
              if (own[d])
                {
                  ia.push_back(grow[d]);
                  ig.push_back(d);
                }
              oa.push_back(grow[d]);
              og.push_back(d);
            }
          in_amg.upload(ia);
          out_amg.upload(oa);
        }
      else
        {
          std::vector<uint32_t> local_of(n0, INVALID_DOF);
          for (uint32_t d = 0; d < local.n_dofs; ++d)
            local_of[grow[d]] = d;
          for (uint32_t g : S.levels[0].rows)
            {
              if (local_of[g] == INVALID_DOF)
                throw std::runtime_error("sharded AMG: a local row of level 0 is not a DoF of this rank");
              ig.push_back(local_of[g]);
            }
          og = ig;
        }
      n_in  = (uint32_t)ig.size();
      n_out = (uint32_t)og.size();
      in_geo.upload(ig);
      out_geo.upload(og);
      ctx->sync();
    }

    // refresh the ghost entries of v (a vector of level L): pack on the main queue, import on `st`
    void
    import_ghosts(Lvl &L, T *v, hipStream_t st)
    {
      if (!L.peers.empty())
        hipLaunchKernelGGL(amg_pack_ghosts_kernel<T>, grid_for(L.n_recv), 256, 0, ctx->stream, L.send.p, v, L.send_idx.p, L.n_recv);
      if (st != ctx->stream)
        ctx->order_after(st, ctx->stream);
      // (a rank without peers on this level still takes part: the simulator's exchange is a barrier of all ranks)
      comm->exchange(L.send.p, v + L.n, L.peers, L.peer_offset, sizeof(T), st);
    }
    // y (rows of M) <- product with x, a vector of level `in` (null: no ghosts to import); n_int: rows that read no ghost
    template <int MODE>
    void
    spmv(const Mat &M, Lvl *in, uint32_t n_int, T *x, T *y, const T *b = nullptr, const T *xold = nullptr, const T *dinv = nullptr,
         double f1 = 0, double f2 = 0)
    {
      if (!in || in->replicated || !comm)
        {
          launch_csr_spmv<T>(ctx->stream, MODE, M.lanes, M.n_rows, M.ptr.p, M.col.p, M.val.p, x, y, b, xold, dinv, f1, f2, nullptr, 0);
          return;
        }
      auto rows = [&](uint32_t r0, uint32_t r1) {
        launch_csr_spmv_range<T>(ctx->stream, MODE, M.lanes, r0, r1, M.ptr.p, M.col.p, M.val.p, x, y, b, xold, dinv, f1, f2);
      };
      if (overlap && !in->peers.empty() && n_int > 0 && n_int < M.n_rows)
        {
          import_ghosts(*in, x, ctx->side);
          rows(0, n_int);
          ctx->order_after(ctx->stream, ctx->side);
          rows(n_int, M.n_rows);
        }
      else
        {
          import_ghosts(*in, x, ctx->stream);
          rows(0, M.n_rows);
        }
    }
    // Chebyshev of degree `degree` in D^-1 A, zero start (deal.II / ML recurrences): result in x (t: scratch)
    void
    smooth_zero(Lvl &L, T *x, T *t, const T *b)
    {
      T *cur = (degree % 2 == 1) ? x : t, *oth = (cur == x) ? t : x;
      hipLaunchKernelGGL(vec_scaled_product_kernel<T>, grid_for(std::max<uint32_t>(L.n, 1)), 256, 0, ctx->stream, cur, T(1.0 / L.theta),
                         L.dinv.p, b, (size_t)L.n);
      double       rhok  = L.delta / L.theta;
      const double sigma = L.theta / L.delta;
      for (unsigned j = 0; j + 1 < degree; ++j)
        {
          const double rhokp = 1.0 / (2.0 * sigma - rhok);
          // (x_old in place)
          spmv<SPMV_CHEB>(*L.A, &L, L.n_int, cur, oth, b, j == 0 ? nullptr : oth, L.dinv.p, rhokp * rhok, 2.0 * rhokp / L.delta);
          rhok = rhokp;
          std::swap(cur, oth);
        }
      // (degree - 1 swaps from the buffer chosen above: cur == x)
    }
    // general start x0 in x: result in x again
    void
    smooth_step(Lvl &L, T *x, T *t, const T *b)
    {
      T *cur = x, *oth = t;
      spmv<SPMV_CHEB>(*L.A, &L, L.n_int, cur, oth, b, nullptr, L.dinv.p, 0.0, 1.0 / L.theta);
      std::swap(cur, oth);
      double       rhok  = L.delta / L.theta;
      const double sigma = L.theta / L.delta;
      for (unsigned j = 0; j + 1 < degree; ++j)
        {
          const double rhokp = 1.0 / (2.0 * sigma - rhok);
          spmv<SPMV_CHEB>(*L.A, &L, L.n_int, cur, oth, b, oth, L.dinv.p, rhokp * rhok, 2.0 * rhokp / L.delta);
          rhok = rhokp;
          std::swap(cur, oth);
        }
      if (cur != x && L.n)
        HIP_CHECK(hipMemcpyAsync(x, cur, (size_t)L.n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    }
    void
    cycle(size_t l, T *x, const T *b)
    {
      Lvl &L = *lv[l];
      if (l + 1 == lv.size())
        {
          hipLaunchKernelGGL(dense_matvec_kernel<T>, (int)std::min<uint32_t>(L.n, 1024), 256, 0, ctx->stream, coarse_inv.p, b, x, (int)L.n);
          return;
        }
      Lvl &C = *lv[l + 1];
      smooth_zero(L, x, L.t.p, b);
      spmv<SPMV_RESID>(*L.A, &L, L.n_int, x, L.r.p, b);
      if (!L.replicated && C.replicated)
        {
          // partial sums over my owned columns, completed over the ranks
          spmv<SPMV_PLAIN>(L.R, nullptr, 0, L.r.p, C.b.p);
          if (comm)
            comm->allreduce_sum(C.b.p, C.n, (int)sizeof(T), ctx->stream);
        }
      else
        spmv<SPMV_PLAIN>(L.R, &L, C.n_int, L.r.p, C.b.p);
      cycle(l + 1, C.x.p, C.b.p);
      spmv<SPMV_ADD>(L.P, &C, L.n_int, C.x.p, x);
      smooth_step(L, x, L.t.p, b);
    }
    // z = V(r): one V-cycle from a zero initial guess on the level-0 vectors of the multigrid (sharded: local numbering,
    // consistent copies)
    void
    vcycle(T *z, const T *r)
    {
      Lvl &L = *lv[0];
      if (!op0)
        cycle(0, z, r);
      else if (L.replicated)
        {
          if (comm)
            L.b.zero(ctx->stream);
          if (n_in)
            hipLaunchKernelGGL(amg_level0_gather_kernel<T>, grid_for(n_in), 256, 0, ctx->stream, L.b.p, in_amg.p, r, in_geo.p, n_in);
          if (comm)
            comm->allreduce_sum(L.b.p, L.n, (int)sizeof(T), ctx->stream);
          cycle(0, L.x.p, L.b.p);
          hipLaunchKernelGGL(amg_level0_scatter_kernel<T>, grid_for(n_out), 256, 0, ctx->stream, z, out_geo.p, L.x.p, out_amg.p, n_out);
        }
      else
        {
          if (n_in)
            hipLaunchKernelGGL(amg_level0_gather_kernel<T>, grid_for(n_in), 256, 0, ctx->stream, L.b.p, (const uint32_t *)nullptr, r,
                               in_geo.p, n_in);
          cycle(0, L.x.p, L.b.p);
          HIP_CHECK(hipMemsetAsync(z, 0, (size_t)op0->n_dofs() * sizeof(T), ctx->stream));
          if (n_out)
            hipLaunchKernelGGL(amg_level0_scatter_kernel<T>, grid_for(n_out), 256, 0, ctx->stream, z, out_geo.p, L.x.p,
                               (const uint32_t *)nullptr, n_out);
          op0->exchange_add_raw(z + op0->tables->n_interior);
        }
      HIP_CHECK(hipGetLastError());
    }
    // per level: global rows, owned rows, ghosts, peers, replicated
    void
    layout(std::vector<uint32_t> &out) const
    {
      out.clear();
      for (const auto &L : lv)
        for (uint32_t v : {L->n_global, L->n_owned, L->n_ghost, (uint32_t)L->peers.size(), (uint32_t)(L->replicated ? 1 : 0)})
          out.push_back(v);
    }
  };

  // x = V(b), then n_cycles - 1 corrections x += V(b - A x) (ML's `cycle applications`, ref CoarseSolverNCycles).
  // vcycle(z, r): z = V(r); residual(rr, b, x): rr = b - A x; rr, zz: scratch of n entries, touched only for n_cycles > 1
  template <typename T, typename VCYCLE, typename RESIDUAL>
  static void
  repeat_cycles(hipStream_t stream, unsigned n_cycles, VCYCLE vcycle, RESIDUAL residual, T *x, const T *b, T *rr, T *zz, size_t n)
  {
    vcycle(x, b);
    for (unsigned c = 1; c < n_cycles; ++c)
      {
        residual(rr, b, x);
        vcycle(zz, rr);
        hipLaunchKernelGGL(vec_sadd_kernel<T>, grid_for(n), 256, 0, stream, x, T(1), T(1), zz, n);
      }
  }

  // ------------------------------------------------------------------------------------------
  // The coarse solver of a multigrid: x = (approximately) A_0^-1 b on level 0.  Which one runs is resolve_coarse_kind's decision
  // (coarse_policy.hpp); every buffer is allocated by the one kind that reads it.
  // ------------------------------------------------------------------------------------------
  template <typename T>
  struct CoarseSolver
  {
    Ctx                         *ctx;
    CoarseKind                   kind;
    LevelOperator<T>            *op0;
    Chebyshev<T>                *sm0;              // CgChebyshev: the preconditioner
    MultigridBase               *nested = nullptr; // Nested
    std::unique_ptr<AmgCycle<T>> amg;              // Amg, CgAmg: one rank, or a sharded level 0 (by request: amg_global)
    unsigned                     n_cycles;         // Nested, Amg, CgAmg: cycles per application
    DBuf<T>                      rep_r, rep_z;     // their residual and correction, n_cycles > 1 only
    DBuf<double>                 inv;              // Direct: dense inverse
    DBuf<T>                      cg_r, cg_z, cg_p, cg_Ap; // Cg, CgChebyshev, CgAmg
    DBuf<double>                 cg_S;             // device scalars of the coarse CG (device_pcg): its own, it runs inside an outer CG
    uint64_t                     iterations = 0;   // inner CG iterations, accumulated

    CoarseSolver(Ctx *c, LevelOperator<T> *op, Chebyshev<T> *smoother, const std::string &name, MultigridBase *nested_mg,
                 unsigned nested_cycles, const LevelTables *amg_global, uint32_t amg_min_sharded_rows)
      : ctx(c)
      , kind(resolve_coarse_kind(name, op->n_dofs(), op->comm != nullptr, nested_mg != nullptr, amg_global != nullptr))
      , op0(op)
      , sm0(smoother)
      , n_cycles(std::max(1u, nested_cycles))
    {
      switch (kind)
        {
          case CoarseKind::Direct:
            setup_direct();
            break;
          case CoarseKind::Nested:
            if (nested_mg->number_type != (int)sizeof(T) || nested_mg->outer_tables() != op0->tables.get())
              throw std::invalid_argument("multigrid: the nested multigrid must act on the DoFs of this hierarchy's level 0 (same number type)");
            nested = nested_mg;
            alloc_repeat();
            break;
          case CoarseKind::CgAmg:
            alloc_cg();
            [[fallthrough]];
          case CoarseKind::Amg:
            if (amg_global)
              amg = std::make_unique<AmgCycle<T>>(ctx, op0, *amg_global, amg_min_sharded_rows);
            else if (op0->tables->sigma != op0->sigma)
              throw std::invalid_argument("multigrid: the mass coefficient of level 0's tables (" + std::to_string(op0->tables->sigma) +
                                          ") was changed after its operator was built with " + std::to_string(op0->sigma) +
                                          "; the AMG coarse solver assembles its matrix from the tables");
            else
              amg = std::make_unique<AmgCycle<T>>(ctx, *op0->tables);
            alloc_repeat();
            break;
          case CoarseKind::CgChebyshev:
            if (!sm0)
              throw std::invalid_argument("multigrid: cg_with_chebyshev needs a smoother on level 0");
            [[fallthrough]];
          case CoarseKind::Cg:
            alloc_cg();
            break;
        }
    }
    void
    alloc_repeat() // residual and correction of the cycles after the first
    {
      if (n_cycles > 1)
        rep_r.alloc(op0->n_dofs()), rep_z.alloc(op0->n_dofs());
    }
    void
    alloc_cg()
    {
      for (DBuf<T> *v : {&cg_r, &cg_z, &cg_p, &cg_Ap})
        v->alloc(op0->n_dofs());
      cg_S.alloc(8);
    }

    // tabulate A_0 column by column through the level operator, symmetrise, invert
    void
    setup_direct()
    {
      const size_t n = op0->n_dofs();
      if (n > MGAMD_DIRECT_COARSE_MAX_DOFS)
        throw std::runtime_error("coarse level too large for the direct solver (" + std::to_string(n) +
                                 " DoFs): use CoarseGridSolverType cg or cg_with_chebyshev");
      std::vector<double> A(n * n, 0.0), Ainv;
      DBuf<T>             e, col;
      e.alloc(n);
      col.alloc(n);
      std::vector<T> h(n);
      for (size_t j = 0; j < n; ++j)
        {
          e.zero(ctx->stream);
          const T one = T(1);
          HIP_CHECK(hipMemcpyAsync(e.p + j, &one, sizeof(T), hipMemcpyHostToDevice, ctx->stream));
          op0->vmult_raw(col.p, e.p);
          HIP_CHECK(hipMemcpyAsync(h.data(), col.p, n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
          ctx->sync();
          for (size_t i = 0; i < n; ++i)
            A[i * n + j] = (double)h[i];
        }
      for (size_t i = 0; i < n; ++i)
        for (size_t j = i + 1; j < n; ++j)
          A[i * n + j] = A[j * n + i] = 0.5 * (A[i * n + j] + A[j * n + i]);
      invert_dense(A, n, Ainv, "coarse matrix is singular");
      inv.upload(Ainv);
    }

    void
    solve(T *x, const T *b)
    {
      const size_t n = op0->n_dofs();
      // z = n_cycles applications of `vcycle` to r
      auto cycles = [&](auto vcycle, T *z, const T *r) {
        repeat_cycles<T>(ctx->stream, n_cycles, vcycle, [&](T *rr, const T *bb, const T *xx) { op0->residual_raw(rr, bb, xx); }, z, r,
                         rep_r.p, rep_z.p, n);
      };
      auto amg_cycles = [&](T *z, const T *r) { cycles([&](T *zz, const T *rr) { amg->vcycle(zz, rr); }, z, r); };
      switch (kind)
        {
          case CoarseKind::Direct:
            hipLaunchKernelGGL(dense_matvec_kernel<T>, (int)std::min<size_t>(n, 1024), 256, 0, ctx->stream, inv.p, b, x, (int)n);
            return;
          case CoarseKind::Nested:
            cycles([&](T *zz, const T *rr) { nested->vcycle_level_raw(zz, rr); }, x, b);
            return;
          case CoarseKind::Amg:
            amg_cycles(x, b);
            return;
          case CoarseKind::Cg:
          case CoarseKind::CgChebyshev:
          case CoarseKind::CgAmg:
            break;
        }
      // SolverCG + ReductionControl(maxiter 10000, abstol 1e-20, reltol 1e-4): ref:multigrid_throughput.cc:888-895;
      // device-resident iteration, inner products over the GLOBAL vector (owned prefix + one scalar all-reduce on a
      // sharded level)
      HIP_CHECK(hipMemcpyAsync(cg_r.p, b, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
      unsigned its = 0;
      double   res = 0;
      device_pcg<T>(
        ctx, op0->comm.get(), cg_S.p, n, op0->n_dot(), x, cg_r.p, cg_z.p, cg_p.p, cg_Ap.p, [&](T *Ap, const T *p) { op0->vmult_raw(Ap, p); },
        [&](T *z, const T *r) {
          if (kind == CoarseKind::CgChebyshev)
            sm0->vmult_raw(z, sm0->tmp.p, r);
          else if (kind == CoarseKind::CgAmg)
            amg_cycles(z, r);
          else
            HIP_CHECK(hipMemcpyAsync(z, r, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        },
        1e-4, 1e-20, 10000, its, res);
      iterations += its;
    }

    // the algebraic coarse solver's levels (AmgCycle::layout); empty: no AMG
    void
    layout(std::vector<uint32_t> &out) const
    {
      out.clear();
      if (amg)
        amg->layout(out);
    }
  };

  // ------------------------------------------------------------------------------------------
  // Multigrid V-cycle  (deal.II Multigrid::level_v_step + PreconditionMG::vmult)
  // ------------------------------------------------------------------------------------------
  template <typename T>
  struct MultigridT : MultigridBase
  {
    unsigned                         nl = 0;
    std::vector<LevelOperator<T> *>  ops;
    std::vector<Transfer2<T> *>      tr;
    std::vector<Chebyshev<T> *>      sm;
    std::vector<std::unique_ptr<DBuf<T>>> defect, S, Tb, res; // defect: only the finest level owns memory,
    DBuf<T>                               defect_slab;        // the coarser defects share one slab (ONE memset per cycle)
    std::vector<T *>                      dptr;               // defect vector of every level
    std::vector<T *>                 sol; // where the level solution currently lives
    // per-cycle views of the finest level: when the outer vectors have the level number type, r IS the
    // finest defect and z is one of the two smoother buffers (no copy_to_mg / copy_from_mg traffic)
    std::vector<const T *> dview;
    std::vector<T *>       sview, tview;
    std::unique_ptr<CoarseSolver<T>> coarse; // level 0
    // The V-cycle restricted to levels 0..collapse_level is a fixed linear map of that level's defect (zero start): on
    // levels this small every kernel is pure launch latency, so the map is tabulated once (n unit defects through the
    // regular level code) and applied as ONE dense matvec.  Not used while stage callbacks are installed (the
    // reference's per-level timers need the real stages).
    unsigned     collapse_level = 0;
    DBuf<double> collapse_M;
    bool         collapse_enabled = true;
    bool         fuse_transfers   = true; // level transfers inside the operator passes where the transfer offers them
    unsigned
    set_collapse(bool on) override
    {
      if (collapse_enabled != on)
        drop_graph(); // a captured cycle replays the work enqueued under the old setting
      collapse_enabled = on;
      return collapse_level;
    }
    void
    drop_graph()
    {
      if (graph_exec)
        (void)hipGraphExecDestroy(graph_exec);
      graph_exec = nullptr;
      graph_z = graph_r = nullptr;
    }
    hipGraphExec_t                   graph_exec = nullptr;
    const void                      *graph_z = nullptr, *graph_r = nullptr;

    // Local smoothing (`HMG-local`): the levels are the refinement levels of the octree; the outer vectors live on the
    // ACTIVE mesh and are copied level by level (copy_to_mg / copy_from_mg index pairs, transfer_tables.hpp)
    struct LsCopy
    {
      DBuf<uint32_t> gidx, lidx;
      uint32_t       n = 0;
    };
    std::vector<std::unique_ptr<LsCopy>> ls_copy;
    size_t                               ls_n_global = 0;
    const LevelTables                   *ls_active   = nullptr;
    const LevelTables *
    outer_tables() const override
    {
      return ls_active ? ls_active : ops[nl - 1]->tables.get();
    }
    void
    setup_local_smoothing(const LevelTables &active) override
    {
      if (collapse_level || coarse->kind == CoarseKind::Nested)
        throw std::invalid_argument("local smoothing: not combinable with a nested coarse solver");
      ls_copy.clear();
      std::vector<uint32_t> g, l;
      size_t                total = 0;
      for (unsigned lv = 0; lv < nl; ++lv)
        {
          const LevelTables &T_l = *ops[lv]->tables;
          if (!T_l.ls_level || T_l.tria->cells.empty())
            throw std::invalid_argument("local smoothing: every level must be built with mgamd_dofs_create_level");
          ls_copy_indices(active, T_l, (int)T_l.tria->cells[0].level, g, l);
          auto c = std::make_unique<LsCopy>();
          c->n   = (uint32_t)g.size();
          if (c->n)
            {
              c->gidx.upload(g);
              c->lidx.upload(l);
            }
          total += g.size();
          ls_copy.push_back(std::move(c));
        }
      if (total != (size_t)active.n_interior + active.n_tail)
        throw std::runtime_error("local smoothing: the levels do not cover every unconstrained DoF of the active mesh exactly once");
      ls_n_global = active.n_dofs;
      ls_active   = &active;
      if (!defect[nl - 1]->p)
        defect[nl - 1]->alloc(ops[nl - 1]->n_dofs());
    }
    size_t
    n_outer() const
    {
      return ls_copy.empty() ? (size_t)ops[nl - 1]->n_dofs() : ls_n_global;
    }

    LevelOperatorBase *
    finest_operator() const override
    {
      return ops[nl - 1];
    }
    uint64_t
    coarse_cg_iterations() const override
    {
      return coarse->iterations;
    }
    void
    amg_layout(std::vector<uint32_t> &out) const override
    {
      coarse->layout(out);
    }
    void
    vcycle_level_raw(void *z, const void *r) override
    {
      vcycle_raw<T>(static_cast<T *>(z), static_cast<const T *>(r));
    }

    MultigridT(Ctx *c, unsigned n_levels, LevelOperatorBase *const *levels, Transfer2Base *const *transfers,
               ChebyshevBase *const *smoothers, const std::string &coarse_name, MultigridBase *nested_mg, unsigned nested_cycles,
               const LevelTables *amg_global = nullptr, uint32_t amg_min_sharded_rows = AMG_MIN_SHARDED_ROWS_DEFAULT)
    {
      ctx         = c;
      nl          = n_levels;
      number_type = (int)sizeof(T);
      if (nl < 1)
        throw std::invalid_argument("multigrid: need at least one level");
      for (unsigned l = 0; l < nl; ++l)
        {
          if (!levels[l] || levels[l]->type != (int)sizeof(T))
            throw std::invalid_argument("multigrid: level operators must share one number type");
          ops.push_back(static_cast<LevelOperator<T> *>(levels[l]));
          tr.push_back(l > 0 ? static_cast<Transfer2<T> *>(transfers[l]) : nullptr);
          sm.push_back(smoothers[l] ? static_cast<Chebyshev<T> *>(smoothers[l]) : nullptr);
          if (l > 0 && (!transfers[l] || !smoothers[l]))
            throw std::invalid_argument("multigrid: missing transfer or smoother");
          if (l > 0 && (transfers[l]->fine != levels[l] || transfers[l]->coarse != levels[l - 1]))
            throw std::invalid_argument("multigrid: transfer does not connect the given levels");
          const size_t n = ops[l]->n_dofs();
          defect.emplace_back(new DBuf<T>);
          S.emplace_back(new DBuf<T>);
          Tb.emplace_back(new DBuf<T>);
          res.emplace_back(new DBuf<T>);
          if (l + 1 == nl)
            defect[l]->alloc(n);
          S[l]->alloc(n);
          Tb[l]->alloc(n);
          res[l]->alloc(n);
        }
      {
        // coarser defects: 256-byte aligned pieces of one allocation
        std::vector<size_t> off(nl, 0);
        size_t              total = 0;
        for (unsigned l = 0; l + 1 < nl; ++l)
          {
            off[l] = total;
            total += (ops[l]->n_dofs() + 31) / 32 * 32;
          }
        defect_slab.alloc(std::max<size_t>(total, 1));
        dptr.assign(nl, nullptr);
        for (unsigned l = 0; l + 1 < nl; ++l)
          dptr[l] = defect_slab.p + off[l];
        dptr[nl - 1] = defect[nl - 1]->p;
      }
      sol.assign(nl, nullptr);
      dview.assign(nl, nullptr);
      sview.assign(nl, nullptr);
      tview.assign(nl, nullptr);
      for (unsigned l = 0; l < nl; ++l)
        {
          dview[l] = dptr[l];
          sview[l] = S[l]->p;
          tview[l] = Tb[l]->p;
        }
      // what runs on level 0: resolve_coarse_kind (coarse_policy.hpp) from the name and what the caller supplies, built by CoarseSolver
      coarse = std::make_unique<CoarseSolver<T>>(ctx, ops[0], sm[0], coarse_name, nested_mg, nested_cycles, amg_global, amg_min_sharded_rows);
      coarse_used = coarse_kind_name(coarse->kind);
      setup_collapse();
    }

    void
    setup_collapse()
    {
      size_t max_n = 2048;
      if (const char *e = getenv("MGAMD_COLLAPSE_MAX_DOFS")) // 0 disables
        max_n = (size_t)atol(e);
      for (unsigned l = 0; l < nl; ++l)
        if (ops[l]->tables->ls_level)
          return; // local smoothing: every level also receives its own part of the outer residual
      unsigned lc = 0;
      for (unsigned l = 1; l < nl; ++l)
        if (ops[l]->n_dofs() <= max_n && !ops[l]->comm)
          lc = l;
        else
          break;
      // an iterative coarse solver (cg, cg_with_chebyshev) is not a linear map of its right-hand side
      if (lc == 0 || ops[0]->comm || coarse->kind != CoarseKind::Direct)
        return;
      const size_t        n = ops[lc]->n_dofs();
      std::vector<T>      col(n);
      std::vector<double> M(n * n);
      const T             one = T(1);
      for (size_t j = 0; j < n; ++j)
        {
          // unit defect on level lc (coarser defects zero), the regular cycle below it
          if (lc + 1 == nl) // (the finest defect is not part of the slab)
            HIP_CHECK(hipMemsetAsync(dptr[lc], 0, n * sizeof(T), ctx->stream));
          defect_slab.zero(ctx->stream);
          HIP_CHECK(hipMemcpyAsync(dptr[lc] + j, &one, sizeof(T), hipMemcpyHostToDevice, ctx->stream));
          level_v_step(lc);
          HIP_CHECK(hipMemcpyAsync(col.data(), sol[lc], n * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
          ctx->sync();
          for (size_t r = 0; r < n; ++r)
            M[r * n + j] = (double)col[r];
        }
      collapse_M.upload(M);
      collapse_level = lc;
    }

    ~MultigridT() override
    {
      release_stage_records();
      drop_graph();
    }

    void
    stage(int s, bool start, unsigned level)
    {
      if (cb)
        {
          ctx->sync();
          cb(s, start ? 1 : 0, level, cb_user);
        }
      if (stage_timing)
        {
          if (start)
            {
              if (stage_used == stage_records.size())
                {
                  StageRecord r{s, level, nullptr, nullptr};
                  HIP_CHECK(hipEventCreate(&r.e0));
                  HIP_CHECK(hipEventCreate(&r.e1));
                  stage_records.push_back(r);
                }
              stage_records[stage_used].stage = s;
              stage_records[stage_used].level = level;
              HIP_CHECK(hipEventRecord(stage_records[stage_used].e0, ctx->stream));
            }
          else
            HIP_CHECK(hipEventRecord(stage_records[stage_used++].e1, ctx->stream));
        }
    }
    unsigned
    n_levels() const override
    {
      return nl;
    }

    // the cycle on level vectors; defect[nl-1] must be set, coarser defects zero.  wide_out (float levels under double outer
    // vectors, finest level only): the last post-smoothing pass stores the level solution there as doubles, see vcycle_raw
    void
    level_v_step(unsigned l, double *wide_out = nullptr)
    {
      if (l == 0)
        {
          stage(3, true, 0);
          coarse->solve(S[0]->p, dptr[0]);
          sol[0] = S[0]->p;
          stage(3, false, 0);
          return;
        }
      if (l == collapse_level && !cb && collapse_enabled)
        {
          // the tabulated cycle below this level: timed as the coarse solve of level l
          const size_t n = ops[l]->n_dofs();
          if (stage_timing)
            stage(3, true, l);
          hipLaunchKernelGGL(dense_matvec_kernel<T>, (int)std::min<size_t>(n, 1024), 256, 0, ctx->stream, collapse_M.p, dview[l], sview[l],
                             (int)n);
          if (stage_timing)
            stage(3, false, l);
          sol[l] = sview[l];
          return;
        }
      // level transfers inside the operator passes (Transfer2::fused_ready; not while stage callbacks want the reference's
      // separate stages): stage 1 is then residual + fused restriction, stage 2 the restriction of the remaining patches, stage 4
      // the un-fused prolongation, and the fused prolongation is part of the first post-smoothing pass (stage 6)
      const bool fuse = fuse_transfers && !cb && tr[l]->fused_ready();
      stage(0, true, l);
      sm[l]->vmult_raw(sview[l], tview[l], dview[l]); // pre-smoothing, zero start
      stage(0, false, l);
      stage(1, true, l);
      if (fuse)
        tr[l]->residual_restrict_raw(dptr[l - 1], res[l]->p, dview[l], sview[l]);
      else
        ops[l]->residual_raw(res[l]->p, dview[l], sview[l]); // t = d - A x
      stage(1, false, l);
      stage(2, true, l);
      if (fuse)
        tr[l]->restrict_unfused_raw(dptr[l - 1], res[l]->p);
      else
        tr[l]->restrict_raw(dptr[l - 1], res[l]->p);
      stage(2, false, l);
      level_v_step(l - 1);
      stage(4, true, l);
      if (fuse)
        tr[l]->prolongate_unfused_raw(sview[l], sol[l - 1]);
      else
        tr[l]->prolongate_raw(sview[l], sol[l - 1]);
      stage(4, false, l);
      stage(5, true, l); // edge_prolongation: no-op for global coarsening (ref:multigrid_throughput.cc:1126-1130)
      if (ops[l]->tables->n_edge)
        {
          // local smoothing, Multigrid::set_edge_in_matrix (ref:multigrid_throughput.cc:1105,1130): the corrected solution on
          // the refinement edge couples into the interior: defect_l -= A_l^{edge unconstrained} (x_l restricted to the edge)
          const size_t n = ops[l]->n_dofs();
          ops[l]->interface_up_raw(res[l]->p, sview[l], tview[l]);
          hipLaunchKernelGGL(vec_sadd_kernel<T>, grid_for(n), 256, 0, ctx->stream, dptr[l], T(1), T(-1), res[l]->p, n);
        }
      stage(5, false, l);
      stage(6, true, l);
      if (fuse)
        {
          FusedTransferHost<T> f = tr[l]->fused;
          f.coarse               = sol[l - 1];
          f.scratch              = res[l]->p; // the residual vector is free again
          sol[l]                 = sm[l]->step_raw(sview[l], tview[l], dview[l], &f, wide_out);
        }
      else
        sol[l] = sm[l]->step_raw(sview[l], tview[l], dview[l], nullptr, wide_out); // post-smoothing
      stage(6, false, l);
    }

    template <typename TO>
    void
    vcycle_ls_raw(TO *z, const TO *r)
    {
      const unsigned L = nl - 1;
      stage(7, true, L); // copy_to_mg: every level receives the residual entries of ITS active cells
      if (nl > 1)
        defect_slab.zero(ctx->stream);
      HIP_CHECK(hipMemsetAsync(dptr[L], 0, (size_t)ops[L]->n_dofs() * sizeof(T), ctx->stream));
      dview[L] = dptr[L];
      sview[L] = S[L]->p;
      tview[L] = Tb[L]->p;
      for (unsigned l = 0; l < nl; ++l)
        if (ls_copy[l]->n)
          hipLaunchKernelGGL((indexed_copy_kernel<T, TO>), grid_for(ls_copy[l]->n), 256, 0, ctx->stream, dptr[l], ls_copy[l]->lidx.p, r,
                             ls_copy[l]->gidx.p, ls_copy[l]->n);
      stage(7, false, L);
      level_v_step(L);
      stage(8, true, L); // copy_from_mg
      HIP_CHECK(hipMemsetAsync(z, 0, ls_n_global * sizeof(TO), ctx->stream));
      for (unsigned l = 0; l < nl; ++l)
        if (ls_copy[l]->n)
          hipLaunchKernelGGL((indexed_copy_kernel<TO, T>), grid_for(ls_copy[l]->n), 256, 0, ctx->stream, z, ls_copy[l]->gidx.p,
                             (const T *)sol[l], ls_copy[l]->lidx.p, ls_copy[l]->n);
      stage(8, false, L);
      HIP_CHECK(hipGetLastError());
    }

    template <typename TO>
    void
    vcycle_raw(TO *z, const TO *r)
    {
      if (!ls_copy.empty())
        {
          vcycle_ls_raw<TO>(z, r);
          return;
        }
      const size_t   n    = ops[nl - 1]->n_dofs();
      const unsigned L    = nl - 1;
      const bool     same = sizeof(TO) == sizeof(T) && nl > 1;
      // copy_to_mg: defect_L = cast(r), coarser defects zero
      stage(7, true, L);
      if (same)
        {
          // r is the finest defect; z takes the role of the smoother buffer the post-smoother ends in
          // (Chebyshev::step_raw returns its second buffer for odd degree, the first for even degree)
          dview[L] = reinterpret_cast<const T *>(r);
          if (sm[L]->degree % 2 == 1)
            {
              sview[L] = S[L]->p;
              tview[L] = reinterpret_cast<T *>(z);
            }
          else
            {
              sview[L] = reinterpret_cast<T *>(z);
              tview[L] = S[L]->p;
            }
        }
      else
        {
          dview[L] = defect[L]->p;
          sview[L] = S[L]->p;
          tview[L] = Tb[L]->p;
          hipLaunchKernelGGL((vec_copy_kernel<T, TO>), grid_for(n), 256, 0, ctx->stream, defect[L]->p, r, n);
        }
      if (nl > 1)
        defect_slab.zero(ctx->stream);
      stage(7, false, L);
      // copy_from_mg inside the last post-smoothing pass (Epilogue::out_wide): float levels, double outer vectors, a smoother of
      // degree >= 2 (its last pass is a plain Chebyshev pass), no stage callbacks (they want the reference's separate stages)
      double *wide_out = nullptr;
      if constexpr (sizeof(T) == 4 && sizeof(TO) == 8)
        if (nl > 1 && !cb)
          wide_out = reinterpret_cast<double *>(z);
      level_v_step(L, wide_out);
      stage(8, true, L);
      // (sol[L] == nullptr: the last smoothing pass has written z; a collapsed finest level leaves its result in a level vector)
      if (sol[L] != nullptr && (const void *)sol[L] != (const void *)z)
        hipLaunchKernelGGL((vec_copy_kernel<TO, T>), grid_for(n), 256, 0, ctx->stream, z, sol[L], n);
      stage(8, false, L);
    }

    void
    vcycle(mgamd_vec &z, const mgamd_vec &r) override
    {
      const size_t n = n_outer();
      if (z.n != n || r.n != n || z.type != r.type || z.data == r.data)
        throw std::invalid_argument("PreconditionMG::vmult: bad vectors");
      if (z.type == MGAMD_F64)
        vcycle_raw<double>(z.as<double>(), r.as<double>());
      else
        vcycle_raw<float>(z.as<float>(), r.as<float>());
    }

    double
    time_vcycles(mgamd_vec &z, const mgamd_vec &r, unsigned n, bool use_graph) override
    {
      if (n == 0)
        return 0.0;
      if (cb || stage_timing)
        throw std::invalid_argument("time_vcycles: remove the stage callback / stage timing first");
      const bool graphable = coarse->kind == CoarseKind::Direct && !ops[nl - 1]->comm; // (nested cycles are not captured)
      vcycle(z, r); // warm-up: sets kernel attributes, touches memory
      ctx->sync();
      if (use_graph && graphable && (!graph_exec || graph_z != z.data || graph_r != r.data))
        {
          drop_graph();
          hipGraph_t graph;
          HIP_CHECK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
          const bool saved = ctx->profile;
          ctx->profile     = false;
          try
            {
              vcycle(z, r);
            }
          catch (...)
            {
              ctx->profile = saved;
              (void)hipStreamEndCapture(ctx->stream, &graph);
              throw;
            }
          ctx->profile = saved;
          HIP_CHECK(hipStreamEndCapture(ctx->stream, &graph));
          HIP_CHECK(hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0));
          HIP_CHECK(hipGraphDestroy(graph));
          graph_z = z.data;
          graph_r = r.data;
          HIP_CHECK(hipGraphLaunch(graph_exec, ctx->stream));
          ctx->sync();
        }
      hipEvent_t e0, e1;
      HIP_CHECK(hipEventCreate(&e0));
      HIP_CHECK(hipEventCreate(&e1));
      HIP_CHECK(hipEventRecord(e0, ctx->stream));
      for (unsigned i = 0; i < n; ++i)
        {
          if (use_graph && graphable)
            HIP_CHECK(hipGraphLaunch(graph_exec, ctx->stream));
          else
            vcycle(z, r);
        }
      HIP_CHECK(hipEventRecord(e1, ctx->stream));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      return (double)ms / n;
    }
  };

  MultigridBase *
  make_multigrid(Ctx *ctx, unsigned n_levels, LevelOperatorBase *const *levels, Transfer2Base *const *transfers,
                 ChebyshevBase *const *smoothers, const std::string &coarse_solver, MultigridBase *nested, unsigned n_cycles,
                 const LevelTables *amg_global, uint32_t amg_min_sharded_rows)
  {
    if (!n_levels || !levels || !levels[0])
      throw std::invalid_argument("multigrid: no levels");
    for (unsigned l = 0; l < n_levels; ++l)
      if (levels[l])
        levels[l]->refuse_singular("multigrid");
    if (levels[0]->type == MGAMD_F64)
      return new MultigridT<double>(ctx, n_levels, levels, transfers, smoothers, coarse_solver, nested, n_cycles, amg_global,
                                    amg_min_sharded_rows);
    return new MultigridT<float>(ctx, n_levels, levels, transfers, smoothers, coarse_solver, nested, n_cycles, amg_global,
                                 amg_min_sharded_rows);
  }

  // ------------------------------------------------------------------------------------------
  // Outer solver: deal.II SolverCG + ReductionControl (ref:multigrid_throughput.cc:1140-1147,1625-1635)
  // ------------------------------------------------------------------------------------------
  template <typename T>
  static void
  solve_cg_T(LevelOperatorBase &A, MultigridBase *M, mgamd_vec &x, const mgamd_vec &b, double reltol, double abstol, unsigned maxiter,
             unsigned &n_iterations, double &residual)
  {
    Ctx         *ctx = A.ctx;
    const size_t n   = A.n_dofs();
    auto        *op  = static_cast<LevelOperator<T> *>(&A);
    std::unique_ptr<mgamd_vec> g(vec_create(ctx, n, A.type)), h(vec_create(ctx, n, A.type)), d(vec_create(ctx, n, A.type)),
      Ad(vec_create(ctx, n, A.type));
    vec_copy(*g, b); // residual r = b - A*0; dst = 0 (ref:multigrid_throughput.cc:1142,1245) is set by device_pcg
    // the V-cycle works on whole vectors (it may alias them as level buffers): hand it the mgamd_vec objects
    device_pcg<T>(
      ctx, op->comm.get(), ctx->d_cg, n, op->n_dot(), x.as<T>(), g->as<T>(), h->as<T>(), d->as<T>(), Ad->as<T>(), [&](T *Ap, const T *p) { op->vmult_raw(Ap, p); },
      [&](T *z, const T *r) {
        (void)z;
        (void)r;
        if (M)
          M->vcycle(*h, *g);
        else
          vec_copy(*h, *g);
      },
      reltol, abstol, maxiter, n_iterations, residual);
    ctx->sync();
  }

  void
  solve_cg(LevelOperatorBase &A, MultigridBase *M, mgamd_vec &x, const mgamd_vec &b, double reltol, double abstol, unsigned maxiter,
           unsigned &n_iterations, double &residual)
  {
    const size_t n = A.n_dofs();
    if (x.n != n || b.n != n || x.type != A.type || b.type != A.type)
      throw std::invalid_argument("SolverCG::solve: bad vectors");
    A.refuse_singular("SolverCG::solve");
    if (A.type == MGAMD_F64)
      solve_cg_T<double>(A, M, x, b, reltol, abstol, maxiter, n_iterations, residual);
    else
      solve_cg_T<float>(A, M, x, b, reltol, abstol, maxiter, n_iterations, residual);
  }

  // ------------------------------------------------------------------------------------------
  // theta time stepper (runtime.hpp, ThetaStepperBase).  The outer solve is FP64, as in solve_cg.
  // ------------------------------------------------------------------------------------------
  struct ThetaStepper : ThetaStepperBase
  {
    LevelOperator<double>     *op;
    MultigridBase             *M;
    std::unique_ptr<mgamd_vec> g, h, d, Ad, delta; // the PCG's r, z, p, A p and x; d and Ad also hold t and w before the solve

    ThetaStepper(LevelOperatorBase &A, MultigridBase *mg, double theta_, double dt_)
      : M(mg)
    {
      theta = theta_;
      dt    = dt_;
      if (!(theta > 0.0 && theta <= 1.0) || !std::isfinite(theta))
        throw std::invalid_argument("time stepper: theta = " + std::to_string(theta) + " is not in (0, 1]");
      if (!(dt > 0.0) || !std::isfinite(dt))
        throw std::invalid_argument("time stepper: dt = " + std::to_string(dt) + " is not a positive finite step");
      if (A.type != MGAMD_F64)
        throw std::invalid_argument("time stepper: the operator is not FP64 (the outer solve is FP64; FP32 belongs to the levels of the "
                                    "multigrid)");
      if (A.tables->ls_level)
        throw std::invalid_argument("time stepper: the operator of a local-smoothing level has no mass matrix (vmult_mass)");
      if (std::fabs(A.sigma * theta * dt - 1.0) > 1e-12)
        {
          char buf[256];
          snprintf(buf, sizeof buf,
                   "time stepper: the operator's mass coefficient sigma = %.17g is not 1 / (theta dt) for theta = %.17g, dt = %.17g "
                   "(build the hierarchy with mass_coefficient(theta, dt))",
                   A.sigma, theta, dt);
          throw std::invalid_argument(buf);
        }
      op             = static_cast<LevelOperator<double> *>(&A);
      const size_t n = A.n_dofs();
      for (auto *v : {&g, &h, &d, &Ad, &delta})
        v->reset(vec_create(A.ctx, n, MGAMD_F64));
    }

    void
    step(mgamd_vec &u, const mgamd_vec *f_old, const mgamd_vec *f_new, double reltol, double abstol, unsigned maxiter, unsigned &n_iterations,
         double &residual) override
    {
      step_data(u, f_old, f_new, nullptr, nullptr, nullptr, reltol, abstol, maxiter, n_iterations, residual);
    }

    // r += the lifting of gd (dirichlet_lift_kernel, alpha = -1).  One rank: straight into r.  Sharded: through the work vector Ad
    // (free after the residual pass) and the exchange, as r is already complete over the ranks.
    void
    add_lift(const double *gd, bool include_mass)
    {
      if (!op->halo)
        return op->dirichlet_lift_add_raw(g->as<double>(), gd, include_mass, -1.0);
      op->rhs_dirichlet_raw(Ad->as<double>(), gd, include_mass);
      vec_sadd(*g, 1.0, 1.0, *Ad);
    }

    void
    step_data(mgamd_vec &u, const mgamd_vec *f_old, const mgamd_vec *f_new, const mgamd_vec *g_old, const mgamd_vec *g_new, const mgamd_vec *load,
              double reltol, double abstol, unsigned maxiter, unsigned &n_iterations, double &residual) override
    {
      Ctx         *ctx = op->ctx;
      const size_t n   = op->n_dofs();
      if ((f_old == nullptr) != (f_new == nullptr))
        throw std::invalid_argument("time stepper: exactly one of f_old / f_new is given (both, or neither for f = 0)");
      if ((g_old == nullptr) != (g_new == nullptr))
        throw std::invalid_argument("time stepper: exactly one of g_old / g_new is given (both, or neither for homogeneous Dirichlet data)");
      for (const mgamd_vec *v : {(const mgamd_vec *)&u, f_old, f_new, g_old, g_new, load})
        if (v && (v->n != n || v->type != MGAMD_F64))
          throw std::invalid_argument("time stepper: a vector of " + std::to_string(v->n) + " entries of " + std::to_string(v->type) +
                                      " bytes where the operator has " + std::to_string(n) + " FP64 DoFs");
      if (g_old)
        op->tables->refuse_dirichlet_lift("time stepper");
      const size_t n_free = (size_t)op->tables->n_interior + op->tables->n_tail; // the constrained DoFs are numbered last
      const int    grid   = grid_for(n);
      double      *up     = u.as<double>();
      hipLaunchKernelGGL(theta_source_kernel<double>, grid, 256, 0, ctx->stream, Ad->as<double>(), up, f_old ? f_old->as<double>() : nullptr,
                         f_new ? f_new->as<double>() : nullptr, theta, op->sigma, n);
      op->vmult_mass_raw(d->as<double>(), Ad->as<double>());
      op->residual_raw(g->as<double>(), d->as<double>(), up);
      // the data terms (DESIGN.md "Dirichlet data"): r = M w + l - A u - K_ID g_old, then r / theta - A_ID (g_new - g_old)
      if (load)
        vec_sadd(*g, 1.0, 1.0, *load);
      if (g_old)
        add_lift(g_old->as<double>(), false);
      hipLaunchKernelGGL(theta_rhs_kernel<double>, grid, 256, 0, ctx->stream, g->as<double>(), theta, n_free, n);
      if (g_old)
        {
          vec_copy(*d, *g_new);
          vec_sadd(*d, 1.0, -1.0, *g_old);
          add_lift(d->as<double>(), true);
        }
      device_pcg<double>(
        ctx, op->comm.get(), ctx->d_cg, n, op->n_dot(), delta->as<double>(), g->as<double>(), h->as<double>(), d->as<double>(), Ad->as<double>(),
        [&](double *Ap, const double *p) { op->vmult_raw(Ap, p); },
        [&](double *, const double *) {
          if (M)
            M->vcycle(*h, *g);
          else
            vec_copy(*h, *g);
        },
        reltol, abstol, maxiter, n_iterations, residual);
      hipLaunchKernelGGL(theta_update_kernel<double>, grid, 256, 0, ctx->stream, up, delta->as<double>(), n_free, n);
      HIP_CHECK(hipGetLastError());
      ctx->sync();
      t += dt;
      ++n_steps;
    }
  };

  ThetaStepperBase *
  make_theta_stepper(LevelOperatorBase &A, MultigridBase *M, double theta, double dt)
  {
    A.refuse_singular("time stepper");
    return new ThetaStepper(A, M, theta, dt);
  }

  // ------------------------------------------------------------------------------------------
  // Type "AMG": SolverCG on the assembled system matrix, preconditioned by the AMG built on it (solve_with_amg,
  // ref:multigrid_throughput.cc:1877-1966).  The matrix lives once on the device: the operator's products and level 0 of the
  // cycle read the same arrays.  Rows of the fine-level matrix at degree 2-4 hold hundreds of entries: K8 above
  // CSR_SPMV_WAVE_MIN_MEAN_ROW, K7 below (degree 1).  The host copy stays: the AMG setup (amg.hpp) starts from it.
  // ------------------------------------------------------------------------------------------
  struct AssembledMatrix : AssembledMatrixBase
  {
    using Mat = AmgCycle<double>::Mat;
    std::shared_ptr<const CSR> host;
    std::shared_ptr<Mat>       dev;
    AssembledMatrix(Ctx *c, const mgamd_dofs *dofs)
    {
      ctx = c;
      if (dofs->halo)
        throw std::invalid_argument("assembled matrix: the level is distributed (one rank only)");
      host   = std::make_shared<const CSR>(assemble_level_matrix(*dofs->tables)); // (refuses local-smoothing levels)
      n_rows = host->n_rows;
      nnz    = host->nnz();
      lanes  = csr_spmv_lanes_long(n_rows, nnz);
      dev    = std::make_shared<Mat>();
      dev->upload(*host);
      dev->lanes = lanes;
    }
    template <int MODE>
    int
    spmv(const double *x, double *y, const double *b = nullptr, double *partial = nullptr) const
    {
      return launch_csr_spmv<double>(ctx->stream, MODE, lanes, n_rows, dev->ptr.p, dev->col.p, dev->val.p, x, y, b, nullptr, nullptr, 0, 0,
                                     partial);
    }
    void
    check(const mgamd_vec &v) const
    {
      if (v.n != n_rows)
        throw std::invalid_argument("assembled matrix: vector size mismatch");
      if (v.type != MGAMD_F64)
        throw std::invalid_argument("assembled matrix: vectors must be MGAMD_F64 (the reference runs this path in double)");
    }
    void
    vmult(mgamd_vec &dst, const mgamd_vec &src) override
    {
      check(dst);
      check(src);
      if (dst.data == src.data)
        throw std::invalid_argument("assembled matrix: vmult in place");
      spmv<SPMV_PLAIN>(src.as<double>(), dst.as<double>());
    }
    double
    time_spmv(int mode, int lanes_, unsigned reps) override
    {
      if (!reps || !n_rows)
        throw std::invalid_argument("time_spmv: nothing to time");
      std::vector<double> h(n_rows);
      for (uint32_t i = 0; i < n_rows; ++i)
        h[i] = 1.0 / (1.0 + (double)(i % 7));
      DBuf<double> x, y, b, dinv;
      for (DBuf<double> *v : {&x, &y, &b, &dinv})
        v->upload(h);
      auto launch = [&] {
        launch_csr_spmv<double>(ctx->stream, mode, lanes_, n_rows, dev->ptr.p, dev->col.p, dev->val.p, x.p, y.p, b.p, nullptr, dinv.p, 0.25, 0.5,
                                ctx->d_partial);
      };
      hipEvent_t e0, e1;
      HIP_CHECK(hipEventCreate(&e0));
      HIP_CHECK(hipEventCreate(&e1));
      launch();
      HIP_CHECK(hipEventRecord(e0, ctx->stream));
      for (unsigned r = 0; r < reps; ++r)
        launch();
      HIP_CHECK(hipEventRecord(e1, ctx->stream));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      return (double)ms / reps;
    }
    // Ap = A p, *out = p . Ap: one pass over the matrix, the block partials summed by vec_dot_final_kernel
    void
    vmult_dot(double *Ap, const double *p, double *out) const
    {
      const int g = spmv<SPMV_DOT>(p, Ap, nullptr, ctx->d_partial);
      hipLaunchKernelGGL(vec_dot_final_kernel<>, 1, 256, 0, ctx->stream, ctx->d_partial, g, out);
    }
  };

  struct AmgPreconditioner : AmgPreconditionerBase
  {
    std::shared_ptr<AssembledMatrix> A;
    AmgCycle<double>                 cycle;
    unsigned                         n_cycles;
    DBuf<double>                     rr, zz; // n_cycles > 1: residual and correction
    AmgPreconditioner(std::shared_ptr<AssembledMatrix> a, unsigned n)
      : A(std::move(a))
      , cycle(A->ctx, *A->host, A->dev)
      , n_cycles(n)
    {
      if (n_cycles > 1)
        {
          rr.alloc(A->n_rows);
          zz.alloc(A->n_rows);
        }
    }
    // z = V(r), then n_cycles - 1 corrections z += V(r - A z) (ML's `cycle applications`)
    void
    apply_raw(double *z, const double *r)
    {
      repeat_cycles<double>(
        A->ctx->stream, n_cycles, [&](double *zc, const double *rc) { cycle.vcycle(zc, rc); },
        [&](double *res, const double *b, const double *x) { A->spmv<SPMV_RESID>(x, res, b); }, z, r, rr.p, zz.p, A->n_rows);
      HIP_CHECK(hipGetLastError());
    }
    void
    vmult(mgamd_vec &z, const mgamd_vec &r) override
    {
      A->check(z);
      A->check(r);
      if (z.data == r.data)
        throw std::invalid_argument("AMG preconditioner: vmult in place");
      apply_raw(z.as<double>(), r.as<double>());
    }
    void
    layout(std::vector<uint32_t> &rows_per_level) const override
    {
      rows_per_level.clear();
      for (const auto &L : cycle.lv)
        rows_per_level.push_back(L->n_global);
    }
  };

  std::shared_ptr<AssembledMatrixBase>
  make_assembled_matrix(Ctx *ctx, const mgamd_dofs *dofs)
  {
    dofs->tables->refuse_singular("assembled matrix (Type AMG)");
    return std::make_shared<AssembledMatrix>(ctx, dofs);
  }
  AmgPreconditionerBase *
  make_amg_preconditioner(const std::shared_ptr<AssembledMatrixBase> &A, unsigned n_cycles)
  {
    if (n_cycles == 0)
      throw std::invalid_argument("AMG preconditioner: n_cycles must be at least 1");
    return new AmgPreconditioner(std::static_pointer_cast<AssembledMatrix>(A), n_cycles);
  }

  void
  solve_cg_matrix(AssembledMatrixBase &Ab, AmgPreconditionerBase *Mb, mgamd_vec &x, const mgamd_vec &b, double reltol, double abstol,
                  unsigned maxiter, unsigned &n_iterations, double &residual)
  {
    auto &A = static_cast<AssembledMatrix &>(Ab);
    auto *M = static_cast<AmgPreconditioner *>(Mb);
    A.check(x);
    A.check(b);
    if (M && M->A.get() != &A)
      throw std::invalid_argument("SolverCG::solve: the AMG preconditioner was built on another matrix");
    Ctx         *ctx = A.ctx;
    const size_t n   = A.n_rows;
    if (!n)
      {
        n_iterations = 0;
        residual     = 0;
        return;
      }
    DBuf<double> g, h, d, Ad;
    for (DBuf<double> *v : {&g, &h, &d, &Ad})
      v->alloc(n);
    HIP_CHECK(hipMemcpyAsync(g.p, b.data, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    std::function<void(double *, const double *, double *)> fused;
    if (getenv("MGAMD_NO_FUSED_DOT") == nullptr)
      fused = [&](double *Ap, const double *p, double *out) { A.vmult_dot(Ap, p, out); };
    device_pcg<double>(
      ctx, nullptr, ctx->d_cg, n, n, x.as<double>(), g.p, h.p, d.p, Ad.p, [&](double *Ap, const double *p) { A.spmv<SPMV_PLAIN>(p, Ap); },
      [&](double *z, const double *r) {
        if (M)
          M->apply_raw(z, r);
        else
          HIP_CHECK(hipMemcpyAsync(z, r, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
      },
      reltol, abstol, maxiter, n_iterations, residual, fused);
    ctx->sync();
  }
} // namespace mgamd
