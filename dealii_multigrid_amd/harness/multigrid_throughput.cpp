// multigrid_throughput -- JSON-in / table-out harness of the MI355X-native path, mirroring the reference's
// driver (ref:multigrid_throughput.cc:1970-2470): same 17 JSON keys (RunParameters::parse, :1989-2014), same
// run protocol (1 warm-up solve, then n_repetitions = 5 timed solves, best time wins, :1140-1147,1238-1268),
// same table columns in the same order (:2328-2335, 1488, 1278-1283, 1381-1401).
//
//   ./multigrid_throughput input_0000.json [input_0001.json ...]
//
// Implemented `Type`s: HMG-global, PMG, HPMG (global coarsening), HMG-local and HPMG-local (local smoothing).  AMG/AMGPETSc
// raise "not implemented" exactly like the reference's AssertThrow(false, ExcNotImplemented()) for unknown strings.
#include "../csrc/mgamd.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <map>
#include <sstream>

using namespace mgamd;

// ---- ScopedTimer (ref:include/scoped_timer.h:1-20) ---------------------------------------------------------
class ScopedTimer
{
public:
  explicit ScopedTimer(double &result)
    : result(result)
    , start(std::chrono::system_clock::now())
  {}
  ~ScopedTimer()
  {
    result += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::system_clock::now() - start).count() / 1e9;
  }

private:
  double                                            &result;
  std::chrono::time_point<std::chrono::system_clock> start;
};

// ---- minimal JSON object reader (flat object; values: string | number | true | false) ----------------------
static std::map<std::string, std::string>
parse_json_object(const std::string &file_name)
{
  std::ifstream f(file_name);
  if (!f)
    throw std::runtime_error("cannot open " + file_name);
  std::stringstream ss;
  ss << f.rdbuf();
  const std::string                  s = ss.str();
  std::map<std::string, std::string> out;
  size_t                             i = 0;
  auto skip = [&]() {
    while (i < s.size() && (isspace((unsigned char)s[i]) || s[i] == ',' || s[i] == ':'))
      ++i;
  };
  auto read_string = [&]() {
    std::string r;
    ++i;
    while (i < s.size() && s[i] != '"')
      {
        if (s[i] == '\\' && i + 1 < s.size())
          ++i;
        r += s[i++];
      }
    ++i;
    return r;
  };
  skip();
  if (i >= s.size() || s[i] != '{')
    throw std::runtime_error(file_name + ": not a JSON object");
  ++i;
  while (true)
    {
      skip();
      if (i >= s.size() || s[i] == '}')
        break;
      if (s[i] != '"')
        throw std::runtime_error(file_name + ": expected a key");
      const std::string key = read_string();
      skip();
      std::string value;
      if (s[i] == '"')
        value = read_string();
      else
        while (i < s.size() && s[i] != ',' && s[i] != '}' && !isspace((unsigned char)s[i]))
          value += s[i++];
      out[key] = value;
    }
  return out;
}

// ---- parameters (ref:multigrid_throughput.cc:297-334, 1970-2015) -------------------------------------------
struct MultigridParameters
{
  struct
  {
    std::string type    = "amg";
    unsigned    maxiter = 10000;
    double      abstol  = 1e-20;
    double      reltol  = 1e-4;
    unsigned    n_cycles = 1;
  } coarse_solver;
  struct
  {
    double   smoothing_range     = 20;
    unsigned degree              = 5;
    unsigned eig_cg_n_iterations = 20;
  } smoother;
  struct
  {
    unsigned maxiter = 10000;
    double   abstol  = 1e-20;
    double   reltol  = 1e-4;
  } cg_normal;
  unsigned n_repetitions = 5;
};

struct RunParameters
{
  std::string  type            = "PMG";
  std::string  geometry_type   = "quadrant_flexible";
  unsigned     n_ref_global    = 6;
  unsigned     n_ref_local     = 0;
  unsigned     fe_degree_fine  = 4;
  bool         paraview        = false;
  bool         verbose         = true;
  unsigned     p               = 0;
  std::string  policy_name     = "";
  std::string  mg_number_type  = "float";
  std::string  simulation_type = "Constant";
  int          min_level       = -1;
  int          min_n_cells     = -1;
  // this project's extensions (sharded runs): "ShardedAMG": true runs the AMG coarse solvers on a sharded coarse level as the
  // library's smoothed-aggregation AMG cut into rows over the ranks instead of the geometric stand-in; default false
  bool         sharded_amg          = false;
  unsigned     amg_min_sharded_rows = MGAMD_AMG_MIN_SHARDED_ROWS_DEFAULT;
  // this project's extension: "MassCoefficient": sigma >= 0 solves -Laplace u + sigma u = f (the operator K + sigma M); default 0,
  // the reference's Laplace problem.  The local-smoothing Types have no mass term: a non-zero value is "not implemented" there.
  double       mass_coefficient     = 0.0;
  // this project's extension: "NeumannFaces": a string of face digits such as "1" or "024" (face f = 2 axis + side: 0 is x = -1,
  // 1 is x = +1, ... 5 is z = +1): those faces are natural (zero flux), the others stay Dirichlet; default "", the reference's
  // boundary id 0 on the whole surface (ref:multigrid_throughput.cc:1585-1593).  Refused for the local-smoothing Types, and for
  // all six faces with MassCoefficient 0 (the singular pure-Neumann problem).
  std::string  neumann_faces        = "";
  // this project's extension: "RobinCoefficients": six comma-separated numbers beta_f >= 0, one per face in the numbering above (a
  // string because this parser is flat), such as "2.5,0,0,0.75,0,0": face f is convective, a grad u . n + beta_f u = 0, where
  // beta_f > 0; such a face must be listed in NeumannFaces.  Default "": no convective face.  Refused for the local-smoothing Types.
  std::string  robin_coefficients   = "";
  MultigridParameters mg_data;

  unsigned
  dirichlet_faces() const
  {
    unsigned mask = 0x3F;
    for (const char c : neumann_faces)
      {
        if (c < '0' || c > '5')
          throw std::runtime_error("NeumannFaces '" + neumann_faces + "': not implemented (a string of face digits 0 to 5)");
        mask &= ~(1u << (c - '0'));
      }
    return mask;
  }

  std::array<double, 6>
  robin() const
  {
    std::array<double, 6> beta{};
    if (robin_coefficients.empty())
      return beta;
    const std::string what = "RobinCoefficients '" + robin_coefficients + "': not implemented (six comma-separated numbers >= 0)";
    std::stringstream in(robin_coefficients);
    std::string       item;
    int               f = 0;
    while (std::getline(in, item, ','))
      {
        size_t used = 0;
        double v    = -1.0;
        try
          {
            v = std::stod(item, &used);
          }
        catch (const std::exception &)
          {
            throw std::runtime_error(what);
          }
        if (f >= 6 || item.find_first_not_of(" \t", used) != std::string::npos || !(v >= 0.0) || !std::isfinite(v))
          throw std::runtime_error(what);
        beta[f++] = v;
      }
    if (f != 6)
      throw std::runtime_error(what);
    return beta;
  }

  void
  parse(const std::string &file_name)
  {
    const auto kv  = parse_json_object(file_name);
    auto       get = [&](const char *k, auto &dst) {
      auto it = kv.find(k);
      if (it == kv.end())
        return;
      using D = std::decay_t<decltype(dst)>;
      if constexpr (std::is_same<D, std::string>::value)
        dst = it->second;
      else if constexpr (std::is_same<D, bool>::value)
        dst = it->second == "true" || it->second == "1";
      else if constexpr (std::is_floating_point<D>::value)
        dst = std::stod(it->second);
      else
        dst = (D)std::stol(it->second);
    };
    get("Type", type);
    get("GeometryType", geometry_type);
    get("NRefGlobal", n_ref_global);
    get("NRefLocal", n_ref_local);
    get("Degree", fe_degree_fine);
    get("Paraview", paraview);
    get("Verbosity", verbose);
    get("Partitioner", p);
    get("PartitionerName", policy_name);
    get("MinLevel", min_level);
    get("MinNCells", min_n_cells);
    get("CoarseGridSolverType", mg_data.coarse_solver.type);
    get("SmootherDegree", mg_data.smoother.degree);
    get("CoarseSolverNCycles", mg_data.coarse_solver.n_cycles);
    get("RelativeTolerance", mg_data.cg_normal.reltol);
    get("MGNumberType", mg_number_type);
    get("ShardedAMG", sharded_amg);
    get("AMGMinShardedRows", amg_min_sharded_rows);
    get("MassCoefficient", mass_coefficient);
    get("NeumannFaces", neumann_faces);
    get("RobinCoefficients", robin_coefficients);
    get("SimulationType", simulation_type); // unknown keys are ignored (skip_undefined = true)
  }
};

// ---- ConvergenceTable stand-in -------------------------------------------------------------------------------
class ConvergenceTable
{
public:
  template <typename V>
  void
  add_value(const std::string &key, const V &value, bool scientific = false)
  {
    std::ostringstream os;
    if constexpr (std::is_arithmetic<V>::value)
      {
        if (scientific)
          os << std::scientific << std::setprecision(4) << (double)value;
        else
          os << value;
      }
    else
      os << value;
    if (std::find(order.begin(), order.end(), key) == order.end())
      order.push_back(key);
    columns[key].push_back(os.str());
  }
  void
  write_text(std::ostream &out) const
  {
    std::vector<size_t> w;
    size_t              rows = 0;
    for (const auto &k : order)
      {
        size_t m = k.size();
        for (const auto &v : columns.at(k))
          m = std::max(m, v.size());
        w.push_back(m);
        rows = std::max(rows, columns.at(k).size());
      }
    for (size_t c = 0; c < order.size(); ++c)
      out << std::left << std::setw(w[c] + 1) << order[c];
    out << "\n";
    for (size_t r = 0; r < rows; ++r)
      {
        for (size_t c = 0; c < order.size(); ++c)
          {
            const auto &col = columns.at(order[c]);
            out << std::left << std::setw(w[c] + 1) << (r < col.size() ? col[r] : "");
          }
        out << "\n";
      }
    out << std::flush;
  }

private:
  std::vector<std::string>                        order;
  std::map<std::string, std::vector<std::string>> columns;
};

static std::string
resolve_policy_name(const RunParameters &params)
{
  // ref:multigrid_throughput.cc:2074-2105
  if (!params.policy_name.empty())
    return params.policy_name;
  static const char *names[] = {"DefaultPolicy", "MinimalGranularityPolicy-40", "CellWeightPolicy-1.0", "CellWeightPolicy-1.5",
                                "CellWeightPolicy-2.0", "CellWeightPolicy-2.5", "FirstChildPolicy", "BalancedGranularityPartitionPolicy"};
  if (params.p > 7)
    throw std::runtime_error("Partitioner: not implemented");
  return names[params.p];
}

// comm != nullptr: the run is SHARDED over comm->n_ranks() GPUs, one rank per GPU (the reference's MPI ranks,
// ref:multigrid_throughput.cc:2403-2442): spatial domain decomposition of the level hierarchy (mgamd.hpp Partition), halo
// exchange and coarse-level all-reduce over RCCL inside the library.  Implemented for Type "HMG-global" (BASELINE configs[3]).
static void
run(const Context &ctx, const RunParameters &params, ConvergenceTable &table, const Communicator *comm = nullptr)
{
  const std::string policy = resolve_policy_name(params);
  {
    // the partitioning policy only matters across ranks; validate the name like ref:multigrid_throughput.cc:2127-2174
    auto pre = [&](const char *x) { return policy.rfind(x, 0) == 0; };
    if (!(policy == "DefaultPolicy" || policy == "BalancedGranularityPartitionPolicy" || pre("MinimalGranularityPolicy") ||
          pre("CellWeightPolicy") || pre("FirstChildPolicy")))
      throw std::runtime_error("PartitionerName '" + policy + "': not implemented");
  }
  int simulation_kind; // ref:multigrid_throughput.cc:2286-2300
  if (params.simulation_type == "Constant")
    simulation_kind = 0;
  else if (params.simulation_type == "Gaussian")
    simulation_kind = 1;
  else
    throw std::runtime_error("SimulationType '" + params.simulation_type + "': not implemented");
  int level_number_type;
  if (params.mg_number_type == "double")
    level_number_type = MGAMD_F64;
  else if (params.mg_number_type == "float")
    level_number_type = MGAMD_F32;
  else
    throw std::runtime_error("MGNumberType '" + params.mg_number_type + "': not implemented");

  const unsigned dirichlet_faces = params.dirichlet_faces();
  // (the convective faces first: they imply another mask than 0x3F, which would answer for them below)
  const std::array<double, 6> robin     = params.robin();
  const bool                  convective = std::any_of(robin.begin(), robin.end(), [](double b) { return b > 0.0; });
  if (convective && (params.type == "HMG-local" || params.type == "HPMG-local"))
    throw std::runtime_error("RobinCoefficients '" + params.robin_coefficients + "' with Type '" + params.type +
                             "': not implemented (local smoothing takes no convective faces)");
  for (int f = 0; f < 6; ++f)
    if (robin[f] > 0.0 && ((dirichlet_faces >> f) & 1))
      throw std::runtime_error("RobinCoefficients '" + params.robin_coefficients + "': not implemented on face " + std::to_string(f) +
                               ", which is Dirichlet (list it in NeumannFaces)");
  if (dirichlet_faces != 0x3F && (params.type == "HMG-local" || params.type == "HPMG-local"))
    throw std::runtime_error("NeumannFaces '" + params.neumann_faces + "' with Type '" + params.type +
                             "': not implemented (local smoothing takes Dirichlet conditions on the whole boundary only)");
  if (dirichlet_faces == 0 && params.mass_coefficient == 0.0 && !convective)
    throw std::runtime_error("NeumannFaces '" + params.neumann_faces + "' with MassCoefficient 0: not implemented (no Dirichlet face and "
                             "no mass term: the operator is singular, and no mean-value projection is built)");
  std::shared_ptr<const Triangulation> tria;
  {
    auto mesh = std::make_shared<Triangulation>(params.geometry_type, params.n_ref_global, params.n_ref_local);
    if (dirichlet_faces != 0x3F)
      mesh->set_dirichlet_faces(dirichlet_faces); // before anything is built on the mesh: coarse meshes and DoFs inherit it
    if (convective)
      mesh->set_robin_coefficients(robin); // after the mask: a convective face must not be Dirichlet
    tria = mesh;
  }

  // ---- level hierarchy (ref:multigrid_throughput.cc:2219-2260, 1506-1596): the meshes here, the levels on them from the library
  // (mgamd_level_plan), which also refuses the Types without levels
  const bool local_smoothing = params.type == "HMG-local", hp_local = params.type == "HPMG-local";
  const double sigma         = params.mass_coefficient;
  if ((local_smoothing || hp_local) && sigma != 0.0)
    throw std::runtime_error("MassCoefficient " + std::to_string(sigma) + " with Type '" + params.type +
                             "': not implemented (the refinement-edge matrices of local smoothing have no mass term)");
  auto       level_meshes    = [&]() { // the refinement levels of the mesh (solve_with_local_smoothing, ref:multigrid_throughput.cc:1670-1873)
    std::vector<std::shared_ptr<const Triangulation>> m;
    for (unsigned l = 0; l < tria->n_global_levels(); ++l)
      m.push_back(tria->level_mesh(l));
    return m;
  };
  std::vector<std::shared_ptr<const Triangulation>> meshes{tria}; // PMG, HPMG-local on one rank: p-levels on the one mesh
  if (local_smoothing)
    meshes = level_meshes();
  else if (params.type == "HMG-global" || params.type == "HPMG" || (comm && params.type == "PMG"))
    meshes = create_geometric_coarsening_sequence(tria); // (sharded PMG: the meshes the partition is built on)
  if (params.type == "HMG-global" && meshes.size() > 1)
    {
      auto ptr = std::find_if(meshes.begin(), meshes.end() - 1, [&](const auto &t) {
        if (params.min_level != -1)
          return params.min_level <= (int)t->n_global_levels();
        if (params.min_n_cells != -1)
          return (int)t->n_global_active_cells() >= params.min_n_cells;
        return true;
      });
      meshes.erase(meshes.begin(), ptr);
    }
  const LevelPlan plan     = level_plan(params.type, meshes.size(), params.fe_degree_fine);
  const unsigned  n_levels = plan.levels.size();
  if (comm && !(params.type == "HMG-global" || params.type == "PMG" || params.type == "HPMG"))
    throw std::runtime_error("sharded harness: Type '" + params.type + "' is not implemented (HMG-global, PMG and HPMG are)");
  // levels of >= ~4 M DoFs are cut into one chunk per rank, those of >= ~1 M DoFs into n_ranks / group parts that a group of ranks
  // holds together, the others are replicated (mgamd_partition_defaults; the counterpart of the reference's
  // min_level / min_n_cells_per_process agglomeration, ref:multigrid_throughput.cc:379-418,1464-1501)
  std::unique_ptr<Partition> partition;
  Communicator               sub_comm;
  LevelStack::Sharding       sharding{nullptr, comm, &sub_comm};
  if (comm)
    {
      unsigned p_low = params.fe_degree_fine, group = 1;
      uint64_t min_root_cells = 0, min_sub_root_cells = 0;
      for (const auto &level : plan.levels)
        p_low = std::min(p_low, level.second);
      check(mgamd_partition_defaults(comm->n_ranks(), p_low, &group, &min_root_cells, &min_sub_root_cells));
      partition          = std::make_unique<Partition>(meshes, comm->n_ranks(), 2.0, min_root_cells, group, min_sub_root_cells);
      sub_comm           = comm->subset(partition->group());
      sharding.partition = partition.get();
    }
  const LevelStack::Sharding *shards = comm ? &sharding : nullptr;

  PreconditionChebyshev::AdditionalData sd;
  sd.smoothing_range     = params.mg_data.smoother.smoothing_range;
  sd.degree              = params.mg_data.smoother.degree;
  sd.eig_cg_n_iterations = params.mg_data.smoother.eig_cg_n_iterations;
  // local smoothing: the DoFs of the active mesh, which the outer vectors live on
  std::unique_ptr<DoFHandler> active_dof_handler;
  if (local_smoothing || hp_local)
    active_dof_handler = std::make_unique<DoFHandler>(tria, plan.levels.front().second);
  // HPMG-local (ref:multigrid_throughput.cc:1685-1695,1846-1860): the coarse problem of the p-levels (lowest degree) is handed to one
  // local-smoothing V-cycle; level 0 acts on the SAME DoFs as that cycle
  LevelStack                      ls;
  std::unique_ptr<PreconditionMG> ls_mg;
  if (hp_local)
    {
      const auto ls_meshes = level_meshes();
      const auto ls_plan   = level_plan("HMG-local", ls_meshes.size(), plan.levels.front().second);
      ls    = LevelStack(ctx, ls_meshes, ls_plan.levels, level_number_type, sd, nullptr, ls_plan.local_smoothing);
      ls_mg = std::make_unique<PreconditionMG>(ctx, ls.operators, ls.transfers, ls.smoothers, params.mg_data.coarse_solver.type, nullptr, 1,
                                               active_dof_handler.get());
    }
  const LevelStack::Given ls_level0{0, active_dof_handler.get()};
  const LevelStack        stack(ctx, meshes, plan.levels, level_number_type, sd, shards, plan.local_smoothing, hp_local ? &ls_level0 : nullptr, sigma);
  const DoFHandler       &fine_dof_handler = local_smoothing ? *active_dof_handler : stack.dof_handlers.back();

  // coarse solver (library policy, include/mgamd.h): the Trilinos/PETSc AMG options are an exact solve on the one-cell coarse
  // level of global coarsening and, on a large coarse level (PMG, MinLevel), the library's own smoothed-aggregation AMG.
  // CoarseGridSolverType "gmg_vcycle" (this project's extension) selects the geometric stand-in of rounds 1-2 instead: V-cycles
  // of the h-multigrid on that level.  The table says what ran in its `coarse_solver` column.
  // What has to be built for it is mgamd_coarse_plan's decision: the stand-in ("gmg_vcycle", and the AMG choices on a SHARDED coarse
  // level: the AMG is built from one rank's matrix) or, with "ShardedAMG": true (sharded runs), the global DoFs of the coarse space,
  // from which every rank sets the AMG up and keeps its rows of the cycle.  HPMG-local has its nested multigrid already.
  const std::string coarse = hp_local ? std::string("gmg_vcycle") : params.mg_data.coarse_solver.type;
  int               extra  = MGAMD_COARSE_PLAIN;
  if (!hp_local)
    check(mgamd_coarse_plan(coarse.c_str(), stack.n_dofs_global(ctx, 0), stack.comms[0] != nullptr, comm && params.sharded_amg, &extra));
  const unsigned                  mesh0 = plan.levels.front().first, degree0 = plan.levels.front().second;
  LevelStack                      c_stack;
  std::unique_ptr<PreconditionMG> coarse_mg;
  if (extra == MGAMD_COARSE_NESTED)
    {
      const auto c_meshes = create_geometric_coarsening_sequence(meshes[mesh0]);
      if (comm && c_meshes.size() != mesh0 + 1)
        throw std::runtime_error("sharded harness: the coarse level's mesh is not the end of the partition's mesh sequence");
      const LevelStack::Given top{(unsigned)c_meshes.size() - 1, &stack.dof_handlers[0], &stack.operators[0], &stack.smoothers[0]};
      c_stack   = LevelStack(ctx, c_meshes, level_plan("HMG-global", c_meshes.size(), degree0).levels, level_number_type, sd, shards, false, &top, sigma);
      coarse_mg = std::make_unique<PreconditionMG>(ctx, c_stack.operators, c_stack.transfers, c_stack.smoothers, "amg");
      std::cout << "note: CoarseGridSolverType '" << coarse << "' on the " << stack.dof_handlers[0].n_dofs() << "-DoF coarse level: "
                << params.mg_data.coarse_solver.n_cycles << " V-cycle(s) of the geometric multigrid on that level" << std::endl;
    }
  std::unique_ptr<DoFHandler> amg_global_dofs;
  if (extra == MGAMD_COARSE_SHARDED_AMG)
    {
      amg_global_dofs = std::make_unique<DoFHandler>(meshes[mesh0], degree0);
      amg_global_dofs->set_mass_coefficient(sigma);
      std::cout << "note: CoarseGridSolverType '" << coarse << "' on the sharded " << amg_global_dofs->n_dofs() << "-DoF coarse level: "
                << params.mg_data.coarse_solver.n_cycles << " cycle(s) of the smoothed-aggregation AMG, rows cut over the ranks (levels of <= "
                << params.amg_min_sharded_rows << " rows replicated)" << std::endl;
    }
  PreconditionMG preconditioner =
    amg_global_dofs ? PreconditionMG(ctx, stack.operators, stack.transfers, stack.smoothers, coarse,
                                     PreconditionMG::ShardedAMG{amg_global_dofs.get(), params.amg_min_sharded_rows}, params.mg_data.coarse_solver.n_cycles) :
                      PreconditionMG(ctx, stack.operators, stack.transfers, stack.smoothers, coarse, hp_local ? ls_mg.get() : coarse_mg.get(),
                                     hp_local ? 1u : params.mg_data.coarse_solver.n_cycles, local_smoothing ? active_dof_handler.get() : nullptr);

  // fine (outer, double) operator, right-hand side (ref:multigrid_throughput.cc:2262-2324)
  Operator op;
  if (level_number_type == MGAMD_F64 && !local_smoothing)
    op = stack.operators.back();
  else if (comm)
    op.reinit(ctx, fine_dof_handler, MGAMD_F64, stack.comms.back());
  else
    op.reinit(ctx, fine_dof_handler, MGAMD_F64);
  // DoFHandler::n_dofs() of the GLOBAL problem
  const uint64_t n_dofs_global = local_smoothing ? fine_dof_handler.n_dofs() : stack.n_dofs_global(ctx, n_levels - 1);
  Vector solution, rhs;
  op.initialize_dof_vector(solution);
  op.initialize_dof_vector(rhs);
  op.rhs(rhs, simulation_kind);

  table.add_value("dim", 3);
  table.add_value("n_cells", tria->n_global_active_cells());
  table.add_value("n_cells_hn", tria->n_cells_with_hanging_nodes());
  table.add_value("n_cells_n", tria->n_global_active_cells() - tria->n_cells_with_hanging_nodes());
  table.add_value("degree", params.fe_degree_fine);
  table.add_value("n_ref_global", params.n_ref_global);
  table.add_value("n_ref_local", params.n_ref_local);
  table.add_value("n_dofs", n_dofs_global);
  // (the reference: the ranks that own cells of the coarsest level, ref:multigrid_throughput.cc:1464-1488; here every rank holds it)
  table.add_value("sub_comm_size", comm ? comm->n_ranks() : 1);

  if (params.verbose)
    {
      ConvergenceTable t;
      for (unsigned l = 0; l < n_levels; ++l)
        {
          t.add_value("cells", meshes[plan.levels[l].first]->n_global_active_cells());
          t.add_value("dofs", stack.dof_handlers[l].n_dofs());
        }
      t.write_text(std::cout);
    }

  // ---- solve protocol (ref:multigrid_throughput.cc:1137-1268)
  ReductionControl solver_control(params.mg_data.cg_normal.maxiter, params.mg_data.cg_normal.abstol, params.mg_data.cg_normal.reltol);
  ctx.synchronize();
  solution = 0.0;
  SolverCG(solver_control).solve(op, solution, rhs, preconditioner); // warm-up

  // Stage times: the reference connects host timers to Multigrid's signals (ref:multigrid_throughput.cc:1150-1234).  Here the
  // stages are bracketed by HIP events on the stream of the UNCHANGED cycle (no host synchronisation, collapsed coarse levels
  // included) and read after each solve, so `time`, `throughput` and the stage columns describe the same run.
  const unsigned n_repetitions = params.mg_data.n_repetitions;
  std::vector<std::vector<std::vector<double>>> all_stage_times(n_repetitions); // [repetition][stage 0..8][level], seconds
  std::vector<double>                           times(n_repetitions);
  preconditioner.enable_stage_timing(true);
  for (unsigned counter = 0; counter < n_repetitions; ++counter)
    {
      ctx.synchronize(); // MPI_Barrier
      double time = 0.0;
      {
        solution = 0.0;
        ScopedTimer timer(time);
        SolverCG(solver_control).solve(op, solution, rhs, preconditioner);
      }
      times[counter] = time;
      preconditioner.read_stage_times(all_stage_times[counter]);
    }
  preconditioner.enable_stage_timing(false);
  const unsigned min_index = std::min_element(times.begin(), times.end()) - times.begin();
  const double   time      = times[min_index];
  const auto    &st        = all_stage_times[min_index];
  double         time_cg   = time;
  for (const auto &stage : st)
    for (const double v : stage)
      time_cg -= v;
  const unsigned its = std::max(1u, solver_control.last_step());
  table.add_value("n_levels", n_levels);
  table.add_value("n_iterations", solver_control.last_step());
  table.add_value("time", time);
  table.add_value("time_cg", time_cg / its);
  table.add_value("throughput", (double)n_dofs_global * solver_control.last_step() / time, true);
  static const char *stage_cols[7] = {"time_pre", "time_residuum", "time_res", "time_cs", "time_pro", "time_edge_pro", "time_post"};
  double             t_v           = 0.0;
  for (unsigned j = 0; j < 7; ++j)
    {
      double s = 0;
      for (unsigned l = 0; l < n_levels; ++l)
        s += st[j][l] / its;
      t_v += s;
      table.add_value(stage_cols[j], s, true);
    }
  double t_to_mg = 0, t_to_global = 0;
  for (unsigned l = 0; l < n_levels; ++l)
    {
      t_to_mg += st[7][l] / its;
      t_to_global += st[8][l] / its;
    }
  table.add_value("time_to_mg", t_to_mg, true);
  table.add_value("time_to_global", t_to_global, true);
  t_v += t_to_mg + t_to_global;
  if (params.verbose)
    {
      // partition statistics of the level meshes (ref:multigrid_throughput.cc:1657-1665, ref:include/mg_tools.h:267-512); the
      // p-levels of PMG/HPMG repeat the finest mesh: every distinct mesh once, coarse -> fine
      // local smoothing: the reference calls the single-triangulation overload (ref:multigrid_throughput.cc:1862-1872,
      // ref:include/mg_tools.h:39-61,85,195), which counts ALL cells of each refinement level of the one mesh (HPMG-local: of the
      // cycle underneath).  PMG on its one mesh: the coarsening sequence.
      auto stat_meshes = hp_local ? level_meshes() : meshes;
      if (!local_smoothing && !hp_local && stat_meshes.size() == 1)
        stat_meshes = create_geometric_coarsening_sequence(tria);
      for (const auto &stat : print_multigrid_statistics(stat_meshes, comm ? comm->n_ranks() : 1))
        table.add_value(stat.first, stat.second, true);
    }
  // this project's additions (after the reference's columns): DoF/s per V-cycle = n_dofs / (sum of the nine stage columns)
  //  and the coarse solver that actually ran
  table.add_value("dofs_per_s_per_vcycle", (double)n_dofs_global / t_v, true);
  table.add_value("coarse_solver", preconditioner.coarse_solver_used());

  if (params.verbose)
    {
      std::cout << "per-level stage times per CG iteration [s] (pre, residuum, res, cs, pro, edge_pro, post):" << std::endl;
      for (unsigned l = 0; l < n_levels; ++l)
        {
          std::cout << "  level " << l << ":";
          for (unsigned j = 0; j < 7; ++j)
            std::cout << " " << std::scientific << std::setprecision(3) << st[j][l] / its;
          std::cout << std::endl;
        }
    }
}

int
main(int argc, char **argv)
{
  try
    {
      if (argc == 1)
        {
          printf("ERROR: No .json parameter files has been provided!\n");
          return 1;
        }
      // One rank per GPU when launched with WORLD_SIZE / RANK / LOCAL_RANK in the environment (torchrun --no-python, mpirun -x,
      // a shell loop): the RCCL id travels through a file that rank 0 writes (MGAMD_RCCL_ID_FILE, default derived from
      // MASTER_PORT and the launcher's run id).  MGAMD_HARNESS_SHARDED=1 runs the sharded code path on one rank too.
      auto env_uint = [](const char *name, unsigned dflt) {
        const char *v = std::getenv(name);
        return v ? (unsigned)std::strtoul(v, nullptr, 10) : dflt;
      };
      const unsigned world = env_uint("WORLD_SIZE", 1), rank = env_uint("RANK", 0), local_rank = env_uint("LOCAL_RANK", rank);
      const bool     sharded = world > 1 || std::getenv("MGAMD_HARNESS_SHARDED") != nullptr;
      Context          ctx((int)(sharded ? local_rank : 0));
      ConvergenceTable table;
      Communicator     comm;
      std::string      id_file;
      if (sharded)
        {
          if (const char *f = std::getenv("MGAMD_RCCL_ID_FILE"))
            id_file = f;
          else
            {
              const char *port = std::getenv("MASTER_PORT"), *run = std::getenv("TORCHELASTIC_RUN_ID");
              id_file = std::string("/tmp/mgamd_rccl_id_") + (port ? port : "0") + "_" + (run ? run : "default");
            }
          if (rank == 0)
            std::remove(id_file.c_str()); // a stale id of an earlier job under the same name
          comm = Communicator::rccl(ctx, world, rank, Communicator::exchange_id_through_file(id_file, rank));
        }
      for (int i = 1; i < argc; i++)
        {
          if (rank == 0)
            std::cout << std::string(argv[i]) << std::endl;
          RunParameters params;
          params.parse(std::string(argv[i]));
          if (rank == 0 && params.mass_coefficient != 0.0)
            std::cout << "MassCoefficient: " << params.mass_coefficient << std::endl;
          if (rank == 0 && !params.neumann_faces.empty())
            std::cout << "NeumannFaces: " << params.neumann_faces << " (dirichlet_faces mask " << params.dirichlet_faces() << ")" << std::endl;
          if (rank == 0 && !params.robin_coefficients.empty())
            std::cout << "RobinCoefficients: " << params.robin_coefficients << std::endl;
          run(ctx, params, table, sharded ? &comm : nullptr);
          if (rank == 0)
            table.write_text(std::cout);
        }
      if (rank == 0)
        table.write_text(std::cout);
      if (sharded && rank == 0)
        std::remove(id_file.c_str());
    }
  catch (std::exception &exc)
    {
      std::cerr << std::endl
                << std::endl
                << "----------------------------------------------------" << std::endl;
      std::cerr << "Exception on processing: " << std::endl << exc.what() << std::endl << "Aborting!" << std::endl
                << "----------------------------------------------------" << std::endl;
      return 1;
    }
  catch (...)
    {
      std::cerr << std::endl
                << std::endl
                << "----------------------------------------------------" << std::endl;
      std::cerr << "Unknown exception!" << std::endl << "Aborting!" << std::endl
                << "----------------------------------------------------" << std::endl;
      return 1;
    }
  return 0;
}
