// Sharded form of the algebraic multigrid coarse solver (amg.hpp), host side: "replicated setup, sharded cycle".
//
// Every rank builds the SAME smoothed-aggregation hierarchy from the global level tables of the coarse space (the mesh is
// replicated on every rank, partition.hpp), so aggregates, P, R A P, lambda_max and the dense coarsest inverse are those of the
// one-rank AMG bit for bit.  Only the CYCLE is cut into rows:
//
//   ownership   level 0: the rank that owns the DoF in the geometric partition (shared_owner: the lowest regular referencer)
//               owns its global row; level k+1: an aggregate belongs to the rank that owns most of its member rows, ties to
//               the lowest rank.  Every row is owned exactly once.
//   mirrors     Dirichlet and hanging DoFs are identity rows that no other row references: every rank that holds a copy of
//               one it does not own computes it as well (a MIRROR row, level 0 only), so no value has to travel.
//   layout      local rows [ mirror | owned interior | owned boundary ], then the ghost columns grouped by peer (ascending
//               rank, ascending global row): the receive buffer IS the end of the vector, received values land in place.
//               Interior rows reference no ghost in any of the products that write them (A, P of this level, R onto it).
//   exchange    Comm::exchange moves the same count both ways between a pair; owner -> ghost import does not, so every pair is
//               padded to the larger of its two counts (the padding is never read: no column points at it).
//   replicated  levels of at most min_sharded_rows global rows and everything below them, and always the dense coarsest level:
//               the restriction onto the first replicated level is the local partial product (owned columns only) followed by
//               an all-reduce, the prolongation from it needs no communication.
//
// The entries of a row keep their order, so the ranged K7 launches (kernels_amg.hpp) add them up exactly as the one-rank kernel.
#pragma once
#include "amg.hpp"

#include <tuple>

namespace mgamd
{
  // A GUESS: nobody has measured where a ghost import per product starts to cost more than a latency-bound replicated level,
  // and no multi-GPU hardware has run this code.  (The geometric levels switch at about 4 M DoFs, but their exchange hides
  // under the interior bricks of a much heavier kernel; a CSR product of 20 k rows is a few microseconds.)
  constexpr uint32_t AMG_MIN_SHARDED_ROWS_DEFAULT = 20000;

  struct AmgShardLevel
  {
    bool                  replicated = true;
    uint32_t              n_global = 0, n_rows = 0, n_mirror = 0, n_interior = 0, n_ghost = 0, n_recv = 0;
    std::vector<uint32_t> rows;  // global row of every local row
    std::vector<uint32_t> ghost; // global row behind every slot of the receive buffer (INVALID_DOF: padding), n_recv entries
    std::vector<int>      peers; // ascending
    std::vector<uint32_t> peer_offset, send_count, recv_count; // padded offsets into the send / receive buffers; true counts
    std::vector<uint32_t> send_idx;                            // local row packed into every send slot (INVALID_DOF: padding)
    CSR                   A, P, R; // local rows; R: rows of the NEXT level (all of them, as partial sums, if that one is replicated)
    uint32_t
    n_owned() const
    {
      return n_rows - n_mirror;
    }
    uint32_t
    launch_interior() const // rows of the launch that runs under the ghost import
    {
      return n_mirror + n_interior;
    }
  };
  struct AmgShardPlan
  {
    int                        n_ranks = 1, rank = 0;
    std::vector<AmgShardLevel> levels; // one per level of the hierarchy, finest first
  };

  inline uint64_t
  pack_key(const DofKey &k)
  {
    return pack_key((uint32_t)k.px, (uint32_t)k.py, (uint32_t)k.pz, k.dirmask, k.level);
  }

  // global row (index in `global`) of every DoF of `local`, matched through the geometric keys
  inline std::vector<uint32_t>
  match_rows_by_key(const LevelTables &global, const LevelTables &local, double local_sigma)
  {
    if (global.p != local.p)
      throw std::invalid_argument("sharded AMG: the global coarse DoFs must have the degree of the hierarchy's level 0");
    // (local_sigma: the mass coefficient the local level's OPERATOR was built with, or of its tables where there is no operator)
    if (global.sigma != local_sigma)
      throw std::invalid_argument("sharded AMG: the global coarse DoFs carry the mass coefficient " + std::to_string(global.sigma) +
                                  ", the local level " + std::to_string(local_sigma) + ": the assembled matrix would be another operator's");
    // and for the faces that are Dirichlet
    if (global.dirichlet_faces != local.dirichlet_faces)
      throw std::invalid_argument("sharded AMG: the global coarse DoFs carry the dirichlet_faces mask " + std::to_string(global.dirichlet_faces) +
                                  ", the local level " + std::to_string(local.dirichlet_faces) + ": the assembled matrix would be another operator's");
    // and for the Robin coefficients of the convective faces
    for (int f = 0; f < 6; ++f)
      if (global.robin[f] != local.robin[f])
        throw std::invalid_argument("sharded AMG: the global coarse DoFs carry the Robin coefficient " + std::to_string(global.robin[f]) +
                                    " on face " + std::to_string(f) + ", the local level " + std::to_string(local.robin[f]) +
                                    ": the assembled matrix would be another operator's");
    // the same holds for the diffusion coefficient of the cells this rank works on
    // (cell by cell: both tables must describe the same mesh; another mesh is refused here, before the keys are matched)
    if (global.tria->cells.size() != local.tria->cells.size())
      throw std::invalid_argument("sharded AMG: the global coarse DoFs live on a mesh of " + std::to_string(global.tria->cells.size()) +
                                  " cells, the local level on one of " + std::to_string(local.tria->cells.size()) + ": not the same space");
    if (!global.coefficient.empty() || !local.coefficient.empty())
      for (size_t ci = 0; ci < local.tria->cells.size(); ++ci)
        if (local.cell_is_local(ci) && global.coefficient_of(ci) != local.coefficient_of(ci))
          throw std::invalid_argument("sharded AMG: the global coarse DoFs carry the diffusion coefficient " +
                                      std::to_string(global.coefficient_of(ci)) + " on cell " + std::to_string(ci) + ", the local level " +
                                      std::to_string(local.coefficient_of(ci)) + ": the assembled matrix would be another operator's");
    std::vector<DofKey> kg, kl;
    global.export_dof_keys(kg);
    local.export_dof_keys(kl);
    std::vector<std::pair<uint64_t, uint32_t>> m(kg.size());
    for (size_t i = 0; i < kg.size(); ++i)
      m[i] = {pack_key(kg[i]), (uint32_t)i};
    std::sort(m.begin(), m.end());
    std::vector<uint32_t> out(kl.size());
    for (size_t d = 0; d < kl.size(); ++d)
      {
        const uint64_t key = pack_key(kl[d]);
        auto           it  = std::lower_bound(m.begin(), m.end(), std::make_pair(key, 0u));
        if (it == m.end() || it->first != key)
          throw std::runtime_error("sharded AMG: a DoF of the local level is not a DoF of the global coarse space (different mesh?)");
        out[d] = it->second;
      }
    return out;
  }

  // 1: this rank owns the local DoF, 0: it holds a copy of a DoF owned by another rank
  inline std::vector<uint8_t>
  local_dof_owned(const LevelTables &local)
  {
    std::vector<uint8_t> own(local.n_dofs, 1);
    for (uint32_t d = local.n_interior + local.n_tail_owned; d < local.n_interior + local.n_tail; ++d)
      own[d] = 0;
    local.keymap_for_each([&](uint64_t key, int32_t idx) {
      if ((uint32_t)idx >= local.first_constrained())
        own[idx] = local.key_owned(key) ? 1 : 0;
    });
    return own;
  }

  // which levels are cut into rows: not the coarsest, more than min_sharded_rows rows, and every finer level is
  inline unsigned
  amg_n_sharded_levels(const AmgHierarchyHost &H, int n_ranks, uint32_t min_sharded_rows)
  {
    unsigned n = 0;
    if (n_ranks > 1)
      while (n + 1 < H.levels.size() && H.levels[n].A.n_rows > min_sharded_rows)
        ++n;
    return n;
  }

  // owner of every row of every sharded level from the owners of level 0
  inline std::vector<std::vector<int32_t>>
  amg_level_owners(const AmgHierarchyHost &H, std::vector<int32_t> owner0, int n_ranks, unsigned n_sharded)
  {
    std::vector<std::vector<int32_t>> owner;
    if (!n_sharded)
      return owner;
    if (owner0.size() != H.levels[0].A.n_rows)
      throw std::invalid_argument("sharded AMG: owner map of the wrong size");
    for (int32_t o : owner0)
      if (o < 0 || o >= n_ranks)
        throw std::runtime_error("sharded AMG: a row of level 0 has no owner");
    owner.push_back(std::move(owner0));
    for (unsigned k = 0; k + 1 < n_sharded; ++k)
      {
        const AmgLevelHost   &L  = H.levels[k];
        const uint32_t        na = L.P.n_cols;
        std::vector<uint32_t> votes((size_t)na * n_ranks, 0);
        for (uint32_t i = 0; i < L.A.n_rows; ++i)
          if (L.agg[i] >= 0)
            ++votes[(size_t)L.agg[i] * n_ranks + owner[k][i]];
        std::vector<int32_t> next(na, -1);
        for (uint32_t a = 0; a < na; ++a)
          {
            uint32_t best = 0;
            for (int r = 0; r < n_ranks; ++r)
              if (votes[(size_t)a * n_ranks + r] > best) // ties: the lowest rank
                {
                  best    = votes[(size_t)a * n_ranks + r];
                  next[a] = r;
                }
            if (next[a] < 0)
              throw std::runtime_error("sharded AMG: an aggregate without members");
          }
        owner.push_back(std::move(next));
      }
    return owner;
  }

  // mirror0: the global rows of level 0 this rank holds a copy of without owning them (constrained DoFs), ascending
  inline AmgShardPlan
  build_amg_shard_plan(const AmgHierarchyHost &H, const std::vector<std::vector<int32_t>> &owner, const std::vector<uint32_t> &mirror0,
                       int n_ranks, int rank)
  {
    AmgShardPlan S;
    S.n_ranks            = n_ranks;
    S.rank               = rank;
    const unsigned ns    = (unsigned)owner.size(), nl = (unsigned)H.levels.size();
    S.levels.resize(nl);
    for (unsigned k = 0; k < nl; ++k)
      {
        S.levels[k].replicated = k >= ns;
        S.levels[k].n_global = S.levels[k].n_rows = H.levels[k].A.n_rows;
      }
    if (!ns)
      return S;
    // who needs which column of which level from whom: (needer, owner, global row), sorted and unique
    using Need = std::tuple<int32_t, int32_t, uint32_t>;
    std::vector<std::vector<Need>> need(ns);
    auto                           scan = [&](const CSR &M, const std::vector<int32_t> &row_owner, unsigned col_level) {
      const std::vector<int32_t> &co = owner[col_level];
      for (uint32_t i = 0; i < M.n_rows; ++i)
        for (uint32_t q = M.ptr[i]; q < M.ptr[i + 1]; ++q)
          if (co[M.col[q]] != row_owner[i])
            need[col_level].push_back(Need{row_owner[i], co[M.col[q]], M.col[q]});
    };
    for (unsigned k = 0; k < ns; ++k)
      {
        scan(H.levels[k].A, owner[k], k);
        if (k + 1 < ns)
          {
            scan(H.levels[k].R, owner[k + 1], k);
            scan(H.levels[k].P, owner[k], k + 1);
          }
      }
    // pass 1: local rows, ghosts, exchange lists, global -> local column maps
    std::vector<std::vector<uint32_t>> colmap(ns);
    for (unsigned k = 0; k < ns; ++k)
      {
        std::sort(need[k].begin(), need[k].end());
        need[k].erase(std::unique(need[k].begin(), need[k].end()), need[k].end());
        AmgShardLevel        &L = S.levels[k];
        const uint32_t        n = L.n_global;
        std::vector<uint8_t>  cls(n, 0); // 1 owned interior, 2 owned boundary, 3 mirror
        for (uint32_t i = 0; i < n; ++i)
          if (owner[k][i] == rank)
            cls[i] = 1;
        for (const Need &e : need[k])
          if (std::get<0>(e) == rank)
            ++L.n_ghost;
        // a row is a boundary row if any product that writes it reads a ghost
        auto mark = [&](const CSR &M, const std::vector<int32_t> &row_owner, const std::vector<int32_t> &col_owner) {
          for (uint32_t i = 0; i < M.n_rows; ++i)
            if (row_owner[i] == rank)
              for (uint32_t q = M.ptr[i]; q < M.ptr[i + 1]; ++q)
                if (col_owner[M.col[q]] != rank)
                  cls[i] = 2;
        };
        mark(H.levels[k].A, owner[k], owner[k]);
        if (k + 1 < ns)
          mark(H.levels[k].P, owner[k], owner[k + 1]);
        if (k > 0)
          mark(H.levels[k - 1].R, owner[k], owner[k - 1]);
        if (k == 0)
          for (uint32_t g : mirror0)
            {
              const CSR &A = H.levels[0].A;
              if (g >= n || cls[g] != 0 || A.ptr[g + 1] - A.ptr[g] != 1 || A.col[A.ptr[g]] != g)
                throw std::runtime_error("sharded AMG: a mirrored row is not an isolated identity row owned by another rank");
              cls[g] = 3;
            }
        for (int c : {3, 1, 2})
          for (uint32_t i = 0; i < n; ++i)
            if (cls[i] == c)
              L.rows.push_back(i);
        L.n_rows = (uint32_t)L.rows.size();
        for (uint32_t i = 0; i < n; ++i)
          {
            L.n_mirror += cls[i] == 3;
            L.n_interior += cls[i] == 1;
          }
        colmap[k].assign(n, INVALID_DOF);
        for (uint32_t t = 0; t < L.n_rows; ++t)
          colmap[k][L.rows[t]] = t;
        // exchange lists: what I need from q (ascending global row), what q needs from me
        std::vector<std::vector<uint32_t>> recv(n_ranks), send(n_ranks);
        for (const Need &e : need[k])
          {
            if (std::get<0>(e) == rank)
              recv[std::get<1>(e)].push_back(std::get<2>(e));
            if (std::get<1>(e) == rank)
              send[std::get<0>(e)].push_back(std::get<2>(e));
          }
        L.peer_offset.push_back(0);
        for (int q = 0; q < n_ranks; ++q)
          {
            if (recv[q].empty() && send[q].empty())
              continue;
            const uint32_t base = L.peer_offset.back(), cnt = (uint32_t)std::max(recv[q].size(), send[q].size());
            L.peers.push_back(q);
            L.recv_count.push_back((uint32_t)recv[q].size());
            L.send_count.push_back((uint32_t)send[q].size());
            L.ghost.resize(base + cnt, INVALID_DOF);
            L.send_idx.resize(base + cnt, INVALID_DOF);
            for (size_t t = 0; t < recv[q].size(); ++t)
              {
                L.ghost[base + t]     = recv[q][t];
                colmap[k][recv[q][t]] = L.n_rows + base + (uint32_t)t;
              }
            for (size_t t = 0; t < send[q].size(); ++t)
              L.send_idx[base + t] = colmap[k][send[q][t]]; // an owned row: numbered above
            L.peer_offset.push_back(base + cnt);
          }
        L.n_recv = L.peer_offset.back();
      }
    // pass 2: the local matrices, entries in the order of the global rows
    auto localise = [&](const CSR &M, const std::vector<uint32_t> &rows, const std::vector<uint32_t> *cmap, uint32_t n_cols, bool owned_cols_only,
                        const std::vector<int32_t> *col_owner) {
      CSR out;
      out.n_rows = (uint32_t)rows.size();
      out.n_cols = n_cols;
      out.ptr.assign(rows.size() + 1, 0);
      for (size_t t = 0; t < rows.size(); ++t)
        {
          const uint32_t i = rows[t];
          for (uint32_t q = M.ptr[i]; q < M.ptr[i + 1]; ++q)
            {
              const uint32_t j = M.col[q];
              if (owned_cols_only && (*col_owner)[j] != rank)
                continue;
              const uint32_t c = cmap ? (*cmap)[j] : j;
              if (c == INVALID_DOF)
                throw std::runtime_error("sharded AMG: a local row references a column that is neither local nor a ghost");
              out.col.push_back(c);
              out.val.push_back(M.val[q]);
            }
          out.ptr[t + 1] = (uint32_t)out.col.size();
        }
      return out;
    };
    for (unsigned k = 0; k < ns; ++k)
      {
        AmgShardLevel &L = S.levels[k];
        L.A              = localise(H.levels[k].A, L.rows, &colmap[k], L.n_rows + L.n_recv, false, nullptr);
        if (k + 1 < ns)
          {
            const AmgShardLevel &C = S.levels[k + 1];
            L.P                    = localise(H.levels[k].P, L.rows, &colmap[k + 1], C.n_rows + C.n_recv, false, nullptr);
            L.R                    = localise(H.levels[k].R, C.rows, &colmap[k], L.n_rows + L.n_recv, false, nullptr);
          }
        else
          {
            // onto a replicated level: all its rows, my owned columns only (partial sums, completed by an all-reduce)
            std::vector<uint32_t> all(H.levels[k].R.n_rows);
            std::iota(all.begin(), all.end(), 0u);
            L.P = localise(H.levels[k].P, L.rows, nullptr, H.levels[k].P.n_cols, false, nullptr);
            L.R = localise(H.levels[k].R, all, &colmap[k], L.n_rows + L.n_recv, true, &owner[k]);
          }
      }
    return S;
  }

  // the ownership check of construction: count[i] = how many ranks claim row i; fail loudly unless it is exactly one
  inline void
  check_owned_once(const std::vector<uint32_t> &count, const char *what)
  {
    for (size_t i = 0; i < count.size(); ++i)
      if (count[i] != 1)
        throw std::runtime_error(std::string("sharded AMG: row ") + std::to_string(i) + " of " + what + " is owned " + std::to_string(count[i]) +
                                 " times (must be exactly once)");
  }
} // namespace mgamd
