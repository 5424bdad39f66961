// Development check (host only): the tail rows the fused residual pass finishes (TransferTables::residual_tail_runs, transfer_tables.hpp).
// For every level with fused bricks:
//   every tail DoF in shell_idx of a slot that is not a fused brick is in S (an accumulator entry somebody adds to),
//   every tail DoF an un-fused patch restricts is in S (a row of t somebody reads),
//   S lies in [0, n_tail) and its runs are sorted and disjoint.
//   g++ -O2 -std=c++17 -I dealii_multigrid_amd/csrc tools/residual_tail_check.cpp -o tools/bin/residual_tail_check
//   tools/bin/residual_tail_check quadrant 6 4
#include "transfer_tables.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

using namespace mgamd;

int
main(int argc, char **argv)
{
  if (argc < 4)
    {
      std::printf("usage: residual_tail_check geometry n_ref degree\n");
      return 2;
    }
  const std::string geo = argv[1];
  const int         L = std::atoi(argv[2]), p = std::atoi(argv[3]);
  std::vector<Tria> trias;
  trias.push_back(Tria::create(geo.c_str(), L, 0));
  while (trias.back().cells.size() > 1 && (int)trias.size() < 12)
    {
      Tria c = trias.back().coarsen_global();
      if (c.cells.size() == trias.back().cells.size())
        break;
      trias.push_back(std::move(c));
    }
  int rc = 0;
  for (size_t l = 0; l + 1 < trias.size(); ++l)
    {
      LevelTables fine(trias[l], p), coarse(trias[l + 1], p);
      int         fuse_group = -1;
      for (size_t gi = 0; gi < fine.groups.size(); ++gi)
        if (fine.groups[gi].N == 17 && !fine.groups[gi].constrained_group && fine.groups[gi].n_slots() > 0)
          fuse_group = (int)gi;
      if (fuse_group < 0)
        continue;
      TransferTables tt(fine, coarse, true, fuse_group);
      size_t         n_fused = 0;
      for (const BrickTransferGroup &bg : tt.bricks)
        if (bg.fused)
          n_fused += bg.n_bricks() - bg.n_unfused;
      const std::vector<uint32_t> &runs = tt.residual_tail_runs;
      if (n_fused == 0)
        {
          if (!runs.empty())
            {
              std::printf("   runs without fused bricks\n");
              rc = 1;
            }
          continue;
        }
      // S as a bitmap; the runs' own shape
      std::vector<bool> in_s(fine.n_tail, false);
      size_t            bad_shape = 0;
      if (runs.size() % 2)
        ++bad_shape;
      for (size_t k = 0; k + 1 < runs.size(); k += 2)
        {
          if (runs[k] >= runs[k + 1] || runs[k + 1] > fine.n_tail || (k && runs[k] < runs[k - 1]))
            {
              ++bad_shape;
              continue;
            }
          for (uint32_t i = runs[k]; i < runs[k + 1]; ++i)
            in_s[i] = true;
        }
      auto tail_of = [&](uint32_t idx, uint32_t &t) {
        if (idx == INVALID_DOF || idx < fine.n_interior || idx - fine.n_interior >= fine.n_tail)
          return false;
        t = idx - fine.n_interior;
        return true;
      };
      // (1) what the slots outside the fused set touch
      size_t missing_touched = 0, missing_restricted = 0;
      for (size_t gi = 0; gi < fine.groups.size(); ++gi)
        {
          const SlotGroup  &g = fine.groups[gi];
          std::vector<bool> slot_fused(g.n_slots(), false);
          for (const BrickTransferGroup &bg : tt.bricks)
            if (bg.fused && bg.fine_group == (int)gi)
              for (size_t q = bg.n_unfused; q < bg.n_bricks(); ++q)
                slot_fused[bg.slot[q]] = true;
          for (size_t s = 0; s < g.n_slots(); ++s)
            if (!slot_fused[s])
              for (int t = 0; t < g.n_shell; ++t)
                {
                  uint32_t ti;
                  if (tail_of(g.shell_idx[s * (size_t)g.n_shell + t], ti) && !in_s[ti])
                    ++missing_touched;
                }
        }
      // (2) what the un-fused patches restrict: the per-cell patches and the bricks outside the fused set
      size_t n_restricted = 0;
      for (int k = 0; k < 3; ++k)
        for (uint32_t idx : tt.groups[k].fine_idx)
          {
            uint32_t ti;
            if (tail_of(idx, ti))
              {
                ++n_restricted;
                if (!in_s[ti])
                  ++missing_restricted;
              }
          }
      for (const BrickTransferGroup &bg : tt.bricks)
        {
          const size_t nsh = (size_t)fine.groups[bg.fine_group].n_shell;
          const size_t nb  = bg.fused ? bg.n_unfused : bg.n_bricks();
          for (size_t i = 0; i < nb * nsh; ++i)
            {
              uint32_t ti;
              if (tail_of(bg.own_shell[i], ti))
                {
                  ++n_restricted;
                  if (!in_s[ti])
                    ++missing_restricted;
                }
            }
        }
      std::printf("%s L=%d p=%d transfer %zu -> %zu: %zu fused bricks, |S| = %zu of n_tail = %u (%.4f) in %zu runs, %zu restricted tail rows; "
                  "missing: %zu touched, %zu restricted, %zu malformed runs\n",
                  geo.c_str(), L, p, trias.size() - 1 - l, trias.size() - 2 - l, n_fused, tt.residual_tail_size(), fine.n_tail,
                  fine.n_tail ? (double)tt.residual_tail_size() / fine.n_tail : 0.0, runs.size() / 2, n_restricted, missing_touched,
                  missing_restricted, bad_shape);
      if (missing_touched || missing_restricted || bad_shape)
        rc = 1;
    }
  return rc;
}
