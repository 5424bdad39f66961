// K1 / K1p / K1c / K2 / K3: the level operator on slot lattices (one workgroup per slot group, persistent workgroups with fused
// level transfers for the 17-point lattices, wave-scoped single cells, p = 1 cell clusters), the tail epilogue and the diagonal.
// See kernels.hpp for the overview.
#pragma once
#include "kernels_common.hpp"

namespace mgamd
{
  // K1: the level operator on the slots of one group.  All global loads of a phase are issued before the
  // first dependent use (fully unrolled, branch-free clamped addresses): a rolled loop keeps ONE load per
  // thread in flight and makes every phase latency-bound (measured 0.9 TB/s -> 3+ TB/s for the gather).
  // K1: the level operator on the slots of one group.  All global loads of a phase are issued before the
  // first dependent use (fully unrolled, branch-free clamped addresses): a rolled loop keeps ONE load per
  // thread in flight and makes every phase latency-bound (measured 0.9 TB/s -> 3+ TB/s for the gather).
  // The epilogue operands (x_old, b, D^-1) are requested BEFORE the sweeps so that their latency hides behind
  // the arithmetic; the gathered x is kept in registers for the Chebyshev update instead of being re-read.
#ifdef MGAMD_KERNEL_DEBUG
#define MGAMD_STAMP(k)                         \
  if (args.stamps && tid == 0)                 \
    args.stamps[(size_t)block * 8 + (k)] = wall_clock64();
#define MGAMD_ABLATED(bit) (args.ablate & (bit))
// stamp 7 of a brick of the persistent kernel: 1 + the workgroup that ran it (tools/stamps.py groups the bricks by workgroup)
#define MGAMD_STAMP_OWNER(w)                   \
  if (args.stamps && tid == 0)                 \
    args.stamps[(size_t)block * 8 + 7] = (w) + 1;
#else
#define MGAMD_STAMP(k)
#define MGAMD_STAMP_OWNER(w)
#define MGAMD_ABLATED(bit) false
#endif

  // Closed-form diagonal of a slot-interior lattice node of TYPE t (t = lattice coordinate mod P per direction: 0 = node shared
  // by two cells, a = a-th interior node of a cell), without the cell size:  d = h (s_K + c s_M),  c = sigma h^2, with
  // s_K = k_x m_y m_z + m_x k_y m_z + m_x m_y k_z and s_M = m_x m_y m_z of the assembled 1D diagonals.
  template <typename T, int P>
  __device__ __forceinline__ void
  interior_diag_terms(const Mats<P, T> &mats, const int t, T &s_K, T &s_M)
  {
    const int tt[3] = {t % P, (t / P) % P, t / (P * P)};
    T         m[3], k[3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
      {
        T dm = T(0), dk = T(0);
        if (tt[d] == 0)
          { // last node of one cell + first node of the next
            dm = T(mats.M[P * (P + 1) + P]) + T(mats.M[0]);
            dk = T(mats.K[P * (P + 1) + P]) + T(mats.K[0]);
          }
#pragma unroll
        for (int q = 1; q < P; ++q)
          if (q == tt[d])
            {
              dm = T(mats.M[q * (P + 1) + q]);
              dk = T(mats.K[q * (P + 1) + q]);
            }
        m[d] = dm;
        k[d] = dk;
      }
    s_K = k[0] * m[1] * m[2] + m[0] * k[1] * m[2] + m[0] * m[1] * k[2];
    s_M = m[0] * m[1] * m[2];
  }

  // waves per SIMD: 2 for the 17^3 lattices (<= 256 VGPRs); 6 for single-cell slots (<= 80 VGPRs, measured 5 % faster at
  // p = 4 than unconstrained with 110 VGPRs)
  // the work of workgroup `block` of `nblocks` on the slots of args.g (kernels below)
  // WAVE (single-cell slots only): the slots are shared by ONE WAVEFRONT instead of a workgroup -- `block` / `nblocks` then count
  // wavefronts, smem_raw is the wavefront's own region, and every barrier below is a compiler-level fence (slot_sync): the nine
  // dependent phases of a hanging cell (three interpolation passes, three sweeps, three transposed passes) cost an LDS round
  // trip each instead of a workgroup barrier with the slowest of four waves (measured with tools/stamps.py on the
  // workgroup-scoped kernel: 5-7 of the 9 us a workgroup lives are spent between those barriers).
  // NTHREADS: the threads of the workgroup if they are more than the lattice's own block (lattice_apply_small_kernel runs the
  // 13-point bricks of p = 6, whose 169 lines make a 192-thread block, in its 256-thread workgroups); 0: Geo's ABLOCK
  // MASS = false compiles the mass term out (lattice_sweeps); the small-slot kernels come in both forms and the host picks by
  // sigma != 0 (lattice_apply_small_kernel), every other caller leaves MASS = true and sigma decides at run time
  template <typename T, int P, int B, int MODE, bool CONSTR = false, bool WAVE = false, int NTHREADS = 0, bool MASS = true>
  __device__ __forceinline__ void
  lattice_apply_body(const ApplyArgs<T, P> &args, const uint32_t block, const uint32_t nblocks, unsigned char *smem_raw)
  {
    static_assert(!WAVE || (B == 1 && !CONSTR), "wave-scoped slots: single cells");
    using G  = Geo<P, B, WAVE ? 64 : 256>;
    using IM = InteriorMap<P, B, WAVE ? 64 : 256>;
    static_assert(G::ROUNDS == 1, "one line per thread: the 17^3 lattices take the persistent kernel");
    T *bufA = reinterpret_cast<T *>(smem_raw);
    T *bufB = bufA + G::SPW * G::N3;

    // every entry loop below strides by BLOCK = the number of threads that run this body
    constexpr int BLOCK = NTHREADS > 0 ? NTHREADS : G::ABLOCK;
    static_assert(BLOCK >= G::ABLOCK && (!WAVE || NTHREADS == 0), "the workgroup holds the lattice's lines");
    constexpr int ITER  = (G::SPW * IM::NIN_ + BLOCK - 1) / BLOCK;
    constexpr int ITERS = (G::SPW * G::N_SHELL + BLOCK - 1) / BLOCK;

    const int tid    = WAVE ? (int)(threadIdx.x & 63u) : (int)threadIdx.x;
    const int slot0  = (int)(WAVE ? block : xcd_contiguous(block, nblocks)) * G::SPW; // (WAVE: the caller has mapped the wavefront)
    const int nslots = min((int)G::SPW, (int)args.g.n_slots - slot0);
    MGAMD_STAMP(0)
    // per-slot scalars of this thread's line (hanging-node mask, constraint mask, cell size): requested with the gather, not
    // between the barriers that follow it (each was a full memory round trip on the critical path of the small-slot kernels)
    const int  sl = tid / G::LINES, ln = tid % G::LINES;
    const int  u = ln % G::N, v = ln / G::N;
    const bool act = tid < G::SPW * G::LINES && sl < nslots;
    uint32_t   mask = 0;
    if (B == 1 && act)
      mask = args.g.mask[slot0 + sl];
    uint32_t fm_early = 0;
    if constexpr (brick_may_be_constrained(B, CONSTR))
      if (args.g.fmask != nullptr && tid < nslots)
        fm_early = args.g.fmask[slot0 + tid];
    const double h_mine  = args.g.h[slot0 + (act ? sl : 0)];
    uint32_t     fm_line = 0; // constraint mask of this thread's line
    if constexpr (brick_may_be_constrained(B, CONSTR))
      if (args.g.fmask != nullptr && act)
        fm_line = args.g.fmask[slot0 + sl];

    // D^-1 of slot-interior DoFs is not read from memory: they only see this slot's cells, so their diagonal is the
    // closed tensor form  d = h (k_x m_y m_z + m_x k_y m_z + m_x m_y k_z)  of the assembled 1D diagonals (what
    // lattice_diag_kernel stores), which depends on the node TYPE per direction only (t = lattice coordinate mod P:
    // 0 = node shared by two cells, a = a-th interior node of a cell): a P^3 table of s = d/h and 1/s in LDS, and 1/h
    // per slot.  One vector word less per interior DoF and Chebyshev pass.
    // Used at P = 1 (one node type: the look-up is a broadcast, -11 % on the 17^3 kernel); at P = 4 the 64-entry look-up
    // per entry pushes the 17^3 kernel over its 256 VGPRs (measured 1113 -> 1829 us), so D^-1 is read from memory there.
    constexpr bool CLOSED_DINV = P == 1 || (P == 4 && B == 4);
    // With the mass term  d = h (s_K + c s_M), c = sigma h^2 of the slot: the table is PER SLOT (TS entries; at P = 1 that is one
    // entry per slot, apply_lds_bytes), formed once per workgroup; the epilogue stays  rh * table.  sigma = 0: s_K + 0 = s_K.
    constexpr int TS = CLOSED_DINV ? P * P * P * (P == 1 ? G::SPW : 1) : P * P * P;
    static_assert(!(CLOSED_DINV && G::N_INT > 0) || P == 1 || G::SPW == 1, "one D^-1 table per slot");
    T *dtab = bufB + G::SPW * G::N3; // [TS] s, [TS] 1/s, [SPW] 1/h
    if (CLOSED_DINV && is_cheb(MODE) && G::N_INT > 0)
      {
        constexpr int P3 = P * P * P;
        for (int i = tid; i < nslots * P3; i += BLOCK)
          {
            const int t = i % P3, s2 = i / P3;
            T         s_K, s_M;
            interior_diag_terms<T, P>(args.m, t, s_K, s_M);
            const T sv   = s_K + (T(args.sigma) * T(args.g.q[slot0 + s2])) * s_M;
            dtab[i]      = sv;
            dtab[TS + i] = T(1) / sv;
          }
        for (int t = tid; t < nslots; t += BLOCK)
          dtab[2 * TS + t] = T(1) / T(args.g.h[slot0 + t]);
        slot_sync<WAVE>();
      }

    // ---- gather: addresses ----------------------------------------------------------------------------
    // interior entry `it` of this thread: global index (always a valid address) and LDS position (-1: no entry) with
    // the node type for the D^-1 table in bits 16+.  With one slot per workgroup the global index is base + entry
    // number and is not held in registers (the 17^3 kernels sit at the 256-VGPR limit).
    constexpr bool REMAT = G::SPW == 1;
    struct Ent
    {
      uint32_t g;
      int      l, t;
    };
    const uint32_t base0 = G::N_INT > 0 ? args.g.interior_base[slot0] : 0u;
    uint32_t       gbase[REMAT ? 1 : ITER];
    int            glds[ITER];
    if (G::N_INT > 0)
      {
#pragma unroll
        for (int it = 0; it < ITER; ++it)
          {
            bool ok;
            int  s2, i, lds;
            IM::decode(tid + it * BLOCK, nslots, ok, s2, i, lds);
            if (!REMAT)
              gbase[REMAT ? 0 : it] = args.g.interior_base[slot0 + s2] + (uint32_t)i;
            const int x = i % IM::NI_ + 1, y = (i / IM::NI_) % IM::NI_ + 1, z = i / (IM::NI_ * IM::NI_) + 1;
            const int t = (x % P) + P * ((y % P) + P * (z % P));
            glds[it]    = ok ? (lds | (t << 16) | (s2 << 24)) : -1;
          }
      }
    auto ent = [&](int it) -> Ent {
      const int      l = glds[it];
      const uint32_t g = REMAT ? base0 + (uint32_t)(l >= 0 ? tid + it * BLOCK : 0) : gbase[REMAT ? 0 : it];
      return Ent{g, l >= 0 ? (l & 0xFFFF) : -1, l >> 16};
    };
    uint32_t sgi[ITERS];
    int      spos[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it)
      {
        const int  idx = tid + it * BLOCK;
        const bool ok  = idx < nslots * G::N_SHELL;
        const int  s2 = ok ? idx / G::N_SHELL : 0, s = idx % G::N_SHELL;
        sgi[it]  = NT_LOAD(&args.g.shell_idx[(size_t)(slot0 + s2) * G::N_SHELL + (ok ? s : 0)]);
        spos[it] = s2 * G::N3 + (int)args.g.shell_pos[s];
        if (!ok)
          spos[it] = -1;
      }
    // ---- gather: values ---------------------------------------------------------------------------------
    constexpr bool x_from_b = MODE == MODE_CHEB_FIRST; // x = c0 dinv b, never stored
    T              xg[ITER]; // gathered interior values, kept for the Chebyshev epilogue
    if (G::N_INT > 0 && !MGAMD_ABLATED(8) && !x_from_b)
      {
#pragma unroll
        for (int it = 0; it < ITER; ++it)
          xg[it] = NT_LOAD(&args.src[ent(it).g]);
      }
    T sval[ITERS];
    if (!MGAMD_ABLATED(16))
      {
        if (x_from_b)
          {
            T sb[ITERS];
#pragma unroll
            for (int it = 0; it < ITERS; ++it)
              {
                const uint32_t gi = sgi[it] < args.gather_limit ? sgi[it] : 0;
                sval[it]          = args.epi.dinv[gi];
                sb[it]            = args.epi.b[gi];
              }
#pragma unroll
            for (int it = 0; it < ITERS; ++it)
              sval[it] = args.epi.c0 * sval[it] * sb[it];
          }
        else
          {
#pragma unroll
            for (int it = 0; it < ITERS; ++it)
              sval[it] = args.src[sgi[it] < args.gather_limit ? sgi[it] : 0];
          }
      }
    // D^-1 of this thread's interior entry `it` (see above); looked up where needed, never held in registers
    auto interior_dinv = [&](int it) -> T {
      constexpr int P3 = P * P * P;
      const int     gl = glds[it] >= 0 ? glds[it] : 0, t = (gl >> 16) & 0xFF, s2 = (gl >> 24) & 0x7F;
      const T       rh = dtab[2 * TS + s2];
      const int     e  = s2 * P3 + t; // this slot's table
      // |d| > 1e-10 ? 1/d : 1 with d = h s  (ref:include/operator.h:228-242)
      return fabs((double)dtab[e]) > 1.0e-10 * fabs((double)rh) ? rh * dtab[TS + e] : T(1);
    };
    // ---- epilogue operands, requested now, consumed after the sweeps ----------------------------------------
    T xo[ITER], bv[ITER], dvm[CLOSED_DINV ? 1 : ITER]; // dvm: D^-1 from memory
    if (G::N_INT > 0 && !MGAMD_ABLATED(4))
      {
#pragma unroll
        for (int it = 0; it < ITER; ++it)
          {
            const uint32_t g = ent(it).g;
            xo[it] = bv[it] = T(0);
            if (MODE == MODE_RESIDUAL)
              bv[it] = NT_LOAD(&args.epi.b[g]);
            if (is_cheb(MODE))
              {
                if (MODE == MODE_CHEB && args.epi.xold)
                  xo[it] = NT_LOAD(&args.epi.xold[g]);
                bv[it] = NT_LOAD(&args.epi.b[g]);
                if (!CLOSED_DINV)
                  dvm[it] = NT_LOAD(&args.epi.dinv[g]);
              }
          }
        if (MODE == MODE_CHEB_FIRST)
          {
#pragma unroll
            for (int it = 0; it < ITER; ++it)
              xg[it] = args.epi.c0 * (CLOSED_DINV ? interior_dinv(it) : dvm[it]) * bv[it];
          }
      }
    // ---- gather: into LDS -------------------------------------------------------------------------------
    if (!MGAMD_ABLATED(16))
      {
#pragma unroll
        for (int it = 0; it < ITERS; ++it)
          if (spos[it] >= 0)
            bufA[spos[it]] = sgi[it] < args.gather_limit ? sval[it] : T(0);
      }
    if (G::N_INT > 0 && !MGAMD_ABLATED(8))
      {
#pragma unroll
        for (int it = 0; it < ITER; ++it)
          {
            const int l = ent(it).l;
            if (l >= 0)
              bufA[l] = xg[it];
          }
      }
    slot_sync<WAVE>();
    MGAMD_STAMP(1)

    // ---- hanging-node interpolation (single-cell slots only) ---------------------------------------------
    bool any_hanging = false;
    if (B == 1)
      {
        any_hanging = (WAVE ? __any((int)(mask >> 3)) : __syncthreads_or((int)(mask >> 3))) != 0 && !MGAMD_ABLATED(32);
        if (any_hanging)
          hanging_passes<T, P, WAVE>(bufA, args.m, sl, u, v, act, mask, false);
      }

    // Which bricks may be constrained (must match LevelTables::build): families (B = 2) at every degree; larger bricks at
    // P = 1 only, in a slot group and kernel instantiation of their own (CONSTR).  Measured on MI355X: at p = 1 the 16^3-cell rim bricks of the octant replace the 2.5x slower single-cell
    // cluster path (V-cycle 1.95 -> 1.76 ms); at p = 4 the 4^3 rim bricks cost what the 2^3 families cost (0.5 vs 0.8 ns per
    // cell, eaten by the passes), while the extra SGPR pressure of the pass code slowed EVERY 17^3 workgroup by 4-6 %.
    if constexpr (brick_may_be_constrained(B, CONSTR))
      {
        // constrained bricks: whole-face / whole-edge hanging nodes (uniform branch: one mask per slot)
        any_hanging = __syncthreads_or((int)(fm_early != 0)) != 0;
        if (any_hanging)
          brick_constraint_passes<T, P, B, BLOCK>(bufA, args.m, tid, nslots, args.g.fmask + slot0, false, &fm_line);
      }
    MGAMD_STAMP(5)

    if (!MGAMD_ABLATED(1))
      {
        if constexpr (MODE == MODE_MASS) // three mass products on the first lattice; the second is not touched
          mass_sweeps<T, P, B, BLOCK, false, false, WAVE>(bufA, args.m, tid, nslots, &h_mine, true);
        else
          lattice_sweeps<T, P, B, BLOCK, NoHook, false, false, WAVE, MASS>(bufA, bufB, args.m, tid, nslots, &h_mine, NoHook(), true, args.sigma, args.g.q + slot0);
      }
    MGAMD_STAMP(6)

    if (B == 1 && any_hanging)
      hanging_passes<T, P, WAVE>(bufA, args.m, sl, u, v, act, mask, true);
    if constexpr (brick_may_be_constrained(B, CONSTR))
      if (any_hanging)
        brick_constraint_passes<T, P, B, BLOCK>(bufA, args.m, tid, nslots, args.g.fmask + slot0, true, &fm_line);
    MGAMD_STAMP(2)

    // ---- interior DoFs are complete: fused epilogue, contiguous stores -----------------------------------
    if (G::N_INT > 0 && !MGAMD_ABLATED(4))
      {
#pragma unroll
        for (int it = 0; it < ITER; ++it)
          if (const Ent e = ent(it); e.l >= 0)
            {
              const T ax = bufA[e.l];
              T       r;
              if (MODE == MODE_VMULT || MODE == MODE_MASS)
                r = ax;
              else if (MODE == MODE_RESIDUAL)
                r = bv[it] - ax;
              else
                {
                  const T dv  = CLOSED_DINV ? interior_dinv(it) : dvm[CLOSED_DINV ? 0 : it];
                  const T xov = MODE == MODE_CHEB_SECOND ? args.epi.c0 * dv * bv[it] : xo[it];
                  r           = xg[it] + args.epi.f1 * (xg[it] - xov) + args.epi.f2 * dv * (bv[it] - ax);
                }
              if (MODE == MODE_CHEB)
                store_result(args.epi, e.g, r);
              else
                NT_STORE(r, &args.epi.out[e.g]);
            }
      }
    MGAMD_STAMP(3)
    // ---- shell DoFs: partial sums into the tail accumulator ------------------------------------------------
    if (!MGAMD_ABLATED(2))
      {
#pragma unroll
        for (int it = 0; it < ITERS; ++it)
          if (spos[it] >= 0 && sgi[it] < args.scatter_limit)
            atomic_add(&args.tail_acc[sgi[it] - args.n_interior], bufA[spos[it]]);
      }
#ifdef MGAMD_KERNEL_DEBUG
    if (args.stamps)
      {
        __builtin_amdgcn_s_waitcnt(0); // drain this wave's memory operations before the final stamp
        slot_sync<WAVE>();
        MGAMD_STAMP(4)
      }
#endif
  }

  // K1p: the same operator application with PERSISTENT workgroups (one-slot-per-workgroup lattices: N^2 >= 256 lines).
  // Measured on MI355X (tools/stamps.py, octant p=4 L=8, 5-word Chebyshev pass): a workgroup of lattice_apply_body lives
  // 16.2 us per brick, 7.8 us of them in the gather (two DEPENDENT global round trips: slot tables -> values, at the
  // loaded-memory latency), 4.4 us in the sweeps, 3.7 us in epilogue + atomics; with 2 workgroups per CU (LDS) nothing hides
  // the gather, and removing 17 % of the kernel's HBM bytes (closed-form D^-1) changed nothing: the pass is bound by that
  // latency chain, not by bytes.  Here workgroup w of the `stride` resident ones (a multiple of 8) takes slot
  // xcd_contiguous(w, n) and then whatever the ticket counter of its XCD hands it inside that XCD's Morton range (TicketSchedule,
  // kernels_common.hpp: with the fixed walk v = w, w + stride, ... the median workgroup of a level-8 pass had finished 130 us
  // before the last one, 14 % of the pass idle), and runs a software pipeline over its slots:
  //     top      values of slot v (requested one iteration earlier) -> LDS;  slot tables of the next slot v' requested, the ticket
  //              of the one after it drawn (and handed to the workgroup before the sweeps begin)
  //     sweeps   (epilogue operands of v in flight, as before)
  //     after    the VALUES of v' are requested (the registers of the sweeps are free again), then epilogue + atomics of v
  // so both round trips of the next gather overlap with work of the current slot.  D^-1 of interior DoFs always in closed
  // form (see lattice_apply_body): that is what frees the registers for the second set of gathered values.
  //
  // FUSED LEVEL TRANSFERS (MODE_RESIDUAL_RESTRICT, MODE_CHEB_PROLONGATE; ref:multigrid_throughput.cc:1600-1604 between
  // Multigrid's residual / restriction and prolongation / post-smoothing steps).  The brick's 17-point lattice is the fine
  // patch of the (B/2)^3 coarse cells under it, so the three embedding sweeps run on the lattice the operator holds in LDS:
  //   RESTRICT    after the operator sweeps the lattice becomes  r = [interior: b - A x | shell: (owned ? b : 0) - this brick's
  //               partial sum of A x], three transposed embedding sweeps reduce it in place to the 9^3 coarse lattice, which is
  //               added to the coarse defect.  Restriction is linear: the partial sums of a shell row restricted by the bricks
  //               that produced them add up to the row's restricted residual.  Neither t nor the tail accumulator is written.
  //   PROLONGATE  before the operator sweeps the 9^3 coarse values are embedded on the scratch lattice and added to the gathered
  //               x (shell entries that an un-fused patch owns arrive corrected already); x + P x_c is stored once (interior in
  //               place, owned shell entries to a scratch vector that tail_kernel folds in) and never re-read by this pass.
  // Slots that are not flagged as fused (no brick patch, halo slots of a sharded level) take the base mode's path.
  // MASS: the operator carries the mass term (args.sigma != 0, checked by the host, which picks the instantiation): the sweeps
  // shift b by c a, and the closed-form D^-1 table is formed for every slot.  MASS = false is the Laplace kernel, unchanged.
  // (no default for MASS, here or on the kernels: a launch site that forgot it would apply the Laplace operator under sigma != 0)
  template <typename T, int P, int B, int MODE_, bool CONSTR, bool MASS>
  __device__ __forceinline__ void
  lattice_apply_persistent_body(const ApplyArgs<T, P> &args, const uint32_t w, const uint32_t stride, unsigned char *smem_raw)
  {
    using G  = Geo<P, B>;
    using IM = InteriorMap<P, B>;
    static_assert(G::SPW == 1 && G::N_INT > 0, "persistent workgroups: one slot per workgroup");
    constexpr int  MODE   = base_mode(MODE_);
    constexpr bool FUSE_R = MODE_ == MODE_RESIDUAL_RESTRICT, FUSE_P = MODE_ == MODE_CHEB_PROLONGATE, FUSE = FUSE_R || FUSE_P;
    static_assert(!FUSE || (!CONSTR && B >= 2 && G::ABLOCK == 256), "fused transfers: plain bricks, 256 threads");
    static_assert(!CONSTR || P == 1, "constrained bricks larger than a family: p = 1 only (LevelTables::build)");
    static_assert(MODE_ != MODE_MASS || !MASS, "the mass pass has no mass TERM: one instantiation, MASS = false");
    constexpr int BC = B >= 2 ? B / 2 : 1, NC = P * BC + 1, NC3 = NC * NC * NC; // coarse lattice under the brick
    T *bufA = reinterpret_cast<T *>(smem_raw);
    T *bufB = bufA + G::N3;
    T *dtab = bufB + G::N3; // [P^3] s = d/h, [P^3] 1/s

    constexpr int BLOCK = G::ABLOCK;
    constexpr int ITER  = (G::N_INT + BLOCK - 1) / BLOCK;
    constexpr int ITERS = (G::N_SHELL + BLOCK - 1) / BLOCK;
    constexpr int ITC   = FUSE ? (NC3 + BLOCK - 1) / BLOCK : 1;
    constexpr int P3    = P * P * P;
    static_assert(!FUSE || 2 * ITERS <= 15, "two flag bits per shell entry in a 16-bit word");

    const int      tid = threadIdx.x;
    const uint32_t n   = args.g.n_slots;
    if (w >= n)
      return;
    // the slots after the first: by ticket (TicketSchedule).  Lane 0 draws; the ticket reaches the others through one LDS word (the
    // 1/h entry of apply_lds_bytes, which this body does not use) behind barriers that the pipeline has anyway
    const TicketSchedule sched(args.tickets, w, stride, n);
    uint32_t *const      ticket_word = reinterpret_cast<uint32_t *>(dtab + 2 * P * P * P);
    uint32_t             drawn       = 0;
    if (sched.active && tid == 0)
      drawn = sched.draw();

    if (is_cheb(MODE))
      {
        for (int t = tid; t < P3; t += BLOCK)
          {
            T sv, s_M;
            interior_diag_terms<T, P>(args.m, t, sv, s_M);
            dtab[t]      = sv;
            dtab[P3 + t] = T(1) / sv;
          }
      }
    // interior entry `it` of this thread is entry i = tid + it BLOCK of the slot (lattice order, NI^3 entries).  Its lattice
    // coordinates are NOT held in registers (14 VGPRs that the pipeline needs): every phase walks them from (x0, y0, z0) of
    // entry `tid` by the constant step BLOCK = DZ NI^2 + DY NI + DX with two carries (InteriorWalk).
    constexpr int NI = IM::NI_;
    struct InteriorWalk
    {
      int x, y, z; // 1-based lattice coordinates of the current entry
      __device__ __forceinline__ int
      pos() const
      {
        return (z * G::N + y) * G::N + x;
      }
      __device__ __forceinline__ int
      type() const
      {
        return (x % P) + P * ((y % P) + P * (z % P));
      }
      __device__ __forceinline__ void
      next()
      {
        constexpr int DZ = BLOCK / (NI * NI), DY = (BLOCK % (NI * NI)) / NI, DX = BLOCK % NI;
        x += DX;
        if (x > NI)
          {
            x -= NI;
            ++y;
          }
        y += DY;
        if (y > NI)
          {
            y -= NI;
            ++z;
          }
        z += DZ;
      }
    };
    const InteriorWalk walk0{tid % NI + 1, (tid / NI) % NI + 1, tid / (NI * NI) + 1};
    // entry `it` exists: always below the last round
    auto has_entry = [&](int it) -> bool { return (it + 1) * BLOCK <= G::N_INT || tid + it * BLOCK < G::N_INT; };
    int spos[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it)
      {
        const int idx = tid + it * BLOCK;
        spos[it]      = idx < G::N_SHELL ? (int)args.g.shell_pos[idx] : -1;
      }
    if (sched.active && tid == 0)
      sched.publish(drawn, ticket_word);
    __syncthreads();

    constexpr bool x_from_b = MODE == MODE_CHEB_FIRST; // x = c0 dinv b, never stored
    // the epilogue operands (x_old, b) of a slot are requested BEFORE its sweeps (their latency hides behind the arithmetic);
    // they are live across the sweeps, which is why the sweeps are streamed cell by cell (line_stream: ~35 instead of ~70
    // doubles per thread).  Requested after the sweeps, or between the y and the x sweep, they fit whole-line sweeps but expose
    // their latency (measured: no gain over the one-workgroup-per-brick kernel).
    // slot tables of slot s
    auto load_tables = [&](uint32_t s, uint32_t &slot, uint32_t &base, uint32_t(&sg)[ITERS], double &h, uint32_t &fm, uint32_t &fl,
                           uint32_t(&cg)[ITC]) {
      slot = s;
      base = args.g.interior_base[slot];
      h    = args.g.h[slot];
      fm   = 0;
      fl   = 0;
      if constexpr (FUSE)
        {
          fl = args.fused.flags[(size_t)slot * BLOCK + tid];
          const uint32_t *__restrict__ c0 = args.fused.coarse_idx + (size_t)slot * NC3;
#pragma unroll
          for (int it = 0; it < ITC; ++it)
            cg[it] = NT_LOAD(c0 + min(tid + it * BLOCK, NC3 - 1));
        }
      if constexpr (brick_may_be_constrained(B, CONSTR)) // the constraint mask travels with the tables (it was three exposed
        if (args.g.fmask != nullptr)                     // memory round trips per constrained brick when loaded where used)
          fm = args.g.fmask[slot];
      // (uniform base + round offset in scalar registers, ONE lane offset for every round: per-round lane offsets cost a VGPR
      // each, were spilled in the 5-word Chebyshev mode and reloaded here behind `s_waitcnt vmcnt(0)` - four exposed memory
      // round trips per slot)
      const uint32_t *__restrict__ p0 = args.g.shell_idx + (size_t)slot * G::N_SHELL;
#pragma unroll
      for (int it = 0; it < ITERS; ++it)
        {
          if ((it + 1) * BLOCK <= G::N_SHELL)
            sg[it] = NT_LOAD(p0 + it * BLOCK + tid);
          else
            sg[it] = NT_LOAD(p0 + min(tid + it * BLOCK, G::N_SHELL - 1));
        }
    };
    // operator input on the lattice of a slot (x_from_b: b and, on the shell, D^-1)
    // (FUSE_R: sbv = b on the shell entries this brick owns; FUSE_P: cv = the coarse values under the brick)
    auto load_values = [&](uint32_t base, const uint32_t(&sg)[ITERS], const uint32_t fl, const uint32_t(&cg)[ITC], T(&xv)[ITER], T(&sv)[ITERS],
                           T(&sbv)[ITERS], T(&cv)[ITC]) {
      const T *__restrict__ in = x_from_b ? args.epi.b : args.src;
#pragma unroll
      for (int it = 0; it < ITER; ++it)
        xv[it] = NT_LOAD(&in[base + (uint32_t)(has_entry(it) ? tid + it * BLOCK : 0)]);
#pragma unroll
      for (int it = 0; it < ITERS; ++it)
        {
          const uint32_t gi = sg[it] < args.gather_limit ? sg[it] : 0;
          sv[it]            = in[gi];
          if (x_from_b)
            sbv[it] = args.epi.dinv[gi];
          if (FUSE_R)
            sbv[it] = args.epi.b[((fl >> (2 * it)) & 1u) ? gi : 0];
        }
      // (the coarse values last: measured 3.80 vs 3.91 ms per octant p=4 post-smoothing against loading them first, which lets
      // the embedding start while x is still in flight but delays x behind 3 more loads)
      if constexpr (FUSE_P)
        {
#pragma unroll
          for (int it = 0; it < ITC; ++it)
            cv[it] = args.fused.coarse[cg[it] != DEV_INVALID ? cg[it] : 0];
        }
    };

    uint32_t slot, base, sgi[ITERS], fmcur, flcur, cgi[ITC];
    double   hcur;
    T        xg[ITER], sval[ITERS], sb[ITERS], cval[ITC];
    load_tables(xcd_contiguous(w, n), slot, base, sgi, hcur, fmcur, flcur, cgi);
    load_values(base, sgi, flcur, cgi, xg, sval, sb, cval);

    for (;;)
      {
        const uint32_t block = slot;
        (void)block;
        // the next slot: the ticket published one iteration ago (or before the loop).  A workgroup draws no more after its first
        // ticket out of range.
        // The ticket of the slot after the next is drawn now and handed on behind the barrier under stamp 1, which every thread
        // passes after it has taken this one: the draw rides under the gather phase, and its register is free again before the
        // sweeps (held across the sweeps or across the epilogue it costs the 5-word modes 3 to 6 spilled VGPRs).
        uint32_t   vn       = slot;
        const bool has_next = sched.active && sched.take(ticket_word, vn);
        if (has_next && tid == 0)
          drawn = sched.draw();
        MGAMD_STAMP(0)
        MGAMD_STAMP_OWNER(w)
        const T rh = T(1) / T(hcur);
        // Mass term: d = h (s_K + c s_M) with c = sigma h^2 of THIS slot, so the table is formed anew for every slot by its first
        // P^3 threads.  The barrier at the end of the slot loop (or the one before the loop) has every reader of the previous
        // table behind it; the first reader of this one is the epilogue, behind the barriers of the sweeps -- except where x is
        // formed from b on the fly (x_from_b), which takes one more barrier.  MASS = false: the table built above.
        if constexpr (MASS && is_cheb(MODE))
          {
            const T c = T(args.sigma) * T(args.g.q[slot]); // (h^2 / a is read where it is used: these kernels have no register to carry it)
            for (int t = tid; t < P3; t += BLOCK)
              {
                T s_K, s_M;
                interior_diag_terms<T, P>(args.m, t, s_K, s_M);
                const T sv   = s_K + c * s_M;
                dtab[t]      = sv;
                dtab[P3 + t] = T(1) / sv;
              }
            if (x_from_b)
              __syncthreads();
          }
        // D^-1 of this thread's interior entry `it`: |d| > 1e-10 ? 1/d : 1 with d = h s  (ref:include/operator.h:228-242)
        auto interior_dinv = [&](int t) -> T { // t: node type (InteriorWalk::type)
          return fabs((double)dtab[t]) > 1.0e-10 * fabs((double)rh) ? rh * dtab[P3 + t] : T(1);
        };
        // one flag word per thread, bit 15 equal in all of them: a workgroup-uniform branch
        const bool fused_slot = FUSE && ((__builtin_amdgcn_readfirstlane((int)flcur) >> 15) & 1);
        T          bv[ITER], xo[ITER];
        // ---- slot tables of the next slot, epilogue operands of this one: requested now ------------------------
        uint32_t slotn = slot, basen = base, sgn[ITERS], fmn = fmcur, fln = flcur, cgn[ITC];
        double   hn = hcur;
        if (has_next)
          load_tables(vn, slotn, basen, sgn, hn, fmn, fln, cgn);
        {
#pragma unroll
          for (int it = 0; it < ITER; ++it)
            {
              const uint32_t g = base + (uint32_t)(has_entry(it) ? tid + it * BLOCK : 0);
              xo[it]           = T(0);
              bv[it]           = x_from_b ? xg[it] : T(0); // (x_from_b: x itself is recomputed in the epilogue: one value less across the sweeps)
              if (MODE == MODE_CHEB && !FUSE_P && args.epi.xold) // (the fused prolongation pass has x_old = 0 by construction)
                xo[it] = NT_LOAD(&args.epi.xold[g]);
              if ((MODE == MODE_RESIDUAL || is_cheb(MODE)) && !x_from_b)
                bv[it] = NT_LOAD(&args.epi.b[g]);
            }
        }
        // ---- fused prolongation: x + P x_c on the lattice -----------------------------------------------------------
        if constexpr (FUSE_P)
          if (fused_slot)
            {
              // the coarse values, COMPACT (NC^3, x fastest) in the first lattice, which is free until this slot's values go
              // there: linear addresses (positions computed from the thread index were hoisted out of the loop and spilled).
              // z sweep from there into the scratch lattice, then y and x in place (a thread reads its line into registers
              // before it writes it back; lines of one sweep are disjoint)
#pragma unroll
              for (int it = 0; it < ITC; ++it)
                if (tid + it * BLOCK < NC3)
                  bufA[tid + it * BLOCK] = ((flcur >> (16 + it)) & 1u) ? T(0) : cval[it]; // (the flag, not the index: 3 registers)
              __syncthreads();
              T cin[NC], cout[G::N];
              for (int l = tid; l < NC * NC; l += BLOCK)
                {
                  const int b0 = (l / NC) * G::N + l % NC;
#pragma unroll
                  for (int i = 0; i < NC; ++i)
                    cin[i] = bufA[l + i * NC * NC];
                  line_embed_sym<T, P, BC>(args.fused.Eh, cin, cout);
#pragma unroll
                  for (int i = 0; i < G::N; ++i)
                    bufB[b0 + i * G::N * G::N] = cout[i];
                }
              __syncthreads();
              for (int l = tid; l < NC * G::N; l += BLOCK)
                {
                  const int b0 = (l / NC) * G::N * G::N + l % NC;
#pragma unroll
                  for (int i = 0; i < NC; ++i)
                    cin[i] = bufB[b0 + i * G::N];
                  line_embed_sym<T, P, BC>(args.fused.Eh, cin, cout);
#pragma unroll
                  for (int i = 0; i < G::N; ++i)
                    bufB[b0 + i * G::N] = cout[i];
                }
              __syncthreads();
              for (int l = tid; l < G::N * G::N; l += BLOCK)
                {
                  const int b0 = l * G::N;
#pragma unroll
                  for (int i = 0; i < NC; ++i)
                    cin[i] = bufB[b0 + i];
                  line_embed_sym<T, P, BC>(args.fused.Eh, cin, cout);
#pragma unroll
                  for (int i = 0; i < G::N; ++i)
                    bufB[b0 + i] = cout[i];
                }
              __syncthreads();
              // x <- x + P x_c: shell entries owned by an un-fused patch are corrected already; this brick's own ones go to the
              // scratch vector (tail_kernel folds them into x), the interior is stored in place
#pragma unroll
              for (int it = 0; it < ITERS; ++it)
                if (spos[it] >= 0 && sgi[it] < args.gather_limit)
                  {
                    const uint32_t f2 = (flcur >> (2 * it)) & 3u;
                    if (!(f2 & 2u))
                      sval[it] += bufB[spos[it]];
                    if (f2 & 1u)
                      args.fused.scratch[sgi[it]] = sval[it];
                  }
              InteriorWalk wk = walk0;
#pragma unroll
              for (int it = 0; it < ITER; ++it, wk.next())
                if (has_entry(it))
                  {
                    xg[it] += bufB[wk.pos()];
                    NT_STORE(xg[it], &args.fused.x_inout[base + (uint32_t)(tid + it * BLOCK)]);
                  }
            }
        // ---- values of this slot -> LDS ---------------------------------------------------------------------
        if (x_from_b)
          {
#pragma unroll
            for (int it = 0; it < ITERS; ++it)
              sval[it] = args.epi.c0 * sb[it] * sval[it];
          }
#pragma unroll
        for (int it = 0; it < ITERS; ++it)
          if (spos[it] >= 0)
            bufA[spos[it]] = sgi[it] < args.gather_limit ? sval[it] : T(0);
        {
          InteriorWalk wk = walk0;
#pragma unroll
          for (int it = 0; it < ITER; ++it, wk.next())
            if (has_entry(it))
              bufA[wk.pos()] = x_from_b ? args.epi.c0 * interior_dinv(wk.type()) * bv[it] : xg[it];
        }
        __syncthreads();
        if (has_next && tid == 0)
          sched.publish(drawn, ticket_word); // (the barrier that ends the iteration publishes it)
        MGAMD_STAMP(1)

        bool any_hanging = false;
        if constexpr (brick_may_be_constrained(B, CONSTR))
          {
            // constrained bricks: whole-face / whole-edge hanging nodes (uniform branch: one mask per slot)
            any_hanging = fmcur != 0;
            if (any_hanging)
              brick_constraint_passes<T, P, B, BLOCK>(bufA, args.m, tid, 1, args.g.fmask + slot, false, &fmcur);
          }
        // cell prefetch in the streamed sweeps (-4 % on the 2-4-word passes); the 5-word mode has no registers left for it
        if constexpr (MODE == MODE_MASS) // (streamed like the operator's sweeps, with the cell prefetch; the second lattice is not touched)
          mass_sweeps<T, P, B, BLOCK, true, true, false>(bufA, args.m, tid, 1, &hcur, false);
        else
          lattice_sweeps<T, P, B, BLOCK, NoHook, true, (MODE != MODE_CHEB || sizeof(T) == 4), false, MASS>(
            bufA, bufB, args.m, tid, 1, &hcur, NoHook(), false, args.sigma, args.g.q + slot);
        if constexpr (brick_may_be_constrained(B, CONSTR))
          if (any_hanging)
            brick_constraint_passes<T, P, B, BLOCK>(bufA, args.m, tid, 1, args.g.fmask + slot, true, &fmcur);
        MGAMD_STAMP(2)

        // ---- values of the next slot: requested now, consumed at the top of the next iteration ------------------
        T xgn[ITER], svaln[ITERS], sbn[ITERS], cvaln[ITC];
        if (has_next)
          load_values(basen, sgn, fln, cgn, xgn, svaln, sbn, cvaln);

        if (FUSE_R && fused_slot)
          {
            // ---- fused restriction: the lattice becomes this brick's part of b - A x, is reduced to the coarse lattice in
            // place (x^T, y^T, z^T) and added to the coarse defect
            if constexpr (FUSE_R)
              {
                InteriorWalk wk = walk0;
#pragma unroll
                for (int it = 0; it < ITER; ++it, wk.next())
                  if (has_entry(it))
                    bufA[wk.pos()] = bv[it] - bufA[wk.pos()];
#pragma unroll
                for (int it = 0; it < ITERS; ++it)
                  if (spos[it] >= 0)
                    bufA[spos[it]] = sgi[it] < args.scatter_limit ? (((flcur >> (2 * it)) & 1u) ? sb[it] : T(0)) - bufA[spos[it]] : T(0);
                __syncthreads();
                T rin[G::N], rout[NC];
                for (int l = tid; l < G::N * G::N; l += BLOCK)
                  {
                    const int b0 = l * G::N;
#pragma unroll
                    for (int i = 0; i < G::N; ++i)
                      rin[i] = bufA[b0 + i];
                    line_embed_sym_T<T, P, BC>(args.fused.Eh, rin, rout);
#pragma unroll
                    for (int i = 0; i < NC; ++i)
                      bufA[b0 + i] = rout[i];
                  }
                __syncthreads();
                for (int l = tid; l < NC * G::N; l += BLOCK)
                  {
                    const int b0 = (l / NC) * G::N * G::N + l % NC;
#pragma unroll
                    for (int i = 0; i < G::N; ++i)
                      rin[i] = bufA[b0 + i * G::N];
                    line_embed_sym_T<T, P, BC>(args.fused.Eh, rin, rout);
#pragma unroll
                    for (int i = 0; i < NC; ++i)
                      bufA[b0 + i * G::N] = rout[i];
                  }
                __syncthreads();
                // (the last sweep leaves the coarse lattice COMPACT in the scratch lattice: linear addresses for the scatter)
                for (int l = tid; l < NC * NC; l += BLOCK)
                  {
                    const int b0 = (l / NC) * G::N + l % NC;
#pragma unroll
                    for (int i = 0; i < G::N; ++i)
                      rin[i] = bufA[b0 + i * G::N * G::N];
                    line_embed_sym_T<T, P, BC>(args.fused.Eh, rin, rout);
#pragma unroll
                    for (int i = 0; i < NC; ++i)
                      bufB[l + i * NC * NC] = rout[i];
                  }
                __syncthreads();
#pragma unroll
                for (int it = 0; it < ITC; ++it)
                  if (tid + it * BLOCK < NC3 && cgi[it] != DEV_INVALID)
                    atomic_add(&args.fused.coarse[cgi[it]], bufB[tid + it * BLOCK]);
              }
          }
        else
          {
            // ---- interior DoFs are complete: fused epilogue, contiguous stores -----------------------------------
            InteriorWalk wk = walk0;
#pragma unroll
            for (int it = 0; it < ITER; ++it, wk.next())
              if (has_entry(it))
                {
                  const uint32_t g  = base + (uint32_t)(tid + it * BLOCK);
                  const T        ax = bufA[wk.pos()];
                  T              r;
                  if (MODE == MODE_VMULT || MODE == MODE_MASS)
                    r = ax;
                  else if (MODE == MODE_RESIDUAL)
                    r = bv[it] - ax;
                  else
                    {
                      const T dv  = interior_dinv(wk.type());
                      const T xov = MODE == MODE_CHEB_SECOND ? args.epi.c0 * dv * bv[it] : xo[it];
                      const T xv  = x_from_b ? args.epi.c0 * dv * bv[it] : xg[it];
                      if (FUSE_P)
                        r = xv + args.epi.f2 * dv * (bv[it] - ax);
                      else
                        r = xv + args.epi.f1 * (xv - xov) + args.epi.f2 * dv * (bv[it] - ax);
                    }
                  if (MODE == MODE_CHEB && !FUSE_P)
                    store_result(args.epi, g, r);
                  else
                    NT_STORE(r, &args.epi.out[g]);
                }
            MGAMD_STAMP(3)
            // ---- shell DoFs: partial sums into the tail accumulator ------------------------------------------------
#pragma unroll
            for (int it = 0; it < ITERS; ++it)
              if (spos[it] >= 0 && sgi[it] < args.scatter_limit)
                atomic_add(&args.tail_acc[sgi[it] - args.n_interior], bufA[spos[it]]);
          }
        MGAMD_STAMP(4)
        if (!has_next)
          break;
        slot  = slotn;
        base  = basen;
        hcur  = hn;
        fmcur = fmn;
        flcur = fln;
#pragma unroll
        for (int it = 0; it < ITC; ++it)
          {
            cgi[it]  = cgn[it];
            cval[it] = cvaln[it];
          }
#pragma unroll
        for (int it = 0; it < ITERS; ++it)
          {
            sgi[it]  = sgn[it];
            sval[it] = svaln[it];
            sb[it]   = sbn[it];
          }
#pragma unroll
        for (int it = 0; it < ITER; ++it)
          xg[it] = xgn[it];
        __syncthreads(); // every thread has read its results of this slot from bufA
      }
  }
#undef MGAMD_STAMP
#undef MGAMD_STAMP_OWNER
#undef MGAMD_ABLATED

  // single cells, WAVE-SCOPED: a 256-thread workgroup = four wavefronts with their own cells (64 / (p+1)^2 cells each) and their
  // own LDS regions; no workgroup barrier anywhere (lattice_apply_body, WAVE)
  constexpr int CELL_WAVES = 4;
  template <typename T, int P>
  constexpr size_t
  cell_wave_lds()
  {
    using G = Geo<P, 1, 64>;
    // (the D^-1 tables of lattice_apply_body are laid out as in apply_lds_bytes: per slot at P = 1, where no wave-scoped kernel exists)
    static_assert(P >= 2, "wave-scoped cells: P >= 2 (at P = 1 the closed-form D^-1 table of lattice_apply_body is per slot, apply_lds_bytes)");
    return (((2 * (size_t)G::SPW * G::N3 + 2 * P * P * P + G::SPW) * sizeof(T) + 15) / 16) * 16;
  }

  // ---- Workgroups per CU that the one-slot-group-per-workgroup kernels are compiled for (the second __launch_bounds__
  // argument).  A CU has 160 KiB of LDS and four SIMDs with 512 VGPRs each; n 4-wave workgroups per CU are n waves per SIMD,
  // that is 512 / n VGPRs per thread (n = 6: 80, 4: 128, 3: 168, 2: 256).  The value is
  //     min(what the kernel was tuned for at the small lattices,  what the LDS of this lattice admits,  VGPR cap)
  // where the VGPR cap is the largest n whose budget holds the kernel's whole-line sweeps (three lines of P B + 1 values, the
  // gathered values and the epilogue operands) without scratch.  For p <= 4 this gives today's 4 / 6 on every lattice; the 11-,
  // 13- and 15-point lattices of p = 5, 6, 7 come out at what their LDS admits or below (DESIGN.md section 4 has the table).
  constexpr size_t CU_LDS_BYTES = 160 * 1024;
  constexpr int
  wgs_lds_admits(size_t lds_bytes)
  {
    return (int)(CU_LDS_BYTES / lds_bytes);
  }
  constexpr int
  min_of(int a, int b, int c)
  {
    return a < b ? (a < c ? a : c) : (b < c ? b : c);
  }
  // dynamic LDS of lattice_apply_small_kernel: the larger of the 2^3-brick lattices and the four wave regions of the cells
  template <typename T, int P>
  constexpr size_t
  small_slots_lds_bytes()
  {
    return apply_lds_bytes<T, P, 2>() > CELL_WAVES * cell_wave_lds<T, P>() ? apply_lds_bytes<T, P, 2>() : CELL_WAVES * cell_wave_lds<T, P>();
  }
  // VGPR caps (double: measured with -Rpass-analysis=kernel-resource-usage, tools/kernel_resources.sh; a float value is half
  // the registers and stays inside the budget of the small lattices)
  template <typename T, int P>
  constexpr int
  brick2_vgpr_cap() // 2^3 bricks: lattice_apply_kernel<P, 2> and lattice_apply_small_kernel
  {
    return (sizeof(T) == 8 && P >= 7) ? 2 : (sizeof(T) == 8 && P >= 5 ? 3 : 4); // 193 VGPRs at p = 7, 152 / 166 at p = 5 / 6
  }
  template <typename T, int P>
  constexpr int
  cell_waves_vgpr_cap() // wave-scoped single cells
  {
    return (sizeof(T) == 8 && P >= 7) ? 4 : ((sizeof(T) == 8 && P == 6) || (sizeof(T) == 4 && P >= 7) ? 5 : 6); // 122; 95, 89 VGPRs
  }
  template <typename T, int P>
  constexpr int
  small_slots_wgs_per_cu()
  {
    return min_of(4, wgs_lds_admits(small_slots_lds_bytes<T, P>()), brick2_vgpr_cap<T, P>());
  }
  template <typename T, int P, int B>
  constexpr int
  lattice_wgs_per_cu()
  {
    if constexpr (B == 2)
      return min_of(4, wgs_lds_admits(apply_lds_bytes<T, P, 2>()), brick2_vgpr_cap<T, P>());
    else
      return B == 1 ? 6 : 1;
  }
  template <typename T, int P>
  constexpr int
  cell_waves_wgs_per_cu()
  {
    return min_of(6, wgs_lds_admits(CELL_WAVES * cell_wave_lds<T, P>()), cell_waves_vgpr_cap<T, P>());
  }
  static_assert(small_slots_wgs_per_cu<double, 2>() == 4 && small_slots_wgs_per_cu<double, 3>() == 4 && small_slots_wgs_per_cu<double, 4>() == 4 &&
                  small_slots_wgs_per_cu<float, 4>() == 4 && lattice_wgs_per_cu<double, 1, 2>() == 4 && lattice_wgs_per_cu<double, 4, 2>() == 4 &&
                  lattice_wgs_per_cu<float, 3, 2>() == 4 && lattice_wgs_per_cu<double, 1, 1>() == 6 && lattice_wgs_per_cu<double, 3, 4>() == 1 &&
                  cell_waves_wgs_per_cu<double, 2>() == 6 && cell_waves_wgs_per_cu<double, 3>() == 6 && cell_waves_wgs_per_cu<double, 4>() == 6 &&
                  cell_waves_wgs_per_cu<float, 4>() == 6,
                "the kernels of p <= 4 keep the occupancy bounds they were measured with");

  template <typename T, int P, int B, int MODE, bool CONSTR = false>
  __global__ void
  __launch_bounds__((Geo<P, B>::ABLOCK), (lattice_wgs_per_cu<T, P, B>())) lattice_apply_kernel(const ApplyArgs<T, P> args)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    lattice_apply_body<T, P, B, MODE, CONSTR>(args, blockIdx.x, gridDim.x, smem_raw);
  }
  template <typename T, int P, int MODE, bool MASS = true>
  __device__ __forceinline__ void
  cell_waves_body(const ApplyArgs<T, P> &args, const uint32_t block, const uint32_t nblocks, unsigned char *smem_raw)
  {
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t n_w  = (args.g.n_slots + Geo<P, 1, 64>::SPW - 1) / Geo<P, 1, 64>::SPW; // wavefronts with work
    // workgroups in XCD-contiguous (Morton) ranges like every other kernel, the four wavefronts of one on neighbouring cells
    const uint32_t vb = xcd_contiguous(block, nblocks) * CELL_WAVES + wave;
    if (vb < n_w)
      lattice_apply_body<T, P, 1, MODE, false, true, 0, MASS>(args, vb, n_w, smem_raw + wave * cell_wave_lds<T, P>());
  }
  template <typename T, int P, int MODE>
  __global__ void
  __launch_bounds__(64 * CELL_WAVES, (cell_waves_wgs_per_cu<T, P>())) cell_waves_kernel(const ApplyArgs<T, P> args)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    cell_waves_body<T, P, MODE>(args, blockIdx.x, gridDim.x, smem_raw);
  }

  // persistent workgroups (lattice_apply_persistent_body); the grid is the number of RESIDENT workgroups (runtime.hip)
  // workgroups per CU: two f64 lattice pairs fill the LDS; three f32 pairs would fit, and at p = 4 the float kernels can be held
  // to 168 VGPRs, but measured no gain (octant p = 4 float 7.07 vs 6.73 ms per V-cycle, boxes 4 % apart): two everywhere
  template <typename T, int P>
  constexpr int
  persistent_wgs_per_cu()
  {
    return 2;
  }
  template <typename T, int P, int B, int MODE, bool CONSTR, bool MASS>
  __global__ void
  __launch_bounds__((Geo<P, B>::ABLOCK), (persistent_wgs_per_cu<T, P>())) lattice_apply_persistent_kernel(const ApplyArgs<T, P> args)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    lattice_apply_persistent_body<T, P, B, MODE, CONSTR, MASS>(args, blockIdx.x, gridDim.x, smem_raw);
  }

  // The plain and the constrained bricks of one size in ONE launch (same lattice, same LDS, same block size): the
  // constrained group alone is a fraction of a round of workgroups on most levels.  Two inlined copies of the body: the plain
  // bricks keep the lean instruction stream (the embedding passes are only in the second copy).
  template <typename T, int P>
  struct BrickPairArgs
  {
    ApplyArgs<T, P> a;             // a.g = the plain group
    SlotGroupDev    g_constrained; // the constrained bricks of the same size
    uint32_t        n_wg_plain;
  };
  static_assert(sizeof(BrickPairArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "BrickPairArgs exceeds the kernel-argument segment");
  template <typename T, int P, int B, int MODE>
  __global__ void
  __launch_bounds__((Geo<P, B>::ABLOCK), 1) lattice_apply_pair_kernel(const BrickPairArgs<T, P> args)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    if (blockIdx.x < args.n_wg_plain)
      lattice_apply_body<T, P, B, MODE, false>(args.a, blockIdx.x, args.n_wg_plain, smem_raw);
    else
      {
        ApplyArgs<T, P> a = args.a;
        a.g               = args.g_constrained;
        a.stamps          = nullptr;
        lattice_apply_body<T, P, B, MODE, true>(a, blockIdx.x - args.n_wg_plain, gridDim.x - args.n_wg_plain, smem_raw);
      }
  }

  // (A 512-thread variant with half-line sweep tasks - 4 waves per SIMD, <= 128 VGPRs - was measured on MI355X: the sweeps alone
  // are 19 % faster (tools/sweep_probe.hip), the kernel is not: vmult 950 -> 964 us per pass, and the Chebyshev modes spill.)
  // the pair launch with persistent workgroups.  n_wg_plain > 0 (all slots resident at once): the first n_wg_plain workgroups
  // take one plain brick each, the others one constrained brick each; n_wg_plain == 0: see below
  template <typename T, int P, int B, int MODE, bool MASS>
  __global__ void
  __launch_bounds__((Geo<P, B>::ABLOCK), 2) lattice_apply_persistent_pair_kernel(const BrickPairArgs<T, P> args)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    if (args.n_wg_plain == 0)
      {
        // more slots than resident workgroups: EVERY workgroup walks its share of the constrained bricks, then its share
        // of the plain ones (a static split of the workgroups between the two kinds is only balanced for one cost ratio:
        // measured 1.59 / 1.52 / 1.50 / 1.54 ms per octant p=1 V-cycle for assumed ratios 1.3 / 1.7 / 2.2 / 3.0)
        ApplyArgs<T, P> a = args.a;
        a.g               = args.g_constrained;
        a.stamps          = nullptr;
        a.tickets += 8; // (the constrained half has a walk of its own: the second set of counters)
        lattice_apply_persistent_body<T, P, B, base_mode(MODE), true, MASS>(a, blockIdx.x, gridDim.x, smem_raw);
        __syncthreads(); // the lattice of the last constrained brick has been read by every thread
        lattice_apply_persistent_body<T, P, B, MODE, false, MASS>(args.a, blockIdx.x, gridDim.x, smem_raw);
      }
    else if (blockIdx.x < args.n_wg_plain)
      lattice_apply_persistent_body<T, P, B, MODE, false, MASS>(args.a, blockIdx.x, args.n_wg_plain, smem_raw);
    else
      {
        ApplyArgs<T, P> a = args.a;
        a.g               = args.g_constrained;
        a.stamps          = nullptr;
        a.tickets += 8;
        lattice_apply_persistent_body<T, P, B, base_mode(MODE), true, MASS>(a, blockIdx.x - args.n_wg_plain, gridDim.x - args.n_wg_plain, smem_raw);
      }
  }

  // The 2^3 bricks and the single cells of a level in ONE launch (both have 256-thread workgroups and 20-35 KB of LDS):
  // on levels where each of them is a fraction of one round of workgroups, a launch costs a workgroup lifetime whatever
  // it does.  (Merging the 17^3 bricks in as well was measured slower: every workgroup then reserves their 78 KB.)
  template <typename T, int P>
  struct SmallSlotsArgs
  {
    ApplyArgs<T, P> a;       // a.g = the 2^3-brick group
    SlotGroupDev    g_cells; // the single-cell group
    uint32_t        n_wg_bricks;
  };
  static_assert(sizeof(SmallSlotsArgs<double, MAX_KERNEL_DEGREE>) <= KERNARG_LIMIT, "SmallSlotsArgs exceeds the kernel-argument segment");
  // The kernel comes with the mass term compiled in and compiled out (MASS, both halves), for every degree and number type, and
  // the host picks by sigma != 0 (launch_bricks_and_cells).  First the float kernel of p = 7, which sits at the 128 VGPRs of its
  // four workgroups per CU and spilled with a run-time sigma; with the diffusion coefficient every degree: the mass term reads
  // h^2 / a of the slot at the x sweep (lattice_sweeps), a load that the sigma = 0 cycle of the flagship paid with +0.2 ... +0.7 %
  // per V-cycle when sigma was a run-time value here (DESIGN.md "Diffusion coefficient"); MASS = false never reads it.
  template <typename T, int P, int MODE, bool MASS = true>
  __global__ void
  __launch_bounds__(256, (small_slots_wgs_per_cu<T, P>())) lattice_apply_small_kernel(const SmallSlotsArgs<T, P> args)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    if (blockIdx.x < args.n_wg_bricks)
      lattice_apply_body<T, P, 2, MODE, false, false, 256, MASS>(args.a, blockIdx.x, args.n_wg_bricks, smem_raw);
    else
      {
        ApplyArgs<T, P> a = args.a;
        a.g               = args.g_cells;
        a.stamps          = nullptr;
        cell_waves_body<T, P, MODE, MASS>(a, blockIdx.x - args.n_wg_bricks, gridDim.x - args.n_wg_bricks, smem_raw);
      }
  }

  // K1c: the level operator on SINGLE CELLS at p = 1, one cell per thread, 256 consecutive (Morton) cells per
  // workgroup (a CLUSTER).  The generic kernel spends one scattered load and one global atomic per (cell, node):
  // 8 of each per cell at p = 1, which bounds it at ~35 G atomics/s (measured: removing the atomics halves its time).
  // Here every distinct node of the cluster is loaded once into LDS, the cell operator runs in registers (2x2x2 lattice,
  // hanging-node interpolation included), results are pre-reduced with LDS atomics and every distinct node costs ONE
  // global atomic.  All nodes of such cells are tail DoFs, so the kernel is the same for every epilogue mode.
  struct CellClusterDev
  {
    const uint32_t *uniq_ptr; // [n_clusters + 1] into uniq_idx
    const uint32_t *uniq_idx; // global DoF index of every cluster-local node (ascending within a cluster)
    const uint16_t *loc;      // [n_slots * 8] cluster-local id of lattice node x + 2y + 4z; 0xFFFF = constrained (zero, no scatter)
    const uint16_t *mask;
    const double   *h; // the scale of the pass, as SlotGroupDev::h
    uint32_t        n_slots;
    uint32_t        max_uniq; // LDS: 2 * max_uniq values
    const double   *q;        // h^2 / a, as SlotGroupDev::q
  };
  constexpr int CLUSTER_CELLS = 256;
  constexpr int CLUSTER_ITERS = 8; // 256 cells x 8 nodes / 256 threads: the worst case, nothing shared

  template <typename T>
  struct ClusterArgs
  {
    CellClusterDev c;
    Mats<1, T>     m;
    const T       *src;
    T             *tail_acc;
    uint32_t       n_interior;
    // from_b = 1: the input is c0 dinv b (Epilogue::from_b), never stored
    const T *b, *dinv;
    T        c0;
    int      from_b;
    uint32_t cluster_offset; // first cluster of this launch (the halo / interior split of sharded levels)
    double   sigma = 0.0;    // mass coefficient of K + sigma M (ApplyArgs::sigma)
  };
  static_assert(sizeof(ClusterArgs<double>) <= KERNARG_LIMIT, "ClusterArgs exceeds the kernel-argument segment");

  template <typename T, bool TRANSPOSE>
  __device__ __forceinline__ void
  hanging_in_registers_p1(T (&x)[8], const uint32_t mask, const Mats<1, T> &m)
  {
    const int  cx = mask & 1, cy = (mask >> 1) & 1, cz = (mask >> 2) & 1;
    const bool fx = (mask >> 3) & 1, fy = (mask >> 4) & 1, fz = (mask >> 5) & 1;
    const bool ex = (mask >> 6) & 1, ey = (mask >> 7) & 1, ez = (mask >> 8) & 1;
#pragma unroll
    for (int dd = 0; dd < 3; ++dd)
      {
        const int d = TRANSPOSE ? 2 - dd : dd;
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
          for (int u = 0; u < 2; ++u)
            {
              bool on;
              int  c;
              // same line classification as hanging_passes with P = 1
              if (d == 0)
                {
                  const bool ou = u == cy, ov = v == cz;
                  on            = (fy && ou) || (fz && ov) || (ex && ou && ov);
                  c             = cx;
                }
              else if (d == 1)
                {
                  const bool ou = u == cx, ov = v == cz;
                  on            = (fx && ou) || (fz && ov) || (ey && ou && ov);
                  c             = cy;
                }
              else
                {
                  const bool ou = u == cx, ov = v == cy;
                  on            = (fx && ou) || (fy && ov) || (ez && ou && ov);
                  c             = cz;
                }
              const int i0 = d == 0 ? (v * 2 + u) * 2 : (d == 1 ? v * 4 + u : v * 2 + u);
              const int i1 = i0 + (d == 0 ? 1 : (d == 1 ? 2 : 4));
              if (on)
                {
                  const T *w       = c ? m.I1 : m.I0;
                  const T       a0 = x[i0], a1 = x[i1];
                  if (TRANSPOSE)
                    {
                      x[i0] = T(w[0]) * a0 + T(w[2]) * a1;
                      x[i1] = T(w[1]) * a0 + T(w[3]) * a1;
                    }
                  else
                    {
                      x[i0] = T(w[0]) * a0 + T(w[1]) * a1;
                      x[i1] = T(w[2]) * a0 + T(w[3]) * a1;
                    }
                }
            }
      }
  }

  // MASS_ONLY (MODE_MASS): the cell's mass matrix h^3 M (x) M (x) M instead of the operator
  template <typename T, bool MASS_ONLY = false>
  __device__ __forceinline__ void
  cell_cluster_body(const ClusterArgs<T> &a, const uint32_t block, const uint32_t nblocks, unsigned char *smem_raw)
  {
    T *U   = reinterpret_cast<T *>(smem_raw);
    T *Acc = U + a.c.max_uniq;

    const int      tid  = threadIdx.x;
    const uint32_t cl   = a.cluster_offset + xcd_contiguous(block, nblocks);
    const uint32_t slot = cl * CLUSTER_CELLS + tid;
    const bool     act  = slot < a.c.n_slots;
    const uint32_t p0   = a.c.uniq_ptr[cl];
    const int      nu   = (int)(a.c.uniq_ptr[cl + 1] - p0);

    // the cell's own table entries: requested first, consumed after the barrier
    const uint4    lw   = reinterpret_cast<const uint4 *>(a.c.loc)[act ? slot : 0];
    const uint32_t mask = act ? a.c.mask[slot] : 0u;
    const T        h    = act ? T(a.c.h[slot]) : T(0);

    // distinct nodes of the cluster -> LDS (all loads in flight before the first use)
    uint32_t gi[CLUSTER_ITERS];
    T        gv[CLUSTER_ITERS];
#pragma unroll
    for (int k = 0; k < CLUSTER_ITERS; ++k)
      {
        const int j = tid + k * CLUSTER_CELLS;
        gi[k]       = nu > 0 ? a.c.uniq_idx[p0 + (j < nu ? j : nu - 1)] : a.n_interior;
      }
    if (a.from_b == 1)
      {
        T gb[CLUSTER_ITERS];
#pragma unroll
        for (int k = 0; k < CLUSTER_ITERS; ++k)
          {
            gv[k] = a.dinv[gi[k]];
            gb[k] = a.b[gi[k]];
          }
#pragma unroll
        for (int k = 0; k < CLUSTER_ITERS; ++k)
          gv[k] = a.c0 * gv[k] * gb[k];
      }
    else
      {
#pragma unroll
        for (int k = 0; k < CLUSTER_ITERS; ++k)
          gv[k] = a.src[gi[k]];
      }
#pragma unroll
    for (int k = 0; k < CLUSTER_ITERS; ++k)
      {
        const int j = tid + k * CLUSTER_CELLS;
        if (j < nu)
          {
            U[j]   = gv[k];
            Acc[j] = T(0);
          }
      }
    __syncthreads();

    uint32_t      l[8];
    const uint32_t lw4[4] = {lw.x, lw.y, lw.z, lw.w};
    T             x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      {
        l[i] = (lw4[i / 2] >> (16 * (i % 2))) & 0xFFFFu;
        x[i] = (act && l[i] != 0xFFFFu) ? U[l[i]] : T(0);
      }
    if (mask >> 3)
      hanging_in_registers_p1<T, false>(x, mask, a.m);
    // three sweeps of the 2x2x2 lattice, as in lattice_sweeps
    const T M0 = T(a.m.M[0]), M1 = T(a.m.M[1]), M2 = T(a.m.M[2]), M3 = T(a.m.M[3]);
    const T K0 = T(a.m.K[0]), K1 = T(a.m.K[1]), K2 = T(a.m.K[2]), K3 = T(a.m.K[3]);
    // sigma h^2 / a: (a h) (K x + M (b + c x)) adds sigma h^3 M (x) M (x) M  (MASS_ONLY: no mass term, h is the cell size)
    T cm = T(0);
    if (!MASS_ONLY && act && a.sigma != 0.0)
      cm = T(a.sigma) * T(a.c.q[slot]);
    T       A[8], Bv[8];
    if constexpr (MASS_ONLY)
      { // three mass products of the 2x2x2 lattice in place (mass_sweeps): z, y, x; x scales by h^3
        const T h3 = h * h * h;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          {
            const T r0 = x[q], r1 = x[q + 4];
            A[q]       = M0 * r0 + M1 * r1;
            A[q + 4]   = M2 * r0 + M3 * r1;
          }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          {
            const int i0 = (q & 1) + 4 * (q >> 1);
            const T   a0 = A[i0], a1 = A[i0 + 2];
            A[i0]        = M0 * a0 + M1 * a1;
            A[i0 + 2]    = M2 * a0 + M3 * a1;
          }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          {
            const T a0 = A[2 * q], a1 = A[2 * q + 1];
            x[2 * q]     = h3 * (M0 * a0 + M1 * a1);
            x[2 * q + 1] = h3 * (M2 * a0 + M3 * a1);
          }
      }
    else
      {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          { // z lines: nodes q, q + 4
            const T r0 = x[q], r1 = x[q + 4];
            A[q]       = M0 * r0 + M1 * r1;
            A[q + 4]   = M2 * r0 + M3 * r1;
            Bv[q]      = K0 * r0 + K1 * r1;
            Bv[q + 4]  = K2 * r0 + K3 * r1;
          }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          { // y lines: nodes i0, i0 + 2 with i0 = x + 4z
            const int i0 = (q & 1) + 4 * (q >> 1);
            const T   a0 = A[i0], a1 = A[i0 + 2], b0 = Bv[i0], b1 = Bv[i0 + 2];
            A[i0]        = M0 * a0 + M1 * a1;
            A[i0 + 2]    = M2 * a0 + M3 * a1;
            Bv[i0]       = K0 * a0 + K1 * a1 + M0 * b0 + M1 * b1;
            Bv[i0 + 2]   = K2 * a0 + K3 * a1 + M2 * b0 + M3 * b1;
          }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          { // x lines: nodes 2q, 2q + 1; the mass term as in lattice_sweeps: b += c a
            const T a0 = A[2 * q], a1 = A[2 * q + 1], b0 = Bv[2 * q] + cm * a0, b1 = Bv[2 * q + 1] + cm * a1;
            x[2 * q]     = h * (K0 * a0 + K1 * a1 + M0 * b0 + M1 * b1);
            x[2 * q + 1] = h * (K2 * a0 + K3 * a1 + M2 * b0 + M3 * b1);
          }
      }
    if (mask >> 3)
      hanging_in_registers_p1<T, true>(x, mask, a.m);
    if (act)
      {
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (l[i] != 0xFFFFu)
            atomic_add(&Acc[l[i]], x[i]);
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CLUSTER_ITERS; ++k)
      {
        const int j = tid + k * CLUSTER_CELLS;
        if (j < nu)
          atomic_add(&a.tail_acc[gi[k] - a.n_interior], Acc[j]);
      }
  }

  template <typename T>
  __global__ void
  __launch_bounds__(CLUSTER_CELLS) cell_cluster_apply_kernel(const ClusterArgs<T> a)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    cell_cluster_body<T>(a, blockIdx.x, gridDim.x, smem_raw);
  }
  // MODE_MASS (a kernel of its own: the operator's cluster kernel is the same for every other mode and keeps its name)
  template <typename T>
  __global__ void
  __launch_bounds__(CLUSTER_CELLS) cell_cluster_mass_kernel(const ClusterArgs<T> a)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    cell_cluster_body<T, true>(a, blockIdx.x, gridDim.x, smem_raw);
  }

  // p = 1: the 8^3 bricks and the cell clusters of a level in one launch (same reason as lattice_apply_small_kernel)
  template <typename T>
  struct P1SmallArgs
  {
    ApplyArgs<T, 1> a; // a.g = the 8^3-brick group
    ClusterArgs<T>  c;
    uint32_t        n_wg_bricks;
  };
  static_assert(sizeof(P1SmallArgs<double>) <= KERNARG_LIMIT, "P1SmallArgs exceeds the kernel-argument segment");
  template <typename T, int MODE>
  __global__ void
  __launch_bounds__(256) lattice_cluster_kernel(const P1SmallArgs<T> args)
  {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    if (blockIdx.x < args.n_wg_bricks)
      lattice_apply_body<T, 1, 8, MODE>(args.a, blockIdx.x, args.n_wg_bricks, smem_raw);
    else
      cell_cluster_body<T, MODE == MODE_MASS>(args.c, blockIdx.x - args.n_wg_bricks, gridDim.x - args.n_wg_bricks, smem_raw);
  }

  // Diagonal of C^T (K + sigma M) C.  Slots without hanging nodes: closed tensor form; single cells with hanging
  // faces/edges: one unit vector per local node through interpolation, sweeps and transpose.
  template <typename T, int P, int B, bool CONSTR = false>
  __global__ void
  __launch_bounds__((Geo<P, B>::BLOCK)) lattice_diag_kernel(const ApplyArgs<T, P> args)
  {
    using G = Geo<P, B>;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T *bufA = reinterpret_cast<T *>(smem_raw);
    T *bufB = bufA + G::SPW * G::N3;
    T *bufD = bufB + G::SPW * G::N3;

    const int tid    = threadIdx.x;
    const int slot0  = blockIdx.x * G::SPW;
    const int nslots = min((int)G::SPW, (int)args.g.n_slots - slot0);
    const int sl     = tid / G::LINES;
    const int ln     = tid % G::LINES;
    const int u = ln % G::N, v = ln / G::N;
    const bool act = tid < G::SPW * G::LINES && sl < nslots;

    uint32_t mask = 0;
    T        h    = T(0), q = T(0);
    if (act)
      {
        h = T(args.g.h[slot0 + sl]); // a h
        q = T(args.g.q[slot0 + sl]); // h^2 / a
        if (B == 1)
          mask = args.g.mask[slot0 + sl];
      }
    // closed form: thread (u,v) = (x,y) fills its z column
    if (act)
      {
        T dM[G::N], dK[G::N];
#pragma unroll
        for (int i = 0; i < G::N; ++i)
          dM[i] = dK[i] = T(0);
#pragma unroll
        for (int c = 0; c < B; ++c)
#pragma unroll
          for (int a = 0; a <= P; ++a)
            {
              dM[c * P + a] += T(args.m.M[a * (P + 1) + a]);
              dK[c * P + a] += T(args.m.K[a * (P + 1) + a]);
            }
        const T sh3 = T(args.sigma) * q * h; // d = a h s_K + sigma h^3 s_M,  h^3 = (h^2 / a) (a h)
        T       mx = T(0), kx = T(0), my = T(0), ky = T(0);
#pragma unroll
        for (int i = 0; i < G::N; ++i)
          {
            if (i == u)
              {
                mx = dM[i];
                kx = dK[i];
              }
            if (i == v)
              {
                my = dM[i];
                ky = dK[i];
              }
          }
#pragma unroll
        for (int i = 0; i < G::N; ++i)
          bufD[sl * G::N3 + (i * G::N + v) * G::N + u] = h * (kx * my * dM[i] + mx * ky * dM[i] + mx * my * dK[i]) + sh3 * (mx * my * dM[i]);
      }
    __syncthreads();
    if (B == 1)
      {
        const bool any_hanging = __syncthreads_or((int)(mask >> 3)) != 0;
        if (any_hanging)
          for (int j = 0; j < G::N3; ++j)
            {
              // e_j on every slot of this workgroup
              for (int idx = tid; idx < G::SPW * G::N3; idx += G::BLOCK)
                bufA[idx] = (idx % G::N3) == j ? T(1) : T(0);
              __syncthreads();
              hanging_passes<T, P>(bufA, args.m, sl, u, v, act, mask, false);
              lattice_sweeps<T, P, B, G::BLOCK>(bufA, bufB, args.m, tid, nslots, args.g.h + slot0, NoHook(), false, args.sigma, args.g.q + slot0);
              hanging_passes<T, P>(bufA, args.m, sl, u, v, act, mask, true);
              if (act && ln == 0 && (mask >> 3))
                bufD[sl * G::N3 + j] = bufA[sl * G::N3 + j];
              __syncthreads();
            }
      }
    if constexpr (brick_may_be_constrained(B, CONSTR))
      {
        // constrained bricks: the parent DoFs on hanging faces/edges need (C^T A C)_jj: one unit vector per shell
        // position through embedding, sweeps and transpose (the other shell entries reproduce the closed form)
        uint32_t fm = 0;
        if (args.g.fmask != nullptr && tid < nslots)
          fm = args.g.fmask[slot0 + tid];
        const bool any_family = __syncthreads_or((int)(fm != 0)) != 0;
        if (any_family)
          for (int s = 0; s < G::N_SHELL; ++s)
            {
              const int j = args.g.shell_pos[s];
              for (int idx = tid; idx < G::SPW * G::N3; idx += G::BLOCK)
                bufA[idx] = (idx % G::N3) == j ? T(1) : T(0);
              __syncthreads();
              brick_constraint_passes<T, P, B, G::BLOCK>(bufA, args.m, tid, nslots, args.g.fmask + slot0, false);
              lattice_sweeps<T, P, B, G::BLOCK>(bufA, bufB, args.m, tid, nslots, args.g.h + slot0, NoHook(), false, args.sigma, args.g.q + slot0);
              brick_constraint_passes<T, P, B, G::BLOCK>(bufA, args.m, tid, nslots, args.g.fmask + slot0, true);
              if (act && ln == 0 && args.g.fmask[slot0 + sl])
                bufD[sl * G::N3 + j] = bufA[sl * G::N3 + j];
              __syncthreads();
            }
      }
    if (G::N_INT > 0)
      for (int idx = tid; idx < nslots * G::N_INT; idx += G::BLOCK)
        {
          const int sl2 = idx / (G::N_INT > 0 ? G::N_INT : 1), i = idx % (G::N_INT > 0 ? G::N_INT : 1);
          const int x = i % (G::NI > 0 ? G::NI : 1), y = (i / (G::NI > 0 ? G::NI : 1)) % (G::NI > 0 ? G::NI : 1),
                    z = i / (G::NI > 0 ? G::NI * G::NI : 1);
          const T d = bufD[sl2 * G::N3 + ((z + 1) * G::N + (y + 1)) * G::N + x + 1];
          apply_epilogue<T, MODE_INVDIAG>(args.epi, args.g.interior_base[slot0 + sl2] + i, d);
        }
    for (int idx = tid; idx < nslots * G::N_SHELL; idx += G::BLOCK)
      {
        const int      sl2 = idx / G::N_SHELL, s = idx % G::N_SHELL;
        const uint32_t gi  = args.g.shell_idx[(size_t)(slot0 + sl2) * G::N_SHELL + s];
        if (gi < args.scatter_limit)
          atomic_add(&args.tail_acc[gi - args.n_interior], bufD[sl2 * G::N3 + args.g.shell_pos[s]]);
      }
  }

  // Convective (Robin) faces: the face term  sum_f beta_f B_f x  of the operator, matrix-free, added into the accumulator of the
  // tail rows before their epilogue (every boundary DoF that is neither Dirichlet nor hanging is a tail row).  One entry of the
  // face table (level_tables.hpp, RobinFaces) is one boundary cell face with N2 = (P+1)^2 nodes: gather, interpolation C2 on the
  // flagged hanging lines, M along u, M along v, scale beta h^2, C2^T, atomic add.
  // Packing: a workgroup of 256 threads holds 256 / N2 faces at a time, one thread per face node (64, 28, 16, 10, 7, 5, 4 faces for
  // P = 1..7: at most 11 of the 256 lanes have no node), two LDS buffers of one value per node that the six 1D passes ping-pong
  // between, and walks the groups of faces with a grid stride.  The gather and the atomic adds are one 4- or 8-byte access per
  // lane at scattered rows, as the shell entries of the slot kernels are.
  // X_FROM_B: MODE_CHEB_FIRST, the source x = c0 D^-1 b is never stored and is formed here (D^-1 through the byte codes of the
  // tail rows where the pass has them).  DIAG: the diagonal of the face term, one unit vector per face node through the same passes.
  template <typename T, int P>
  struct RobinArgs
  {
    const uint32_t *idx;   // [n_faces][N2], DEV_INVALID on Dirichlet DoFs
    const uint8_t  *flags; // [n_faces]
    const double   *scale; // [n_faces] beta h^2
    uint32_t        n_faces;
    T               M[(P + 1) * (P + 1)], I0[(P + 1) * (P + 1)], I1[(P + 1) * (P + 1)];
    const T        *src;
    T              *tail_acc;
    uint32_t        n_interior, gather_limit, scatter_limit;
    // X_FROM_B only
    const T       *b, *dinv;
    T              c0;
    const uint8_t *dinv_code;
    const T       *dinv_table;
  };
  template <int P>
  constexpr int
  robin_faces_per_workgroup()
  {
    return 256 / ((P + 1) * (P + 1));
  }

  template <typename T, int P, bool X_FROM_B, bool DIAG>
  __global__ void
  __launch_bounds__(256) robin_face_kernel(RobinArgs<T, P> a)
  {
    constexpr int N = P + 1, N2 = N * N, FPB = robin_faces_per_workgroup<P>();
    __shared__ T  bufA[FPB * N2], bufB[FPB * N2], sM[N2], sI[2 * N2];
    const int     tid = threadIdx.x;
    for (int i = tid; i < N2; i += 256)
      {
        sM[i]      = a.M[i];
        sI[i]      = a.I0[i];
        sI[N2 + i] = a.I1[i];
      }
    const int      fl = tid / N2, node = tid - fl * N2, au = node % N, av = node / N;
    T             *A = bufA + (fl < FPB ? fl : 0) * N2, *B = bufB + (fl < FPB ? fl : 0) * N2;
    const uint32_t n_groups = (a.n_faces + FPB - 1) / FPB;
    for (uint32_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) // (uniform over the workgroup: the barriers below are safe)
      {
        const uint32_t face = grp * FPB + fl;
        const bool     act  = fl < FPB && face < a.n_faces;
        uint32_t       gi = DEV_INVALID, flg = 0;
        T              scale = T(0);
        if (act)
          {
            gi    = a.idx[(size_t)face * N2 + node];
            flg   = a.flags[face];
            scale = (T)a.scale[face];
          }
        const bool on_u = (flg & 1u) && av == (int)((flg >> 3) & 1u) * P; // this node's line along u hangs
        const bool on_v = (flg & 2u) && au == (int)((flg >> 2) & 1u) * P; // this node's line along v hangs
        const T   *Iu = sI + ((flg >> 2) & 1u) * N2, *Iv = sI + ((flg >> 3) & 1u) * N2;
        const bool gathered = act && gi < a.gather_limit;
        T          x = T(0);
        if (!DIAG && gathered)
          {
            if (X_FROM_B)
              {
                T d;
                if (a.dinv_code != nullptr && gi >= a.n_interior) // (entry i of the codes belongs to DoF n_interior + i)
                  {
                    const uint32_t c = a.dinv_code[gi - a.n_interior];
                    d                = c != 255u ? a.dinv_table[c] : a.dinv[gi];
                  }
                else
                  d = a.dinv[gi];
                x = a.c0 * d * a.b[gi];
              }
            else
              x = a.src[gi];
          }
        T result = T(0);
        for (int j = 0; j < (DIAG ? N2 : 1); ++j)
          {
            if (DIAG)
              x = (gathered && node == j) ? T(1) : T(0);
            if (act)
              A[node] = x;
            __syncthreads();
            T v = T(0);
            if (act) // C2 along u
              {
                v = A[node];
                if (on_u)
                  {
                    v = T(0);
#pragma unroll
                    for (int b = 0; b < N; ++b)
                      v += Iu[au * N + b] * A[av * N + b];
                  }
                B[node] = v;
              }
            __syncthreads();
            if (act) // C2 along v
              {
                v = B[node];
                if (on_v)
                  {
                    v = T(0);
#pragma unroll
                    for (int b = 0; b < N; ++b)
                      v += Iv[av * N + b] * B[b * N + au];
                  }
                A[node] = v;
              }
            __syncthreads();
            if (act) // M along u
              {
                v = T(0);
#pragma unroll
                for (int b = 0; b < N; ++b)
                  v += sM[au * N + b] * A[av * N + b];
                B[node] = v;
              }
            __syncthreads();
            if (act) // M along v, beta h^2
              {
                v = T(0);
#pragma unroll
                for (int b = 0; b < N; ++b)
                  v += sM[av * N + b] * B[b * N + au];
                A[node] = scale * v;
              }
            __syncthreads();
            if (act) // C2^T along v
              {
                v = A[node];
                if (on_v)
                  {
                    v = T(0);
#pragma unroll
                    for (int b = 0; b < N; ++b)
                      v += Iv[b * N + av] * A[b * N + au];
                  }
                B[node] = v;
              }
            __syncthreads();
            if (act) // C2^T along u
              {
                v = B[node];
                if (on_u)
                  {
                    v = T(0);
#pragma unroll
                    for (int b = 0; b < N; ++b)
                      v += Iu[b * N + au] * B[av * N + b];
                  }
                if (!DIAG || node == j)
                  result = v;
              }
          }
        if (act && gi >= a.n_interior && gi < a.scatter_limit)
          atomic_add(&a.tail_acc[gi - a.n_interior], result);
      }
  }

  // Epilogue for the tail (accumulated shell sums) and the constrained DoFs (identity rows:
  // ref:include/operator.h:170-172; MODE_MASS: zero rows); re-zeroes the accumulator for the next application.
  // tail_rows is the epilogue of the U rows row[u] (tail index; row >= n_tail: a constrained DoF) with live[u]; the two kernels
  // below differ in the rows they hand it: tail_kernel a contiguous range, tail_runs_kernel a list of runs.
  constexpr int TAIL_U = 4;
  template <typename T, int MODE_>
  __device__ __forceinline__ void
  tail_rows(T *__restrict__ tail_acc, const uint32_t n_interior, const uint32_t n_tail, const uint32_t (&row)[TAIL_U], const bool (&live)[TAIL_U],
            const Epilogue<T> &epi, const T *dtable, const bool coded)
  {
    constexpr int  MODE   = base_mode(MODE_); // (MODE_RESIDUAL_RESTRICT: plain residual rows for the un-fused restriction)
    constexpr bool FUSE_P = MODE_ == MODE_CHEB_PROLONGATE;
    constexpr int  U      = TAIL_U;
    T ax[U], xv[U], xo[U], bv[U], dv[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      {
        const uint32_t i  = row[u];
        const uint32_t gi = n_interior + i;
        ax[u] = xv[u] = xo[u] = bv[u] = dv[u] = T(0);
        if (live[u])
          {
            if (MODE != MODE_INVDIAG && MODE != MODE_CHEB_FIRST && MODE != MODE_MASS && (is_cheb(MODE) || i >= n_tail))
              {
                if (FUSE_P && i < n_tail && NT_LOAD(&epi.xs_flag[i]))
                  { // x + P x_c as the owning fused brick left it: folded into x here, after every brick has gathered x
                    xv[u] = NT_LOAD(&epi.xs[gi]);
                    epi.x_inout[gi] = xv[u];
                  }
                else
                  xv[u] = NT_LOAD(&epi.x[gi]);
              }
            ax[u] = i < n_tail ? tail_acc[i] : xv[u]; // (MODE_MASS: x is not read and the rows of constrained DoFs are zero)
            if (MODE == MODE_RESIDUAL || is_cheb(MODE))
              bv[u] = NT_LOAD(&epi.b[gi]);
            if (is_cheb(MODE))
              {
                if (MODE == MODE_CHEB && epi.xold)
                  xo[u] = NT_LOAD(&epi.xold[gi]);
                if (coded)
                  {
                    const uint32_t c = NT_LOAD(&epi.dinv_code[i]);
                    dv[u]            = c != 255u ? dtable[c] : epi.dinv[gi];
                  }
                else
                  dv[u] = epi.dinv[gi];
              }
          }
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
      {
        const uint32_t i  = row[u];
        const uint32_t gi = n_interior + i;
        if (live[u])
          {
            if (i < n_tail)
              NT_STORE(T(0), &tail_acc[i]);
            if (MODE == MODE_CHEB_FIRST || MODE == MODE_CHEB_SECOND)
              {
                const T x1 = epi.c0 * dv[u] * bv[u];
                if (MODE == MODE_CHEB_FIRST)
                  {
                    xv[u] = x1;
                    if (i >= n_tail)
                      ax[u] = x1; // identity row
                  }
                else
                  xo[u] = x1;
              }
            if (MODE == MODE_VMULT || MODE == MODE_MASS)
              NT_STORE(ax[u], &epi.out[gi]);
            else if (MODE == MODE_RESIDUAL)
              NT_STORE(bv[u] - ax[u], &epi.out[gi]);
            else if (is_cheb(MODE))
              {
                const T r = xv[u] + epi.f1 * (xv[u] - xo[u]) + epi.f2 * dv[u] * (bv[u] - ax[u]);
                if (MODE_ == MODE_CHEB)
                  store_result(epi, gi, r);
                else
                  NT_STORE(r, &epi.out[gi]);
              }
            else
              epi.out[gi] = (i < n_tail && fabs((double)ax[u]) > 1.0e-10) ? T(1) / ax[u] : T(1);
          }
      }
  }

  template <typename T, int MODE_>
  __global__ void
  __launch_bounds__(256) tail_kernel(T *__restrict__ tail_acc, uint32_t n_interior, uint32_t n_tail, uint32_t n_rest, Epilogue<T> epi)
  {
    constexpr int  MODE   = base_mode(MODE_);
    constexpr int  U      = TAIL_U;
    const uint32_t total  = n_tail + n_rest;
    const uint32_t stride = gridDim.x * blockDim.x;
    __shared__ T   dtable[256];
    const bool     coded = is_cheb(MODE) && epi.dinv_code != nullptr;
    if (coded)
      {
        dtable[threadIdx.x] = epi.dinv_table[threadIdx.x]; // 256 threads
        __syncthreads();
      }
    for (uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < total; i0 += U * stride)
      {
        uint32_t row[U];
        bool     live[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
          {
            row[u]  = i0 + u * stride;
            live[u] = row[u] < total;
          }
        tail_rows<T, MODE_>(tail_acc, n_interior, n_tail, row, live, epi, dtable, coded);
      }
  }

  // The same epilogue on a list of runs of rows (the fused residual pass, level_operator_apply.hpp: only the rows somebody
  // reads).  The host has cut the runs into chunks of at most TAIL_CHUNK = 64 rows, chunks[2c] <= row < chunks[2c+1]: a
  // wavefront takes U consecutive chunks, one row per lane.  Rows >= n_tail are constrained DoFs, as in tail_kernel.
  constexpr uint32_t TAIL_CHUNK = 64;
  template <typename T, int MODE_>
  __global__ void
  __launch_bounds__(256) tail_runs_kernel(T *__restrict__ tail_acc, uint32_t n_interior, uint32_t n_tail, const uint32_t *__restrict__ chunks,
                                          uint32_t n_chunks, Epilogue<T> epi)
  {
    constexpr int MODE = base_mode(MODE_);
    constexpr int U    = TAIL_U;
    static_assert(!is_cheb(MODE), "run-walking epilogue: modes without the D^-1 code table");
    const uint32_t c0   = (blockIdx.x * (256 / TAIL_CHUNK) + threadIdx.x / TAIL_CHUNK) * U;
    const uint32_t lane = threadIdx.x % TAIL_CHUNK;
    uint32_t       row[U];
    bool           live[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      {
        const uint32_t c = c0 + u;
        row[u]           = 0;
        live[u]          = false;
        if (c < n_chunks)
          {
            row[u]  = chunks[2 * c] + lane;
            live[u] = row[u] < chunks[2 * c + 1];
          }
      }
    tail_rows<T, MODE_>(tail_acc, n_interior, n_tail, row, live, epi, nullptr, false);
  }

} // namespace mgamd
