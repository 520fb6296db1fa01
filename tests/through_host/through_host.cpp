// through_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_through.h (the bodies of k_through_init, k_through_count,
// k_through_hops, k_through_exit, k_through_link, k_through_accumulate, k_through_outlet, k_through_plane and k_through_area) behind
// the drainage chain of tests/drainage_host and the spill chain's bodies of soil_spill.h.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run with the lanes of a workgroup looped one
// after the other and the workgroups of a launch one after the other, in ascending or descending order, as spill_host does; the
// bodies without a barrier (the sweeps, the exit, the link, the two walks) run lane by lane, so the order decides how far a level or
// a hop count travels in one sweep and which lane finishes a walk -- and must not decide any result. The host loops around the
// sweeps are the library's. The planes are shared as the library shares them: the boundary marks and the pending words are one plane,
// the boundary list and the area another. The relax sweeps, the hop sweeps and the exit have min(a lane per cell, relax_blocks)
// workgroups, as the library caps their launches: the workgroups stride over the rest of the boundary list.
// tests/analysis_host_lib.py builds and binds this file; the product never loads it.
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_through.h"

struct ThroughOut {
  std::vector<SpillAcc> sacc;
  std::vector<ThroughAcc> acc;
  std::vector<uint32_t> area, outlets;
  uint32_t level_sweeps = 0, hop_sweeps = 0, batches = 0;
};

template <int TX, int TY, int PS, int SLOTS>
static int run_through(std::vector<LakeMember> tab, uint32_t lanes, int descending, int lanes_descending, uint32_t relax_blocks, bool want_area, bool want_outlets, size_t words,
                       ThroughOut& o, uint32_t* nbasins) {
  static double hs[(TX + 2) * (TY + 2)];             // (the "LDS")
  static uint32_t ls[(TX + 2) * (TY + 2)];
  static SpillPassTable<PS> ptable;
  static ThroughCountTable<SLOTS> ctable;
  Planes p;   // (as the device's planes: whatever the last call left)
  p.T.assign(words, 0xDEADBEEFu); p.B.assign(words, 0xDEADBEEFu); p.R.assign(words, 0xDEADBEEFu);
  std::vector<uint32_t> M(words, 0xDEADBEEFu), Q(words, 0xDEADBEEFu);
  std::vector<double> H(words, -12345.0);
  std::vector<BasinAcc> none(1);
  for (LakeMember& m : tab) { m.cap = 0u; m.rec0 = 0u; }   // the drainage chain touches no record
  run_drainage<TX, TY, SLOTS>(tab, lanes, descending, lanes_descending, false, p, none, nbasins);
  uint64_t nrec = 0;
  uint32_t most = 0;
  for (size_t k = 0; k < tab.size(); k++) { tab[k].cap = nbasins[k]; tab[k].rec0 = (uint32_t)nrec; nrec += nbasins[k]; most = nbasins[k] > most ? nbasins[k] : most; }
  o.sacc.resize(nrec); o.acc.resize(nrec);
  memset(o.sacc.data(), 0xAB, o.sacc.size() * sizeof(SpillAcc));
  memset(o.acc.data(), 0xAB, o.acc.size() * sizeof(ThroughAcc));
  SpillAcc* sacc = o.sacc.data();
  ThroughAcc* acc = o.acc.data();
  DrainHostGroup g{lanes};
  const uint32_t* T = p.T.data();
  auto flat_blocks = [&](const LakeMember& m) { return (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes); };
  auto relax_groups = [&](const LakeMember& m) { return std::min<uint32_t>(flat_blocks(m), relax_blocks); };   // (the library's cap: the rest is strided)
  auto basin_blocks = [&](const LakeMember& m) { return (m.cap + lanes - 1) / lanes; };
  // a body with a barrier: the workgroup's lanes looped inside it
  auto groups = [&](auto&& blocks, auto&& body) {
    for (const LakeMember& m : tab) {
      const uint32_t nb = blocks(m);
      for (uint32_t b = 0; b < nb; b++) body(m, g, nth(b, nb, descending), nb);
    }
  };
  // a body without one: every lane by itself, in the order asked for
  auto each_lane = [&](auto&& blocks, auto&& body) {
    for (const LakeMember& m : tab) {
      const uint32_t nb = blocks(m);
      for (uint32_t b = 0; b < nb; b++)
        for (uint32_t l = 0; l < lanes; l++) {
          DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
          body(m, one, nth(b, nb, descending), nb);
        }
    }
  };
  auto tiles = [&](const LakeMember& m) { return lake_tiles(m, TX, TY); };
  auto stat_blocks = [&](const LakeMember& m) { const uint32_t per = lake_stats_cells(SLOTS, lanes); return (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per); };
  // the spill chain, its boundary marks in M: R stays the receivers
  groups(basin_blocks, [&](const LakeMember& m, DrainHostGroup& gg, uint32_t b, uint32_t) { spill_init_group(m, gg, b, sacc); });
  groups(basin_blocks, [&](const LakeMember& m, DrainHostGroup& gg, uint32_t b, uint32_t) { through_init_group(m, gg, b, acc); });
  groups(tiles, [&](const LakeMember& m, DrainHostGroup& gg, uint32_t b, uint32_t) {
    spill_pass_group<TX, TY, PS, 0>(m, gg, b, hs, ls, ptable, T, p.B.data(), M.data(), H.data(), sacc);
  });
  groups(tiles, [&](const LakeMember& m, DrainHostGroup& gg, uint32_t b, uint32_t) {
    spill_pass_group<TX, TY, PS, 1>(m, gg, b, hs, ls, ptable, T, (const uint32_t*)nullptr, (uint32_t*)nullptr, H.data(), sacc);
  });
  uint32_t run = 0;
  for (size_t i = 0; i < words; i++) { p.B[i] = run; run += M[i]; }
  groups(flat_blocks, [&](const LakeMember& m, DrainHostGroup& gg, uint32_t b, uint32_t) { spill_list_group(m, gg, b, p.B.data(), M.data(), Q.data()); });
  groups(basin_blocks, [&](const LakeMember& m, DrainHostGroup& gg, uint32_t b, uint32_t) { spill_point_group(m, gg, b, T, sacc); });
  groups(stat_blocks, [&](const LakeMember& m, DrainHostGroup& gg, uint32_t b, uint32_t) { through_count_group<SLOTS>(m, gg, b, ctable, T, acc); });
  o.level_sweeps = 0; o.hop_sweeps = 0; o.batches = 0;
  for (int what = 0; what < 2; what++) {   // the levels, then the hop counts: the library's loop, twice
    uint32_t& sweeps = what ? o.hop_sweeps : o.level_sweeps;
    for (bool done = false; !done;) {
      if ((uint64_t)sweeps >= (uint64_t)most + 2u) return -1;
      uint32_t changed[SPILL_BATCH];
      for (uint32_t j = 0; j < SPILL_BATCH; j++) {
        changed[j] = 0u;
        each_lane(relax_groups, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t nb) {
          if (what) through_hops_group(m, one, b, nb, T, p.B.data(), M.data(), Q.data(), H.data(), sacc, acc, changed + j);
          else spill_relax_group(m, one, b, nb, sweeps + j + 1u, T, p.B.data(), M.data(), Q.data(), H.data(), sacc, changed + j);
        });
      }
      sweeps += SPILL_BATCH; o.batches += 1u;
      for (uint32_t j = 0; j < SPILL_BATCH; j++) done = done || changed[j] == 0u;
    }
  }
  each_lane(relax_groups, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t nb) {
    through_exit_group(m, one, b, nb, T, p.B.data(), M.data(), Q.data(), H.data(), sacc, acc);
  });
  uint32_t* P = M.data();    // the marks and the list are done with: the pending words and the area take their planes
  uint32_t* AR = want_area ? Q.data() : nullptr;
  if (want_area)
    each_lane(flat_blocks, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t) { drain_pending_group(m, one, b, p.R.data(), P, AR); });
  each_lane(basin_blocks, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t) { through_link_group<0>(m, one, b, T, H.data(), sacc, acc); });
  each_lane(basin_blocks, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t) { through_link_group<1>(m, one, b, T, H.data(), sacc, acc); });
  each_lane(basin_blocks, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t) { through_accumulate_group(m, one, b, acc, AR); });
  each_lane(basin_blocks, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t) { through_outlet_group(m, one, b, sacc, acc); });
  if (want_outlets) {
    each_lane(flat_blocks, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t) { through_plane_group(m, one, b, T, acc, p.B.data()); });
    o.outlets = p.B;
  }
  if (want_area) {
    each_lane(flat_blocks, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, uint32_t) { through_area_group(m, one, b, p.R.data(), P, AR); });
    o.area = Q;
  }
  return 0;
}

extern "C" {

int th_variants() { return (int)std::size(PASS_SHAPES); }
// (tile columns, tile rows, slots of the pass table, slots of the count table) of a variant
int th_variant(int v, int* tx, int* ty, int* pslots, int* slots) {
  const Shape* s = shape_at(PASS_SHAPES, v);
  if (!s) return -2;
  *tx = s->tx; *ty = s->ty; *pslots = s->pslots; *slots = s->slots;
  return 0;
}
uint32_t th_batch() { return SPILL_BATCH; }

// The through-drainage of maps[0..nm) in one go, as smx_ensemble_through runs it (nm == 1: smx_through). out: nm * cap records of
// struct_size bytes (the prefix of each 64-byte record, as the library cuts it), map i's from record i * cap; nbasins: one count per
// map; through_area / outlets: the planes of all maps, one after the other (NULL = skip); sweeps[3]: level sweeps, hop sweeps,
// batches. lanes and order as dh_drainage; relax_blocks: the workgroups of a relax sweep, a hop sweep and the exit at most (>= 1). 0,
// -2 for a bad argument, -1 where the sweeps did not settle within the bound.
int th_through(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int order, uint32_t relax_blocks, uint32_t cap, void* out, uint64_t struct_size,
               uint32_t* nbasins, uint32_t* through_area, uint32_t* outlets, uint32_t* sweeps) {
  if (nm == 0 || struct_size == 0 || !lanes_ok(lanes) || relax_blocks == 0 || !nbasins || !sweeps || (!out && cap)) return -2;
  Members pl = plan_members(maps, nm, cap, CAP_NONE);
  ThroughOut o;
  const int desc = order & 1, ldesc = (order >> 1) & 1;
  int rc = 0;
  if (!with_shape<PASS_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        rc = run_through<S::TX, S::TY, S::PS, S::SLOTS>(pl.tab, lanes, desc, ldesc, relax_blocks, through_area != nullptr, outlets != nullptr, (size_t)pl.words, o, nbasins);
      })) return -2;
  if (rc) return rc;
  sweeps[0] = o.level_sweeps; sweeps[1] = o.hop_sweeps; sweeps[2] = o.batches;
  plan_basins(pl, nbasins);   // (as run_through laid its copy of the table out)
  cut_records<ThroughRec>(pl, nbasins, cap, out, (size_t)struct_size, [&](size_t j, ThroughRec& rec) { through_finish(o.sacc[j], o.acc[j], rec); });
  copy_plane(through_area, o.area.data(), pl.words);
  copy_plane(outlets, o.outlets.data(), pl.words);
  return 0;
}

}  // extern "C"
