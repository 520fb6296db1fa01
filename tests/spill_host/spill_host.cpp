// spill_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_spill.h (the bodies of k_spill_init, k_spill_pass, k_spill_list,
// k_spill_point, k_spill_relax and k_spill_store) behind the drainage chain of tests/drainage_host.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run with the lanes of a workgroup looped one
// after the other and the workgroups of a launch one after the other, in ascending or descending order, as drainage_host does; the
// relax sweeps run lane by lane (the body has no barrier), so the order decides how far a level travels in one sweep -- and must not
// decide where it ends. The host loop around the sweeps is the library's: batches of SPILL_BATCH, stop after the batch that holds a
// sweep that changed nothing, give up after nbasins + 2. A relax sweep has min(a lane per cell, relax_blocks) workgroups, as the
// library caps its launch: the workgroups stride over the rest of the boundary list. tests/analysis_host_lib.py builds and binds this
// file; the product never loads it.
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_spill.h"

template <int TX, int TY, int PS, int SLOTS>
static int run_spill(std::vector<LakeMember> tab, uint32_t lanes, int descending, int lanes_descending, uint32_t relax_blocks, bool filled, std::vector<double>& H,
                     std::vector<SpillAcc>& acc, uint32_t* nbasins, uint32_t* sweeps, uint32_t* batches) {
  static double hs[(TX + 2) * (TY + 2)];             // (the "LDS")
  static uint32_t ls[(TX + 2) * (TY + 2)];
  static SpillPassTable<PS> ptable;
  static SpillStoreTable<SLOTS> stable;
  const size_t words = H.size();
  Planes p;   // (as the device's planes: whatever the last call left)
  p.T.assign(words, 0xDEADBEEFu); p.B.assign(words, 0xDEADBEEFu); p.R.assign(words, 0xDEADBEEFu);
  std::vector<uint32_t> Q(words, 0xDEADBEEFu);
  std::vector<BasinAcc> none(1);
  for (LakeMember& m : tab) { m.cap = 0u; m.rec0 = 0u; }   // the drainage chain touches no record
  run_drainage<TX, TY, SLOTS>(tab, lanes, descending, lanes_descending, false, p, none, nbasins);
  uint64_t nrec = 0;
  uint32_t most = 0;
  for (size_t k = 0; k < tab.size(); k++) { tab[k].cap = nbasins[k]; tab[k].rec0 = (uint32_t)nrec; nrec += nbasins[k]; most = nbasins[k] > most ? nbasins[k] : most; }
  acc.resize(nrec);
  memset(acc.data(), 0xAB, acc.size() * sizeof(SpillAcc));
  DrainHostGroup g{lanes};
  const uint32_t *T = p.T.data();
  for (const LakeMember& m : tab) {
    const uint32_t nb = (m.cap + lanes - 1) / lanes;
    for (uint32_t b = 0; b < nb; b++) spill_init_group(m, g, nth(b, nb, descending), acc.data());
  }
  for (const LakeMember& m : tab) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++)
      spill_pass_group<TX, TY, PS, 0>(m, g, nth(b, nt, descending), hs, ls, ptable, T, p.B.data(), p.R.data(), H.data(), acc.data());
  }
  for (const LakeMember& m : tab) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++)
      spill_pass_group<TX, TY, PS, 1>(m, g, nth(b, nt, descending), hs, ls, ptable, T, (const uint32_t*)nullptr, (uint32_t*)nullptr, H.data(), acc.data());
  }
  uint32_t run = 0;
  for (size_t i = 0; i < words; i++) { p.B[i] = run; run += p.R[i]; }
  for (const LakeMember& m : tab) {
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes);
    for (uint32_t b = 0; b < nb; b++) spill_list_group(m, g, nth(b, nb, descending), p.B.data(), p.R.data(), Q.data());
  }
  for (const LakeMember& m : tab) {
    const uint32_t nb = (m.cap + lanes - 1) / lanes;
    for (uint32_t b = 0; b < nb; b++) spill_point_group(m, g, nth(b, nb, descending), T, acc.data());
  }
  *sweeps = 0; *batches = 0;
  for (bool done = false; !done;) {
    if ((uint64_t)*sweeps >= (uint64_t)most + 2u) return -1;
    uint32_t changed[SPILL_BATCH];
    for (uint32_t j = 0; j < SPILL_BATCH; j++) {
      changed[j] = 0u;
      for (const LakeMember& m : tab) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes, relax_blocks);   // (the library's cap: the rest is strided)
        for (uint32_t b = 0; b < nb; b++)
          for (uint32_t l = 0; l < lanes; l++) {
            DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
            spill_relax_group(m, one, nth(b, nb, descending), nb, *sweeps + j + 1u, T, p.B.data(), p.R.data(), Q.data(), H.data(), acc.data(), changed + j);
          }
      }
    }
    *sweeps += SPILL_BATCH; *batches += 1u;
    for (uint32_t j = 0; j < SPILL_BATCH; j++) done = done || changed[j] == 0u;
  }
  for (const LakeMember& m : tab) {
    const uint32_t per = lake_stats_cells(SLOTS, lanes);
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per);
    for (uint32_t b = 0; b < nb; b++) spill_store_group<SLOTS>(m, g, nth(b, nb, descending), stable, T, H.data(), acc.data(), filled);
  }
  return 0;
}

extern "C" {

int sh_variants() { return (int)std::size(PASS_SHAPES); }
// (tile columns, tile rows, slots of the pass table, slots of the store table) of a variant
int sh_variant(int v, int* tx, int* ty, int* pslots, int* slots) {
  const Shape* s = shape_at(PASS_SHAPES, v);
  if (!s) return -2;
  *tx = s->tx; *ty = s->ty; *pslots = s->pslots; *slots = s->slots;
  return 0;
}
uint32_t sh_batch() { return SPILL_BATCH; }

// The spill analysis of maps[0..nm) in one go, as smx_ensemble_spill runs it (nm == 1: smx_spill). out: nm * cap records of
// struct_size bytes (the prefix of each 64-byte record, as the library cuts it), map i's from record i * cap; nbasins: one count
// per map; filled: the planes of all maps, one after the other (NULL = skip); sweeps / batches: as smx_get_spill_sweeps. lanes and order as dh_drainage;
// relax_blocks: the workgroups of a relax sweep at most (>= 1). 0, -2 for a bad argument, -1 where the levels did not settle within
// the bound.
int sh_spill(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int order, uint32_t relax_blocks, uint32_t cap, void* out, uint64_t struct_size,
             uint32_t* nbasins, double* filled, uint32_t* sweeps, uint32_t* batches) {
  if (nm == 0 || struct_size == 0 || !lanes_ok(lanes) || relax_blocks == 0 || !nbasins || !sweeps || !batches || (!out && cap)) return -2;
  Members pl = plan_members(maps, nm, cap, CAP_NONE);
  std::vector<double> H(pl.words, -12345.0);
  std::vector<SpillAcc> acc;
  const int desc = order & 1, ldesc = (order >> 1) & 1;
  int rc = 0;
  if (!with_shape<PASS_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        rc = run_spill<S::TX, S::TY, S::PS, S::SLOTS>(pl.tab, lanes, desc, ldesc, relax_blocks, filled != nullptr, H, acc, nbasins, sweeps, batches);
      })) return -2;
  if (rc) return rc;
  plan_basins(pl, nbasins);   // (as run_spill laid its copy of the table out)
  cut_records<SpillRec>(pl, nbasins, cap, out, (size_t)struct_size, [&](size_t j, SpillRec& rec) { spill_finish(acc[j], rec); });
  copy_plane(filled, H.data(), pl.words);
  return 0;
}

}  // extern "C"
