// drainage_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_drain.h (the bodies of k_drain_recv, k_drain_resolve,
// k_drain_stats, k_drain_pending and k_drain_area) and of the census bodies of soil_lakes.h that label the wet cells for them.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run with the lanes of a workgroup looped one
// after the other and the workgroups of a launch one after the other (in ascending or descending order; lanes_descending: the lanes
// of every workgroup last to first as well): legal orders of the device's. A map is the top records of a snapshot's columns; several
// maps share the planes as the members of an ensemble do. tests/analysis_host_lib.py builds and binds this file; the product never
// loads it.
#include "../analysis_host/analysis_host.h"
#include "../../soilmachine_amd/csrc/soil_drain.h"

using dh_map = ah_map;

struct DrainHostGroup {   // a workgroup whose lanes the caller runs one after the other
  uint32_t n;
  uint32_t lanes() const { return n; }
  uint32_t lo() const { return 0u; }
  uint32_t hi() const { return n; }
  void barrier() const {}
};
// ONE lane of a workgroup of n: the caller loops the lanes itself, in the order it likes, once per stretch between two barriers --
// which only the bodies WITHOUT a barrier allow (resolve, pending, area: the ones whose lanes meet in memory)
struct DrainHostLane {
  uint32_t n, l;
  uint32_t lanes() const { return n; }
  uint32_t lo() const { return l; }
  uint32_t hi() const { return l + 1u; }
  void barrier() const {}
};

struct Planes { std::vector<uint32_t> T, B, R, P, AR; };

template <int TX, int TY, int SLOTS>
static void run_drainage(const std::vector<LakeMember>& tab, uint32_t lanes, int descending, int lanes_descending, bool area, Planes& p,
                         std::vector<BasinAcc>& acc, uint32_t* nbasins) {
  static uint32_t lab[TX * TY];                      // (the "LDS")
  static double hs[(TX + 2) * (TY + 2)];
  static BasinTable<SLOTS> table;
  DrainHostGroup g{lanes};
  uint32_t* T = p.T.data();
  std::vector<LakeMember> wet_tab(tab);              // the census's kernels: cap 0, they touch no record
  for (LakeMember& m : wet_tab) m.cap = 0u;
  for (const LakeMember& m : wet_tab) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++) lake_tile_group<TX, TY>(m, g, nth(b, nt, descending), nt, lab, T, (LakeAcc*)nullptr);
  }
  for (const LakeMember& m : wet_tab) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++) lake_merge_group<TX, TY>(m, g, nth(b, nt, descending), T);
  }
  for (const LakeMember& m : wet_tab) {
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes);
    for (uint32_t b = 0; b < nb; b++) lake_flatten_group(m, g, nth(b, nb, descending), T);
  }
  for (const LakeMember& m : tab) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++) drain_recv_group<TX, TY>(m, g, nth(b, nt, descending), nt, hs, T, p.R.data(), acc.data());
  }
  // the bodies without a barrier: every lane by itself, in the order asked for
  auto each_lane = [&](auto&& body) {
    for (const LakeMember& m : tab) {
      const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes);
      for (uint32_t b = 0; b < nb; b++)
        for (uint32_t l = 0; l < lanes; l++) {
          DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
          body(m, one, nth(b, nb, descending));
        }
    }
  };
  each_lane([&](const LakeMember& m, DrainHostLane& one, uint32_t b) { drain_resolve_group(m, one, b, T); });
  uint32_t run = 0;
  for (size_t i = 0; i < p.T.size(); i++) { p.B[i] = run; run += lake_mark(T, i); }
  for (size_t k = 0; k < tab.size(); k++) {
    const LakeMember& m = tab[k];
    const uint32_t per = lake_stats_cells(SLOTS, lanes);
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per);
    for (uint32_t b = 0; b < nb; b++) drain_stats_group<SLOTS>(m, g, nth(b, nb, descending), table, T, p.B.data(), acc.data(), nbasins + k);
  }
  if (!area) return;
  each_lane([&](const LakeMember& m, DrainHostLane& one, uint32_t b) { drain_pending_group(m, one, b, p.R.data(), p.P.data(), p.AR.data()); });
  each_lane([&](const LakeMember& m, DrainHostLane& one, uint32_t b) { drain_area_group(m, one, b, p.R.data(), p.P.data(), p.AR.data()); });
}

extern "C" {

dh_map* dh_create(int dimx, int dimy, const uint32_t* count, const uint32_t* type, const double* size, const double* floor) {
  return ah_create(dimx, dimy, count, type, size, floor);
}
void dh_destroy(dh_map* m) { delete m; }

int dh_variants() { return (int)std::size(TILE_SHAPES); }
// (tile columns, tile rows, slots of the statistics table) of a variant
int dh_variant(int v, int* tx, int* ty, int* slots) {
  const Shape* s = shape_at(TILE_SHAPES, v);
  if (!s) return -2;
  *tx = s->tx; *ty = s->ty; *slots = s->slots;
  return 0;
}

// The drainage of maps[0..nm) in one go, as smx_ensemble_drainage runs it (nm == 1: smx_drainage). out: nm * cap records of 48 bytes,
// map i's from record i * cap; nbasins: one count per map; receivers / labels / area: the planes of all maps, one after the other
// (NULL = skip; without `area` the two accumulation steps do not run). Receivers are cell indices of the map they belong to.
// lanes: 64, 128 or 256; order bit 0: every launch runs its workgroups last to first; bit 1: the lanes of a workgroup run last to
// first in the steps without a barrier. 0, or -2 for a bad argument.
int dh_drainage(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int order, uint32_t cap, void* out, uint32_t* nbasins,
                uint32_t* receivers, uint32_t* labels, uint32_t* area) {
  if (nm == 0 || !lanes_ok(lanes)) return -2;
  const Members pl = plan_members(maps, nm, cap, CAP_CELLS);
  const std::vector<LakeMember>& tab = pl.tab;
  const uint64_t words = pl.words;
  Planes p;
  poison({&p.T, &p.B, &p.R}, words);
  if (area) poison({&p.P, &p.AR}, words);
  std::vector<BasinAcc> acc = poisoned_records<BasinAcc>(pl.nrec);
  const int desc = order & 1, ldesc = (order >> 1) & 1;
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_drainage<S::TX, S::TY, S::SLOTS>(tab, lanes, desc, ldesc, area != nullptr, p, acc, nbasins);
      })) return -2;
  cut_records<BasinRec>(pl, nbasins, cap, out, sizeof(BasinRec), [&](size_t j, BasinRec& rec) { drain_finish(acc[j], rec); });
  if (receivers)
    for (uint32_t i = 0; i < nm; i++)
      for (uint64_t c = 0, n = (uint64_t)tab[i].dimx * tab[i].dimy; c < n; c++) {
        const uint32_t r = p.R[tab[i].off + c];
        receivers[tab[i].off + c] = r == DRAIN_NONE ? DRAIN_NONE : r - tab[i].off;
      }
  copy_plane(labels, p.T.data(), words);
  copy_plane(area, p.AR.data(), words);
  return 0;
}

}  // extern "C"
