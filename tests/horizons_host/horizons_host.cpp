// horizons_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_horizon.h (the bodies of k_horizon_heights, k_horizon_scan and
// k_horizon_sky, and horizon_finish).
//
// The same header the kernels are made of, compiled by g++ (-ffp-contract=off) and run as tests/drainage_host runs its bodies: the
// lanes of a workgroup one after the other, the workgroups of a launch one after the other, first to last or last to first -- legal
// orders of the device's (the lanes of k_horizon_sky, which has no barrier, in either order too). The maps and the lane groups are
// those of the drainage host build, which this file includes for them; the tile sides (fine, coarse) are a variant of its own,
// HORIZON_SHAPES. Built with -DSMX_HORIZON_NO_TILES the scan walks every step. tests/horizons_host_lib.py builds and binds this file;
// the product never loads it.
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_horizon.h"

// (tx: the fine side, ty: the coarse side.) Shape 0 is the kernels' own; shape 3 has one level in effect; shape 4 tiles of one cell.
static constexpr Shape HORIZON_SHAPES[5] = {{HORIZON_FINE, HORIZON_COARSE, 0, 0}, {4, 16, 0, 0}, {2, 4, 0, 0}, {16, 16, 0, 0}, {1, 2, 0, 0}};

struct HorizonHost {   // the planes of a call, as horizons_run of soilmx.hip carves them
  std::vector<double> H, FM, CM, S, sky;
  std::vector<uint64_t> MM;
  std::vector<uint32_t> K, open, lit, counts;
  std::vector<HorizonAcc> acc;
};

// The call as the library queues it: the tables zeroed, heights over the coarse tiles of every member, the scan over every member,
// direction and block of cells, and, where something folded is asked for, sky.
template <int F, int C>
static void run_horizons(const std::vector<LakeMember>& tab, const std::vector<LakeMember>& tiles, uint32_t lanes, int descending, int lanes_descending, uint32_t mask,
                         uint32_t reach, const HorizonSun* suns, uint32_t nsuns, uint64_t words, bool kept, bool want_sky, bool want_open, bool want_lit, HorizonHost& p) {
  static HorizonTileMax<F, C> tmax;                  // (the "LDS")
  static HorizonFold fold;
  DrainHostGroup g{lanes};
  const uint32_t nd = horizon_count(mask);
  for (size_t k = 0; k < tab.size(); k++) {
    const uint32_t nt = horizon_tiles(tab[k], C);
    for (uint32_t b = 0; b < nt; b++) horizon_heights_group<F, C>(tab[k], tiles[k], g, nth(b, nt, descending), tmax, p.H.data(), p.FM.data(), p.CM.data(), p.MM.data());
  }
  const HorizonView v{p.H.data(), p.FM.data(), p.CM.data(), p.MM.data()};
  for (uint32_t jj = 0; jj < nd; jj++) {
    const uint32_t j = nth(jj, nd, descending);
    for (size_t k = 0; k < tab.size(); k++) {
      const uint32_t nb = (uint32_t)(((uint64_t)tab[k].dimx * tab[k].dimy + lanes - 1) / lanes);
      for (uint32_t b = 0; b < nb; b++)
        horizon_scan_group<F, C>(tab[k], tiles[k], g, nth(b, nb, descending), fold, v, horizon_nth(mask, j), j, reach, suns, nsuns, words, kept ? p.S.data() : nullptr,
                                 kept ? p.K.data() : nullptr, p.acc.data(), p.counts.data());
    }
  }
  if (!(want_sky || want_open || want_lit)) return;
  for (size_t k = 0; k < tab.size(); k++) {
    const uint32_t nb = (uint32_t)(((uint64_t)tab[k].dimx * tab[k].dimy + lanes - 1) / lanes);
    for (uint32_t b = 0; b < nb; b++)
      for (uint32_t l = 0; l < lanes; l++) {
        DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
        horizon_sky_group(tab[k], one, nth(b, nb, descending), mask, suns, nsuns, words, p.S.data(), p.K.data(), want_sky ? p.sky.data() : nullptr,
                          want_open ? p.open.data() : nullptr, want_lit ? p.lit.data() : nullptr);
      }
  }
}

extern "C" {

int hz_variants() { return (int)std::size(HORIZON_SHAPES); }
// (the fine side, the coarse side) of a variant
int hz_variant(int v, int* fine, int* coarse) {
  const Shape* s = shape_at(HORIZON_SHAPES, v);
  if (!s) return -2;
  *fine = s->tx; *coarse = s->ty;
  return 0;
}
int hz_tiles_off() {
#ifdef SMX_HORIZON_NO_TILES
  return 1;
#else
  return 0;
#endif
}

// The horizons of maps[0..nm) in one go, as smx_ensemble_horizons runs it (nm == 1: smx_horizons). out: nm * nd records, map i's from
// record i * nd, the first struct_size bytes of each; lit_cells: nm * nsuns counts; slope / step: nd planes of the cells of all maps,
// plane j from j * words on, the maps one after the other inside it; sky / open / lit: the cells of all maps (NULL = skip, and without
// any of the five the slopes and steps are not kept at all). probes (NULL = skip): the rays, the tile bounds computed and the heights
// loaded by this call. variant: a shape of hz_variant; lanes: 64, 128 or 256; order bit 0: every launch runs its workgroups last to
// first; bit 1: the lanes of k_horizon_sky run last to first. 0, or -2 for a bad argument.
int hz_horizons(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int order, uint32_t mask, uint32_t reach, void* out, uint64_t struct_size,
                const HorizonSun* suns, uint32_t nsuns, uint32_t* lit_cells, double* slope, uint32_t* step, double* sky, uint32_t* open, uint32_t* lit, uint64_t* probes) {
  if (nm == 0 || !out || !struct_size || !lanes_ok(lanes) || mask == 0u || (mask >> HORIZON_DIRS) || nsuns > HORIZON_MAX_SUNS || (nsuns && (!suns || !lit_cells)) || (lit && !nsuns))
    return -2;
  const uint32_t nd = horizon_count(mask);
  for (uint32_t i = 0; i < nsuns; i++)
    if (suns[i].direction >= HORIZON_DIRS || !((mask >> suns[i].direction) & 1u) || !(suns[i].tangent >= 0.0) || std::isinf(suns[i].tangent)) return -2;
  Members pl = plan_members(maps, nm, nd, CAP_CELLS);
  const Shape* shape = shape_at(HORIZON_SHAPES, variant);
  if (!shape) return -2;
  std::vector<LakeMember> tiles(pl.tab);
  uint64_t nfine = 0, ncoarse = 0;
  for (uint32_t i = 0; i < nm; i++) {
    pl.tab[i].cap = nd; pl.tab[i].rec0 = i * nd;
    tiles[i].off = (uint32_t)nfine; tiles[i].rec0 = (uint32_t)ncoarse; tiles[i].cap = i;
    nfine += horizon_tiles(pl.tab[i], shape->tx); ncoarse += horizon_tiles(pl.tab[i], shape->ty);
  }
  const uint64_t words = pl.words;
  const bool kept = slope || step || sky || open || lit;
  const double poison64 = -1.5e300;                  // (whatever the last call left: every word that is read has been written by this one)
  HorizonHost p;
  p.H.assign(words, poison64); p.FM.assign(nfine, poison64); p.CM.assign(ncoarse, poison64); p.MM.assign(nm, 0ull);
  if (kept) { p.S.assign((size_t)nd * words, poison64); p.K.assign((size_t)nd * words, 0xDEADBEEFu); }
  p.sky.assign(words, poison64); p.open.assign(words, 0xDEADBEEFu); p.lit.assign(words, 0xDEADBEEFu);
  p.counts.assign((size_t)nm * nsuns + 1u, 0u);
  p.acc.resize((size_t)nm * nd);
  memset(p.acc.data(), 0, p.acc.size() * sizeof(HorizonAcc));
  const HorizonProbes before = horizon_probes();
  const int desc = order & 1, ldesc = (order >> 1) & 1;
  if (!with_shape<HORIZON_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_horizons<S::TX, S::TY>(pl.tab, tiles, lanes, desc, ldesc, mask, reach, suns, nsuns, words, kept, sky != nullptr, open != nullptr, lit != nullptr, p);
      })) return -2;
  for (size_t r = 0; r < p.acc.size(); r++) {
    HorizonRec rec;
    horizon_finish(p.acc[r], horizon_nth(mask, (uint32_t)(r % nd)), rec);
    memcpy(static_cast<char*>(out) + r * struct_size, &rec, std::min<size_t>(struct_size, sizeof(HorizonRec)));
  }
  if (nsuns) memcpy(lit_cells, p.counts.data(), (size_t)nm * nsuns * 4);
  copy_plane(slope, (const double*)p.S.data(), (uint64_t)nd * words);
  copy_plane(step, (const uint32_t*)p.K.data(), (uint64_t)nd * words);
  copy_plane(sky, (const double*)p.sky.data(), words);
  copy_plane(open, (const uint32_t*)p.open.data(), words);
  copy_plane(lit, (const uint32_t*)p.lit.data(), words);
  if (probes) {
    const HorizonProbes now = horizon_probes();
    probes[0] = now.rays - before.rays; probes[1] = now.bounds - before.bounds; probes[2] = now.loads - before.loads;
  }
  return 0;
}

}  // extern "C"
