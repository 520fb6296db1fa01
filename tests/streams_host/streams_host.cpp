// streams_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_streams.h (the bodies of k_stream_mark, k_stream_order and
// k_stream_segments) on top of the drainage chain of soil_drain.h and the census bodies of soil_lakes.h that it needs.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run as tests/drainage_host runs them: the lanes
// of a workgroup one after the other, the workgroups of a launch one after the other, both first to last or last to first -- legal
// orders of the device's. The maps, the lane groups and the tile variants are those of tests/drainage_host/drainage_host.cpp, which
// this file includes. tests/streams_host_lib.py builds and binds this file; the product never loads it.
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_streams.h"

struct StreamPlanes { std::vector<uint32_t> T, R, P, AR, D, O, H, RE, B, SG; };

// The chain as the library queues it: the census on T, receivers, terminals, pending and area (the statistics of the basins are not
// needed: T stays the terminal), then mark, order, the prefix sum of the start marks, segments. P is the pending plane of both walks.
template <int TX, int TY>
static void run_streams(const std::vector<LakeMember>& tab, uint32_t lanes, int descending, int lanes_descending, uint32_t threshold, bool with_plane,
                        StreamPlanes& p, std::vector<StreamRec>& out, uint32_t* nstreams) {
  static uint32_t lab[TX * TY];                      // (the "LDS")
  static double hs[(TX + 2) * (TY + 2)];
  DrainHostGroup g{lanes};
  uint32_t* T = p.T.data();
  std::vector<LakeMember> bare(tab);                 // the census's and the drainage's kernels: cap 0, they touch no record
  for (LakeMember& m : bare) m.cap = 0u;
  for (const LakeMember& m : bare) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++) lake_tile_group<TX, TY>(m, g, nth(b, nt, descending), nt, lab, T, (LakeAcc*)nullptr);
  }
  for (const LakeMember& m : bare) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++) lake_merge_group<TX, TY>(m, g, nth(b, nt, descending), T);
  }
  for (const LakeMember& m : bare) {
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes);
    for (uint32_t b = 0; b < nb; b++) lake_flatten_group(m, g, nth(b, nb, descending), T);
  }
  for (const LakeMember& m : bare) {
    const uint32_t nt = lake_tiles(m, TX, TY);
    for (uint32_t b = 0; b < nt; b++) drain_recv_group<TX, TY>(m, g, nth(b, nt, descending), nt, hs, T, p.R.data(), (BasinAcc*)nullptr);
  }
  auto each_lane = [&](const std::vector<LakeMember>& members, auto&& body) {
    for (size_t k = 0; k < members.size(); k++) {
      const LakeMember& m = members[k];
      const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + lanes - 1) / lanes);
      for (uint32_t b = 0; b < nb; b++)
        for (uint32_t l = 0; l < lanes; l++) {
          DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
          body(m, one, nth(b, nb, descending), k);
        }
    }
  };
  uint32_t *R = p.R.data(), *P = p.P.data(), *AR = p.AR.data(), *D = p.D.data(), *O = p.O.data(), *H = p.H.data(), *RE = p.RE.data();
  each_lane(bare, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, size_t) { drain_resolve_group(m, one, b, T); });
  each_lane(bare, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, size_t) { drain_pending_group(m, one, b, R, P, AR); });
  each_lane(bare, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, size_t) { drain_area_group(m, one, b, R, P, AR); });
  each_lane(bare, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, size_t) { stream_mark_group(m, one, b, threshold, R, AR, D, P, O, H, RE, p.SG.data()); });
  each_lane(bare, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, size_t) { stream_order_group(m, one, b, threshold, R, AR, D, P, O, H, RE); });
  uint32_t run = 0;
  for (size_t i = 0; i < p.D.size(); i++) { p.B[i] = run; run += stream_mark(D, i); }
  each_lane(tab, [&](const LakeMember& m, DrainHostLane& one, uint32_t b, size_t k) {
    stream_segments_group(m, one, b, with_plane, T, R, AR, D, O, H, p.B.data(), p.SG.data(), out.data(), nstreams + k);
  });
}

extern "C" {

// The streams of maps[0..nm) in one go, as smx_ensemble_streams runs it (nm == 1: smx_streams). out: nm * cap records of 64 bytes,
// map i's from record i * cap; nstreams: one count per map; order / segments / reach / heads: the planes of all maps, one after the
// other (NULL = skip). variant: a tile shape of dh_variant; lanes: 64, 128 or 256; order bit 0: every launch runs its workgroups last
// to first; bit 1: the lanes of a workgroup run last to first. 0, or -2 for a bad argument.
int sh_streams(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int launch_order, uint32_t threshold, uint32_t cap, void* out, uint32_t* nstreams,
               uint32_t* order, uint32_t* segments, uint32_t* reach, uint32_t* heads) {
  if (nm == 0 || threshold == 0 || !(lanes == 64 || lanes == 128 || lanes == 256)) return -2;
  std::vector<LakeMember> tab(nm);
  uint64_t words = 0, nrec = 0;
  for (uint32_t i = 0; i < nm; i++) {
    LakeMember& m = tab[i];
    m.cells = maps[i]->cells.data(); m.dimx = maps[i]->dimx; m.dimy = maps[i]->dimy; m.pad = 0;
    m.off = (uint32_t)words; m.rec0 = (uint32_t)nrec;
    const uint64_t most = (uint64_t)m.dimx * m.dimy;
    m.cap = (uint32_t)(cap < most ? cap : most);
    words += most; nrec += m.cap;
  }
  StreamPlanes p;   // (as the device's planes: whatever the last call left)
  for (std::vector<uint32_t>* v : {&p.T, &p.R, &p.P, &p.AR, &p.D, &p.O, &p.H, &p.RE, &p.B, &p.SG}) v->assign(words, 0xDEADBEEFu);
  std::vector<StreamRec> recs(nrec ? nrec : 1);
  memset(recs.data(), 0xAB, recs.size() * sizeof(StreamRec));
  const int desc = launch_order & 1, ldesc = (launch_order >> 1) & 1;
  const bool with_plane = segments != nullptr;
  switch (variant) {
    case 0: run_streams<16, 64>(tab, lanes, desc, ldesc, threshold, with_plane, p, recs, nstreams); break;   // the kernels' own shape
    case 1: run_streams<8, 8>(tab, lanes, desc, ldesc, threshold, with_plane, p, recs, nstreams); break;
    case 2: run_streams<5, 7>(tab, lanes, desc, ldesc, threshold, with_plane, p, recs, nstreams); break;     // a tile no dimension is a multiple of
    case 3: run_streams<32, 4>(tab, lanes, desc, ldesc, threshold, with_plane, p, recs, nstreams); break;
    default: return -2;
  }
  for (uint32_t i = 0; i < nm; i++) {
    const uint32_t w = nstreams[i] < tab[i].cap ? nstreams[i] : tab[i].cap;
    if (w) memcpy(static_cast<char*>(out) + (size_t)i * cap * sizeof(StreamRec), recs.data() + tab[i].rec0, (size_t)w * sizeof(StreamRec));
  }
  if (order) memcpy(order, p.O.data(), words * 4);
  if (segments) memcpy(segments, p.SG.data(), words * 4);
  if (reach) memcpy(reach, p.RE.data(), words * 4);
  if (heads) memcpy(heads, p.H.data(), words * 4);
  return 0;
}

}  // extern "C"
