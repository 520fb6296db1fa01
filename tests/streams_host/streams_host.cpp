// streams_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_streams.h (the bodies of k_stream_mark, k_stream_order and
// k_stream_segments) on top of the drainage chain of soil_drain.h and the census bodies of soil_lakes.h that it needs.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run as tests/drainage_host runs them: the lanes
// of a workgroup one after the other, the workgroups of a launch one after the other, both first to last or last to first -- legal
// orders of the device's. The maps, the lane groups and the tile variants are those of tests/drainage_host/drainage_host.cpp, which
// this file includes. tests/analysis_host_lib.py builds and binds this file; the product never loads it.
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
  if (nm == 0 || threshold == 0 || !lanes_ok(lanes)) return -2;
  const Members pl = plan_members(maps, nm, cap, CAP_CELLS);
  StreamPlanes p;
  poison({&p.T, &p.R, &p.P, &p.AR, &p.D, &p.O, &p.H, &p.RE, &p.B, &p.SG}, pl.words);
  std::vector<StreamRec> recs = poisoned_records<StreamRec>(pl.nrec);
  const int desc = launch_order & 1, ldesc = (launch_order >> 1) & 1;
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        run_streams<S::TX, S::TY>(pl.tab, lanes, desc, ldesc, threshold, segments != nullptr, p, recs, nstreams);
      })) return -2;
  cut_records<StreamRec>(pl, nstreams, cap, out, sizeof(StreamRec), [&](size_t j, StreamRec& rec) { memcpy(&rec, &recs[j], sizeof(rec)); });   // (the bodies write whole records)
  copy_plane(order, p.O.data(), pl.words);
  copy_plane(segments, p.SG.data(), pl.words);
  copy_plane(reach, p.RE.data(), pl.words);
  copy_plane(heads, p.H.data(), pl.words);
  return 0;
}

}  // extern "C"
