// dispersal_host -- TEST-ONLY host build of soilmachine_amd/csrc/soil_disp.h (the bodies of k_disp_pending, k_disp_flow, k_disp_fold
// and k_disp_peak), behind the drainage chain of tests/drainage_host/drainage_host.cpp, which this file includes.
//
// The same headers the kernels are made of, compiled by g++ (-ffp-contract=off) and run as tests/drainage_host runs them: the lanes of
// a workgroup one after the other, the workgroups of a launch one after the other, both first to last or last to first -- legal
// orders of the device's (the lanes of k_disp_pending and k_disp_fold, which have barriers, always first to last). The flow launches
// take their own order and their own number of workgroups, so that the ready list is taken first to last or last to first and in
// one stride or in many. tests/analysis_host_lib.py builds and binds this file; the product never loads it.
#include <algorithm>
#include "../drainage_host/drainage_host.cpp"
#include "../../soilmachine_amd/csrc/soil_disp.h"

// The call as the library queues it: the drainage chain with its statistics and the basins' records, pending, the flow launches until
// one finds its range empty, fold and peak. flow_order: the order of the flow's workgroups (bit 0) and lanes (bit 1); flow_blocks:
// the flow's workgroups at most. Returns the launches that found work in some map, or 0xFFFFFFFF where the library's loop would give up (cells + 2 launches).
template <int TX, int TY, int SLOTS>
static uint32_t run_disp(const std::vector<LakeMember>& tab, uint32_t lanes, int descending, int lanes_descending, int flow_order, uint32_t flow_blocks, uint32_t exponent,
                         Planes& p, std::vector<uint32_t>& RC, std::vector<uint32_t>& Q, std::vector<uint64_t>& AQ, std::vector<BasinAcc>& bacc, std::vector<DispAcc>& acc,
                         std::vector<uint32_t>& ring, uint32_t* nbasins, bool want_donors, bool want_receivers) {
  static double hs[(TX + 2) * (TY + 2)];               // (the "LDS")
  static uint32_t ds[(TX + 2) * (TY + 2)], sl[TX * TY], wc[2];
  static DispTable<SLOTS> table;
  run_drainage<TX, TY, SLOTS>(tab, lanes, descending, lanes_descending, false, p, bacc, nbasins);
  uint32_t* const T = p.T.data(); uint32_t* const R = p.R.data(); uint32_t* const P = p.P.data();
  DrainHostGroup g{lanes};
  for (size_t k = 0; k < tab.size(); k++) {
    const uint32_t nt = lake_tiles(tab[k], TX, TY);
    for (uint32_t b = 0; b < nt; b++)
      disp_pending_group<TX, TY>(tab[k], g, nth(b, nt, descending), nt, hs, ds, sl, wc, P, RC.data(), Q.data(), AQ.data(), acc.data(), ring.data() + DISP_RING * k);
  }
  uint64_t largest = 0;
  for (const LakeMember& m : tab) largest = std::max<uint64_t>(largest, (uint64_t)m.dimx * m.dimy);
  // the library's round loop: DISP_BATCH launches -- all of them, the empty ones too -- then a look at the batch's word, in which
  // launch j sets bit j for every member with work; the loop ends with the first batch that has a clear bit
  uint32_t rounds = 0;
  const uint32_t full = DISP_BATCH == 32u ? 0xFFFFFFFFu : (1u << (DISP_BATCH & 31u)) - 1u;
  for (uint64_t launched = 0;; launched += DISP_BATCH) {
    if (launched >= largest + 2u) return 0xFFFFFFFFu;
    uint32_t busy = 0;
    for (uint32_t j = 0; j < DISP_BATCH; j++)
      for (size_t k = 0; k < tab.size(); k++) {   // (the grid is sized for the largest member: every member sees the same gridDim.x)
        const uint32_t nb = (uint32_t)std::min<uint64_t>((largest + lanes - 1) / lanes, flow_blocks);
        for (uint32_t b = 0; b < nb; b++)
          for (uint32_t l = 0; l < lanes; l++) {
            DrainHostLane one{lanes, nth(l, lanes, (flow_order >> 1) & 1)};
            disp_flow_group(tab[k], one, nth(b, nb, flow_order & 1), nb, (uint32_t)((launched + j) % 3u), exponent, T, R, P, RC.data(), Q.data(), AQ.data(), acc.data(),
                            ring.data() + DISP_RING * k, &busy, 1u << j);
          }
      }
    rounds += (uint32_t)__builtin_popcount(busy);
    if (busy != full) break;
  }
  for (size_t k = 0; k < tab.size(); k++) {
    const LakeMember& m = tab[k];
    const uint32_t per = lake_stats_cells(SLOTS, lanes);
    const uint32_t nb = (uint32_t)(((uint64_t)m.dimx * m.dimy + per - 1) / per);
    for (uint32_t b = 0; b < nb; b++) disp_fold_group<SLOTS>(m, g, nth(b, nb, descending), table, T, R, RC.data(), AQ.data(), acc.data());
  }
  for (size_t k = 0; k < tab.size(); k++) {
    const uint32_t nb = (uint32_t)(((uint64_t)tab[k].dimx * tab[k].dimy + lanes - 1) / lanes);
    for (uint32_t b = 0; b < nb; b++)
      for (uint32_t l = 0; l < lanes; l++) {
        DrainHostLane one{lanes, nth(l, lanes, lanes_descending)};
        disp_peak_group(tab[k], one, nth(b, nb, descending), T, P, RC.data(), AQ.data(), acc.data(), want_donors ? 1u : 0u, want_receivers ? 1u : 0u);
      }
  }
  return rounds;
}

extern "C" {

// The dispersed flow of maps[0..nm) in one go, as smx_ensemble_dispersal runs it (nm == 1: smx_dispersal). out: nm * cap records of 64
// bytes, map i's from record i * cap; nbasins: one count per map; the planes of all maps one after the other (NULL = skip); rounds
// (NULL = skip): the flow launches that found work. variant: a tile shape of dh_variant; lanes: 64, 128 or 256; order bit 0: every
// launch runs its workgroups last to first; bit 1: the lanes of a workgroup run last to first in the steps without a barrier; bits 2
// and 3: the same for the flow launches alone, XORed onto bits 0 and 1; flow_blocks: the workgroups of a flow launch at most (>= 1).
// 0; -2 for a bad argument, an exponent above 16 among them; -1 where the ready list did not run empty within cells + 2 launches.
int dph_dispersal(dh_map* const* maps, uint32_t nm, int variant, uint32_t lanes, int launch_order, uint32_t flow_blocks, uint32_t exponent, uint32_t cap, void* out,
                  uint32_t* nbasins, uint64_t* area, uint32_t* donors, uint32_t* receivers, uint32_t* rounds_out) {
  if (nm == 0 || !nbasins || !lanes_ok(lanes) || flow_blocks == 0 || exponent > DISP_MAX_EXPONENT || (!out && cap)) return -2;
  const Members pl = plan_members(maps, nm, cap, CAP_CELLS);
  const uint64_t words = pl.words;
  Planes p;
  std::vector<uint32_t> RC, Q;
  poison({&p.T, &p.B, &p.R, &p.P, &RC, &Q}, words);
  std::vector<uint64_t> AQ(words, 0xABABABABABABABABull);
  std::vector<BasinAcc> bacc = poisoned_records<BasinAcc>(pl.nrec);
  std::vector<DispAcc> acc = poisoned_records<DispAcc>(pl.nrec);
  std::vector<uint32_t> ring((size_t)nm * DISP_RING, 0u);   // (the library clears them in front of the chain)
  const int desc = launch_order & 1, ldesc = (launch_order >> 1) & 1, fo = (launch_order ^ (launch_order >> 2)) & 3;
  uint32_t rounds = 0;
  if (!with_shape<TILE_SHAPES>(variant, [&](auto s) {
        using S = decltype(s);
        rounds = run_disp<S::TX, S::TY, S::SLOTS>(pl.tab, lanes, desc, ldesc, fo, flow_blocks, exponent, p, RC, Q, AQ, bacc, acc, ring, nbasins, donors != nullptr,
                                                  receivers != nullptr);
      })) return -2;
  if (rounds == 0xFFFFFFFFu) return -1;
  if (rounds_out) *rounds_out = rounds;
  cut_records<DispRec>(pl, nbasins, cap, out, sizeof(DispRec), [&](size_t j, DispRec& rec) { disp_finish(bacc[j], acc[j], rec); });
  copy_plane(area, AQ.data(), words);
  copy_plane(donors, p.P.data(), words);
  copy_plane(receivers, RC.data(), words);
  return 0;
}

}  // extern "C"
