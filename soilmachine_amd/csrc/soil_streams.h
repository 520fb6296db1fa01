// soil_streams.h -- the stream network (smx_streams / smx_ensemble_streams): the channel cells on top of the drainage planes, their
// Strahler order, Shreve magnitude and reach, and one record per segment. The bodies of k_stream_mark, k_stream_order and
// k_stream_segments. Nothing here writes a map.
//
// Cells, h(c), wet cells, receivers, sinks, terminals and area(c) are those of soil_drain.h. A CHANNEL cell is a dry cell with
// area(c) >= threshold. Area strictly grows downstream, so the receiver of a channel cell is a channel cell or a wet cell. The
// channel DONORS of c are the channel cells whose receiver is c (0 to 8): a HEAD has none, a CONFLUENCE two or more. order(c) is the
// Strahler order (a head: 1; else m = the largest order among the donors, m + 1 where two or more donors have it), heads(c) the Shreve
// magnitude (a head: 1; else the u32 sum over the donors), reach(c) the cells on the longest channel path from a head down to and
// including c (a head: 1; else 1 + the largest among the donors); all three are 0 off the channels. A SEGMENT starts at a head or a
// confluence (its identity first_cell) and runs downstream through cells with exactly one donor; its last_cell is the cell whose
// receiver is a confluence or a wet cell, or which is a sink. Its rank is its place in ascending first_cell.
//
// The planes of soil_drain.h are read as the drainage chain left them BEFORE its statistics step: T holds the terminal of every cell
// (a plane index), R the receiver, AR the area. The planes of this file, u32 per cell, member i at words [off_i, off_i + cells_i):
//   D    the channel donors of the cell, STREAM_OFF for a cell that is no channel cell. Written by mark, read-only afterwards.
//   P2   donors still to report (order only).   O, H, RE   order, heads, reach.   SG   the segment's rank, STREAM_OFF off the channels.
//   B    the exclusive prefix sum of the start marks (stream_mark) over the whole plane: the caller's business, as in the census.
// The steps, each one launch for all members (blockIdx.y = member):
//   mark      D[g] counted from R and AR over the eight neighbours without atomics; P2[g] = D[g], STREAM_LEAF for a head, STREAM_OFF_P
//             for a cell off the channels (a wet cell among them); a head gets order = heads = reach = 1, a cell off the channels 0;
//             SG[g] = STREAM_OFF.
//   order     a lane that owns a head walks downstream: it decrements the receiver's P2 (a release: its own cell's three values are
//             stored in front of it); only the lane whose decrement is the last one goes on -- it acquires, RECOMPUTES the receiver's
//             three values from the receiver's donors and stores them. Nothing is folded with atomics and no lane ever waits or polls.
//   segments  a lane that owns a start (a channel cell with D != 1) walks its segment, writes its rank into SG and its record.
//             Segments are disjoint: no atomics.
// What the walks cost: a lane of `order` takes at most as many turns as the longest channel path has cells (the largest reach), each
// turn one atomic and up to eight neighbour probes; a lane of `segments` takes as many turns as its segment has cells. The lanes of
// a wavefront wait for the longest walk among them.
// The file compiles for the device and, under SMX_D / SMX_HOSTSIM, for the host (tests/streams_host), as soil_drain.h does.
#pragma once
#include "soil_drain.h"

namespace smx {

constexpr uint32_t STREAM_OFF = 0xFFFFFFFFu;     // D, SG: no channel cell
constexpr uint32_t STREAM_LEAF = 0xFFFFFFFFu;    // P2: a head (nobody ever decrements it)
constexpr uint32_t STREAM_OFF_P = 0x80000000u;   // P2: off the channels; at most eight decrements: it never reads 1, 0 or STREAM_LEAF
constexpr uint32_t STREAM_F_WET = 1u, STREAM_F_SINK = 2u, STREAM_F_HEAD = 4u, STREAM_F_BORDER = 8u;

struct StreamRec {    // == smx_segment (include/soilmx.h)
  uint32_t first_cell, last_cell, cells, order;
  uint32_t down, basin, flags, heads;
  uint32_t straight, diagonal, area_first, area_last;
  double height_first, height_last;
};
static_assert(sizeof(StreamRec) == 64, "stream record layout");

// the scan's input: 1 where plane word g starts a segment
SMX_HD uint32_t stream_mark(const uint32_t* D, size_t g) { return D[g] != 1u && D[g] != STREAM_OFF ? 1u : 0u; }

// ---- mark: workgroup `block` takes g.lanes() cells (R and AR are read-only here) ----
template <class G>
SMX_D void stream_mark_group(const LakeMember& m, G& g, uint32_t block, uint32_t threshold, const uint32_t* R, const uint32_t* AR, uint32_t* D,
                             uint32_t* P2, uint32_t* O, uint32_t* H, uint32_t* RE, uint32_t* SG) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    SG[a] = STREAM_OFF;
    if (m.cells[c].type == AIR || AR[a] < threshold) {   // off the channels: no decrement ever takes its word from 1 to 0
      D[a] = STREAM_OFF; P2[a] = STREAM_OFF_P; O[a] = 0u; H[a] = 0u; RE[a] = 0u;
      continue;
    }
    const int x = (int)(c / (uint64_t)m.dimy), y = (int)(c % (uint64_t)m.dimy);
    uint32_t donors = 0u;
    for (int dx = -1; dx <= 1; dx++)
      for (int dy = -1; dy <= 1; dy++) {
        const int u = x + dx, v = y + dy;
        if ((dx == 0 && dy == 0) || u < 0 || v < 0 || u >= m.dimx || v >= m.dimy) continue;
        const size_t d = (size_t)m.off + (size_t)u * m.dimy + v;
        if (R[d] == a && AR[d] >= threshold) donors++;   // (a cell with a receiver is dry)
      }
    D[a] = donors;
    P2[a] = donors ? donors : STREAM_LEAF;
    const uint32_t one = donors ? 0u : 1u;   // (a cell with donors is written again by the walk that completes it)
    O[a] = one; H[a] = one; RE[a] = one;
  }
}

// ---- order: workgroup `block` takes g.lanes() cells; every access to P2, O, H and RE is an agent-scope atomic (other workgroups
//      walk through the same words, and a plain load may be served from a cache that never sees their writes); R, AR and D were
//      finished by earlier launches and are read plainly ----
template <class G>
SMX_D void stream_order_group(const LakeMember& m, G& g, uint32_t block, uint32_t threshold, const uint32_t* R, const uint32_t* AR, const uint32_t* D,
                              uint32_t* P2, uint32_t* O, uint32_t* H, uint32_t* RE) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    uint32_t cur = m.off + (uint32_t)c;
    if (D[cur] != 0u) continue;   // not a head (its three values were stored by the launch before)
    // Every turn moves cur to its receiver, one step down a path that strictly descends in h: the walk ends at a sink, at a wet cell,
    // or earlier, where another donor is still to report. It never waits: the lane whose decrement is the last one goes on.
    for (;;) {
      const uint32_t r = R[cur];
      if (r == DRAIN_NONE) break;                        // cur is a sink
      if (SMX_DRAIN_DEC_RELEASE(P2 + r) != 1u) break;    // a donor of r is still to come (or r is wet); cur's values lie in front of the release
      SMX_DRAIN_ACQUIRE();                               // every donor stored its values before its decrement: they are final
      const uint32_t rc = r - m.off;
      const int x = (int)(rc / (uint32_t)m.dimy), y = (int)(rc % (uint32_t)m.dimy);
      uint32_t top = 0u, ntop = 0u, heads = 0u, reach = 0u;
      for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++) {
          const int u = x + dx, v = y + dy;
          if ((dx == 0 && dy == 0) || u < 0 || v < 0 || u >= m.dimx || v >= m.dimy) continue;
          const size_t d = (size_t)m.off + (size_t)u * m.dimy + v;
          if (R[d] != r || AR[d] < threshold) continue;
          const uint32_t od = SMX_LAKE_LD(O + d, SMX_LAKE_AGENT), rd = SMX_LAKE_LD(RE + d, SMX_LAKE_AGENT);
          heads += SMX_LAKE_LD(H + d, SMX_LAKE_AGENT);
          if (od > top) { top = od; ntop = 1u; } else if (od == top) ntop++;
          if (rd > reach) reach = rd;
        }
      SMX_LAKE_ST(O + r, ntop >= 2u ? top + 1u : top, SMX_LAKE_AGENT);
      SMX_LAKE_ST(H + r, heads, SMX_LAKE_AGENT);
      SMX_LAKE_ST(RE + r, reach + 1u, SMX_LAKE_AGENT);
      cur = r;
    }
  }
}

// ---- segments: workgroup `block` takes g.lanes() cells; every plane it reads was finished by an earlier launch. (m.cap: records kept
//      for the member; with_plane: SG is wanted, so a segment beyond cap is walked all the same) ----
template <class G>
SMX_D void stream_segments_group(const LakeMember& m, G& g, uint32_t block, bool with_plane, const uint32_t* T, const uint32_t* R, const uint32_t* AR,
                                 const uint32_t* D, const uint32_t* O, const uint32_t* H, const uint32_t* B, uint32_t* SG, StreamRec* out, uint32_t* nstreams) {
  const uint32_t nl = g.lanes();
  const uint64_t n = (uint64_t)m.dimx * (uint64_t)m.dimy;
  for (uint32_t l = g.lo(); l < g.hi(); l++) {
    const uint64_t c = (uint64_t)block * nl + l;
    if (c >= n) continue;
    const uint32_t a = m.off + (uint32_t)c;
    if (c == n - 1) *nstreams = B[a] + stream_mark(D, a) - B[m.off];
    if (!stream_mark(D, a)) continue;
    const uint32_t rank = B[a] - B[m.off];
    if (rank >= m.cap && !with_plane) continue;
    const uint32_t dimy = (uint32_t)m.dimy;
    uint32_t cur = a, cells = 1u, straight = 0u, diagonal = 0u, down = STREAM_OFF;
    uint32_t flags = D[a] == 0u ? STREAM_F_HEAD : 0u;
    SG[a] = rank;
    // Every turn moves cur to its receiver while that one has exactly one donor -- cur: one step down a path that strictly descends
    // in h, so the walk is finite.
    for (;;) {
      const uint32_t r = R[cur];
      if (r == DRAIN_NONE) { flags |= STREAM_F_SINK; break; }
      const uint32_t cc = cur - m.off, rc = r - m.off;
      if (cc / dimy != rc / dimy && cc % dimy != rc % dimy) diagonal++; else straight++;
      const uint32_t dr = D[r];
      if (dr == STREAM_OFF) { flags |= STREAM_F_WET; break; }   // (the receiver of a channel cell is a channel cell or a wet cell)
      if (dr >= 2u) { down = rc; break; }
      cur = r; cells++;
      SG[cur] = rank;
    }
    if (rank >= m.cap) continue;
    const uint32_t lc = cur - m.off, x = lc / dimy, y = lc % dimy;
    if (x == 0u || y == 0u || x == (uint32_t)m.dimx - 1u || y == (uint32_t)m.dimy - 1u) flags |= STREAM_F_BORDER;
    StreamRec rec;
    rec.first_cell = (uint32_t)c; rec.last_cell = lc; rec.cells = cells; rec.order = O[a];
    rec.down = down; rec.basin = T[a] - m.off; rec.flags = flags; rec.heads = H[a];
    rec.straight = straight; rec.diagonal = diagonal; rec.area_first = AR[a]; rec.area_last = AR[cur];
    rec.height_first = drain_height(m.cells[c]); rec.height_last = drain_height(m.cells[lc]);
    out[m.rec0 + rank] = rec;
  }
}

}  // namespace smx
