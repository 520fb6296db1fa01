// streams_check -- a stand-alone run of the stream network bodies for the sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -o streams_check streams_check.cpp && ./streams_check
// Without arguments: a cone, a ramp, a plateau, random heights and random heights under a Bernoulli(0.2) wet mask at 33 x 47 and
// 96 x 80, and three maps in one call, thresholds 1 and 3, every tile shape, 64 and 256 lanes, the four launch orders, against plain
// loops (order, heads, reach and segment rank per cell; the records field by field), with caps above and below the count.
// With arguments: each names a dump written by tests/test_streams_host.py -- an input of tests/drainage_ref.py or the hand-built
// network with the restatement's result for one threshold: the columns' top records exactly as the snapshot holds them, then the
// count, the four planes and the records, all compared bit by bit. Every tile shape, 64 and 256 lanes, workgroups and lanes first to
// last and last to first. Little-endian words:
//   u32 magic 0x4D525453, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec], f64 floor[nsec],
//   u32 threshold, u32 nstreams, u32 order[cells], u32 segments[cells], u32 reach[cells], u32 heads[cells], 64-byte records[nstreams]
// Exit status 0 = all equal.
#include "streams_host.cpp"
#include "../analysis_host/analysis_check.h"

struct Want { std::vector<uint32_t> order, seg, reach, heads; std::vector<StreamRec> recs; };
static Want plain(const Input& in, uint32_t threshold) {
  const int dx = in.dx, dy = in.dy;
  const size_t n = in.h.size();
  auto height = [&](size_t c) { return in.wet[c] ? in.h[c] + 0.5 : in.h[c]; };
  std::vector<uint32_t> recv(n, DRAIN_NONE), area(n, 1u), term(n, DRAIN_NONE), stack;
  for (uint32_t c0 = 0; c0 < n; c0++) {   // lakes by a flood fill in cell order: term[c] = the smallest cell of c's lake
    if (!in.wet[c0] || term[c0] != DRAIN_NONE) continue;
    term[c0] = c0; stack.push_back(c0);
    while (!stack.empty()) {
      const uint32_t c = stack.back(); stack.pop_back();
      for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) {
        const int u = (int)(c / dy) + a, v = (int)(c % dy) + b;
        if ((a || b) && u >= 0 && v >= 0 && u < dx && v < dy && in.wet[(size_t)u * dy + v] && term[(size_t)u * dy + v] == DRAIN_NONE) {
          term[(size_t)u * dy + v] = c0; stack.push_back((uint32_t)(u * dy + v));
        }
      }
    }
  }
  for (uint32_t c = 0; c < n; c++) {
    if (in.wet[c]) continue;
    double best = height(c);
    for (int a = -1; a <= 1; a++) for (int b = -1; b <= 1; b++) {
      const int u = (int)(c / dy) + a, v = (int)(c % dy) + b;
      if ((a || b) && u >= 0 && v >= 0 && u < dx && v < dy && height((size_t)u * dy + v) < best) { best = height((size_t)u * dy + v); recv[c] = (uint32_t)(u * dy + v); }
    }
  }
  std::vector<uint32_t> by_h(n);   // donors before receivers: descending height (a receiver is strictly lower; no NaN in these inputs)
  std::iota(by_h.begin(), by_h.end(), 0u);
  std::stable_sort(by_h.begin(), by_h.end(), [&](uint32_t a, uint32_t b) { return height(a) > height(b); });
  for (uint32_t c : by_h) if (recv[c] != DRAIN_NONE) area[recv[c]] += area[c];
  for (size_t i = n; i-- > 0;) {
    const uint32_t c = by_h[i];
    if (!in.wet[c]) term[c] = recv[c] == DRAIN_NONE ? c : term[recv[c]];
  }
  auto channel = [&](uint32_t c) { return !in.wet[c] && area[c] >= threshold; };
  Want w;
  w.order.assign(n, 0u); w.seg.assign(n, STREAM_OFF); w.reach.assign(n, 0u); w.heads.assign(n, 0u);
  std::vector<uint32_t> nd(n, 0u), top(n, 0u), ntop(n, 0u);
  for (uint32_t c : by_h) {   // donors first: every donor of c has pushed its values into c's accumulators
    if (!channel(c)) continue;
    if (nd[c] == 0u) { w.order[c] = w.heads[c] = w.reach[c] = 1u; }
    else { w.order[c] = ntop[c] >= 2u ? top[c] + 1u : top[c]; w.reach[c] += 1u; }
    const uint32_t r = recv[c];
    if (r == DRAIN_NONE || !channel(r)) continue;
    nd[r]++; w.heads[r] += w.heads[c]; w.reach[r] = std::max(w.reach[r], w.reach[c]);
    if (w.order[c] > top[r]) { top[r] = w.order[c]; ntop[r] = 1u; } else if (w.order[c] == top[r]) ntop[r]++;
  }
  for (uint32_t c = 0; c < n; c++) {
    if (!channel(c) || nd[c] == 1u) continue;
    StreamRec s;
    memset(&s, 0, sizeof(s));
    const uint32_t k = (uint32_t)w.recs.size();
    uint32_t cur = c;
    s.first_cell = c; s.cells = 1u; s.down = STREAM_OFF; s.flags = nd[c] == 0u ? STREAM_F_HEAD : 0u;
    w.seg[c] = k;
    for (;;) {
      const uint32_t r = recv[cur];
      if (r == DRAIN_NONE) { s.flags |= STREAM_F_SINK; break; }
      if (r / dy != cur / dy && r % dy != cur % dy) s.diagonal++; else s.straight++;
      if (in.wet[r]) { s.flags |= STREAM_F_WET; break; }
      if (nd[r] >= 2u) { s.down = r; break; }
      cur = r; s.cells++; w.seg[cur] = k;
    }
    const uint32_t x = cur / dy, y = cur % dy;
    if (x == 0u || y == 0u || x == (uint32_t)dx - 1u || y == (uint32_t)dy - 1u) s.flags |= STREAM_F_BORDER;
    s.last_cell = cur; s.order = w.order[c]; s.heads = w.heads[c]; s.basin = term[c];
    s.area_first = area[c]; s.area_last = area[cur]; s.height_first = height(c); s.height_last = height(cur);
    w.recs.push_back(s);
  }
  return w;
}

static int check(const char* name, const std::vector<Input>& ins) {
  std::vector<dh_map*> maps;
  size_t words = 0;
  for (const Input& in : ins) { maps.push_back(host_map(in)); words += in.h.size(); }
  const uint32_t nm = (uint32_t)ins.size();
  int bad = 0;
  size_t shown = 0;
  for (uint32_t threshold : {1u, 3u}) {
    std::vector<Want> wants;
    uint32_t most = 0;
    for (const Input& in : ins) { wants.push_back(plain(in, threshold)); most = std::max<uint32_t>(most, (uint32_t)wants.back().recs.size()); }
    shown = wants[0].recs.size();
    for (int v = 0; v < dh_variants(); v++)
      for (uint32_t lanes : {64u, 256u})
        for (int order = 0; order < 4; order++) {
          const uint32_t cap = order == 1 ? most / 2u : most + 2u;   // (one launch order with fewer records than segments)
          std::vector<uint32_t> ns(nm, 0), o(words), sg(words), re(words), hd(words);
          std::vector<StreamRec> out((size_t)nm * cap + 1u);
          if (sh_streams(maps.data(), nm, v, lanes, order, threshold, cap, out.data(), ns.data(), o.data(), sg.data(), re.data(), hd.data()) != 0) { bad++; continue; }
          bool ok = true;
          size_t at = 0;
          for (uint32_t i = 0; i < nm && ok; i++) {
            const Want& w = wants[i];
            const size_t n = w.order.size();
            ok = ns[i] == w.recs.size() && std::equal(w.order.begin(), w.order.end(), o.begin() + at) && std::equal(w.seg.begin(), w.seg.end(), sg.begin() + at) &&
                 std::equal(w.reach.begin(), w.reach.end(), re.begin() + at) && std::equal(w.heads.begin(), w.heads.end(), hd.begin() + at);
            const size_t k = std::min<size_t>(cap, w.recs.size());
            ok = ok && (k == 0 || memcmp(out.data() + (size_t)i * cap, w.recs.data(), k * sizeof(StreamRec)) == 0);
            at += n;
          }
          if (!ok) { printf("FAIL %s threshold %u variant %d lanes %u order %d\n", name, threshold, v, lanes, order); bad++; }
        }
  }
  for (dh_map* m : maps) dh_destroy(m);
  printf("%-10s %zu map(s), %5zu segments in the first at threshold 3  %s\n", name, ins.size(), shown, bad ? "FAILED" : "ok");
  return bad;
}

static int check_dump(const char* path) {
  Columns in;
  uint32_t tn[2] = {0, 0};
  std::vector<uint32_t> o, sg, re, hd;
  std::vector<StreamRec> recs;
  if (!read_dump(path, 0x4D525453u, in, [&](FILE* f) {
        const size_t n = in.cells;
        return fread(tn, 4, 2, f) == 2 && tn[0] >= 1u && tn[1] <= n && take(f, o, n) && take(f, sg, n) && take(f, re, n) && take(f, hd, n) && take(f, recs, tn[1]);
      })) return 1;
  const size_t n = in.cells;
  const uint32_t threshold = tn[0], ns = tn[1];
  dh_map* h = in.map();
  int bad = 0;
  for (int v = 0; v < dh_variants(); v++)
    for (uint32_t lanes : {64u, 256u})
      for (int order : {0, 3}) {
        uint32_t got = 0;
        std::vector<uint32_t> a(n), b(n), c(n), d(n);
        std::vector<StreamRec> out((size_t)ns + 2u);
        memset(out.data(), 0, out.size() * sizeof(StreamRec));
        const bool same = sh_streams(&h, 1, v, lanes, order, threshold, ns + 2u, out.data(), &got, a.data(), b.data(), c.data(), d.data()) == 0 && got == ns && a == o &&
                          b == sg && c == re && d == hd && (ns == 0 || memcmp(out.data(), recs.data(), (size_t)ns * sizeof(StreamRec)) == 0);
        if (!same) { printf("FAIL %s variant %d lanes %u order %d: %u segments, expected %u\n", path, v, lanes, order, got, ns); bad++; }
      }
  dh_destroy(h);
  printf("%-36s %4ux%-4u threshold %2u %6u segments  %s\n", file_name(path), in.dimx, in.dimy, threshold, ns, bad ? "FAILED" : "ok");
  return bad;
}

int main(int argc, char** argv) {
  return check_main(argc, argv, check_dump, {"cone", "ramp", "plateau", "random", "lakes"}, {{"lakes", 33, 47}, {"cone", 70, 1}, {"random", 1, 70}},
                    [](const char* name, const std::vector<MapSpec>& specs) { return check(name, make_all(specs)); });
}
