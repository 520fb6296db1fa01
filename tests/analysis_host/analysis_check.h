// analysis_check.h -- TEST-ONLY: what the stand-alone check programs of the terrain analyses (tests/<name>_host/<name>_check.cpp) share:
// the random sequence, the inputs they make of it, the reader of a dump's head and the walk of main. A check program includes its
// <name>_host.cpp first (this file needs dh_map, dh_create and dh_destroy of drainage_host.cpp) and keeps what is its own: its Want,
// its plain restatement, its check and the part of check_dump behind the common head.
//
// rnd is ONE sequence for the whole program, so the inputs depend on the order and the number of the draws: make shuffles a
// permutation and then draws once per cell of a "lakes" map; make_columns draws once or twice per cell and shuffles nothing. Neither
// may draw more, less or in another order, or every program's inputs change.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <numeric>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

// ---- an input as heights and a wet mask (drainage, streams, hillslopes, flowpaths, dispersal). kind: "cone", "ramp", "plateau",
// "lakes" (random heights under a Bernoulli(0.2) wet mask); anything else: random heights, all different
struct Input { int dx, dy; std::vector<double> h; std::vector<uint8_t> wet; };

static Input make(const char* kind, int dx, int dy) {
  Input in{dx, dy, std::vector<double>((size_t)dx * dy), std::vector<uint8_t>((size_t)dx * dy, 0)};
  const size_t n = in.h.size();
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  for (size_t i = n; i > 1; i--) std::swap(perm[i - 1], perm[rnd() % i]);
  for (size_t c = 0; c < n; c++) {
    const int x = (int)(c / dy), y = (int)(c % dy);
    double v = perm[c];
    if (!strcmp(kind, "cone")) v = ((x - dx / 2) * (x - dx / 2) + (y - dy / 2) * (y - dy / 2)) * 16384.0 + perm[c];
    if (!strcmp(kind, "ramp")) v = (double)c;
    if (!strcmp(kind, "plateau")) v = 1024.0;
    in.h[c] = v * 0.0009765625;
    if (!strcmp(kind, "lakes")) in.wet[c] = (double)(rnd() >> 11) * (1.0 / 9007199254740992.0) < 0.2 ? 1 : 0;
  }
  return in;
}

static dh_map* host_map(const Input& in) {
  const size_t n = in.h.size();
  std::vector<uint32_t> count(n), type;
  std::vector<double> size, floor;
  for (size_t c = 0; c < n; c++) {
    count[c] = in.wet[c] ? 2 : 1;
    type.push_back(1); size.push_back(in.h[c]); floor.push_back(0.0);
    if (in.wet[c]) { type.push_back(0); size.push_back(0.5); floor.push_back(in.h[c]); }
  }
  return dh_create(in.dx, in.dy, count.data(), type.data(), size.data(), floor.data());
}

// ---- an input as a map at once (spill, through): heights of rnd() % 4096, so with ties. kind: "plateau", "sawtooth", "lakes" (a
// cell in five wet); anything else: the random heights
static dh_map* make_columns(const char* kind, int dx, int dy) {
  const size_t n = (size_t)dx * dy;
  std::vector<uint32_t> count(n), type;
  std::vector<double> size, floor;
  for (size_t c = 0; c < n; c++) {
    double h = (double)(rnd() % 4096) * 0.0009765625;
    if (!strcmp(kind, "plateau")) h = 1.0;
    if (!strcmp(kind, "sawtooth")) h = (c % 2 ? 1.0 : 0.25) + (double)(c / dy) * 4.0;
    const bool wet = !strcmp(kind, "lakes") && rnd() % 5 == 0;
    count[c] = wet ? 2 : 1;
    type.push_back(1); size.push_back(h); floor.push_back(0.0);
    if (wet) { type.push_back(0); size.push_back(0.5); floor.push_back(h); }
  }
  return dh_create(dx, dy, count.data(), type.data(), size.data(), floor.data());
}

static bool same_bits(const std::vector<double>& a, const double* b) { return a.empty() || memcmp(a.data(), b, a.size() * 8) == 0; }

template <class T> static bool take(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }

// ---- a dump of tests/test_<name>_host.py: u32 magic, i32 dimx, i32 dimy, u32 nsec, u32 count[cells], u32 type[nsec], f64 size[nsec],
// f64 floor[nsec] -- the columns exactly as the snapshot holds them -- and then what the analysis adds
struct Columns {
  uint32_t dimx = 0, dimy = 0;
  size_t cells = 0;
  std::vector<uint32_t> count, type;
  std::vector<double> size, floor;
  dh_map* map() const { return dh_create((int)dimx, (int)dimy, count.data(), type.data(), size.data(), floor.data()); }
};
// the head of the dump at `path` into `in`, then rest(f) for what follows it; false, with a FAIL line, where either does not hold
template <class Rest>
static bool read_dump(const char* path, uint32_t magic, Columns& in, Rest&& rest) {
  FILE* f = fopen(path, "rb");
  if (!f) { printf("FAIL cannot open %s\n", path); return false; }
  uint32_t head[4] = {0, 0, 0, 0};
  bool ok = fread(head, 4, 4, f) == 4 && head[0] == magic && (int32_t)head[1] > 0 && (int32_t)head[2] > 0 && head[1] <= 4096u && head[2] <= 4096u;
  in.dimx = head[1]; in.dimy = head[2];
  in.cells = ok ? (size_t)head[1] * head[2] : 0;
  ok = ok && take(f, in.count, in.cells) && take(f, in.type, head[3]) && take(f, in.size, head[3]) && take(f, in.floor, head[3]);
  uint64_t sum = 0;
  for (uint32_t c : in.count) sum += c;
  ok = ok && sum == head[3] && rest(f);
  fclose(f);
  if (!ok) printf("FAIL %s is not a dump\n", path);
  return ok;
}
static const char* file_name(const char* path) { const char* name = strrchr(path, '/'); return name ? name + 1 : path; }

// ---- main: with arguments, check_dump of each; without, check(name, maps) of one map of every kind at 33 x 47 and at 96 x 80 and of
// the `three` maps in one call. check makes its maps itself, in the order given. Exit status 0 = all equal.
struct MapSpec { const char* kind; int dx, dy; };
static std::vector<Input> make_all(const std::vector<MapSpec>& specs) {
  std::vector<Input> ins;
  for (const MapSpec& s : specs) ins.push_back(make(s.kind, s.dx, s.dy));
  return ins;
}
// check(name, maps) over the maps that make_columns makes of `specs`
template <class Check>
static int check_columns(const char* name, const std::vector<MapSpec>& specs, Check&& check) {
  std::vector<dh_map*> maps;
  for (const MapSpec& s : specs) maps.push_back(make_columns(s.kind, s.dx, s.dy));
  const int bad = check(name, maps);
  for (dh_map* m : maps) dh_destroy(m);
  return bad;
}
template <class Check>
static int check_main(int argc, char** argv, int (*check_dump)(const char*), std::initializer_list<const char*> kinds, const std::vector<MapSpec>& three, Check&& check) {
  int bad = 0;
  if (argc > 1) {
    for (int i = 1; i < argc; i++) bad += check_dump(argv[i]);
    return bad ? 1 : 0;
  }
  const int dims[2][2] = {{33, 47}, {96, 80}};
  for (const auto& d : dims)
    for (const char* kind : kinds) bad += check(kind, std::vector<MapSpec>{{kind, d[0], d[1]}});
  bad += check("three maps", three);
  return bad ? 1 : 0;
}
