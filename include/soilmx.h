/* soilmx -- C-ABI of the MI355X-native SoilMachine particle-transport hot path.
 *
 * The reference (weigert/SoilMachine) has no FFI layer: its boundary is a source-level C++ header API
 * consumed by one translation unit (SoilMachine.cpp:19-28). This header is the seam a maintainer would
 * bind instead: every entry point names the reference interface it replaces (paths relative to the
 * reference root). Plain pointers and sizes only; no C++ or torch types cross this line.
 *
 * Conventions: all functions return 0 on success, <0 on error (smx_last_error() gives the text);
 * the caller is single-threaded per context (as the reference is, SURVEY.md §8b "Threading");
 * buffers are caller-allocated; "cell order" is the Layermap index x*dimy + y (source/layermap.h:151),
 * "frequency order" is y*dimx + x (source/particle/water.h:53,349).
 *
 * Exactness contract: under SMX_ENGINE_SERIAL and SMX_ENGINE_SPECULATIVE smx_tick* executes the reference's sequential
 * semantics (SoilMachine.cpp:283-329) -- results are bit-identical to the reference CPU path for the same soil table,
 * terrain, SCALE and libc rand() stream. SMX_ENGINE_BATCHED / SMX_ENGINE_RELAXED are deterministic throughput schedules that
 * do NOT keep the reference's particle order: statistical parity only, measured against the reference's own sensitivity to
 * its rand() stream.
 */
#ifndef SOILMX_H
#define SOILMX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smx_ctx smx_ctx;

/* POD mirror of SurfParam (source/surface.h:11-39); render-only fields (name, color, phong) dropped. */
typedef struct smx_soil {
  uint32_t transports, erodes, cascades, abrades;
  float density, porosity, solubility, equrate, friction, erosionrate, maxdiff, settling, suspension, abrasion;
} smx_soil;

/* POD mirror of SurfLayer (source/surface.h:65-101). */
typedef struct smx_layer {
  uint32_t type;
  float min, bias, scale, octaves, lacunarity, gain, frequency;
} smx_layer;

enum { SMX_ENGINE_SERIAL = 0,      /* one device walker, reference order (parity anchor)            */
       SMX_ENGINE_SPECULATIVE = 1, /* optimistic parallel particles, ordered commit, same results    */
       SMX_ENGINE_BATCHED = 2,     /* THROUGHPUT mode: all particles of a phase advance concurrently, one step
                                      per epoch, each step atomic and isolated (claim tiles). Deterministic, but NOT
                                      the reference's particle order: statistical parity only        */
       SMX_ENGINE_RELAXED = 3      /* the batched engine with RELAXED isolation (csrc/soil_relax.h): every running particle steps
                                      in every epoch on the epoch's start state; erosion / deposit are queued per cell and applied
                                      in slot order with Layermap::add / remove, Particle::cascade runs once per touched cell in nine
                                      colour passes; floods and nested particles as in BATCHED. Deterministic; statistical parity  */ };

typedef struct smx_config {
  int32_t dimx, dimy;              /* SIZEX, SIZEY (SoilMachine.cpp:9-10)                            */
  int32_t scale;                   /* SCALE (SoilMachine.cpp:11)                                     */
  int32_t device;                  /* HIP device ordinal                                             */
  uint64_t pool_capacity;          /* POOLSIZE (SoilMachine.cpp:16): max live sections               */
  int32_t engine;                  /* SMX_ENGINE_*                                                   */
  int32_t reserved;
} smx_config;

typedef struct smx_counters {
  uint64_t steps_water_top;        /* WaterParticle::move()==true for top-level particles            */
  uint64_t steps_water_all;        /* ... including nested particles (water.h:251-262)               */
  uint64_t steps_wind;
  uint64_t nested_particles;
  uint64_t floods;
  uint64_t cascade_calls;          /* Particle::cascade (particle.h:24)                              */
  uint64_t cascade_transfers;
  uint64_t wcascade_calls;         /* WaterParticle::cascade (water.h:151)                           */
  uint64_t grid_active_cells;      /* cells the exact grid pass had to visit                         */
  uint64_t rand_calls;             /* rand() draws consumed since smx_srand                          */
  uint64_t pool_free;              /* == map.pool.free.size() (layermap.h:69, SoilMachine.cpp:116)   */
  uint64_t pool_overflow;          /* pool.get() on an empty pool (layermap.h:92-95)                 */
  uint64_t spec_rounds;            /* speculative engine: execution rounds                           */
  uint64_t spec_aborts;            /* speculative engine: particle executions thrown away            */
  uint64_t reserved[2];            /* [0] phases the speculative engine handed to the serial walker, [1] particle executions         */
  uint64_t spec_subphases_cut;     /* speculative engine: sub-phases that ended early (nested-slot budget used up) and were re-armed  */
  uint64_t spec_serial_particles;  /* ... single particles run by the serial walker between two sub-phases (more nested particles    */
                                   /*     than a sub-phase has slots)                                                                */
  uint64_t flood_nested_steps;     /* round 6 (sized getter only): steps of the nested particles that ran INSIDE floods of the relaxed  */
  uint64_t grid_nested_steps;      /* schedule / INSIDE grid tiles -- both are part of steps_water_all; bench.py prices those launches */
} smx_counters;

/* Elapsed device time of the phases of the last smx_tick* calls, measured with HIP events on the
 * context's stream (milliseconds, accumulated since smx_timing_reset). */
typedef struct smx_timing {
  double ms_water, ms_grid, ms_wind, ms_freq;
  uint64_t launches_water, launches_grid, launches_wind, launches_freq;
  /* the particle kernels alone (k_water_serial / k_wind_serial, or every k_spec_exec launch of the speculative
   * engine), each launch bracketed by its own pair of HIP events */
  double ms_kernel_water, ms_kernel_wind;
  uint64_t launches_kernel_water, launches_kernel_wind;
  /* the O(cells) streaming kernels on their own: grid-pass classification (k_grid_classify), the batched engine's nine
   * colour passes (k_batch_grid), water.h:358-365 (k_map_frequency) */
  double ms_kernel_classify, ms_kernel_gridtiles, ms_kernel_mapfreq;
  uint64_t launches_kernel_classify, launches_kernel_gridtiles, launches_kernel_mapfreq;
  /* round 5 (smx_get_timing_sized only): ALL launches of the throughput engines' step kernels (k_relax_step / k_batch_epoch), whether
   * bracketed by events or not. The relaxed water step kernel is bracketed every 8th launch (SMX_STEP_EVENT_SAMPLE): ms_kernel_water /
   * launches_kernel_water is then the average duration over the bracketed launches, and the algorithmic bytes per launch are the
   * steps of ALL launches over launches_step_water (bench.py). */
  uint64_t launches_step_water, launches_step_wind;
  /* round 6 (smx_get_timing_sized only): the relaxed water phase's persistent launches, each between its own pair of HIP events --
   * k_relax_epochs (the dense epochs of a generation: step, apply, filter, colour lists and floods behind device-wide barriers) and
   * k_relax_tail (the same phases inside one workgroup once <= 256 particles run): milliseconds, launches, epochs the launches covered;
   * and the generations of suspended nested particles the grid pass leaves behind (part of ms_grid) */
  double ms_kernel_epochs, ms_kernel_tail, ms_kernel_grid_children;
  uint64_t launches_kernel_epochs, epochs_kernel_epochs, launches_kernel_tail, epochs_kernel_tail, launches_kernel_grid_children;
  /* k_relax_floods: every 7th launch of a context is bracketed (ms / launches_kernel_floods); launches_floods_all counts every launch. Under
   * smx_set_relax_settle mode 2 the launch is k_relax_settle_floods: the figures then time the JOINED launch, settle included. */
  double ms_kernel_floods;
  uint64_t launches_kernel_floods, launches_floods_all;
} smx_timing;

/* ---- life cycle: replaces Layermap::Layermap + secpool::reserve (layermap.h:64-119,218-226) ---- */
int smx_create(const smx_config* cfg, smx_ctx** out);
/* A context that HOLDS only the columns [x_lo, x_hi) of the dimx x dimy map -- one column strip with its halo, for smx_strips_*: cells,
 * flags and the engines' per-cell planes are allocated for that range (indexing stays global), so per-device memory follows the strip,
 * not the map (the frequency planes, 12 B/cell, stay full-size: their index y*dimx + x is not contiguous in x). x_lo * dimy must be a
 * multiple of 64. Whole-map calls (exact engines, save/load, vertices, point operations) refuse such a context; import / export /
 * read_heights / digest act on the held range. pool_capacity is this context's own. */
int smx_create_strip(const smx_config* cfg, int32_t x_lo, int32_t x_hi, smx_ctx** out);
void smx_destroy(smx_ctx* ctx);
const char* smx_last_error(smx_ctx* ctx);

/* ---- tables: replaces the globals soils[] / SCALE read by every particle (surface.h:41, SoilMachine.cpp:11) ---- */
int smx_set_soils(smx_ctx* ctx, const smx_soil* soils, int32_t n);
int smx_set_scale(smx_ctx* ctx, int32_t scale);

/* ---- libc rand() stream hand-off: replaces srand(SEED)/rand() (SoilMachine.cpp:41, water.h:13, wind.h:15) ---- */
int smx_srand(smx_ctx* ctx, uint32_t seed);
int smx_rand(smx_ctx* ctx, int32_t* out);               /* draw one value on behalf of the host */
int smx_rand_advance(smx_ctx* ctx, uint64_t ndraws);    /* discard ndraws values (resume a stream at a known offset) */
/* the generator itself (glibc TYPE_3: the last 31 words, the running index, draws since smx_srand): hand the stream from one
 * context to another (the compat Layermap does when the host re-initialises with a new map size, SoilMachine.cpp:111-114) */
int smx_get_rand_state(smx_ctx* ctx, uint32_t ring31[31], uint32_t* idx, uint64_t* calls);
int smx_set_rand_state(smx_ctx* ctx, const uint32_t ring31[31], uint32_t idx, uint64_t calls);

/* ---- terrain: replaces Layermap::initialize + SurfLayer::get + FastNoiseLite (layermap.h:163-216, surface.h:82-99) ---- */
int smx_initialize(smx_ctx* ctx, int32_t seed, const smx_layer* layers, int32_t nlayers);

/* ---- state hand-over (snapshot layout, columns bottom->top in cell order); replaces direct access to
 *      Layermap::dat / sec lists (layermap.h:37-62,131) and WaterParticle/WindParticle::frequency,track ---- */
int smx_import_columns(smx_ctx* ctx, const uint32_t* count, const uint32_t* type, const double* size,
                       const double* floor, const double* sat);
int smx_import_frequency(smx_ctx* ctx, const float* wfreq, const float* wtrack, const float* windfreq);
int smx_num_sections(smx_ctx* ctx, uint64_t* out);
int smx_export_columns(smx_ctx* ctx, uint32_t* count, uint32_t* type, double* size, double* floor, double* sat);
int smx_read_frequency(smx_ctx* ctx, float* wfreq, float* wtrack, float* windfreq);   /* NULL = skip */
int smx_read_heights(smx_ctx* ctx, double* out);        /* Layermap::height(ivec2) for every cell (layermap.h:422) */
int smx_read_surface(smx_ctx* ctx, uint32_t* out);      /* Layermap::surface(ivec2) for every cell (layermap.h:417) */

/* ---- checkpoint / resume on disk (the reference has none: SURVEY.md 5; io.h:232 "Should be able to also WRITE to file").
 * File = the snapshot layout of soilmachine_amd/snapshot.py (64-byte header "SMXSNAP1", per-cell section counts, sections
 * bottom -> top, the three frequency planes) followed by a trailer "SMXRAND1" with the rand() generator's 31-word ring, its
 * index and the number of draws -- a loaded context continues the libc stream exactly where the saved one stopped.
 * Since round 4 a second trailer "SMXFLAG1" carries the per-column flag plane (one byte per cell; its sticky "has held a saturation"
 * bit is context state the column records cannot express, and the throughput engines fix the active set of their grid pass from
 * it): every engine now continues bit-identically from a file (tests/test_gpu_depth.py). A bare snapshot without the trailers still
 * loads (return 1: re-seed the generator; the flag plane is re-derived from the saturations present). ---- */
int smx_save(smx_ctx* ctx, const char* path);
int smx_load(smx_ctx* ctx, const char* path);           /* dims must match the context; SCALE and soils are the caller's */

/* ---- the hot path, phase by phase: replaces SoilMachine.cpp:287-320 ---- */
int smx_tick_water(smx_ctx* ctx, int32_t nwater);       /* :287-298  NWATER x {WaterParticle ctor; move/interact; flood} */
int smx_grid_pass(smx_ctx* ctx);                        /* :300-301  WaterParticle::seep(map) (water.h:335-343)          */
int smx_tick_wind(smx_ctx* ctx, int32_t nwind);         /* :303-307  NWIND x {WindParticle ctor; move/interact}          */
int smx_map_frequency(smx_ctx* ctx);                    /* :314      WaterParticle::mapfrequency (water.h:358-365)       */
int smx_reset_frequency(smx_ctx* ctx);                  /* :319      WaterParticle::resetfrequency (water.h:353-356)     */
int smx_tick(smx_ctx* ctx, int32_t nwater, int32_t nwind, int32_t dowater, int32_t dowind);   /* all of the above, in order */
int smx_sync(smx_ctx* ctx);                             /* wait for all queued device work */

/* ---- ensembles: many independent maps on the exact SERIAL engine, ticked together; replaces a host loop of
 *      SoilMachine.cpp:283-329 over several worlds (seeds, soil tables, sizes, SCALE) ----
 * A member is an ordinary full-map context, created by smx_ensemble_add on the ensemble's stream and owned by the ensemble:
 * every single-context entry point works on it (set_soils, set_scale, srand, initialize, import / export, save / load, digest,
 * counters, read_*, smx_tick between two ensemble ticks), and work queued through the member and through the ensemble stays in
 * order. smx_destroy on a member frees nothing (smx_last_error says so); smx_ensemble_remove frees one member, smx_ensemble_destroy
 * the ensemble and all its members.
 * smx_ensemble_tick leaves member i in exactly the state smx_tick(member_i, nwater[i], nwind[i], dowater, dowind) would: columns,
 * frequency planes, the rand() generator and every counter. Each phase is a fixed number of launches for all members, one
 * wavefront per member on the walkers, so the launch count of a tick does not depend on the member count; the member table is
 * the only per-tick copy.
 * Limits: at most SMX_ENSEMBLE_MAX_MEMBERS members, all on the ensemble's device, each with cfg->engine == SMX_ENGINE_SERIAL
 * (others: -2). A member's section pool is cfg->pool_capacity as given -- the reference's POOLSIZE (10 M sections, 360 MB with
 * the free list) is far too much for hundreds of members; a member whose pool runs out counts pool_overflow in its own counters
 * and drops sections exactly as a standalone context does, without touching its neighbours. An add that runs out of device
 * memory returns < 0 and leaves the ensemble as it was. */
typedef struct smx_ensemble smx_ensemble;
enum { SMX_ENSEMBLE_MAX_MEMBERS = 4096 };
int smx_ensemble_create(int32_t device, smx_ensemble** out);   /* -3 + error text without a device; destroy is safe on the handle */
void smx_ensemble_destroy(smx_ensemble* e);                    /* frees the ensemble AND its members */
const char* smx_ensemble_last_error(smx_ensemble* e);
int smx_ensemble_add(smx_ensemble* e, const smx_config* cfg, smx_ctx** member);   /* Layermap::Layermap per member (as smx_create) */
/* waits for the ensemble's queued work, takes the member out (the members after it move up one place in the order of addition) and
 * frees it; -2 if it is not a member of e */
int smx_ensemble_remove(smx_ensemble* e, smx_ctx* member);
int smx_ensemble_size(smx_ensemble* e, int32_t* n);
/* SoilMachine.cpp:283-329 for every member: nwater[i] / nwind[i] per member in order of addition; nwater[i] < 0 = member i sits
 * this tick out entirely. nwind may be NULL when dowind == 0. */
int smx_ensemble_tick(smx_ensemble* e, const int32_t* nwater, const int32_t* nwind, int32_t dowater, int32_t dowind);
int smx_ensemble_sync(smx_ensemble* e);                                              /* wait for all queued device work */
/* phase times and launch counts of the ensemble's ticks (the smx_timing fields of the serial engine: water / grid / wind / freq
 * phases, and the kernels k_ens_water, k_ens_wind, k_ens_classify, k_ens_frequency in the kernel_water / _wind / _classify /
 * _mapfreq fields), written as smx_get_timing_sized does */
int smx_ensemble_get_timing(smx_ensemble* e, smx_timing* out, uint64_t struct_size);
int smx_ensemble_timing_reset(smx_ensemble* e);
/* ---- an ensemble observed as one thing: per-member figures and cross-member statistics of a plane ----
 * Both calls run on the ensemble's stream (they see every tick queued before them), launch a fixed number of kernels whatever the
 * member count (one table upload, k_ens_figures or k_ens_plane_stats, one copy of the RESULTS back), synchronise once before they
 * return and change no member state. Layermap::height(ivec2) = floor + size of the top section, 0 for an empty column
 * (layermap.h:422-425); Layermap::surface(ivec2) = the top section's type, 0 (Air) for an empty column (layermap.h:417-420) -- a wet
 * cell is a NON-EMPTY column whose top section is Air.
 * Every field is bit-identical to what the per-member path gives on the same state: sumh / nsec / typehash to the digest of the
 * "observability" block below, rand_calls and live_sections to their getters, the water fields to the same folds over exported columns. */
typedef struct smx_member_figures {      /* 80 bytes; a caller passes sizeof(ITS struct) and gets that prefix */
  double   sumh;          /* sum of Layermap::height over the cells in index order x*dimy+y, sequential f64 accumulation  */
  uint64_t nsec;          /* number of sections                                                                          */
  uint64_t typehash;      /* h = (h ^ type) * 1099511628211 from 1469598103934665603: cells in index order, top -> bottom */
  uint64_t wet_cells;     /* cells whose top section is water (type Air = 0)                                             */
  double   water_volume;  /* sum of the sizes of those top sections, cells in index order, sequential f64 accumulation   */
  double   hmin, hmax;    /* extremes of Layermap::height (an empty column counts as 0)                                  */
  uint64_t empty_cells;
  uint64_t rand_calls;    /* rand() draws since the member's last srand (`calls` of the generator state)                 */
  uint64_t live_sections; /* the context's own section counter; equals nsec on a sound map                               */
} smx_member_figures;
/* one entry per member in member order, entry i at byte i * struct_size. An empty ensemble: 0, nothing written. A section chain that
 * leaves the pool or has more links than the member's pool holds: -5, the error text names the member, nothing written. */
int smx_ensemble_figures(smx_ensemble* e, smx_member_figures* out, uint64_t struct_size);
/* Per cell c, over the n members which[0..n) IN THAT ORDER (which == NULL: all members in member order, n ignored), with v_i =
 *   SMX_PLANE_HEIGHT    floor + size of member i's top section in c (0 for an empty column: Layermap::height)
 *   SMX_PLANE_WATER     that section's size if its type is Air, else 0
 *   SMX_PLANE_WFREQ / _WINDFREQ   the f32 value of the water / wind frequency plane, widened to f64:
 *   mean = (((v_0 + v_1) + ...) + v_{n-1}) / n and var = (((v_0 - mean)^2 + (v_1 - mean)^2) + ...) / n (population variance, a second
 *   pass, run only where var != NULL) in f64 without contraction, so that a host loop `acc += v[i]` over the members gives the same
 *   bits; vmin / vmax; nonzero = members with v_i != 0 (on WATER: in how many runs the cell holds water). A NULL output is skipped.
 * Outputs hold dimx*dimy values in the plane's own indexing: x*dimy+y for HEIGHT / WATER (as the heights reader), y*dimx+x for the
 * frequency planes (as the frequency reader). The selected members must have equal dimx and dimy; unequal dims, an index out of
 * range, a repeated index or n == 0 return -2 and the error text names the offender. */
enum { SMX_PLANE_HEIGHT = 0, SMX_PLANE_WATER = 1, SMX_PLANE_WFREQ = 2, SMX_PLANE_WINDFREQ = 3 };
int smx_ensemble_plane_stats(smx_ensemble* e, int32_t plane, const int32_t* which, int32_t n,
                             double* mean, double* var, double* vmin, double* vmax, uint32_t* nonzero);
/* ---- forking: a map that already exists becomes the state of another context, or of n new ensemble members, on the device ----
 * smx_copy_state leaves dst in the state that smx_save(src, f); smx_set_soils(dst, <src's table>); smx_load(dst, f) == 0 leaves it in:
 * the columns, the three frequency planes, the rand() generator (ring, index, draw count), SCALE, the soil table, the flag plane
 * as smx_load builds it (water on top, any saturation in the column, OR src's sticky "has held a saturation" bit) and the live-section
 * count. dst's other counters, its engine and its engine settings stay as they are. dst's pool is laid out as smx_import_columns lays
 * it out -- buried sections at pool indices 0..used-1 in cell order, bottom -> top within a column, freelist[i] = cap-1-i -- whatever
 * src's pool looks like, so the two may differ in pool_capacity. Nothing but a few words (totals, an error flag) crosses the host: the
 * source is counted (k_fork_count), the counts are scanned, the sections are scattered (k_fork_scatter), the planes copied
 * (k_fork_planes). The call is ordered behind the work queued on src's stream by an event and synchronises before it returns.
 * smx_ensemble_fork appends n new members to e, each with src's dims and SCALE, the SERIAL engine, pool_capacity sections (0 = src's
 * own capacity), the smx_copy_state state and every counter zero but the live sections. seeds == NULL: every member continues src's
 * generator exactly (identical copies, the caller's to perturb); otherwise member i is as after smx_srand(member_i, seeds[i]). src
 * is any full-map context on the ensemble's device -- standalone of any engine, a member of e or of another ensemble -- and is only
 * read. The source is counted and scanned once and all members are written by the same two launches, whatever n.
 * Errors leave dst / e, its members and src exactly as they were: -2 a null argument, n <= 0, more than SMX_ENSEMBLE_MAX_MEMBERS,
 * dst == src, unequal dims (copy_state), another device, a strip context; -4 src holds more live sections (tops included) than the
 * destination's pool_capacity; -5 a chain of src leaves its pool or has more links than the pool holds (the text names the cell); a
 * fork that runs out of device memory returns < 0 and frees every member it had made. */
int smx_copy_state(smx_ctx* dst, smx_ctx* src);
int smx_ensemble_fork(smx_ensemble* e, smx_ctx* src, int32_t n, uint64_t pool_capacity, const uint32_t* seeds, smx_ctx** members /* n handles out */);
/* ---- the lake census: which lakes are there, how big, how deep, how level -- connected wet cells labelled on the device ----
 * A WET CELL is a non-empty column whose top section is Air (type 0), the rule of smx_member_figures.wet_cells: empty columns and
 * buried water are dry. A LAKE is a maximal set of wet cells connected through the EIGHT neighbours, the neighbourhood
 * WaterParticle::cascade levels water over (source/particle/water.h:155-164); cells do not connect across the map border. A lake's
 * IDENTITY is its smallest cell index x*dimy+y, first_cell; lakes are listed in ascending first_cell, and lake k of that order has
 * RANK k. Every field of a record is an integer or an order-free extreme: nothing depends on a summation order, and a host
 * restatement reproduces each bit.
 *   volume_q40   sum over the lake's cells of floor(size * 2^40), size = the top Air section's size: an exact integer (the scaling
 *                and the floor are exact in f64). volume_q40 * 2^-40 lies below the exact sum of the sizes by less than cells * 2^-40.
 *   level_min / level_max   extremes of Layermap::height (floor + size) over the lake: equal on a levelled lake, their spread says
 *                how far the lake is from settled.     depth_max   the largest top-section size.     For all three, -0 < +0.
 *   x0, y0, x1, y1   the inclusive bounding box.
 *   flags        bit 0: a cell of the lake lies on the map border. bit 1: the volume is unreliable -- a size was not finite, was
 *                negative or was >= 2^24 (such a cell contributes 0), or the 64-bit sum wrapped.
 * A caller passes sizeof(ITS struct) and gets that prefix of each record, as with smx_member_figures. */
typedef struct smx_lake {                /* 64 bytes */
  uint32_t first_cell, cells;
  uint64_t volume_q40;
  double   level_min, level_max;
  double   depth_max;
  uint16_t x0, y0, x1, y1;
  uint32_t flags;
  uint32_t reserved[3];                  /* written as 0 */
} smx_lake;
/* *nlakes = the number of lakes, whatever cap is; the first min(cap, *nlakes) records are written in rank order, record k at byte
 * k * struct_size; out may be NULL when cap is 0 (counting only). labels (NULL = skip): dimx*dimy words in cell order, the rank of
 * the cell's lake or 0xFFFFFFFF for a dry cell. In the ensemble call member i's records start at out + i * cap_per_member records
 * and nlakes holds one count per member in member order; an empty ensemble: 0, nothing written.
 * Both calls run on the context's / the ensemble's stream (they see every tick queued before them), launch the same kernels
 * whatever the map holds and however many members there are (one table upload; k_lake_tiles, k_lake_merge, k_lake_flatten, a
 * prefix sum, k_lake_stats; the RESULTS copied back), synchronise once and change neither a map nor a counter. Only the 32-byte
 * top records are read, so a context of any engine serves; a strip context, a null context and struct_size == 0 return -2. The
 * scratch -- two u32 planes per cell and the records asked for -- is allocated by the first census and kept; an allocation that
 * fails returns < 0 and leaves the context / the ensemble usable. Maps of up to 65536 cells a side and 2^32 - 2 cells per call. */
int smx_lakes(smx_ctx* ctx, smx_lake* out, uint64_t struct_size, uint32_t cap, uint32_t* nlakes, uint32_t* labels);
int smx_ensemble_lakes(smx_ensemble* e, smx_lake* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nlakes);
/* ---- drainage: where the water goes -- every dry cell's receiver, the basin every cell drains into, the contributing area ----
 * Cells are indexed c = x*dimy+y; h(c) is Layermap::height (floor + size of the top record in one f64 addition, 0.0 for an empty
 * column); a WET cell and a LAKE are those of smx_lakes. A wet cell has no RECEIVER. A dry cell's receiver is the in-map cell n among
 * its eight neighbours (cells do not connect across the map border) with h(n) < h(c) and the smallest (h(n), n): plain f64 `<` on h,
 * then the smaller cell index -- so -0.0 and +0.0 tie, and a NaN height is never lower and never has a lower neighbour. A dry cell
 * without one is a SINK. Every path strictly descends in h, so it ends at a sink or at the first wet cell it meets. A BASIN is the set
 * of cells whose path ends at one sink or in one lake (a wet cell belongs to its own lake's basin); its IDENTITY first_cell is the
 * sink's index or the lake's first_cell -- join on it with the records of smx_lakes --, basins are listed in ascending first_cell,
 * and basin k of that order has RANK k. area(c) = 1 + the sum of area(d) over the cells d whose receiver is c, as u32: the basin's
 * size at a sink, one plus the dry land that enters the lake there at a wet cell; over all sinks and wet cells it sums to dimx*dimy.
 * Every figure is a comparison, an integer or an order-free extreme: a host restatement reproduces each bit. */
typedef struct smx_basin {               /* 48 bytes; a caller passes sizeof(ITS struct) and gets that prefix of each record */
  uint32_t first_cell;                   /* the sink's cell, or the lake's first_cell */
  uint32_t cells;                        /* cells of the basin, wet ones included */
  uint32_t wet_cells;                    /* 0 for a sink's basin, the lake's cells otherwise */
  uint32_t flags;                        /* bit 0: the terminal is a lake; bit 1: the sink lies on, or the lake touches, the map border */
  double   height_min, height_max;       /* extremes of h over the basin, -0 < +0 as in smx_lake */
  uint16_t x0, y0, x1, y1;               /* the inclusive bounding box of the basin */
  uint32_t reserved[2];                  /* written as 0 */
} smx_basin;
/* *nbasins = the number of basins, whatever cap is; the first min(cap, *nbasins) records are written in rank order, record k at byte
 * k * struct_size; out may be NULL when cap is 0 (counting only). The planes (NULL = skip) hold dimx*dimy words in cell order:
 * receivers -- the receiver's cell index, 0xFFFFFFFF for a sink and for a wet cell; labels -- the rank of the cell's basin (no cell is
 * without one); area -- as defined above (with area == NULL the two accumulation launches are skipped). In the ensemble call member
 * i's records start at out + i * cap_per_member records and nbasins holds one count per member; an empty ensemble: 0, nothing written.
 * Both calls run on the context's / the ensemble's stream (they see every tick queued before them), launch the same kernels whatever
 * the map holds and however many members there are (one table upload; k_lake_tiles, k_lake_merge, k_lake_flatten on the call's own
 * scratch, k_drain_recv, k_drain_resolve, a prefix sum, k_drain_stats, and for the area k_drain_pending, k_drain_area; the RESULTS
 * copied back), synchronise once and change no map, flag, counter or generator. Only the 32-byte top records are read, so a context
 * of any engine serves; a strip context, a null argument, struct_size == 0 and records asked for with out == NULL return -2. The
 * scratch -- three u32 planes per cell, five once an area was asked for, and the records asked for -- is the call's own (smx_lakes
 * keeps its own), allocated at first use and kept; an allocation that fails returns < 0 and leaves the context / the ensemble usable.
 * Maps of up to 65536 cells a side and 2^32 - 2 cells per call. */
int smx_drainage(smx_ctx* ctx, smx_basin* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins,
                 uint32_t* receivers, uint32_t* labels, uint32_t* area);
int smx_ensemble_drainage(smx_ensemble* e, smx_basin* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins);
/* ---- streams: the channel network on top of the drainage -- Strahler order, Shreve magnitude, reach, one record per segment ----
 * Cells, h(c), wet cells, lakes, receivers, sinks, basins and area are those of smx_drainage; threshold is a u32 >= 1. A CHANNEL cell
 * is a dry cell with area(c) >= threshold; area strictly grows downstream, so the receiver of a channel cell is a channel cell or a
 * wet cell, and threshold 1 makes every dry cell a channel cell. The channel DONORS of c are the channel cells whose receiver is c
 * (0 to 8). A HEAD is a channel cell with no channel donor, a CONFLUENCE one with two or more. order(c) is the Strahler order: 1 at
 * a head; else, with m the largest order among the channel donors, m where exactly one donor has it and m + 1 where two or more do.
 * heads(c) is the Shreve magnitude: 1 at a head, else the u32 sum of the donors' heads. reach(c) is the number of cells on the
 * longest channel path from a head down to and including c: 1 at a head, else 1 + the largest reach among the donors. All three are
 * 0 off the channels. A SEGMENT starts at a head or at a confluence -- its IDENTITY first_cell -- and runs downstream through channel
 * cells that have exactly one channel donor; its last_cell is the cell whose receiver is a confluence (the segment ends above it) or
 * a wet cell (the segment enters a lake), or which is a sink. The segments partition the channel cells, order and heads are constant
 * along one, segments are listed in ascending first_cell, and segment k of that order has RANK k. Every figure is a comparison, an
 * integer or a copied double: a host restatement reproduces each bit, whatever the launch shape and the order of arrival. */
typedef struct smx_segment {              /* 64 bytes; a caller passes sizeof(ITS struct) and gets that prefix of each record */
  uint32_t first_cell, last_cell;        /* the two end cells (the same cell for a one-cell segment) */
  uint32_t cells;                        /* cells of the segment */
  uint32_t order;                        /* the Strahler order */
  uint32_t down;                         /* first_cell of the segment it joins (the confluence below last_cell), else 0xFFFFFFFF */
  uint32_t basin;                        /* first_cell of the basin it lies in: join with smx_drainage / smx_lakes */
  uint32_t flags;                        /* 1: last_cell drains into a wet cell  2: last_cell is a sink  4: first_cell is a head (else a
                                            confluence)  8: last_cell lies on the map border */
  uint32_t heads;                        /* the Shreve magnitude */
  uint32_t straight, diagonal;           /* receiver steps from first_cell to last_cell PLUS the step that leaves last_cell (where it has
                                            a receiver), split by whether both x and y change: length = straight + diagonal * sqrt(2),
                                            the caller's arithmetic */
  uint32_t area_first, area_last;        /* area at the two end cells */
  double   height_first, height_last;    /* h of the two end cells, bits as stored */
} smx_segment;
/* *nstreams = the number of segments, whatever cap is; the first min(cap, *nstreams) records are written in rank order, record k at
 * byte k * struct_size; out may be NULL when cap is 0 (counting only). The planes (NULL = skip) hold dimx*dimy words in cell order:
 * order, reach and heads as defined above; segments -- the rank of the cell's segment, 0xFFFFFFFF off the channels. In the ensemble
 * call member i's records start at out + i * cap_per_member records and nstreams holds one count per member; an empty ensemble: 0,
 * nothing written. Both calls run on the context's / the ensemble's stream (they see every tick queued before them), launch the same
 * kernels whatever the map holds and however many members there are (one table upload; the drainage chain with the area on the
 * call's own scratch -- k_lake_tiles, k_lake_merge, k_lake_flatten, k_drain_recv, k_drain_resolve, k_drain_pending, k_drain_area --,
 * then k_stream_mark, k_stream_order, a prefix sum, k_stream_segments; the RESULTS copied back), synchronise once and change no map,
 * flag, counter or generator; the results and the scratch of smx_drainage and smx_lakes are not touched. No kernel waits for
 * another lane: k_stream_order takes at most as many turns per lane as the longest channel path has cells, k_stream_segments as
 * many as the segment has. A strip context, a null argument, struct_size == 0, threshold == 0 and records asked for with out == NULL
 * return -2, a context without a device -3. The scratch -- ten u32 planes per cell and the records asked for -- is allocated at
 * first use and kept; an allocation that fails returns < 0 and leaves the context / the ensemble usable. Maps of up to 65536 cells a
 * side and 2^32 - 2 cells per call. */
int smx_streams(smx_ctx* ctx, uint32_t threshold, smx_segment* out, uint64_t struct_size, uint32_t cap, uint32_t* nstreams,
                uint32_t* order, uint32_t* segments, uint32_t* reach, uint32_t* heads);
int smx_ensemble_streams(smx_ensemble* e, uint32_t threshold, smx_segment* out, uint64_t struct_size, uint32_t cap_per_member,
                         uint32_t* nstreams);
/* ---- spill analysis: where a lake or a pit overflows, into which basin, how much more it holds, how high water must rise before
 *      it leaves the map -- pour points, fill levels, storage and the filled surface ----
 * Cells, h(c), wet cells, lakes, basins, their identity first_cell and their rank are those of smx_drainage. Heights are ORDERED by
 * their ordered image K(v): the bits of v with the sign bit set where v is positive, all bits inverted where it is negative -- a total
 * order on bit patterns in which -0 is below +0 and a positive NaN above +inf. "max" and "min" of heights below mean "by K", and the
 * height of a pass is a copied double, never computed.
 * A PASS of basin a is a pair (c, n) with c in a and n an in-map cell among c's eight neighbours that lies in another basin; its height
 * is w = max(h(c), h(n)). Every cell c of a on the map border also has the off-map pass (c, 0xFFFFFFFF) with w = h(c): water leaves
 * the map there. Every basin has at least one pass. The POUR POINT of a basin is its pass with the smallest (K(w), c, n), compared
 * lexicographically -- so at an equal height and the same c an in-map neighbour beats the off-map pass.
 * The FILL LEVEL L(a) = min over the passes (c, n) of a of max(w, L(basin(n))), and w itself for an off-map pass: the minimax height
 * over basin-to-basin routes to the edge of the map. The value is unique, so any order of evaluation gives the same bits. A lake
 * counts as one pool: moving inside it costs nothing. filled(c) = max(h(c), L(basin(c))): where the map has no wet cell this is
 * exactly the priority-flood surface (the minimax over 8-connected cell paths to off-map), with wet cells it is never above it.
 * storage_q40 is the sum, over the basin's cells with K(h(c)) < K(pour_height), of floor((pour_height - h(c)) * 2^40) as u64 -- an
 * exact integer, as smx_lake.volume_q40 --, cells_below counts those cells, fill_storage_q40 is the same sum against fill_height. A
 * difference that is not finite, is negative or is >= 2^24 contributes 0 and sets the "unreliable" flag; a wrapped sum sets it too.
 * Every figure is a comparison, an exact integer or a copied double: a host restatement reproduces each bit. */
typedef struct smx_spill_record {        /* 64 bytes; record k belongs to basin k of smx_drainage on the same state */
  uint32_t first_cell;                   /* the basin's identity */
  uint32_t pour_cell, pour_to;           /* c and n of the pour point; pour_to 0xFFFFFFFF: off the map */
  uint32_t to_basin;                     /* first_cell of basin(pour_to), 0xFFFFFFFF off the map */
  uint32_t flags;                        /* 1 lake terminal  2 pours off the map  4 K(fill_height) > K(pour_height) (nested in a larger
                                            depression)  8 storage_q40 unreliable  16 fill_storage_q40 unreliable */
  uint32_t cells_below;
  double   pour_height, fill_height;
  uint64_t storage_q40, fill_storage_q40;
  uint32_t reserved[2];                  /* written as 0 */
} smx_spill_record;
/* *nbasins = the number of basins, whatever cap is; the first min(cap, *nbasins) records are written in rank order, record k at byte
 * k * struct_size (a caller passes sizeof(ITS struct) and gets that prefix of each record); out may be NULL when cap is 0 (counting
 * only). filled (NULL = skip): dimx*dimy doubles in cell order. In the ensemble call member i's records start at out + i *
 * cap_per_member records and nbasins holds one count per member; an empty ensemble: 0, nothing written. Both calls run on the
 * context's / the ensemble's stream (they see every tick queued before them) and change no map, flag, counter or generator; the
 * scratch and the results of smx_lakes, smx_drainage and smx_streams are not touched. The launches, each one for all members: the
 * drainage chain through k_drain_stats on the call's own scratch; k_spill_init, k_spill_pass twice (the key (K(w), c, n) is wider
 * than 64 bits: first the lowest K(w) per basin, then the lowest (c, n) among the passes that attain it), a prefix sum of the
 * boundary marks, k_spill_list, k_spill_point; k_spill_relax, ONE SWEEP per launch, each boundary cell lowering its basin's level in
 * place with fetch_min(max(w, L[basin(n)])); k_spill_store. No kernel waits for another lane or workgroup. THE NUMBER OF SWEEPS
 * DEPENDS ON THE MAP, so this call, unlike its siblings, SYNCHRONISES MORE THAN ONCE: once behind the drainage chain (the basins'
 * table is sized by the counts), then once per batch of 8 sweeps -- the host reads the sweeps' change counts and stops after the
 * batch that holds the first sweep that changed nothing --, once at the end. After more sweeps than the largest member has basins,
 * plus 2, the call gives up with -1 (that cannot happen). smx_get_spill_sweeps gives the sweeps launched and the batches of the
 * context's / the ensemble's last call. A strip context, a null argument, struct_size == 0 and records asked for with out == NULL
 * return -2, a context without a device -3. The scratch -- four u32 planes and one f64 plane per cell and 64 bytes per basin -- is
 * allocated at first use and kept; an allocation that fails returns < 0 and leaves the context / the ensemble usable. Maps of up to
 * 65536 cells a side and 2^32 - 2 cells per call. */
int smx_spill(smx_ctx* ctx, smx_spill_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, double* filled);
int smx_ensemble_spill(smx_ensemble* e, smx_spill_record* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins);
int smx_get_spill_sweeps(smx_ctx* ctx, uint32_t* sweeps, uint32_t* batches);
int smx_ensemble_get_spill_sweeps(smx_ensemble* e, uint32_t* sweeps, uint32_t* batches);
/* ---- through-drainage: when the pits and lakes are full, where does the water of a cell leave the map, and how much land drains
 *      through a point -- one cycle-free outflow per basin, the forest of basins, catchments and the through area ----
 * Cells, h(c), K, wet cells, basins, first_cell, the rank, the passes (c, n), w and the fill level L(a) are those of smx_drainage and
 * smx_spill. Following smx_spill_record.to_basin from basin to basin does NOT lead to the edge of the map: two basins that share their
 * lowest pass pour into each other. So:
 * A pass (c, n) of basin a is TIGHT when K(max(w, L(basin(n)))) == K(L(a)); the off-map pass is tight when K(w) == K(L(a)). Every
 * basin has one: the first pass of a minimax route is tight.
 * hops(a) = 1 if a has a tight off-map pass, otherwise 1 + the smallest hops(basin(n)) over its tight in-map passes. It is finite for
 * every basin: a tight step never raises (L, length of the shortest optimal route), and it lowers one of the two.
 * The EXIT of a is the tight pass with the smallest (c, n) among those whose target has hops(a) - 1; the off-map side counts as 0, so a
 * basin with hops == 1 exits off the map even where a tight in-map pass has a smaller (c, n). down(a) = basin(exit_to), or none. hops
 * strictly falls along down: the basins form a forest whose roots all exit off the map. The exit may differ from smx_spill's pour
 * point; flag 4 says so.
 * through_cells(a) = cells(a) + the sum of through_cells(u) over down(u) == a; upstream_basins(a) is the number of basins strictly
 * above a in the forest; outlet(a) is the root below a (a itself for a root), outlet_cell that root's exit_cell.
 * through_area(c) = 1 + the sum of through_area over the donors of c (the cells whose receiver is c) + the sum of through_cells(b)
 * over the basins b whose exit_to == c. Inside a basin the paths are smx_drainage's own; the filled part is a pool, so a basin's
 * total arrives at its terminal and re-appears at the entry cell of the next basin, a wet entry cell included. For every basin the
 * through_area over its sink or its wet cells sums to its through_cells; over the roots through_cells sums to dimx*dimy.
 * outlets(c) is the RANK of outlet(basin(c)). Every figure is a comparison, an exact u32 / u64 integer or a copied double. */
typedef struct smx_through_record {      /* 64 bytes; record k belongs to basin k of smx_drainage on the same state */
  uint32_t first_cell;                   /* the basin's identity */
  uint32_t exit_cell, exit_to;           /* c and n of the exit; exit_to 0xFFFFFFFF: off the map */
  uint32_t down;                         /* first_cell of basin(exit_to), 0xFFFFFFFF off the map */
  uint32_t outlet, outlet_cell;          /* first_cell of the root below the basin, and that root's exit_cell */
  uint32_t hops;                         /* exits on the way off the map, this basin's included: 1 for a root */
  uint32_t flags;                        /* 1 lake terminal  2 exits off the map  4 exit is not smx_spill's pour point  8 exit_to is a
                                            wet cell */
  uint32_t cells, through_cells, upstream_basins;
  uint32_t reserved;                     /* written as 0 */
  double   exit_height;                  /* w of the exit, copied */
  double   fill_height;                  /* L, as smx_spill_record.fill_height */
} smx_through_record;
/* *nbasins, out, struct_size, cap and the ensemble call's layout are smx_spill's. through_area, outlets (NULL = skip): dimx*dimy u32 in
 * cell order. Both calls run on the context's / the ensemble's stream (they see every tick queued before them) and change no map,
 * flag, counter or generator; the scratch and the results of smx_lakes, smx_drainage, smx_streams and smx_spill are not touched. The
 * launches, each one for all members: the drainage chain through k_drain_stats on the call's own scratch; smx_spill's k_spill_init,
 * k_spill_pass twice, the prefix sum, k_spill_list, k_spill_point and the k_spill_relax sweeps in batches of 8 (their boundary marks
 * in a plane of their own: the receivers stay); k_through_count (cells per basin); k_through_hops, ONE SWEEP per launch over the
 * boundary cells, fetch_min(hops[a], hops[basin(n)] + 1) per tight pass in place, in batches of 8 as the level sweeps; k_through_exit
 * (atomic min of (c << 32 | n) per basin); k_through_link twice (down, heights, flags, the pending counts; then the leaf marks);
 * k_through_accumulate, the never-waiting walk of k_drain_area over the basins, which also adds every finished basin's through_cells
 * to the area word of its exit_to; k_through_outlet; and where the planes are asked for k_drain_pending, k_through_plane and
 * k_through_area -- k_drain_area's walk, except that a leaf cell starts from its own word: an entry cell may have no donor. No
 * kernel waits for another lane or workgroup. The call SYNCHRONISES once behind the drainage chain, once per batch of level sweeps
 * and of hop sweeps, once at the end; after more sweeps of either kind than the largest member has basins, plus 2, it gives up with
 * -1 (that cannot happen). smx_get_through_sweeps gives the level sweeps, the hop sweeps and the batches (of both kinds together) of
 * the context's / the ensemble's last call. A strip context, a null argument, struct_size == 0 and records asked for with out ==
 * NULL return -2, a context without a device -3; an empty ensemble 0. The scratch -- five u32 planes and one f64 plane per cell
 * and 128 bytes per basin -- is allocated at first use and kept; an allocation that fails returns < 0 and leaves the context / the
 * ensemble usable. Maps of up to 65536 cells a side and 2^32 - 2 cells per call. */
int smx_through(smx_ctx* ctx, smx_through_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint32_t* through_area,
                uint32_t* outlets);
int smx_ensemble_through(smx_ensemble* e, smx_through_record* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins);
int smx_get_through_sweeps(smx_ctx* ctx, uint32_t* level_sweeps, uint32_t* hop_sweeps, uint32_t* batches);
int smx_ensemble_get_through_sweeps(smx_ensemble* e, uint32_t* level_sweeps, uint32_t* hop_sweeps, uint32_t* batches);
/* ---- hillslopes: where the land enters the channel network, how far it is from there, how high it stands above it (HAND), and one
 *      record per segment of the land that drains into it from the side ----
 * Cells, h(c), wet cells, receivers R and sinks are those of smx_drainage; channel cells, segments and their ranks are those of
 * smx_streams on the same state with the same threshold, a u32 >= 1. For a dry cell c follow c, R(c), R(R(c)), ...: its ENTRY e(c) is
 * the first cell on that path, c itself included, that is a channel cell, a sink or a wet cell. A wet cell has no entry.
 * straight(c) / diagonal(c) are the numbers of straight and diagonal steps from c to e(c): the flow length is straight + diagonal *
 * sqrt(2), as in smx_segment. hand(c) = h(c) - h(e(c)) is one f64 subtraction, the height above the nearest drainage: the cells with
 * hand < stage are the ones under water at that stage. hillslope(c) is the rank of the segment that e(c) lies on, 0xFFFFFFFF where
 * e(c) is no channel cell: that land is unchannelled, it drains into a pit or a lake directly. A wet cell gets entry = hillslope =
 * 0xFFFFFFFF, straight = diagonal = 0 and hand = +0.0; a channel cell, and a sink off the channels, is its own entry with 0 steps
 * and hand = +0.0. A path has at most min(threshold, cells) - 1 steps: every dry cell before the entry is off the channels, so its
 * area is below threshold, and the area is at least the number of cells upstream. Every figure of a record is an integer add or an
 * order-free extreme: a host restatement reproduces each bit, whatever the launch shape and the order of arrival. */
typedef struct smx_hillslope {            /* 64 bytes; record k belongs to segment k of smx_streams on the same state with the same threshold */
  uint32_t first_cell;                   /* the segment's identity: join on it with smx_segment */
  uint32_t cells;                        /* dry cells off the channels whose entry lies on the segment */
  uint32_t steps_max;                    /* the largest straight + diagonal among them */
  uint32_t farthest_cell;                /* the cell that has steps_max, the smallest cell index among equals; 0xFFFFFFFF when cells == 0 */
  uint64_t straight_sum, diagonal_sum;   /* exact sums over those cells */
  double   hand_max;                     /* the largest hand by the ordered image K of smx_spill; +0.0 when cells == 0 */
  uint64_t hand_sum_q40;                 /* the sum of floor(hand * 2^40) as u64, as smx_lake.volume_q40: a term that is not finite, is
                                            negative or is >= 2^24 contributes 0 and sets flag 1; a wrapped sum sets it too */
  uint32_t bank_cells;                   /* those with exactly one step */
  uint32_t head_cells;                   /* those whose entry is the segment's first_cell */
  uint32_t flags;                        /* 1: hand_sum_q40 unreliable */
  uint32_t reserved;                     /* written as 0 */
} smx_hillslope;
/* *nsegments = the number of segments, whatever cap is; the first min(cap, *nsegments) records are written in rank order, record k at
 * byte k * struct_size (a caller passes sizeof(ITS struct) and gets that prefix of each record); out may be NULL when cap is 0
 * (counting only). The planes (NULL = skip) hold dimx*dimy words -- hand: doubles -- in cell order, as defined above, entry as a cell
 * index. In the ensemble call member i's records start at out + i * cap_per_member records and nsegments holds one count per member;
 * an empty ensemble: 0, nothing written. Both calls run on the context's / the ensemble's stream (they see every tick queued before
 * them), launch the same kernels whatever the map holds and however many members there are (one table upload; the streams chain on
 * the call's own scratch with k_stream_segments writing its plane and no record; k_hill_init; k rounds of k_hill_jump, pointer
 * doubling between two sets of planes, k the smallest number with 2^k >= min(threshold, cells of the largest map) - 1, known before
 * the launch; k_hill_fold; the RESULTS copied back), synchronise once and change no map, flag, counter or generator; the results
 * and the scratch of the sibling analyses are not touched. No kernel waits for another lane or workgroup. A strip context, a null
 * argument, struct_size == 0, threshold == 0 and records asked for with out == NULL return -2, a context without a device -3. The
 * scratch -- ten u32 planes and one f64 plane per cell and the records asked for -- is allocated at first use and kept; an
 * allocation that fails returns < 0 and leaves the context / the ensemble usable. Maps of up to 65536 cells a side and 2^32 - 2 cells
 * per call. */
int smx_hillslopes(smx_ctx* ctx, uint32_t threshold, smx_hillslope* out, uint64_t struct_size, uint32_t cap, uint32_t* nsegments,
                   uint32_t* entry, uint32_t* hillslope, uint32_t* straight, uint32_t* diagonal, double* hand);
int smx_ensemble_hillslopes(smx_ensemble* e, uint32_t threshold, smx_hillslope* out, uint64_t struct_size, uint32_t cap_per_member,
                            uint32_t* nsegments);
/* ---- flow paths: how far every cell is from where its water ends up and how far it falls on the way, the longest path that arrives
 *      at every cell, and per basin the main stem with the ordered list of its cells, the long profile ----
 * Cells, h(c), wet cells, lakes, receivers R, sinks, basins, first_cell and the rank are those of smx_drainage, the ordered image K
 * that of smx_spill. The TERMINAL t(c) of a dry cell is the last cell of the path c, R(c), R(R(c)), ...: a sink (c itself where c is
 * a sink) or the first wet cell the path meets. A wet cell is its own terminal. straight(c) / diagonal(c) count the steps from c to
 * t(c), the step into a wet cell included, split as in smx_segment; steps = straight + diagonal. drop(c) = h(c) - h(t(c)) is one f64
 * subtraction, +0.0 where t(c) == c: a NaN cell, always a sink, has drop +0.0.
 * key(c) = (steps(c) << 32) | (0xFFFFFFFF - c). up(c) is the largest key(u) over the cells u whose path passes through c, c
 * included. upstream(c) = (up(c) >> 32) - steps(c) is the number of steps of the longest flow path that arrives at c,
 * source(c) = 0xFFFFFFFF - (u32)up(c) the cell it starts at: among equally long paths the smallest cell index.
 * For a basin b, far(b) is the largest key over its cells: it gives steps_max and source_cell. The MAIN STEM of b is the set of cells
 * with up(c) == far(b). Keys are unique, so it is exactly the path from source_cell to t(source_cell), steps_max + 1 cells; in a
 * lake's basin with several entry cells only one path qualifies. stem(c) = steps_max(b) - steps(c) on the stem, the position counted
 * from the source, and 0xFFFFFFFF off the stems. The PROFILE is the stems of all basins in rank order, each from source to terminal:
 * profile_at(b) is the sum of steps_max + 1 over the basins of lower rank, profile[profile_at(b) + stem(c)] = c, and nprofile, the
 * total, is at most the number of cells. A lake without dry land has a stem of one cell, its first_cell. Every figure is a
 * comparison, an exact integer, an order-free extreme or a copied / once-subtracted double: a host restatement reproduces each bit. */
typedef struct smx_flowpath {             /* 64 bytes; record k belongs to basin k of smx_drainage on the same state */
  uint32_t first_cell, cells;            /* the basin's identity and size */
  uint32_t source_cell, terminal_cell;   /* the two ends of the main stem */
  uint32_t steps_max, diagonal;          /* its steps, and how many of them are diagonal */
  uint32_t profile_at;                   /* index of source_cell in the profile (the ensemble call: within the member) */
  uint32_t flags;                        /* 1: terminal_cell is wet */
  uint64_t straight_sum, diagonal_sum;   /* exact sums of straight(c), diagonal(c) over the basin's cells */
  double   drop_source;                  /* drop(source_cell), the copied double */
  double   drop_max;                     /* the largest drop in the basin by K */
} smx_flowpath;
/* *nbasins = the number of basins, whatever cap is; the first min(cap, *nbasins) records are written in rank order, record k at byte
 * k * struct_size (a caller passes sizeof(ITS struct) and gets that prefix of each record); out may be NULL when cap is 0 (counting
 * only). The planes (NULL = skip) hold dimx*dimy words -- drop: doubles -- in cell order, terminal and source as cell indices.
 * *nprofile (NULL = skip) = the profile's length, whatever profile_cap is; the first min(profile_cap, *nprofile) entries of profile
 * are written, and profile may be NULL when profile_cap is 0. The profile and every plane cover ALL basins, whatever cap is: only
 * the records are cut at cap. In the ensemble call member i's records start at out + i * cap_per_member records, nbasins holds one
 * count per member and profile_at counts within the member; an empty ensemble: 0, nothing written. Both calls run on the context's /
 * the ensemble's stream (they see every tick queued before them), launch the same kernels whatever the map holds and however many
 * members there are (one table upload; the drainage chain with its statistics on the call's own scratch, writing no basin record;
 * k_drain_pending; k_path_init; k rounds of k_hill_jump, k the smallest number with 2^k >= cells of the largest map - 1, at most 32
 * and known before the launch; k_path_fold; k_path_up; k_path_lengths; a prefix sum; k_path_stem; the RESULTS copied back),
 * synchronise once and change no map, flag, counter or generator; the results and the scratch of the sibling analyses are not
 * touched. No kernel waits for another lane or workgroup. A strip context, a null argument, struct_size == 0, records asked for
 * with out == NULL and profile_cap > 0 with profile == NULL return -2, a context without a device -3. The scratch -- ten u32 planes
 * and one 64-bit plane per cell, the records asked for and min(profile_cap, cells) words -- is allocated at first use and kept; an
 * allocation that fails returns < 0 and leaves the context / the ensemble usable. Maps of up to 65536 cells a side and 2^32 - 2 cells
 * per call. */
int smx_flowpaths(smx_ctx* ctx, smx_flowpath* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins, uint32_t* terminal,
                  uint32_t* straight, uint32_t* diagonal, double* drop, uint32_t* upstream, uint32_t* source, uint32_t* stem,
                  uint32_t* profile, uint32_t profile_cap, uint32_t* nprofile);
int smx_ensemble_flowpaths(smx_ensemble* e, smx_flowpath* out, uint64_t struct_size, uint32_t cap_per_member, uint32_t* nbasins);
/* ---- catchments of listed outlets: which land drains through each cell of the caller's list (a gauge, a dam site, the last cell of
 *      a stream segment), one record per listed cell, the tree the gauges form along the flow, and per catchment a height
 *      distribution (hypsometry) ----
 * Cells, h(c), wet cells, receivers R, sinks, basins and their ranks are those of smx_drainage, the ordered image K that of
 * smx_spill. The GAUGES are the n >= 1 distinct cell indices x*dimy + y of the list; any cell may be one: dry, wet or a sink. The
 * ENTRY e(c) of a dry cell is the first cell on c, R(c), R(R(c)), ..., c included, that is a gauge, a sink or a wet cell; a wet cell
 * is its own entry. gauge(c) is the position of e(c) in the list, 0xFFFFFFFF where e(c) is no gauge. straight(c) / diagonal(c) count
 * the steps from c to e(c), split as in smx_segment; drop(c) = h(c) - h(e(c)) is one f64 subtraction, +0.0 where e(c) == c. These
 * three are defined for EVERY cell; where no gauge lies on a cell's path they are the straight, diagonal and drop of smx_flowpaths.
 * The OWN CATCHMENT of gauge i is the set of cells with gauge(c) == i, the gauge cell included. For a gauge cell g that is dry and
 * no sink, downstream(i) = gauge(R(g)), the next gauge down the flow; otherwise 0xFFFFFFFF. A path strictly descends, so the gauges
 * form a forest: the whole catchment of gauge i is its own plus those of the gauges above it, and area(i) is cells summed over them.
 * Hypsometry: a cell of own catchment i counts in bin b of row i, q = drop(c) / bin_height in one f64 division and
 * b = q < nbins ? (u32)q : nbins - 1, so that a NaN and an infinity land in the last bin. Every figure is an exact integer, an
 * order-free extreme or one f64 subtraction or division: a host restatement reproduces each bit. */
enum { SMX_CATCHMENT_MAX_BINS = 64 };
typedef struct smx_catchment {            /* 64 bytes; record i belongs to position i of the list */
  uint32_t cell;                         /* the gauge cell, cells[i] */
  uint32_t cells;                        /* the size of the own catchment, at least 1 */
  uint32_t area;                         /* cells summed over the gauge and every gauge above it; for a dry gauge the area plane of smx_drainage at the cell */
  uint32_t downstream;                   /* list position of the next gauge down the flow, 0xFFFFFFFF without one */
  uint32_t basin;                        /* the rank of the gauge cell's basin (the label plane of smx_drainage) */
  uint32_t steps_max;                    /* the largest straight + diagonal in the own catchment */
  uint32_t farthest_cell;                /* the cell that has it, the smallest cell index among equals; the gauge cell for a catchment of one cell */
  uint32_t flags;                        /* 1: drop_sum_q40 unreliable, 2: the gauge cell is wet, 4: the gauge cell is a sink */
  uint64_t straight_sum, diagonal_sum;   /* exact sums over the own catchment */
  double   drop_max;                     /* the largest drop in it by K */
  uint64_t drop_sum_q40;                 /* the sum of floor(drop * 2^40), as smx_hillslope.hand_sum_q40 */
} smx_catchment;
/* n records are written per map, record i at byte i * struct_size (a caller passes sizeof(ITS struct) and gets that prefix of each
 * record); there is no cap and no counting call. nbins (0 to 64) > 0: hist holds n * nbins u32 per map, row i for gauge i, and every
 * row sums to cells of its record; nbins == 0: hist and bin_height are not looked at and no histogram work is launched. The planes
 * (NULL = skip; smx_catchments only) hold dimx*dimy words in cell order: gauge, straight and diagonal u32, drop doubles. In the
 * ensemble call ONE list serves every member, as an index into each member's own plane; member i's records start at out + i * n
 * records and its table at hist + i * n * nbins; an empty ensemble: 0, nothing written. Refused with -2, the error text naming the
 * offending position, before anything is launched or written: cells NULL, n == 0, out NULL, a cell outside a member, a cell listed
 * twice, nbins > 64, nbins > 0 with hist NULL or with a bin_height that is not finite and positive, n * nbins >= 2^31; also a strip
 * context and struct_size == 0; a context without a device -3. Both calls run on the context's / the ensemble's stream (they see
 * every tick queued before them), launch the same kernels whatever the map holds and however many members there are (one upload of
 * the tables and the list; k_catch_mark; the drainage chain with its statistics and WITHOUT its area walk on the call's own scratch;
 * k_catch_init; k rounds of k_hill_jump, k the smallest number with 2^k >= cells of the largest map - 1, at most 32 and known before
 * the launch; k_catch_fold; with bins k_catch_hist; the RESULTS copied back), synchronise once and change no map, flag, counter or
 * generator; the results and the scratch of the sibling analyses are not touched. No kernel waits for another lane or workgroup.
 * area is folded on the host, children into parents, in O(n). The scratch -- ten u32 planes and one f64 plane per cell, n records
 * and n * nbins words per map and the list -- is allocated at first use and kept; an allocation that fails returns < 0 and leaves
 * the context / the ensemble usable. Maps of up to 65536 cells a side and 2^32 - 2 cells per call. */
int smx_catchments(smx_ctx* ctx, const uint32_t* cells, uint32_t n, smx_catchment* out, uint64_t struct_size, uint32_t* hist,
                   uint32_t nbins, double bin_height, uint32_t* gauge, uint32_t* straight, uint32_t* diagonal, double* drop);
int smx_ensemble_catchments(smx_ensemble* e, const uint32_t* cells, uint32_t n, smx_catchment* out, uint64_t struct_size,
                            uint32_t* hist, uint32_t nbins, double bin_height);
/* ---- horizons: what every cell sees when it looks UP along sixteen lattice directions -- the sky-view factor, cast shadows for a
 *      list of suns, the shelter from a wind (Winstral's Sx is the horizon slope of the upwind direction within a reach) ----
 * Cells, c = x*dimy + y and h(c) are those of smx_drainage: Layermap::height of the top record, so a lake's surface counts and an
 * empty column is 0.0; the ordered image K is that of smx_spill. The DIRECTIONS d = 0..15 run counter-clockwise from +x:
 *   (1,0) (2,1) (1,1) (1,2) (0,1) (-1,2) (-1,1) (-2,1) (-1,0) (-2,-1) (-1,-1) (-1,-2) (0,-1) (1,-2) (1,-1) (2,-1)
 * and len(d) is 1.0, the f64 nearest sqrt 2 (0x3FF6A09E667F3BCD) or the f64 nearest sqrt 5 (0x4001E3779B97F4A8). A caller selects
 * directions by a 16-bit mask; nd is its popcount, at least 1. The RAY of c = (x, y) in direction d is the cells c_k = (x + k ux,
 * y + k uy), k = 1, 2, ..., while c_k lies in the map and k <= reach (reach 0: no limit). No cell is interpolated: a knight's-move ray
 * visits only the lattice points on it. s_k = (h(c_k) - h(c)) / ((double)k * len(d)): one subtraction, one multiplication, one
 * division, nothing contracted. The HORIZON STEP K_d(c) is the smallest k with the largest s_k among those with s_k > +0.0, by plain
 * f64 > -- a NaN is never a horizon and a NaN cell has none --, 0 where no s_k > 0 exists; the HORIZON SLOPE S_d(c) is that s_k,
 * +0.0 where there is none. The planes (NULL = skip; smx_horizons only), in cell order:
 *   slope  f64, nd * cells: plane j belongs to the j-th selected direction in ascending d (indices are 64 bits wide)
 *   step   u32, the same layout, K
 *   sky    f64 per cell: the sum over the selected directions in ascending d, from 0.0, of 1.0 / (1.0 + S*S), then divided by
 *          (double)nd -- the sky-view factor of a cell whose horizon in every direction stands for an equal sector; 1.0 on open ground
 *   open   u32 per cell: bit d set where d is selected and K_d(c) == 0
 *   lit    u32 per cell: the number of suns that light the cell
 * A SUN has a lattice direction TOWARDS it, which has to be selected, and tangent = tan(elevation), finite and >= 0; it lights c
 * unless S_d(c) > tangent. lit_cells[i] is the number of cells sun i lights. Every figure is a comparison, an exact integer, an
 * order-free extreme or a fixed sequence of single f64 operations: a host restatement reproduces each bit. */
enum { SMX_HORIZON_DIRECTIONS = 16, SMX_HORIZON_MAX_SUNS = 64 };
typedef struct smx_sun {                  /* 16 bytes */
  uint32_t direction;                    /* the lattice direction towards the sun, 0..15, a bit of the mask */
  uint32_t reserved;
  double   tangent;                      /* tan(elevation), finite and >= 0 */
} smx_sun;
typedef struct smx_horizon_record {       /* 64 bytes; one per selected direction, in ascending d */
  uint32_t direction;                    /* d */
  int16_t  ux, uy;                       /* its lattice step */
  uint32_t bounded;                      /* the cells with K != 0: something stands above them in this direction */
  uint32_t step_max;                     /* the largest K */
  uint32_t step_max_cell;                /* the cell that has it, the smallest cell index among equals; 0xFFFFFFFF when bounded == 0 */
  uint32_t reserved0;                    /* 0 */
  uint64_t step_sum;                     /* the exact sum of K */
  double   slope_max;                    /* the largest S by K (the ordered image), +0.0 when bounded == 0 */
  uint32_t reserved[6];                  /* 0 */
} smx_horizon_record;
/* nd records are written per map, record j at byte j * struct_size (a caller passes sizeof(ITS struct) and gets that prefix of each
 * record); there is no cap and no counting call. suns: nsuns (0 to 64) of them, lit_cells: nsuns counts per map. In the ensemble
 * call ONE mask, reach and sun list serve every member; member i's records start at out + i * nd records and its counts at
 * lit_cells + i * nsuns; an empty ensemble: 0, nothing written. Refused with -2, the error text naming the offender, before anything
 * is launched or written: a null or a strip context, struct_size == 0, out NULL, a mask of 0 or with a bit above 15, nsuns > 64,
 * nsuns > 0 with suns or lit_cells NULL, a sun outside the mask or with a tangent that is not finite and >= 0, lit asked for with
 * nsuns == 0; a context without a device -3. Both calls run on the context's / the ensemble's stream (they see every tick queued
 * before them), launch the same kernels whatever the map holds and however many members there are (one upload of the tables and the
 * suns; k_horizon_heights: the f64 height plane and the maxima of its 8 x 8 and 64 x 64 tiles and of the map; k_horizon_scan, a
 * lane per cell and selected direction, which asks the map's, the coarse and the fine maximum before it loads a height and steps
 * past a tile that cannot hold the horizon -- the result is the plain walk's bit for bit --, and folds the records and the sun
 * counts; with sky, open or lit k_horizon_sky over the slopes and steps of all directions; the RESULTS copied back), synchronise
 * once and change no map, flag, counter or generator; the results and the scratch of the sibling analyses are not touched. No
 * kernel waits for another lane or workgroup; no launch strides, so smx_set_analysis_launch has no family for them. The scratch --
 * a double per cell and per tile; with a plane asked for also nd doubles and nd words per cell, a double for sky, a word each for
 * open and lit -- is allocated at first use and kept; an allocation that fails returns < 0 and leaves the context / the ensemble
 * usable. Maps of up to 65536 cells a side and 2^32 - 2 cells per call. */
int smx_horizons(smx_ctx* ctx, uint32_t directions, uint32_t reach, smx_horizon_record* out, uint64_t struct_size,
                 const smx_sun* suns, uint32_t nsuns, uint32_t* lit_cells,
                 double* slope, uint32_t* step, double* sky, uint32_t* open, uint32_t* lit);
int smx_ensemble_horizons(smx_ensemble* e, uint32_t directions, uint32_t reach, smx_horizon_record* out, uint64_t struct_size,
                          const smx_sun* suns, uint32_t nsuns, uint32_t* lit_cells);
/* ---- proximity: how far every cell is from water or from a listed cell as the crow flies (the exact Euclidean distance transform),
 *      which lake or listed cell is nearest (allocation zones), and how much of every zone lies how far out (buffers) ----
 * Cells, c = x*dimy + y, wet cells, lakes and lake ranks are those of smx_lakes. The SITES are a set of cells, each with a GROUP.
 * LIST mode (cells != NULL, n >= 1): the sites are the n distinct listed cells, the group of site cells[i] is i; any cell may be
 * listed, wet or dry. WATER mode (cells == NULL, n == 0): the sites are the wet cells and a site's group is the rank of its lake; a
 * map without a wet cell has no site and no record.
 * d2(c, s) = (xc - xs)^2 + (yc - ys)^2, an exact integer. nearest(c) is the site with the smallest (d2(c, s), s): the smaller squared
 * distance, then the smaller site cell index; a site is its own nearest. dist2(c) = d2(c, nearest(c)) and group(c) =
 * group(nearest(c)). Without any site all three are 0xFFFFFFFF for every cell. The ZONE of group g is the set of cells with
 * group(c) == g, sites included. Buffers: r(c) is the integer with r^2 <= dist2(c) < (r+1)^2, and a cell of zone g counts in bin
 * min(r / bin_width, nbins - 1) of row g, by integer division; every row sums to cells of its record. Every figure is an exact
 * integer or an order-free extreme: a host restatement reproduces each bit. No floating point enters but the f64 square root that
 * starts r, exact for an integer below 2^52 and corrected in integers. */
enum { SMX_PROXIMITY_MAX_BINS = 64, SMX_PROXIMITY_MAX_SIDE = 32768 };
typedef struct smx_proximity_record {     /* 64 bytes; record g belongs to group g */
  uint32_t site;                         /* LIST: cells[g]; WATER: the lake's first_cell */
  uint32_t sites;                        /* LIST: 1; WATER: the lake's cells */
  uint32_t cells;                        /* the size of the zone, at least sites */
  uint32_t dist2_max;                    /* the largest dist2 in the zone */
  uint32_t farthest_cell;                /* the cell that has it, the smallest cell index among equals */
  uint32_t flags;                        /* 1: the zone has a cell on the map border */
  uint64_t dist2_sum;                    /* the exact sum of dist2 over the zone */
  uint16_t x0, y0, x1, y1;               /* the zone's bounding box, inclusive */
  uint32_t reserved[6];                  /* 0 */
} smx_proximity_record;
/* Record g is written at byte g * struct_size (a caller passes sizeof(ITS struct) and gets that prefix of each record). LIST mode
 * writes n records per map: cap must be at least n, and *nrecords = n. WATER mode sets *nrecords to the number of lakes whatever cap
 * is and writes the first min(cap, *nrecords) records in rank order; out may be NULL with cap == 0 (the counting call). nbins (0 to
 * 64) > 0: hist row g holds nbins u32, for the records that are written; nbins == 0: hist and bin_width are not looked at and no
 * histogram work is launched. The planes nearest, group and dist2 (NULL = skip; smx_proximity only) hold dimx*dimy u32 in cell
 * order, for EVERY cell whatever cap is. In the ensemble call ONE list serves every member, as an index into each member's own
 * plane; member i's records start at out + i * cap_per_member records, its rows at hist + i * cap_per_member * nbins, and there is
 * one count per member; an empty ensemble: 0, nothing written. Refused with -2, the error text naming the offender, before anything
 * is launched or written: a null or a strip context, struct_size == 0, nrecords NULL, cells NULL with n != 0 or cells given with
 * n == 0, a cell outside a member, a cell listed twice, cap < n in LIST mode, records asked for (cap > 0) with out NULL, nbins > 64,
 * nbins > 0 with hist NULL or bin_width == 0, cap * nbins >= 2^31, a member with a side above 32768 (that keeps dist2 below 2^31 and
 * 0xFFFFFFFF free for "no site"); a context without a device -3. Both calls run on the context's / the ensemble's stream (they see
 * every tick queued before them), launch the same kernels whatever the map holds and however many members there are (one upload of
 * the tables and the list; WATER: the census's labelling and the rank scan; k_prox_mark; k_prox_columns, a workgroup per column;
 * k_prox_envelope, a lane per row and band of columns, the one serial pass, of dimx / bands steps; k_prox_query, a lane per cell,
 * which takes the nearest over the bands; with bins k_prox_hist; the
 * RESULTS copied back), synchronise once and change no map, flag, counter or generator; the results and the scratch of the sibling
 * analyses are not touched. No kernel waits for another lane or workgroup; no launch strides, so smx_set_analysis_launch has no
 * family for them. The scratch -- eight u32 planes per cell, the records, the rows and the list -- is allocated at first use and
 * kept; an allocation that fails returns < 0 and leaves the context / the ensemble usable. At most 2^32 - 2 cells per call. */
int smx_proximity(smx_ctx* ctx, const uint32_t* cells, uint32_t n, smx_proximity_record* out, uint64_t struct_size, uint32_t cap,
                  uint32_t* nrecords, uint32_t* hist, uint32_t nbins, uint32_t bin_width,
                  uint32_t* nearest, uint32_t* group, uint32_t* dist2);
int smx_ensemble_proximity(smx_ensemble* e, const uint32_t* cells, uint32_t n, smx_proximity_record* out, uint64_t struct_size,
                           uint32_t cap_per_member, uint32_t* nrecords, uint32_t* hist, uint32_t nbins, uint32_t bin_width);
/* ---- dispersed flow: the multiple-flow-direction (MFD) contributing area in fixed point, every cell's donors and receivers, and per
 *      basin what arrives at its terminal and what leaks over its divides ----
 * Cells, h(c), wet cells, lakes, the receiver R(c), sinks, basins, first_cell and the rank are those of smx_drainage.
 * ONE = 2^24. exponent is a u32 from 0 to 16.
 * The LOWER neighbours of a dry cell c are the in-map cells n among its eight neighbours with h(n) < h(c), plain f64 `<`: a NaN is
 * never lower and never has a lower neighbour. A dry cell with at least one lower neighbour is a GIVER; sinks and wet cells give
 * nothing; R(c) is always one of c's lower neighbours.
 * For a lower neighbour n of c: s = (h(c) - h(n)) * k, k = 1.0 for a straight step and 0x3FE6A09E667F3BCD (0.7071067811865476) for a
 * diagonal one; w(n) is the product of `exponent` factors s, multiplied left to right, starting from 1.0 (exponent 0: every lower
 * neighbour weighs 1.0); W is the f64 sum of the w(n) in ascending cell index, starting from 0.0; no operation is contracted.
 * If W > 0 and W is finite, f(n) = (u32)((w(n) / W) * 16777216.0), truncated; otherwise -- the products overflowed or all underflowed
 * -- every f(n) is 0. The f(n) sum to at most ONE.
 * A(c), a u64, is ONE plus what c is given. A giver c hands share(n) = (A(c) * f(n)) >> 24, the product 128 bits wide, to every lower
 * neighbour n, and the remainder A(c) - sum of the shares to R(c) on top of its share: nothing is lost, and with all f = 0 the cell
 * behaves exactly as in D8. A(c) is at most cells * ONE < 2^56.
 * donors(c) is the number of givers among c's neighbours that are higher than c (counted for a wet cell too); receivers(c) the number
 * of lower neighbours of a giver, 0 for a sink and for a wet cell.
 * Per basin b, in rank order: inflow_q24 is the sum of A over the basin's terminal cells (the sink, or every wet cell of the lake);
 * leak_out_q24 the sum of every amount, remainders included, that a giver labelled b hands to a cell of another basin; leak_in_q24
 * the same sum seen from the receiving basin; peak_q24 the largest A among the basin's dry cells and peak_cell the smallest cell that
 * holds it (a lake without dry land: 0 and 0xFFFFFFFF); givers counts the basin's givers, split_cells those with receivers(c) >= 2.
 * So inflow = cells * ONE + leak_in - leak_out for every basin, the inflows sum to dimx * dimy * ONE, and the leak_in sum to the
 * leak_out. Every figure is a comparison or an exact integer: a host restatement reproduces each bit. */
typedef struct smx_dispersal_record {    /* 64 bytes; record k belongs to basin k of smx_drainage on the same state */
  uint32_t first_cell, cells;            /* the basin's identity and D8 size */
  uint32_t flags;                        /* as smx_basin.flags */
  uint32_t peak_cell;
  uint64_t inflow_q24, leak_in_q24, leak_out_q24, peak_q24;
  uint32_t givers, split_cells;
  uint32_t reserved[2];                  /* written as 0 */
} smx_dispersal_record;
/* *nbasins = the number of basins, whatever cap is; the first min(cap, *nbasins) records are written in rank order, record k at byte
 * k * struct_size; out may be NULL when cap is 0 (counting only). The planes (NULL = skip) hold dimx*dimy words in cell order -- area:
 * u64, A(c); divide by 2^24 for cells -- and cover the whole map: only the records are cut at cap. In the ensemble call member i's
 * records start at out + i * cap_per_member records and nbasins holds one count per member; an empty ensemble: 0, nothing written.
 * Both calls run on the context's / the ensemble's stream (they see every tick queued before them): the drainage chain with its
 * statistics on the call's own scratch; k_disp_pending; k_disp_flow in rounds, one ready giver per lane, each lane carrying on with a
 * receiver its hand-over completed and listing the others for the next round -- the launches are queued in batches, after each batch
 * one word is read back (a bit per launch, whatever the member count), and the loop ends with the first launch that found its part of the list empty (smx_get_dispersal_rounds:
 * the launches that found work, and the batches, of the last call); k_disp_fold; k_disp_peak; the RESULTS copied back. No kernel
 * waits for another lane or workgroup; the result does not depend on the launch shape or on the order of arrival. The calls change
 * no map, flag, counter or generator and do not touch the results or the scratch of the sibling analyses. A strip context, a null
 * argument, struct_size == 0, exponent > 16 and records asked for with out == NULL return -2, a context without a device -3. The
 * scratch -- six u32 planes and one 64-bit plane per cell and two records per basin asked for -- is allocated at first use and
 * kept; an allocation that fails returns < 0 and leaves the context / the ensemble usable. Maps of up to 65536 cells a side and
 * 2^32 - 2 cells per call. */
int smx_dispersal(smx_ctx* ctx, uint32_t exponent, smx_dispersal_record* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins,
                  uint64_t* area, uint32_t* donors, uint32_t* receivers);
int smx_ensemble_dispersal(smx_ensemble* e, uint32_t exponent, smx_dispersal_record* out, uint64_t struct_size, uint32_t cap_per_member,
                           uint32_t* nbasins);
int smx_get_dispersal_rounds(smx_ctx* ctx, uint32_t* rounds, uint32_t* batches);
int smx_ensemble_get_dispersal_rounds(smx_ensemble* e, uint32_t* rounds, uint32_t* batches);
/* ---- the strata read on the device: how much of each soil there is, how thick a soil lies and how deep it is buried, and the
 *      columns under listed cells -- without exporting the map ----
 * A column is walked TOP -> BOTTOM, the inline top record first, then the prev links, one lane per column (k_strata_totals,
 * k_strata_thickness, k_core_count, k_core_scatter; bodies in soil_strata.h). Every link is validated as the fork validates it
 * (prev < pool_capacity, no more links than pool_capacity): a bad chain returns -5, the error text names the lowest bad cell (and,
 * in the ensemble call, the first member that has one) and nothing is written to the caller's outputs. Every call runs on the
 * context's / the ensemble's stream (it sees every tick queued before it), changes no map, flag, counter or generator, serves a
 * context of any engine and returns -2 for a strip context or a null argument. The totals calls synchronise once; the thickness and
 * cores calls wait once for the verdict (and the total) and once more for the results they then copy out. The scratch is allocated
 * at first use and kept; an allocation that fails returns < 0 and leaves the context / the ensemble usable.
 *
 * SOIL TOTALS. Record t describes the sections of type t, top sections included; every field is an integer, so no result depends
 * on the launch shape or on an order of summation. volume_q40 * 2^-40 lies below the exact sum of the sizes by less than
 * sections * 2^-40; a section smaller than 2^-40 contributes 0. Records 0..ntypes-1 (ntypes 1..64, else -2) are always written,
 * zeros where a type is absent; sections of a type >= ntypes are only counted, into *other_sections (NULL = skip). In the ensemble
 * call member i's records start at record i * ntypes and other_sections holds one count per member; one table upload and the same
 * launch whatever the member count; an empty ensemble: 0, nothing written. */
enum { SMX_TOTALS_MAX_TYPES = 64 };
typedef struct smx_soil_total {   /* 48 bytes; a caller passes sizeof(ITS struct) and gets that prefix of each record */
  uint64_t sections;              /* sections of this type, top sections included */
  uint64_t cells;                 /* columns that hold at least one section of this type */
  uint64_t top_cells;             /* columns whose TOP section is of this type (type 0: smx_member_figures.wet_cells) */
  uint64_t volume_q40;            /* sum over those sections of floor(size * 2^40): an exact integer */
  uint64_t held_q40;              /* sum of floor((size * sat) * 2^40), the product rounded once in f64: pore water before porosity */
  uint32_t flags;                 /* bit 0: volume unreliable, bit 1: held unreliable -- a term was not finite, was < 0 (-0 is 0) or
                                     was >= 2^24 (such a term contributes 0), or the 64-bit sum wrapped */
  uint32_t reserved;              /* written as 0 */
} smx_soil_total;
int smx_soil_totals(smx_ctx* ctx, smx_soil_total* out, uint64_t struct_size, uint32_t ntypes, uint64_t* other_sections);
int smx_ensemble_soil_totals(smx_ensemble* e, smx_soil_total* out, uint64_t struct_size, uint32_t ntypes, uint64_t* other_sections);
/* THICKNESS PLANES. Each output may be NULL; each holds ntypes planes in cell order x*dimy+y, type-major ([k*ncells + c]). All three
 * come from ONE walk of the column with f64 accumulation in walk order (top -> bottom) and no contraction, so a host loop over the
 * exported column, reversed, gives the same bits:
 *   thickness   the sum of the sizes of the sections of type types[k], starting from +0.0
 *   cover       the sum of the sizes of ALL sections above the highest section of types[k] (the running sum before that section is
 *               added); -1.0 where the column has none
 *   sections    how many sections of that type the column holds
 * A repeated type or an ntypes outside 1..8 returns -2. */
int smx_soil_thickness(smx_ctx* ctx, const uint32_t* types, int32_t ntypes /* 1..8 */, double* thickness, double* cover, uint32_t* sections);
/* CORES. The columns of the n listed cells (indices x*dimy+y; repeats allowed) in the snapshot layout: columns in list order, sections
 * bottom -> top, count[i] sections for cells[i], the bits exactly those the column export holds for those cells. *total = the number
 * of sections the list holds; where it exceeds cap (the room of each section array), count and *total are written, the section
 * arrays are left untouched and the call returns 1. A cell index >= dimx*dimy returns -2 and the text names it; n == 0 returns 0.
 * Count, scan and scatter run on the device, as the fork's do; only the listed columns come back. */
int smx_cores(smx_ctx* ctx, const uint32_t* cells, uint32_t n, uint32_t* count, uint64_t cap, uint64_t* total,
              uint32_t* type, double* size, double* floor, double* sat);
/* ---- the sediment budget: what a run did to the land -- cut, fill and soil change from a BASE map to the map of NOW, per drainage
 *      basin of the base, per soil type and per cell, without exporting either map ----
 * "now" is the calling context's map (or an ensemble member's), "base" another context of the same dimensions on the same device,
 * typically the copy kept before the run with the copy-state call or the source of an ensemble fork. Cells, h(c), wet cells, lakes and
 * basins are those of the drainage call; the strata are read as the soil totals read them.
 * Per map and cell: ground(c) is 0.0 for an empty column, the top section's floor where the top section is Air (type 0), else its
 * floor + size in one f64 addition -- only the top record is read. V_t(c) is the sum over ALL sections of type t in the column, the
 * top one included, of floor(size * 2^40); a term that is not finite, is negative (-0 is 0) or is >= 2^24 contributes 0 and raises
 * flag bit 0. H_t(c) is the same on size * sat, the product rounded once. S(c) is the sum of V_t(c) over every t != 0, types >= ntypes
 * included; W(c) = V_0(c). These sums are taken modulo 2^64 and a wrap raises flag bit 1; "x is positive" below means x_now > x_base
 * as u64.
 * Per cell, now against base: dground = ground_now - ground_base and dheight = h_now - h_base, one f64 subtraction each; dsolid =
 * (int64)(S_now - S_base); dwater = (int64)(W_now - W_base). A cell is LOWERED where ground_now < ground_base and RAISED where >,
 * plain f64 comparisons; where either ground is a NaN the cell is neither and raises flag bit 2 of its basin. A cell is RESURFACED
 * where the top types differ, an empty column counting as a type of its own.
 * BASINS. One record per basin of the BASE's drainage, in rank order; first_cell and cells are the drainage record's: the join key. */
typedef struct smx_budget_basin {   /* 96 bytes; a caller passes sizeof(ITS struct) and gets that prefix of each record */
  uint32_t first_cell, cells;
  uint32_t lowered_cells, raised_cells, resurfaced_cells;
  uint32_t flags;                   /* bit 0: a volume term of a cell of the basin was unreliable (it contributed 0), bit 1: a 64-bit sum
                                       wrapped (S or W of a cell, or a sum below), bit 2: a NaN ground */
  uint64_t eroded_q40;              /* the sum over the basin's cells of S_base - S_now where that is positive */
  uint64_t deposited_q40;           /* ... of S_now - S_base where that is positive: net = deposited - eroded, the sediment yield is -net */
  uint64_t water_gained_q40;        /* ... of W_now - W_base where that is positive */
  uint64_t water_lost_q40;          /* ... of W_base - W_now where that is positive */
  double cut_max, fill_max;         /* the largest -dground over the lowered cells, the largest dground over the raised ones; +0.0: none */
  uint32_t cut_cell, fill_cell;     /* the smallest cell that attains it; 0xFFFFFFFF: none */
  uint32_t reserved[4];             /* written as 0 */
} smx_budget_basin;
/* SOILS. Record t covers the sections of type t < ntypes (1..64, as for the soil totals) over the whole map, whatever cap is; sections of a
 * type >= ntypes count in S alone. */
typedef struct smx_budget_soil {    /* 64 bytes; the caller passes soil_struct_size likewise */
  uint64_t gained_q40, lost_q40;            /* the sums over the cells of V_t,now - V_t,base where positive, of V_t,base - V_t,now where positive */
  uint64_t held_gained_q40, held_lost_q40;  /* the same on H_t */
  uint32_t cells_gained, cells_lost;        /* the cells with V_t,now > V_t,base, with V_t,now < V_t,base */
  uint32_t surfaced, covered;               /* cells whose top is t now and was not in base; whose top was t in base and is not now */
  uint32_t flags;                           /* bit 0: a term of this type (volume or held) was unreliable, bit 1: a sum of this type wrapped */
  uint32_t reserved[3];                     /* written as 0 */
} smx_budget_soil;
/* *nbasins = the number of the base's basins, whatever cap is; the first min(cap, *nbasins) records are written in rank order; out may
 * be NULL when cap is 0 (counting only). soils (NULL = skip) takes ntypes records. The planes (NULL = skip; the context call only) hold
 * dimx*dimy values in cell order: dground and dheight f64, dsolid and dwater i64; they cover the whole map. The ensemble call compares
 * every member with the ONE base: member i's basin records start at out + i * cap_per_member records, its soil records at record
 * i * ntypes, *nbasins is the single count of the base; the members are folded by the same launches; an empty ensemble: 0, nothing
 * written.
 * Both calls run on the context's / the ensemble's stream, behind the work queued on the base's stream (an event, as for the state
 * copy): the drainage chain with its statistics ONCE, on the base, on the call's own scratch; k_budget_fold, one lane per cell walking
 * both columns at once; k_budget_where; the results copied back, one synchronisation (the context call waits once more for the planes
 * it then copies out). Every link of both maps is validated as the soil totals validate it: a bad chain returns -5, the text names
 * the map and its lowest bad cell, and nothing is written to the caller. Only integers are added, every add detects a wrap, and the
 * extremes are order-free: no result depends on the launch shape, and a plain loop over two exported maps reproduces each bit. The
 * calls change no map, flag, counter or generator. -2: a null argument, base being the context or a member compared, unequal
 * dimensions, another device, a strip context, struct_size == 0, records asked for with out == NULL, and with soils given
 * soil_struct_size == 0 or ntypes outside 1..64; -3: no device. The scratch -- three u32 planes per cell, a 64-bit plane per plane
 * asked for, a record per basin asked for and member -- is allocated at first use and kept; an allocation that fails returns < 0 and
 * leaves the context / the ensemble usable. */
int smx_budget(smx_ctx* ctx, smx_ctx* base, smx_budget_basin* out, uint64_t struct_size, uint32_t cap, uint32_t* nbasins,
               smx_budget_soil* soils, uint64_t soil_struct_size, uint32_t ntypes,
               double* dground, double* dheight, int64_t* dsolid, int64_t* dwater);
int smx_ensemble_budget(smx_ensemble* e, smx_ctx* base, smx_budget_basin* out, uint64_t struct_size, uint32_t cap_per_member,
                        uint32_t* nbasins, smx_budget_soil* soils, uint64_t soil_struct_size, uint32_t ntypes);

/* ---- point operations for API fidelity (Layermap::add/remove, Particle::cascade, ... called by host code) ---- */
int smx_add(smx_ctx* ctx, int32_t x, int32_t y, double size, uint32_t type);            /* layermap.h:230 */
int smx_remove(smx_ctx* ctx, int32_t x, int32_t y, double h, double* remainder);        /* layermap.h:310 */
int smx_particle_cascade(smx_ctx* ctx, float px, float py, int32_t transferloop);       /* particle.h:24  */
int smx_water_cascade(smx_ctx* ctx, int32_t x, int32_t y, int32_t spill);               /* water.h:151    */
int smx_seep(smx_ctx* ctx, int32_t x, int32_t y);                                       /* water.h:285    */
int smx_top(smx_ctx* ctx, int32_t x, int32_t y, uint32_t* type, double* size, double* floor, double* sat,
            int32_t* empty);                                                            /* Layermap::top layermap.h:150 (a copy) */
int smx_normals(smx_ctx* ctx, float* out3);             /* Layermap::normal(ivec2) for every cell, xyz interleaved (layermap.h:341) */
/* Layermap::update(Vertexpool&) (layermap.h:551-555 -> :475-549, no SLICE cut): the visible vertex of every column in
 * one pass -- 44-byte records {position[3], normal[3], color[4], index} (source/include/vertexpool.h:9-28) in cell
 * order x*dimy+y: position = (x, SCALE*height, y), normal = Layermap::normal(ivec2), color = colors4[type], index =
 * type; an empty column is (x, 0, y), (0,1,0), colors4[0], 0. colors4 = ncolors x RGBA (SurfParam::color,
 * surface.h:17); out = dimx*dimy*44 bytes, caller-allocated. */
int smx_fill_vertices(smx_ctx* ctx, const float* colors4, int32_t ncolors, void* out_vertices44);
/* the same with a horizontal cut through the sediment: mode 0 = Layermap::update's rule with the global SLICE = (int)cut
 * (layermap.h:477-510: first section starting at or below SLICE/SCALE; a section reaching above it is drawn flat at y = SLICE,
 * blended with Air's colour where its water table reaches the cut), mode 1 = Layermap::slice(s = cut) (layermap.h:557-613). */
int smx_fill_vertices_cut(smx_ctx* ctx, const float* colors4, int32_t ncolors, int32_t mode, double cut, void* out_vertices44);
/* ONE column's vertex under the same rules (mode < 0: no cut) -- Layermap::update(ivec2, Vertexpool&) (layermap.h:475-549) for a
 * host-driven single edit; out = 44 bytes. */
int smx_fill_vertex_cut(smx_ctx* ctx, const float* colors4, int32_t ncolors, int32_t mode, double cut, int32_t x, int32_t y, void* out_vertex44);
int smx_heights_bilinear(smx_ctx* ctx, const float* pos2, int32_t n, double* out);      /* Layermap::height(vec2) (layermap.h:427) */
/* (reads the four cells (px..px+1, py..py+1) as the reference does: every position must lie in [0, dimx-1) x [0, dimy-1), else -2 and nothing is read) */

/* ---- observability ---- */
/* The state digest of SURVEY.md Appendix E, computed from a device->host copy: sum of Layermap::height(ivec2) over the
 * cells in x-outer / y-inner order (sequential double accumulation), number of sections, and the 64-bit hash
 * h = (h ^ type) * 1099511628211 (start 1469598103934665603) over every column walked top -> bottom, same cell order. */
int smx_digest(smx_ctx* ctx, double* sumh, uint64_t* nsec, uint64_t* typehash);
/* The sized getters write min(struct_size, sizeof) bytes: pass sizeof(smx_counters) / sizeof(smx_timing) of the header you compiled
 * against. The unsized ones keep the layouts they were introduced with (smx_counters: the first 16 words, i.e. without
 * spec_subphases_cut / spec_serial_particles; smx_timing: the first 144 bytes) so that older binaries are never written past their
 * struct -- an ABI note for callers of rounds 1-4: INTEGRATION.md "ABI notes". */
/* The run-time switches (environment variables SMX_*, read once per process; README.md "Run-time switches") as text, one line per
 * switch: "NAME=value default class\n" -- the value this process read (the default where the variable is not set; "-" = not set and no
 * default), the default, and the class: neutral (selects code or a launch shape, results bit-identical), changes_results (part of a
 * schedule's definition) or diagnostic (tracing, profiling, poll pacing, the spin budget). Read-only; needs no context and no device.
 * Writes a NUL-terminated string of *needed bytes (needed may be NULL); -2 and nothing written where cap is smaller (or buf NULL). */
int smx_switches(char* buf, uint64_t cap, uint64_t* needed);
int smx_get_counters_sized(smx_ctx* ctx, smx_counters* out, uint64_t struct_size);
int smx_get_timing_sized(smx_ctx* ctx, smx_timing* out, uint64_t struct_size);
int smx_get_counters(smx_ctx* ctx, smx_counters* out);
int smx_get_timing(smx_ctx* ctx, smx_timing* out);
int smx_timing_reset(smx_ctx* ctx);
int smx_set_engine(smx_ctx* ctx, int32_t engine);
/* speculative engine (round 4): a particle phase runs in sub-phases of at most `particles_per_subphase` top-level particles, each owning
 * `nested_slots` rand() slots for the nested particles its floods spawn (water.h:246-264); a sub-phase whose slots are used up commits
 * and is re-armed from the continued stream. 0 = defaults (4096 / 8192). Results never depend on the values. */
int smx_set_spec_limits(smx_ctx* ctx, uint32_t particles_per_subphase, uint32_t nested_slots);
/* batched engine only: widen every reservation by `tiles` 4x4-cell tiles (0 = default; >= the map's tile count makes
 * the engine run the particles strictly one after the other, i.e. in the reference's order) */
int smx_set_batch_dilate(smx_ctx* ctx, int32_t tiles);
/* relaxed schedule (SMX_ENGINE_RELAXED), wind phase: relaxed epochs -- every running particle takes up to `steps_per_epoch` (1..8)
 * steps on the epoch's start state -- while more than `min_running` particles run; the survivors, a few thousand particles that fly
 * on for up to ~13 000 steps, go on under the exclusive schedule (32 steps per launch). Part of the schedule's definition: results
 * depend on it. Default: min_running = 0xFFFFFFFF, i.e. wind always runs the exclusive schedule (measured faster, profiles/r03_relaxed.md);
 * 4 steps per epoch. */
int smx_set_relax_wind(smx_ctx* ctx, uint32_t min_running, int32_t steps_per_epoch);
/* relaxed schedule, water phase: the LAUNCH SHAPE of its epochs -- never the result (tests/test_gpu_relaxed.py runs every shape against the
 * same host-thread states). persistent: 0 = five launches per epoch (step, apply, filter, colour lists, floods: the default), 1 = the dense
 * epochs of a chunk as one cooperative launch with device-wide barriers (k_relax_epochs, round 6: measured 15-45 % slower on the headline,
 * profiles/r06_persistent_epochs.md); tail_at: from this many running particles down one workgroup runs whole epochs back to back
 * (k_relax_tail; 0..256, default 256). -1 = leave as is / back to the default. */
int smx_set_relax_launch(smx_ctx* ctx, int32_t persistent, int32_t tail_at);
/* relaxed schedule, dense epochs (water, and relaxed wind): the LAUNCH SHAPE of what follows apply -- never the result (tests/test_gpu_relaxed_settle.py).
 * mode: 1 = ONE dataflow launch (k_relax_settle: classify every flagged cell, cascade the isolated ones at once and the crowded ones in colour order
 * behind per-cell waits) in every epoch whose worst-case grid is resident on the device all at once, 0 = two launches (k_relax_filter, then the colour
 * lists through k_relax_cascade_flow), 2 = as 1, and in water epochs the floods join that launch (k_relax_settle_floods: a flood that will act waits only
 * for the flagged cells within one cell of the tiles it holds) where settle and flood wavefronts are resident together, else mode 1's two launches
 * (k_relax_settle, k_relax_floods); -1 = the default. Contexts under column strips and processes with SMX_RELAX_CASC_FLOW=0 always take the two
 * launches. max_waves > 0 caps the resident wavefronts the fused launch may count on (a small value forces the two-launch path: the fall-back, testable on
 * a small map); lanes = flagged cells per wavefront of k_relax_settle / k_relax_filter, 1..64 (0 = the rule in relax_settle_lanes). */
int smx_set_relax_settle(smx_ctx* ctx, int32_t mode, int32_t max_waves, int32_t lanes);
/* ... and what the context did so far: cells that went through the waiting (crowded) path of k_relax_settle, dense epochs that took the fused launch,
 * dense epochs that took the two launches. Synchronises the context's stream. Any pointer may be null. */
int smx_get_relax_settle(smx_ctx* ctx, uint64_t* crowded_cells, uint64_t* epochs_fused, uint64_t* epochs_split);
/* ... and of the fused epochs, the mode-2 part: water epochs that took k_relax_settle_floods (they count under epochs_fused too), floods that acted in
 * them, and those of them that found at least one cell flagged in the epoch in their tiles' rectangle widened by one cell -- a function of the input,
 * not of timing (whether the flood had to spin is not counted). Synchronises the context's stream. Any pointer may be null. */
int smx_get_relax_flood_flow(smx_ctx* ctx, uint64_t* epochs_joined, uint64_t* floods_acted, uint64_t* floods_gated);
/* the terrain analyses and the strata readers: the LAUNCH SHAPE of their three families of strided launches -- never the result
 * (tests/test_gpu_analysis_launch.py runs small maps through the second and later iterations of every stride). Each value is the most
 * workgroups (grid.x) of the family's launches; the workgroups stride over the rest of the work:
 *   flow_blocks    k_disp_flow (smx_dispersal), default 1024: strides once a round's part of the ready list exceeds flow_blocks * 256 givers
 *   relax_blocks   k_spill_relax, k_through_hops, k_through_exit (smx_spill, smx_through), default 2048: strides once a map has more than
 *                  relax_blocks * 256 boundary cells
 *   strata_blocks  k_strata_totals, k_strata_thickness, k_core_count, k_core_scatter (smx_soil_totals, smx_soil_thickness, smx_cores),
 *                  default 8192: strides above strata_blocks * 64 columns or listed cells; smx_ensemble_soil_totals gives every member
 *                  strata_blocks / members workgroups (at least one)
 * 0 = the default; 1 .. the default = that many. Anything else: -2, a text in smx_last_error, nothing changed. The values belong to the
 * owner of the call's scratch: a context's hold for the calls on that context, an ensemble's for the smx_ensemble_* calls, and neither
 * reaches the other. Records, their order, the counts, every plane and the batches of smx_get_*_sweeps / smx_get_dispersal_rounds are
 * bit-identical for every value; the number of relax and hop sweeps and of dispersal rounds may differ (a sweep works in place, a walk
 * carries on into the next round's cells). */
int smx_set_analysis_launch(smx_ctx* ctx, int32_t flow_blocks, int32_t relax_blocks, int32_t strata_blocks);
int smx_ensemble_set_analysis_launch(smx_ensemble* ens, int32_t flow_blocks, int32_t relax_blocks, int32_t strata_blocks);
/* ... and what is in force: blocks[3] = the three values (a default as its number), last_grid[3] = the grid.x that the last call on this
 * owner gave the launches of each family (0: none yet). Needs no device work. Either pointer may be null. */
int smx_get_analysis_launch(smx_ctx* ctx, int32_t* blocks, uint32_t* last_grid);
int smx_ensemble_get_analysis_launch(smx_ensemble* ens, int32_t* blocks, uint32_t* last_grid);
/* REMOVED in round 5 (nested particles run inside their parent since then; there is nothing to interleave): kept as a symbol that fails
 * loudly (-2, smx_last_error says so) so that a round-4 caller neither crashes at load time nor silently runs another schedule. */
int smx_set_grid_interleave(smx_ctx* ctx, int32_t k);
/* throughput engines: smx_tick_water(n) (and smx_strips_tick) run the n particles as k consecutive top-level generations of n/k. DEFAULT 8
 * since round 6 (round 5: 4; rounds 3-4: 1). The particles of one generation advance together and do not see the lakes their own generation
 * makes; in the reference particle i sees what particles < i of the same tick did (SoilMachine.cpp:287-298), and every wet cell stops the
 * particles that reach it (water.h:56 with soils["Air"].friction = 0). k generations give a particle (k-1)/k of that view for k epoch chains.
 * At the headline workload, against 33 rand() streams of the reference itself (profiles/r06_p2_reference_4096.json): k = 1 is outside by up
 * to 7.9 sigma, k = 4 outside on three of eight figures (2.3-3.0 sigma), k = 8 inside |z| < 2 on all eight. Callers of round 5 see a
 * behaviour and a cost change (the water phase ~1.3 x) unless they call smx_set_water_generations(4). Identical to k calls of n/k with k = 1. */
int smx_set_water_generations(smx_ctx* ctx, int32_t k);
int smx_get_water_generations(smx_ctx* ctx, int32_t* k);   /* the value in force (bench.py reports it instead of a literal) */
/* relaxed engine: STAGGERED generations. gap_epochs > 0: a water phase of n particles is ONE phase whose k batches of ceil(n / k) particles (by slot) are
 * born gap_epochs apart -- batch b takes its first step in epoch b * gap --; 0: k consecutive generations, each run to its end. A particle of batch b
 * finds what the batches before it did in the epochs they are ahead (the lakes their stopped particles made); the tick's epoch chain is (k - 1) * gap + one
 * generation long instead of k generations. Part of the schedule's definition (results depend on it); default 0 (SMX_WATER_STAGGER in csrc/soil_batch.h).
 * Measured against the same 33 reference streams (profiles/r06_alt1_stagger_sweep_..., r06_alt2_stagger_ensembles_p2_reference_4096.json): k = 16, gap = 140 takes
 * 30 % off the water phase (64 M instead of 50 M particle-steps/s at the headline) and passes the parity gate with SEED 0's stream and under two strips, but two
 * of three further device streams fail it and neighbouring (k, gap) points do too: a measured step away from the reference, hence an option. */
int smx_set_water_stagger(smx_ctx* ctx, int32_t gap_epochs);
int smx_get_water_stagger(smx_ctx* ctx, int32_t* gap_epochs);
/* batched engine: column strips (DESIGN.md "Multi-GPU"). The schedule alternates INTERIOR chunks (a particle acts iff its
 * reservation lies `inset` cells inside one of `nstrips` equal x-strips) and SEAM chunks (iff inside one seam zone of
 * +-seam_halfwidth cells around a strip boundary). nstrips == 1 (default) = the single-strip schedule. The result is a
 * function of (nstrips, inset, seam_halfwidth) only -- not of how many devices run the strips. */
int smx_set_batch_strips(smx_ctx* ctx, int32_t nstrips, int32_t inset, int32_t seam_halfwidth);
/* ---- column strips on SEVERAL devices, step by step (library driver: smx_strips_*; its Python restatement over these entry points: tests/strips_ref.py; one context per strip, each with
 * the full-size map of which it keeps its strip + right halo current). A generation of a particle phase:
 *   smx_d_gen_begin   draws the generation's rand() values (identical on every rank) and, for nested particles
 *                     (`children` = BChild records: u64 key, i32 tx,ty,bx,by,spill,pad, f64 volume), answers what this rank
 *                     knows about each child's `contains` (0xFFFFFFFF = random cell not in my strip; ranks combine by min)
 *   smx_d_gen_spawn   constructs the particles; those outside [own_x0, own_x1) live on another rank
 *   smx_d_chunk       32 epochs; the schedule follows the GLOBAL number of running particles; chunks alternate INTERIOR /
 *                     SEAM (smx_d_next_phase tells which comes next: 0 interior, 1 seam)
 *   smx_d_gen_end     counters + this rank's newly spawned children
 * smx_d_pack_columns / _particles serialise the changed halo columns (dirty 4x4 tiles with x in [x0,x1)) and the running
 * particles with ipos.x in [x0,x1) (they leave this rank) into a caller-provided host buffer; _unpack_ applies them. */
int smx_d_set_own(smx_ctx* ctx, int32_t own_x0, int32_t own_x1);
int smx_d_gen_begin(smx_ctx* ctx, int32_t wind, uint32_t nslots, const void* children, uint32_t* contains_out);
int smx_d_gen_spawn(smx_ctx* ctx, const uint32_t* contains, uint32_t* nlive_local);
int smx_d_next_phase(smx_ctx* ctx);
int smx_d_chunk(smx_ctx* ctx, uint32_t nlive_global, uint32_t* nlive_local);
int smx_d_gen_end(smx_ctx* ctx, void* children_out, uint32_t cap, uint32_t* n);
int smx_d_pack_columns(smx_ctx* ctx, int32_t x0, int32_t x1, void* buf, uint64_t cap, uint64_t* bytes);
int smx_d_unpack_columns(smx_ctx* ctx, const void* buf, uint64_t bytes);
int smx_d_pack_particles(smx_ctx* ctx, int32_t x0, int32_t x1, void* buf, uint64_t cap, uint64_t* bytes);
int smx_d_unpack_particles(smx_ctx* ctx, const void* buf, uint64_t bytes);
int smx_d_grid_begin(smx_ctx* ctx);                                            /* classification of the grid pass       */
/* (rounds 2-4 exported `smx_d_grid_sweep` over 4x4-TILE indices; the arguments are CELL columns since round 5, so the
 *  entry point carries a new name: a caller of the old one fails to link instead of sweeping the wrong range) */
int smx_d_grid_sweep_cols(smx_ctx* ctx, int32_t phase, int32_t x_lo, int32_t x_hi);   /* the grid tiles of the COLUMNS [x_lo, x_hi) that belong to `phase`, colour by colour */
/* ---- column strips driven INSIDE the library (csrc/soil_strips_host.h): the tick of SoilMachine.cpp:283-329 on this rank's strip of ONE
 * map; halo columns and migrating particles go from the pack kernel to the unpack kernel of the neighbour without leaving device memory.
 *   smx_strips_attach_rccl   transport = RCCL (ncclSend / ncclRecv / ncclAllReduce / ncclAllGather over xGMI) on this context's stream;
 *                            rank 0 makes the 128-byte id with smx_strips_rccl_unique_id and hands it to the other ranks (any side channel)
 *   smx_strips_attach        transport = the caller's callbacks on HOST buffers (loop-back threads, gloo, MPI ...; all calls block; send must
 *                            not wait for the matching recv to be posted... recv returns 0 and *bytes, or 1 and the needed *bytes if cap is short)
 *   smx_strips_tick          every rank calls it with the same arguments; requires the batched engine
 * The result is a function of (world, inset, seam_halfwidth) only -- smx_set_batch_strips runs the same schedule in ONE context. */
typedef struct smx_transport {
  void* user;
  int (*send)(void* user, int32_t dst, const void* buf, uint64_t bytes);
  int (*recv)(void* user, int32_t src, void* buf, uint64_t cap, uint64_t* bytes);
  int (*allreduce_sum_u64)(void* user, uint64_t* v);
  int (*allreduce_max_u64)(void* user, uint64_t* v);
  int (*allreduce_min_u32)(void* user, uint32_t* a, uint64_t n);
  /* every rank contributes `bytes` (<= each) bytes; all = world blocks of `each` bytes in rank order, sizes[r] = rank r's bytes */
  int (*allgather)(void* user, const void* mine, uint64_t bytes, void* all, uint64_t each, uint64_t* sizes);
} smx_transport;
int smx_strips_rccl_unique_id(void* out128);
int smx_strips_attach_rccl(smx_ctx* ctx, const void* unique_id128, int32_t rank, int32_t world, int32_t inset, int32_t seam_halfwidth);
int smx_strips_attach(smx_ctx* ctx, const smx_transport* t, int32_t rank, int32_t world, int32_t inset, int32_t seam_halfwidth);
int smx_strips_detach(smx_ctx* ctx);
int smx_strips_tick(smx_ctx* ctx, int32_t nwater, int32_t nwind, int32_t dowater, int32_t dowind);
/* what the transport itself cost since it was attached: stream synchronisations it asked for and ncclGroupStart/End pairs (RCCL: 2 groups and at most
 * 2 synchronisations per seam exchange since round 6 -- pack counts, incoming header --, plus one per all-reduce) */
int smx_strips_sync_stats(smx_ctx* ctx, uint64_t* host_syncs, uint64_t* groups);
/* one synthetic seam message (nrec column records in nbytes bytes, npart particle records) from this rank to this very rank through the attached transport's
 * exchange -- with RCCL: the grouped ncclSend / ncclRecv pairs of a real seam exchange -- compared byte for byte on return (0; -4 = it came back changed).
 * What a single device can check of the path several GPUs depend on; nothing in the reference corresponds to it. */
int smx_strips_selfcheck(smx_ctx* ctx, uint32_t nrec, uint32_t nbytes, uint32_t npart);
int smx_strips_stats(smx_ctx* ctx, uint64_t* chunks, uint64_t* seam_chunks, uint64_t* generations, uint64_t* bytes_sent, uint64_t* messages);
/* batched engine: epochs (kernel rounds), generations and dropped child particles since the context was created */
int smx_get_batch_stats(smx_ctx* ctx, uint64_t* epochs, uint64_t* generations, uint64_t* children_lost);
void* smx_stream(smx_ctx* ctx);                          /* the hipStream_t all work is queued on */

/* ---- LBM wind: the D3Q19 two-relaxation-time lattice Boltzmann solver the reference runs as OpenGL
 * compute shaders (source/include/lbmwind/lbmwind.h:75-197; shader/LBM/{lbm,init,collide,stream}.cs; shader/move.cs). It is
 * visual only in the reference (it never feeds WindParticle). A lattice is its own object; cell index (x*NY + y)*NZ + z and
 * the distribution order F[cell*19 + q] at this boundary are the reference's (lbm.cs:8-26,60-80); on the device the
 * distributions are stored direction-major and collide + stream are ONE kernel per step (csrc/soil_lbm.h).
 *   smx_lbm_create / _destroy      lbmw::initialize's buffers (lbmwind.h:77-96) / lbmw::quit (:152-172)
 *   smx_lbm_set_boundary           lbmw::b->fill(NX*NY*NZ, boundary) (lbmwind.h:89, SoilMachine.cpp:239): > 0 = solid
 *   smx_lbm_boundary_from_map      SoilMachine.cpp:235-238 on the device: solid where map.height(ivec2(sx*x, sz*z)) > (sy*y)/SCALE
 *   smx_lbm_initialize             init.cs (lbmwind.h:98-109)
 *   smx_lbm_step(n)                n x { collide.cs; stream.cs } (lbmw::update, lbmwind.h:176-188); rho and v are those collide.cs
 *                                  writes: the moments of the state the step started from
 *   smx_lbm_read                   RHO (n floats), V (n vec4), F (n*19, reference order); any pointer may be NULL
 *   smx_lbm_write_f                overwrite F (tests, restart)
 *   smx_lbm_move                   move.cs on the caller's tracer array (n vec4, in place); the respawn of lbmwind.h:199-218 stays host code.
 *                                  Tracers whose cell or cell+1 lies outside the lattice (the reference moves BEFORE its range check,
 *                                  lbmwind.h:193-215) sample the nearest lattice cell: indices are clamped, never out of bounds
 *   smx_lbm_get_timing             HIP-event time of the step kernels since the last reset */
typedef struct smx_lbm smx_lbm;
int smx_lbm_create(int32_t nx, int32_t ny, int32_t nz, int32_t device, smx_lbm** out);
void smx_lbm_destroy(smx_lbm* l);
const char* smx_lbm_last_error(smx_lbm* l);
int smx_lbm_set_boundary(smx_lbm* l, const float* boundary);
int smx_lbm_boundary_from_map(smx_lbm* l, smx_ctx* map, float sx, float sy, float sz);
int smx_lbm_initialize(smx_lbm* l);
int smx_lbm_step(smx_lbm* l, int32_t n);
int smx_lbm_read(smx_lbm* l, float* rho, float* v4, float* f);
int smx_lbm_write_f(smx_lbm* l, const float* f);
int smx_lbm_move(smx_lbm* l, float* pos4, int32_t n);
int smx_lbm_get_timing(smx_lbm* l, double* ms_steps, uint64_t* steps, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* SOILMX_H */
