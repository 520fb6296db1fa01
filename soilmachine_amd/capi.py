"""ctypes binding of the C-ABI in include/soilmx.h (libsoilmx.so, hand-written HIP for gfx950).

There is NO CPU fallback: importing the library without a built ``libsoilmx.so`` raises, and creating a
context without a visible HIP device fails with the library's own error text.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsoilmx.so")

ENGINE_SERIAL = 0
ENGINE_SPECULATIVE = 1
ENGINE_BATCHED = 2
ENGINE_RELAXED = 3


class Config(C.Structure):
    _fields_ = [("dimx", C.c_int32), ("dimy", C.c_int32), ("scale", C.c_int32), ("device", C.c_int32),
                ("pool_capacity", C.c_uint64), ("engine", C.c_int32), ("reserved", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "steps_water_top", "steps_water_all", "steps_wind", "nested_particles", "floods", "cascade_calls",
        "cascade_transfers", "wcascade_calls", "grid_active_cells", "rand_calls", "pool_free", "pool_overflow",
        "spec_rounds", "spec_aborts")] + [("reserved", C.c_uint64 * 2), ("spec_subphases_cut", C.c_uint64), ("spec_serial_particles", C.c_uint64),
                                           ("flood_nested_steps", C.c_uint64), ("grid_nested_steps", C.c_uint64)]

    def as_dict(self) -> dict:
        d = {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}
        d["spec_fallbacks"], d["spec_executed"] = int(self.reserved[0]), int(self.reserved[1])
        return d


# smx_transport (include/soilmx.h): callbacks on host buffers for smx_strips_attach
SEND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64)
RECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64))
RED64_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64))
MIN32_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint64)
GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64))


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("send", SEND_FN), ("recv", RECV_FN), ("allreduce_sum_u64", RED64_FN), ("allreduce_max_u64", RED64_FN),
                ("allreduce_min_u32", MIN32_FN), ("allgather", GATHER_FN)]


class Timing(C.Structure):
    _fields_ = [("ms_water", C.c_double), ("ms_grid", C.c_double), ("ms_wind", C.c_double), ("ms_freq", C.c_double),
                ("launches_water", C.c_uint64), ("launches_grid", C.c_uint64), ("launches_wind", C.c_uint64),
                ("launches_freq", C.c_uint64), ("ms_kernel_water", C.c_double), ("ms_kernel_wind", C.c_double),
                ("launches_kernel_water", C.c_uint64), ("launches_kernel_wind", C.c_uint64),
                ("ms_kernel_classify", C.c_double), ("ms_kernel_gridtiles", C.c_double), ("ms_kernel_mapfreq", C.c_double),
                ("launches_kernel_classify", C.c_uint64), ("launches_kernel_gridtiles", C.c_uint64),
                ("launches_kernel_mapfreq", C.c_uint64),
                ("launches_step_water", C.c_uint64), ("launches_step_wind", C.c_uint64),
                ("ms_kernel_epochs", C.c_double), ("ms_kernel_tail", C.c_double), ("ms_kernel_grid_children", C.c_double),
                ("launches_kernel_epochs", C.c_uint64), ("epochs_kernel_epochs", C.c_uint64), ("launches_kernel_tail", C.c_uint64),
                ("epochs_kernel_tail", C.c_uint64), ("launches_kernel_grid_children", C.c_uint64),
                ("ms_kernel_floods", C.c_double), ("launches_kernel_floods", C.c_uint64), ("launches_floods_all", C.c_uint64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class MemberFigures(C.Structure):
    """smx_member_figures: one member's entry of smx_ensemble_figures (80 bytes)."""
    _fields_ = [("sumh", C.c_double), ("nsec", C.c_uint64), ("typehash", C.c_uint64), ("wet_cells", C.c_uint64),
                ("water_volume", C.c_double), ("hmin", C.c_double), ("hmax", C.c_double), ("empty_cells", C.c_uint64),
                ("rand_calls", C.c_uint64), ("live_sections", C.c_uint64)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["typehash"] = f"{int(self.typehash):016x}"          # as Snapshot.digest() and tests/golden/digests.json spell it
        return d


class Lake(C.Structure):
    """smx_lake: one lake of smx_lakes / smx_ensemble_lakes (64 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("cells", C.c_uint32), ("volume_q40", C.c_uint64), ("level_min", C.c_double),
                ("level_max", C.c_double), ("depth_max", C.c_double), ("x0", C.c_uint16), ("y0", C.c_uint16), ("x1", C.c_uint16),
                ("y1", C.c_uint16), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}
        d["volume"] = int(self.volume_q40) * 2.0 ** -40      # below the exact sum of the sizes by less than cells * 2^-40
        return d


class Basin(C.Structure):
    """smx_basin: one basin of smx_drainage / smx_ensemble_drainage (48 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("cells", C.c_uint32), ("wet_cells", C.c_uint32), ("flags", C.c_uint32),
                ("height_min", C.c_double), ("height_max", C.c_double), ("x0", C.c_uint16), ("y0", C.c_uint16), ("x1", C.c_uint16),
                ("y1", C.c_uint16), ("reserved", C.c_uint32 * 2)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class Stream(C.Structure):
    """smx_segment: one segment of smx_streams / smx_ensemble_streams (64 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("last_cell", C.c_uint32), ("cells", C.c_uint32), ("order", C.c_uint32),
                ("down", C.c_uint32), ("basin", C.c_uint32), ("flags", C.c_uint32), ("heads", C.c_uint32),
                ("straight", C.c_uint32), ("diagonal", C.c_uint32), ("area_first", C.c_uint32), ("area_last", C.c_uint32),
                ("height_first", C.c_double), ("height_last", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class Spill(C.Structure):
    """smx_spill_record: one basin's record of smx_spill / smx_ensemble_spill (64 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("pour_cell", C.c_uint32), ("pour_to", C.c_uint32), ("to_basin", C.c_uint32),
                ("flags", C.c_uint32), ("cells_below", C.c_uint32), ("pour_height", C.c_double), ("fill_height", C.c_double),
                ("storage_q40", C.c_uint64), ("fill_storage_q40", C.c_uint64), ("reserved", C.c_uint32 * 2)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}
        d["storage"] = int(self.storage_q40) * 2.0 ** -40      # below the exact sum of the differences by less than cells_below * 2^-40
        d["fill_storage"] = int(self.fill_storage_q40) * 2.0 ** -40
        return d


class Through(C.Structure):
    """smx_through_record: one basin's record of smx_through / smx_ensemble_through (64 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("exit_cell", C.c_uint32), ("exit_to", C.c_uint32), ("down", C.c_uint32),
                ("outlet", C.c_uint32), ("outlet_cell", C.c_uint32), ("hops", C.c_uint32), ("flags", C.c_uint32),
                ("cells", C.c_uint32), ("through_cells", C.c_uint32), ("upstream_basins", C.c_uint32), ("reserved", C.c_uint32),
                ("exit_height", C.c_double), ("fill_height", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class Hillslope(C.Structure):
    """smx_hillslope: one segment's record of smx_hillslopes / smx_ensemble_hillslopes (64 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("cells", C.c_uint32), ("steps_max", C.c_uint32), ("farthest_cell", C.c_uint32),
                ("straight_sum", C.c_uint64), ("diagonal_sum", C.c_uint64), ("hand_max", C.c_double), ("hand_sum_q40", C.c_uint64),
                ("bank_cells", C.c_uint32), ("head_cells", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}
        d["hand_sum"] = int(self.hand_sum_q40) * 2.0 ** -40    # below the exact sum of the hands by less than cells * 2^-40
        return d


class Flowpath(C.Structure):
    """smx_flowpath: one basin's record of smx_flowpaths / smx_ensemble_flowpaths (64 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("cells", C.c_uint32), ("source_cell", C.c_uint32), ("terminal_cell", C.c_uint32),
                ("steps_max", C.c_uint32), ("diagonal", C.c_uint32), ("profile_at", C.c_uint32), ("flags", C.c_uint32),
                ("straight_sum", C.c_uint64), ("diagonal_sum", C.c_uint64), ("drop_source", C.c_double), ("drop_max", C.c_double)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["length"] = (int(self.steps_max) - int(self.diagonal)) + int(self.diagonal) * math.sqrt(2.0)    # of the main stem, in cell widths
        return d


class Catchment(C.Structure):
    """smx_catchment: one listed cell's record of smx_catchments / smx_ensemble_catchments (64 bytes)."""
    _fields_ = [("cell", C.c_uint32), ("cells", C.c_uint32), ("area", C.c_uint32), ("downstream", C.c_uint32),
                ("basin", C.c_uint32), ("steps_max", C.c_uint32), ("farthest_cell", C.c_uint32), ("flags", C.c_uint32),
                ("straight_sum", C.c_uint64), ("diagonal_sum", C.c_uint64), ("drop_max", C.c_double), ("drop_sum_q40", C.c_uint64)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["drop_sum"] = int(self.drop_sum_q40) * 2.0 ** -40    # below the exact sum of the drops by less than cells * 2^-40
        return d


class Horizon(C.Structure):
    """smx_horizon_record: one selected direction's record of smx_horizons / smx_ensemble_horizons (64 bytes)."""
    _fields_ = [("direction", C.c_uint32), ("ux", C.c_int16), ("uy", C.c_int16), ("bounded", C.c_uint32), ("step_max", C.c_uint32),
                ("step_max_cell", C.c_uint32), ("reserved0", C.c_uint32), ("step_sum", C.c_uint64), ("slope_max", C.c_double), ("reserved", C.c_uint32 * 6)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("reserved")}


class Proximity(C.Structure):
    """smx_proximity_record: one group's record of smx_proximity / smx_ensemble_proximity (64 bytes)."""
    _fields_ = [("site", C.c_uint32), ("sites", C.c_uint32), ("cells", C.c_uint32), ("dist2_max", C.c_uint32), ("farthest_cell", C.c_uint32),
                ("flags", C.c_uint32), ("dist2_sum", C.c_uint64), ("x0", C.c_uint16), ("y0", C.c_uint16), ("x1", C.c_uint16), ("y1", C.c_uint16),
                ("reserved", C.c_uint32 * 6)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class Sun(C.Structure):
    """smx_sun: a sun of smx_horizons / smx_ensemble_horizons (16 bytes): the lattice direction towards it and tan(elevation)."""
    _fields_ = [("direction", C.c_uint32), ("reserved", C.c_uint32), ("tangent", C.c_double)]


class Dispersal(C.Structure):
    """smx_dispersal_record: one basin's record of smx_dispersal / smx_ensemble_dispersal (64 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("cells", C.c_uint32), ("flags", C.c_uint32), ("peak_cell", C.c_uint32),
                ("inflow_q24", C.c_uint64), ("leak_in_q24", C.c_uint64), ("leak_out_q24", C.c_uint64), ("peak_q24", C.c_uint64),
                ("givers", C.c_uint32), ("split_cells", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    def as_dict(self) -> dict:
        d = {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}
        for f in ("inflow", "leak_in", "leak_out", "peak"):
            d[f] = d[f + "_q24"] / DISPERSAL_ONE               # in cells
        return d


class SoilTotal(C.Structure):
    """smx_soil_total: one soil type's record of smx_soil_totals / smx_ensemble_soil_totals (48 bytes)."""
    _fields_ = [("sections", C.c_uint64), ("cells", C.c_uint64), ("top_cells", C.c_uint64), ("volume_q40", C.c_uint64),
                ("held_q40", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self) -> dict:
        d = {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}
        d["volume"] = d["volume_q40"] * 2.0 ** -40            # below the exact sum of the sizes by less than sections * 2^-40
        d["held"] = d["held_q40"] * 2.0 ** -40
        return d


class BudgetBasin(C.Structure):
    """smx_budget_basin: one basin's record of smx_budget / smx_ensemble_budget (96 bytes)."""
    _fields_ = [("first_cell", C.c_uint32), ("cells", C.c_uint32), ("lowered_cells", C.c_uint32), ("raised_cells", C.c_uint32),
                ("resurfaced_cells", C.c_uint32), ("flags", C.c_uint32),
                ("eroded_q40", C.c_uint64), ("deposited_q40", C.c_uint64), ("water_gained_q40", C.c_uint64), ("water_lost_q40", C.c_uint64),
                ("cut_max", C.c_double), ("fill_max", C.c_double), ("cut_cell", C.c_uint32), ("fill_cell", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]

    def as_dict(self) -> dict:
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}
        d["eroded"] = d["eroded_q40"] / BUDGET_ONE             # in height units x cells
        d["deposited"] = d["deposited_q40"] / BUDGET_ONE
        d["net"] = (d["deposited_q40"] - d["eroded_q40"]) / BUDGET_ONE     # the basin's sediment yield is -net
        return d


class BudgetSoil(C.Structure):
    """smx_budget_soil: one soil type's record of smx_budget / smx_ensemble_budget (64 bytes)."""
    _fields_ = [("gained_q40", C.c_uint64), ("lost_q40", C.c_uint64), ("held_gained_q40", C.c_uint64), ("held_lost_q40", C.c_uint64),
                ("cells_gained", C.c_uint32), ("cells_lost", C.c_uint32), ("surfaced", C.c_uint32), ("covered", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def as_dict(self) -> dict:
        d = {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}
        d["gained"] = d["gained_q40"] / BUDGET_ONE
        d["lost"] = d["lost_q40"] / BUDGET_ONE
        d["net"] = (d["gained_q40"] - d["lost_q40"]) / BUDGET_ONE
        return d


BUDGET_ONE = 1 << 40                   # one height unit on one cell (the *_q40 fields of the budget records)
BUDGET_NONE = 0xFFFFFFFF               # smx_budget_basin.cut_cell / fill_cell: no lowered / raised cell
BUDGET_TERM_UNRELIABLE, BUDGET_WRAPPED, BUDGET_NAN_GROUND = 1, 2, 4    # smx_budget_basin.flags (the first two: smx_budget_soil.flags too)
TOTALS_MAX_TYPES = 64                  # SMX_TOTALS_MAX_TYPES
TOTAL_VOLUME_UNRELIABLE, TOTAL_HELD_UNRELIABLE = 1, 2                  # smx_soil_total.flags
THICKNESS_MAX_TYPES = 8

LAKE_DRY = 0xFFFFFFFF                  # a dry cell of the label plane
LAKE_BORDER, LAKE_VOLUME_UNRELIABLE = 1, 2                             # smx_lake.flags
DRAIN_NONE = 0xFFFFFFFF                # the receiver plane: a sink or a wet cell
BASIN_LAKE, BASIN_BORDER = 1, 2                                        # smx_basin.flags
STREAM_NONE = 0xFFFFFFFF               # smx_segment.down: the segment joins no other; the segments plane: no channel cell
STREAM_WET, STREAM_SINK, STREAM_HEAD, STREAM_BORDER = 1, 2, 4, 8       # smx_segment.flags

SPILL_NONE = 0xFFFFFFFF                # smx_spill_record.pour_to / to_basin: off the map
SPILL_LAKE, SPILL_OFFMAP, SPILL_NESTED, SPILL_STORAGE_UNRELIABLE, SPILL_FILL_STORAGE_UNRELIABLE = 1, 2, 4, 8, 16   # smx_spill_record.flags

THROUGH_NONE = 0xFFFFFFFF              # smx_through_record.exit_to / down: off the map
THROUGH_LAKE, THROUGH_OFFMAP, THROUGH_NOT_POUR, THROUGH_WET_ENTRY = 1, 2, 4, 8   # smx_through_record.flags
HILL_NONE = 0xFFFFFFFF                 # the entry / hillslope planes: a wet cell; hillslope: unchannelled land; smx_hillslope.farthest_cell: no cell
HILL_HAND_UNRELIABLE = 1                # smx_hillslope.flags
PATH_NONE = 0xFFFFFFFF                 # the stem plane: a cell off the stems
PATH_TERMINAL_WET = 1                  # smx_flowpath.flags
CATCH_NONE = 0xFFFFFFFF                # the gauge plane: the entry is no gauge; smx_catchment.downstream: no gauge down the flow
CATCH_DROP_UNRELIABLE, CATCH_WET, CATCH_SINK = 1, 2, 4                 # smx_catchment.flags
CATCHMENT_MAX_BINS = 64                # SMX_CATCHMENT_MAX_BINS
HORIZON_DIRECTIONS = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1),
                      (-1, 0), (-2, -1), (-1, -1), (-1, -2), (0, -1), (1, -2), (1, -1), (2, -1))   # (ux, uy) of direction d, counter-clockwise from +x
HORIZON_MAX_SUNS = 64                  # SMX_HORIZON_MAX_SUNS
HORIZON_NONE = 0xFFFFFFFF              # smx_horizon_record.step_max_cell: no bounded cell
PROXIMITY_NONE = 0xFFFFFFFF            # the nearest, group and dist2 planes: the map has no site
PROXIMITY_BORDER = 1                   # smx_proximity_record.flags
PROXIMITY_MAX_BINS, PROXIMITY_MAX_SIDE = 64, 32768                     # SMX_PROXIMITY_MAX_BINS, SMX_PROXIMITY_MAX_SIDE
DISPERSAL_ONE = 1 << 24               # one cell of dispersed area (the area plane, the *_q24 fields)
DISPERSAL_MAX_EXPONENT = 16

PLANE_HEIGHT, PLANE_WATER, PLANE_WFREQ, PLANE_WINDFREQ = 0, 1, 2, 3    # SMX_PLANE_*
PLANES = {"height": PLANE_HEIGHT, "water": PLANE_WATER, "wfreq": PLANE_WFREQ, "windfreq": PLANE_WINDFREQ}


# every symbol include/soilmx.h declares (tests/test_capi_symbols.py checks the library exports them all)
SYMBOLS = [
    "smx_create", "smx_create_strip", "smx_destroy", "smx_last_error", "smx_set_soils", "smx_set_scale", "smx_srand", "smx_rand", "smx_rand_advance", "smx_get_rand_state", "smx_set_rand_state",
    "smx_initialize", "smx_import_columns", "smx_import_frequency", "smx_num_sections", "smx_export_columns",
    "smx_read_frequency", "smx_read_heights", "smx_read_surface", "smx_tick_water", "smx_grid_pass", "smx_tick_wind",
    "smx_map_frequency", "smx_reset_frequency", "smx_tick", "smx_sync", "smx_add", "smx_remove",
    "smx_particle_cascade", "smx_water_cascade", "smx_seep", "smx_top", "smx_normals", "smx_heights_bilinear", "smx_fill_vertices", "smx_fill_vertices_cut", "smx_fill_vertex_cut",
    "smx_digest", "smx_save", "smx_load", "smx_get_counters", "smx_get_timing", "smx_get_counters_sized", "smx_get_timing_sized", "smx_timing_reset", "smx_set_engine", "smx_set_spec_limits", "smx_stream", "smx_set_batch_dilate", "smx_get_batch_stats", "smx_set_batch_strips", "smx_set_relax_wind", "smx_set_relax_launch", "smx_set_relax_settle", "smx_get_relax_settle", "smx_get_relax_flood_flow", "smx_set_grid_interleave", "smx_set_water_generations", "smx_get_water_generations", "smx_set_water_stagger", "smx_get_water_stagger", "smx_strips_rccl_unique_id", "smx_strips_attach_rccl", "smx_strips_attach", "smx_strips_detach", "smx_strips_tick", "smx_strips_stats", "smx_strips_sync_stats", "smx_strips_selfcheck",
    "smx_d_set_own", "smx_d_gen_begin", "smx_d_gen_spawn", "smx_d_next_phase", "smx_d_chunk", "smx_d_gen_end", "smx_d_pack_columns",
    "smx_d_unpack_columns", "smx_d_pack_particles", "smx_d_unpack_particles", "smx_d_grid_begin", "smx_d_grid_sweep_cols",
    "smx_lbm_create", "smx_lbm_destroy", "smx_lbm_last_error", "smx_lbm_set_boundary", "smx_lbm_boundary_from_map", "smx_lbm_initialize",
    "smx_lbm_step", "smx_lbm_read", "smx_lbm_write_f", "smx_lbm_move", "smx_lbm_get_timing",
    "smx_ensemble_create", "smx_ensemble_destroy", "smx_ensemble_last_error", "smx_ensemble_add", "smx_ensemble_remove", "smx_ensemble_size",
    "smx_ensemble_tick", "smx_ensemble_sync", "smx_ensemble_get_timing", "smx_ensemble_timing_reset",
    "smx_ensemble_figures", "smx_ensemble_plane_stats", "smx_copy_state", "smx_ensemble_fork",
    "smx_lakes", "smx_ensemble_lakes", "smx_drainage", "smx_ensemble_drainage",
    "smx_streams", "smx_ensemble_streams",
    "smx_spill", "smx_ensemble_spill", "smx_get_spill_sweeps", "smx_ensemble_get_spill_sweeps",
    "smx_through", "smx_ensemble_through", "smx_get_through_sweeps", "smx_ensemble_get_through_sweeps",
    "smx_hillslopes", "smx_ensemble_hillslopes",
    "smx_flowpaths", "smx_ensemble_flowpaths",
    "smx_catchments", "smx_ensemble_catchments",
    "smx_horizons", "smx_ensemble_horizons",
    "smx_proximity", "smx_ensemble_proximity",
    "smx_dispersal", "smx_ensemble_dispersal", "smx_get_dispersal_rounds", "smx_ensemble_get_dispersal_rounds",
    "smx_soil_totals", "smx_ensemble_soil_totals", "smx_soil_thickness", "smx_cores",
    "smx_budget", "smx_ensemble_budget",
    "smx_set_analysis_launch", "smx_ensemble_set_analysis_launch", "smx_get_analysis_launch", "smx_ensemble_get_analysis_launch",
    "smx_switches",
]

ENSEMBLE_MAX_MEMBERS = 4096    # SMX_ENSEMBLE_MAX_MEMBERS

_lib = None


def load() -> C.CDLL:
    """Load libsoilmx.so and declare the prototypes. Fails loudly if the HIP library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build the HIP extension first "
                           f"(python -c 'import __graft_entry__ as g; g.build()'); soilmx has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, u64, dbl, flt = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_double, C.c_float
    L.smx_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.smx_destroy.argtypes = [vp]; L.smx_destroy.restype = None
    L.smx_last_error.argtypes = [vp]; L.smx_last_error.restype = C.c_char_p
    L.smx_set_soils.argtypes = [vp, vp, i32]
    L.smx_set_scale.argtypes = [vp, i32]
    L.smx_srand.argtypes = [vp, u32]
    L.smx_rand.argtypes = [vp, C.POINTER(i32)]
    L.smx_rand_advance.argtypes = [vp, u64]
    L.smx_get_rand_state.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u64)]
    L.smx_set_rand_state.argtypes = [vp, vp, u32, u64]
    L.smx_initialize.argtypes = [vp, i32, vp, i32]
    L.smx_import_columns.argtypes = [vp] + [vp] * 5
    L.smx_import_frequency.argtypes = [vp] + [vp] * 3
    L.smx_num_sections.argtypes = [vp, C.POINTER(u64)]
    L.smx_export_columns.argtypes = [vp] + [vp] * 5
    L.smx_read_frequency.argtypes = [vp] + [vp] * 3
    L.smx_read_heights.argtypes = [vp, vp]
    L.smx_read_surface.argtypes = [vp, vp]
    L.smx_tick_water.argtypes = [vp, i32]
    L.smx_grid_pass.argtypes = [vp]
    L.smx_tick_wind.argtypes = [vp, i32]
    L.smx_map_frequency.argtypes = [vp]
    L.smx_reset_frequency.argtypes = [vp]
    L.smx_tick.argtypes = [vp, i32, i32, i32, i32]
    L.smx_sync.argtypes = [vp]
    L.smx_add.argtypes = [vp, i32, i32, dbl, u32]
    L.smx_remove.argtypes = [vp, i32, i32, dbl, C.POINTER(dbl)]
    L.smx_particle_cascade.argtypes = [vp, flt, flt, i32]
    L.smx_water_cascade.argtypes = [vp, i32, i32, i32]
    L.smx_seep.argtypes = [vp, i32, i32]
    L.smx_top.argtypes = [vp, i32, i32, C.POINTER(u32), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(dbl), C.POINTER(i32)]
    L.smx_normals.argtypes = [vp, vp]
    L.smx_fill_vertices.argtypes = [vp, vp, C.c_int32, vp]
    L.smx_fill_vertices_cut.argtypes = [vp, vp, C.c_int32, C.c_int32, dbl, vp]
    L.smx_fill_vertex_cut.argtypes = [vp, vp, C.c_int32, C.c_int32, dbl, C.c_int32, C.c_int32, vp]
    L.smx_heights_bilinear.argtypes = [vp, vp, i32, vp]
    L.smx_save.argtypes = [vp, C.c_char_p]
    L.smx_load.argtypes = [vp, C.c_char_p]
    L.smx_digest.argtypes = [vp, C.POINTER(dbl), C.POINTER(u64), C.POINTER(u64)]
    L.smx_get_counters.argtypes = [vp, C.POINTER(Counters)]
    L.smx_get_timing.argtypes = [vp, C.POINTER(Timing)]
    L.smx_get_counters_sized.argtypes = [vp, C.POINTER(Counters), u64]
    L.smx_get_timing_sized.argtypes = [vp, C.POINTER(Timing), u64]
    L.smx_timing_reset.argtypes = [vp]
    L.smx_set_engine.argtypes = [vp, i32]
    L.smx_set_water_generations.argtypes = [vp, i32]
    L.smx_get_water_generations.argtypes = [vp, C.POINTER(i32)]
    L.smx_set_water_stagger.argtypes = [vp, i32]
    L.smx_get_water_stagger.argtypes = [vp, C.POINTER(i32)]
    L.smx_set_spec_limits.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.smx_set_batch_dilate.argtypes = [vp, i32]
    L.smx_set_batch_strips.argtypes = [vp, i32, i32, i32]
    L.smx_set_relax_wind.argtypes = [vp, u32, i32]
    L.smx_set_relax_launch.argtypes = [vp, i32, i32]
    L.smx_set_relax_settle.argtypes = [vp, i32, i32, i32]
    L.smx_get_relax_settle.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.smx_get_relax_flood_flow.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.smx_create_strip.argtypes = [C.POINTER(Config), i32, i32, C.POINTER(vp)]
    L.smx_strips_rccl_unique_id.argtypes = [vp]
    L.smx_strips_attach_rccl.argtypes = [vp, vp, i32, i32, i32, i32]
    L.smx_strips_attach.argtypes = [vp, C.POINTER(Transport), i32, i32, i32, i32]
    L.smx_strips_detach.argtypes = [vp]
    L.smx_strips_tick.argtypes = [vp, i32, i32, i32, i32]
    L.smx_strips_stats.argtypes = [vp] + [C.POINTER(u64)] * 5
    L.smx_strips_sync_stats.argtypes = [vp] + [C.POINTER(u64)] * 2
    L.smx_strips_selfcheck.argtypes = [vp, u32, u32, u32]
    L.smx_d_set_own.argtypes = [vp, i32, i32]
    L.smx_d_gen_begin.argtypes = [vp, i32, u32, vp, vp]
    L.smx_d_gen_spawn.argtypes = [vp, vp, C.POINTER(u32)]
    L.smx_d_next_phase.argtypes = [vp]
    L.smx_d_chunk.argtypes = [vp, u32, C.POINTER(u32)]
    L.smx_d_gen_end.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.smx_d_pack_columns.argtypes = [vp, i32, i32, vp, u64, C.POINTER(u64)]
    L.smx_d_unpack_columns.argtypes = [vp, vp, u64]
    L.smx_d_pack_particles.argtypes = [vp, i32, i32, vp, u64, C.POINTER(u64)]
    L.smx_d_unpack_particles.argtypes = [vp, vp, u64]
    L.smx_d_grid_begin.argtypes = [vp]
    L.smx_d_grid_sweep_cols.argtypes = [vp, i32, i32, i32]
    L.smx_get_batch_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    L.smx_lbm_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.smx_lbm_destroy.argtypes = [vp]; L.smx_lbm_destroy.restype = None
    L.smx_lbm_last_error.argtypes = [vp]; L.smx_lbm_last_error.restype = C.c_char_p
    L.smx_lbm_set_boundary.argtypes = [vp, vp]
    L.smx_lbm_boundary_from_map.argtypes = [vp, vp, flt, flt, flt]
    L.smx_lbm_initialize.argtypes = [vp]
    L.smx_lbm_step.argtypes = [vp, i32]
    L.smx_lbm_read.argtypes = [vp, vp, vp, vp]
    L.smx_lbm_write_f.argtypes = [vp, vp]
    L.smx_lbm_move.argtypes = [vp, vp, i32]
    L.smx_lbm_get_timing.argtypes = [vp, C.POINTER(dbl), C.POINTER(u64), i32]
    L.smx_stream.argtypes = [vp]; L.smx_stream.restype = vp
    L.smx_ensemble_create.argtypes = [i32, C.POINTER(vp)]
    L.smx_ensemble_destroy.argtypes = [vp]; L.smx_ensemble_destroy.restype = None
    L.smx_ensemble_last_error.argtypes = [vp]; L.smx_ensemble_last_error.restype = C.c_char_p
    L.smx_ensemble_add.argtypes = [vp, C.POINTER(Config), C.POINTER(vp)]
    L.smx_ensemble_remove.argtypes = [vp, vp]
    L.smx_ensemble_size.argtypes = [vp, C.POINTER(i32)]
    L.smx_ensemble_tick.argtypes = [vp, vp, vp, i32, i32]
    L.smx_ensemble_sync.argtypes = [vp]
    L.smx_ensemble_get_timing.argtypes = [vp, C.POINTER(Timing), u64]
    L.smx_ensemble_timing_reset.argtypes = [vp]
    L.smx_ensemble_figures.argtypes = [vp, vp, u64]
    L.smx_ensemble_plane_stats.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.smx_copy_state.argtypes = [vp, vp]
    L.smx_ensemble_fork.argtypes = [vp, vp, i32, u64, vp, C.POINTER(vp)]
    L.smx_lakes.argtypes = [vp, vp, u64, u32, C.POINTER(u32), vp]
    L.smx_ensemble_lakes.argtypes = [vp, vp, u64, u32, vp]
    L.smx_drainage.argtypes = [vp, vp, u64, u32, C.POINTER(u32), vp, vp, vp]
    L.smx_ensemble_drainage.argtypes = [vp, vp, u64, u32, vp]
    L.smx_streams.argtypes = [vp, u32, vp, u64, u32, C.POINTER(u32), vp, vp, vp, vp]
    L.smx_ensemble_streams.argtypes = [vp, u32, vp, u64, u32, vp]
    L.smx_spill.argtypes = [vp, vp, u64, u32, C.POINTER(u32), vp]
    L.smx_ensemble_spill.argtypes = [vp, vp, u64, u32, vp]
    L.smx_get_spill_sweeps.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.smx_ensemble_get_spill_sweeps.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.smx_through.argtypes = [vp, vp, u64, u32, C.POINTER(u32), vp, vp]
    L.smx_ensemble_through.argtypes = [vp, vp, u64, u32, vp]
    L.smx_get_through_sweeps.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.smx_ensemble_get_through_sweeps.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.smx_hillslopes.argtypes = [vp, u32, vp, u64, u32, C.POINTER(u32), vp, vp, vp, vp, vp]
    L.smx_ensemble_hillslopes.argtypes = [vp, u32, vp, u64, u32, vp]
    L.smx_flowpaths.argtypes = [vp, vp, u64, u32, C.POINTER(u32), vp, vp, vp, vp, vp, vp, vp, vp, u32, C.POINTER(u32)]
    L.smx_ensemble_flowpaths.argtypes = [vp, vp, u64, u32, vp]
    L.smx_catchments.argtypes = [vp, vp, u32, vp, u64, vp, u32, dbl, vp, vp, vp, vp]
    L.smx_ensemble_catchments.argtypes = [vp, vp, u32, vp, u64, vp, u32, dbl]
    L.smx_horizons.argtypes = [vp, u32, u32, vp, u64, vp, u32, vp, vp, vp, vp, vp, vp]
    L.smx_ensemble_horizons.argtypes = [vp, u32, u32, vp, u64, vp, u32, vp]
    L.smx_proximity.argtypes = [vp, vp, u32, vp, u64, u32, vp, vp, u32, u32, vp, vp, vp]
    L.smx_ensemble_proximity.argtypes = [vp, vp, u32, vp, u64, u32, vp, vp, u32, u32]
    L.smx_dispersal.argtypes = [vp, u32, vp, u64, u32, C.POINTER(u32), vp, vp, vp]
    L.smx_ensemble_dispersal.argtypes = [vp, u32, vp, u64, u32, vp]
    L.smx_get_dispersal_rounds.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.smx_ensemble_get_dispersal_rounds.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.smx_soil_totals.argtypes = [vp, vp, u64, u32, vp]
    L.smx_ensemble_soil_totals.argtypes = [vp, vp, u64, u32, vp]
    L.smx_soil_thickness.argtypes = [vp, vp, i32, vp, vp, vp]
    L.smx_cores.argtypes = [vp, vp, u32, vp, u64, C.POINTER(u64), vp, vp, vp, vp]
    L.smx_budget.argtypes = [vp, vp, vp, u64, u32, C.POINTER(u32), vp, u64, u32, vp, vp, vp, vp]
    L.smx_ensemble_budget.argtypes = [vp, vp, vp, u64, u32, C.POINTER(u32), vp, u64, u32]
    L.smx_set_analysis_launch.argtypes = [vp, i32, i32, i32]
    L.smx_ensemble_set_analysis_launch.argtypes = [vp, i32, i32, i32]
    L.smx_get_analysis_launch.argtypes = [vp, vp, vp]
    L.smx_ensemble_get_analysis_launch.argtypes = [vp, vp, vp]
    L.smx_switches.argtypes = [C.c_char_p, u64, C.POINTER(u64)]
    for name in SYMBOLS:
        f = getattr(L, name)
        if name not in ("smx_destroy", "smx_last_error", "smx_stream", "smx_lbm_destroy", "smx_lbm_last_error",
                        "smx_ensemble_destroy", "smx_ensemble_last_error"):
            f.restype = C.c_int
    _lib = L
    return L


def switches() -> dict:
    """The library's run-time switches (smx_switches): name -> {"value", "default", "class"} as this process read them; "-" = not set
    and no default. Needs no device."""
    L = load()
    need = C.c_uint64()
    L.smx_switches(None, 0, C.byref(need))
    buf = C.create_string_buffer(int(need.value))
    rc = L.smx_switches(buf, need.value, None)
    if rc != 0:
        raise RuntimeError(f"smx_switches failed (rc={rc})")
    out = {}
    for line in buf.value.decode().splitlines():
        name, rest = line.split("=", 1)
        value, default, cls = rest.rsplit(" ", 2)
        out[name] = {"value": value, "default": default, "class": cls}
    return out


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def proximity_cells(cells, dimy: int):
    """(list, n) as smx_proximity takes them: (None, 0) for ``cells`` None (the wet cells), else the flat uint32 indices of a
    sequence of flat indices x*dimy + y or of (x, y) pairs."""
    if cells is None:
        return None, 0
    cl = np.asarray(cells if isinstance(cells, np.ndarray) else list(cells), np.int64)
    if cl.ndim == 2 and cl.shape[1] == 2:
        cl = cl[:, 0] * int(dimy) + cl[:, 1]
    cl = np.ascontiguousarray(cl.reshape(-1), np.uint32)
    if not len(cl):
        raise ValueError("proximity: cells is empty (None means the wet cells)")
    return cl, len(cl)


# ---- the horizons' small helpers (pure Python: no device, no library)
def horizon_mask(directions) -> int:
    """The 16-bit mask of ``directions``: a mask already, or an iterable of indices 0..15 or of (ux, uy) pairs of HORIZON_DIRECTIONS."""
    if isinstance(directions, (int, np.integer)):
        return int(directions)
    mask = 0
    for d in directions:
        if not isinstance(d, (int, np.integer)):
            pair = (int(d[0]), int(d[1]))
            if pair not in HORIZON_DIRECTIONS:
                raise ValueError(f"{pair} is no lattice direction (the sixteen of capi.HORIZON_DIRECTIONS)")
            d = HORIZON_DIRECTIONS.index(pair)
        if not 0 <= int(d) < 16:
            raise ValueError(f"direction {d} is outside 0..15")
        mask |= 1 << int(d)
    return mask


def horizon_direction(azimuth: float, elevation: float) -> tuple:
    """(d, tangent) of a sun or a wind at ``azimuth`` and ``elevation``, both in degrees: the lattice direction whose own azimuth
    atan2(uy, ux) is nearest (of two equally near the smaller d) and tan(elevation). The azimuth is counted from +x towards +y."""
    if not 0.0 <= elevation < 90.0:
        raise ValueError(f"elevation {elevation} is outside [0, 90) degrees")
    a = math.radians(azimuth)

    def off(d):
        ux, uy = HORIZON_DIRECTIONS[d]
        return abs(math.remainder(math.atan2(uy, ux) - a, 2.0 * math.pi))

    return min(range(16), key=lambda d: (off(d), d)), math.tan(math.radians(elevation))


def horizon_suns(positions):
    """A ctypes array of Sun from (azimuth, elevation) pairs in degrees (horizon_direction), as ``suns=`` of ``horizons`` takes it;
    an entry that is a Sun already, or a (d, tangent) pair with an integer d, is taken as it is."""
    out = (Sun * max(1, len(positions)))()
    for i, p in enumerate(positions):
        if isinstance(p, Sun):
            d, t = p.direction, p.tangent
        elif isinstance(p[0], (int, np.integer)):
            d, t = int(p[0]), float(p[1])
        else:
            d, t = horizon_direction(float(p[0]), float(p[1]))
        out[i].direction, out[i].reserved, out[i].tangent = d, 0, t
    return out
